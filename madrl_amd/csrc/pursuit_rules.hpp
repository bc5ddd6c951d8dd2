// pursuit_rules.hpp -- the PursuitEvade rules the four Pursuit step kernels share: the RNG contract and the reference's float64
// statement order, stated once for the kernels that call them.  Not every kernel calls every function: pursuit_wave.hpp and pursuit_group.hpp
// keep their own map draw, evader action draw and done bits, the wave kernel its rejection draw too.  The C oracle of the
// tests is the independent statement and does not include this file; tests/host/pursuit_rules_check.cpp holds the two against each other.
// Small pure functions, scalars in and small structs out, no pointer into device memory: "is this cell free" is a byte grid in one kernel
// and a dword layer in another, so the occupancy test, the `att < 1024` loop and every LDS read stay at the call sites.  No HIP include:
// a plain host compiler takes it too.  Which kernel calls which function, and why not the others: profiles/r20_pursuit_rules/README.md.
#pragma once

#include "philox.hpp"

#if defined(__HIPCC__)
#define MADRL_PR_HD __host__ __device__
#else
#define MADRL_PR_HD
#endif

namespace madrl {
namespace pr {

struct Window { int xlb, xub, ylb, yub; };   // agents are placed in [xlb, xub) x [ylb, yub)
struct Cell { int x, y; };
struct Counts { int np, ne; };
// ---- reset (pursuit_evade.py:173-207): draws 0, 1, 2 of TAG_RESET_ENV, then TAG_RESET_POS | attempt << 8 per agent
// draw 0: the episode's map (sample_maps, :182-183)
MADRL_PR_HD inline int reset_map_id(uint32_t gid, uint32_t tick, uint32_t k0, uint32_t k1, int n_maps) {
    return (int)mulhi32(philox4x32_10(gid, tick, 0u, TAG_RESET_ENV, k0, k1).x, (uint32_t)n_maps);
}
// draw 1: the constraint window (:185-191), float64 like the reference
MADRL_PR_HD inline Window reset_window(uint32_t gid, uint32_t tick, uint32_t k0, uint32_t k1, double cw, int xs, int ys) {
    const u32x4 rw = philox4x32_10(gid, tick, 1u, TAG_RESET_ENV, k0, k1);
    const double sx = u53(rw.x, rw.y) * (1.0 - cw);
    const double sy = u53(rw.z, rw.w) * (1.0 - cw);
    return Window{(int)(xs * sx), (int)(xs * (sx + cw)), (int)(ys * sy), (int)(ys * (sy + cw))};
}
// draw 2: random_opponents (:177-181): the episode has n_create <= cap evaders; the slots above are not created and count as gone
MADRL_PR_HD inline int reset_n_create(uint32_t gid, uint32_t tick, uint32_t k0, uint32_t k1, int max_opponents, int cap) {
    const int n = 1 + (int)mulhi32(philox4x32_10(gid, tick, 2u, TAG_RESET_ENV, k0, k1).x, (uint32_t)(max_opponents - 1));
    return n < cap ? n : cap;
}
// attempt `att` of feasible_position's rejection sampling (agent_utils.py:37-47) for agent `aidx`
MADRL_PR_HD inline Cell reset_cell(uint32_t gid, uint32_t tick, uint32_t aidx, uint32_t att, uint32_t k0, uint32_t k1, const Window &w) {
    const u32x4 r = philox4x32_10(gid, tick, aidx, TAG_RESET_POS | (att << 8), k0, k1);
    return Cell{w.xlb + (int)mulhi32(r.x, (uint32_t)(w.xub - w.xlb)), w.ylb + (int)mulhi32(r.y, (uint32_t)(w.yub - w.ylb))};
}
// per-env agent counts: agent a of the capacity layout (P pursuers, then the evader slots) in the LIVE layout (np pursuers, then the evaders):
// an env with live (np, ne) draws what env n of a fixed (np, ne) batch draws
MADRL_PR_HD inline uint32_t live_agent_index(int a, int P, int np) { return a >= P ? (uint32_t)(np + a - P) : (uint32_t)a; }
// the pending counts as a reset takes them: clamped to the capacity (the caller's array is not trusted with LDS indices or lanes)
MADRL_PR_HD inline Counts clamp_pending(int np_pending, int ne_pending, int P, int E) {
    const int np = np_pending > 1 ? np_pending : 1, ne = ne_pending > 0 ? ne_pending : 0;
    return Counts{np < P ? np : P, ne < E ? ne : E};
}
// ---- step (pursuit_evade.py:209-262)
// RandomPolicy.act (Controllers.py:15-16): evader k of the evader LAYER (the alive evaders in slot order); pursuer a under evader control
MADRL_PR_HD inline int evader_action(uint32_t gid, uint32_t tick, uint32_t kidx, uint32_t k0, uint32_t k1) {
    return (int)mulhi32(philox4x32_10(gid, tick, kidx, TAG_EVADER_ACT, k0, k1).x, 5u);
}
MADRL_PR_HD inline int pursuer_action(uint32_t gid, uint32_t tick, uint32_t a, uint32_t k0, uint32_t k1) {
    return (int)mulhi32(philox4x32_10(gid, tick, a, TAG_PURSUER_ACT, k0, k1).x, 5u);
}
// a pursuer's reward (:254-262, :359-381), three float64 statements in the reference's order.  kpre: evaders on the four neighbour cells
// before the move; sur: non-zero when the pursuer took part in a catch
MADRL_PR_HD inline double pursuer_reward(double catchr, int kpre, double term_pursuit, uint32_t sur, double urgency) {
    double r = catchr * (double)kpre;
    r += term_pursuit * (sur ? 1.0 : 0.0);
    r += urgency;
    return r;
}
// the done byte's episode bits (:383-389): 1 = no evader left, 2 = max_steps reached (tstep counts this step)
MADRL_PR_HD inline uint32_t done_bits(bool all_gone, int max_steps, int tstep) {
    uint32_t bits = 0u;
    if (all_gone) bits |= 1u;
    if (max_steps > 0 && tstep >= max_steps) bits |= 2u;
    return bits;
}
// ---- the dword layers of the one-wavefront and multi-wavefront kernels (pursuit_wave.hpp: padded layers, GW dwords per row)
// an agent's (x, y) from the record dword of agents 2j (low half) and 2j + 1 (high half)
MADRL_PR_HD inline Cell unpack_xy(uint32_t xyw, bool odd) {
    const uint32_t xy = odd ? (xyw >> 16) : (xyw & 0xFFFFu);
    return Cell{(int)(xy & 0xFF), (int)(xy >> 8)};
}
// np.clip keeps a border pursuer on its own cell (:374-380): the steps to the four cells the pre-move sum reads, 0 at a border
struct Clip4 { int dxm, dxp, dym, dyp; };
template <int GW, int XS, int YS>
MADRL_PR_HD inline Clip4 clipped_neighbours(int x, int y) { return Clip4{(x > 0) ? GW : 0, (x < XS - 1) ? GW : 0, (y > 0) ? 1 : 0, (y < YS - 1) ? 1 : 0}; }
// DiscreteAgent.step (DiscreteAgent.py:69-97): action 0 / 1 = x - 1 / x + 1, 2 / 3 = y + 1 / y - 1, 4 stays
template <int GW>
MADRL_PR_HD inline int move_dcell(int act) { return (act == 0 ? -GW : 0) + (act == 1 ? GW : 0) + (act == 2 ? 1 : 0) + (act == 3 ? -1 : 0); }
MADRL_PR_HD inline int move_dx(int act) { return (act == 1) - (act == 0); }
MADRL_PR_HD inline int move_dy(int act) { return (act == 2) - (act == 3); }
// how many of an evader's four neighbour cells hold pursuers (:150): a count >= 1 that is not `sent`, the mark of a cell outside the map
MADRL_PR_HD inline int cells_with_pursuers(uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t sent) {
    return (int)(n0 - 1u < sent - 1u) + (int)(n1 - 1u < sent - 1u) + (int)(n2 - 1u < sent - 1u) + (int)(n3 - 1u < sent - 1u);
}
// a caught evader on one of a pursuer's four neighbour cells (:489-495): its evader-count cell carries `caught`
MADRL_PR_HD inline bool caught_beside(uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t sent, uint32_t caught) {
    return ((n0 != sent) & (n0 >= caught)) | ((n1 != sent) & (n1 >= caught)) | ((n2 != sent) & (n2 >= caught)) | ((n3 != sent) & (n3 >= caught));
}

}  // namespace pr
}  // namespace madrl
