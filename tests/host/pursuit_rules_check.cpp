// pursuit_rules_check.cpp -- the device side's one statement of the PursuitEvade rules (madrl_amd/csrc/pursuit_rules.hpp) against the
// oracle's independent one (oracle/pursuit_oracle.c, linked in; it does not include the header) on a CPU.
// tests/test_pursuit_rules_cpu.py compiles both with -fsanitize=address,undefined and runs this.
//
// For 64 envs (env_id_base 500, a 64-bit seed with both halves non-zero) the oracle creates and resets a batch; every env's map id, evader
// count and every agent's position are recomputed from the header alone -- the occupancy test on the host map -- and must be equal:
//   a  16 x 16, 8 v 30, three maps with a 6 x 6 building block each at a different place, sample_maps, constraint_window 0.5, max_opponents 10
//   b  the same with 8 v 4: min(n_create, E) clamps
//   c  5 x 10, 16 v 7, constraint_window 1.0, no random opponents: a non-square map, window = map
//   d  a for live counts: the rules at capacity 8 v 30 with live (5, 12) against the oracle of a fixed 5 v 12 batch (live_agent_index)
//   e  a second reset of a's handle: the ticks differ per call
// The program checks that its inputs exercise the rules (a: a rejected draw, two map ids, two windows; b: the clamp binds in one env and
// not in another) and pursuer_reward / done_bits on hand-written values.  Exit status 1 and a line on stderr per failure.
#include <stdint.h>
#include <stdio.h>

#include <set>
#include <tuple>
#include <vector>

#include "../../madrl_amd/csrc/pursuit_rules.hpp"

extern "C" {
struct po_config {   // as oracle/pursuit_oracle.c declares it
    int32_t xs, ys, n_pursuers, n_evaders, obs_range, n_catch, surround, flatten, include_id, reward_global, sample_maps, n_maps, max_opponents,
        train_pursuit;
    double catchr, term_pursuit, urgency_reward, layer_norm, constraint_window;
};
struct po_handle;
int po_obs_dim_of(const po_config *c);
po_handle *po_create(const po_config *cfg, const int8_t *maps, int64_t n_envs, uint64_t seed, int64_t env_id_base);
void po_destroy(po_handle *h);
void po_reset(po_handle *h, const uint8_t *mask, const int32_t *inj_pos, const int32_t *inj_map, float *obs);
void po_get_state(const po_handle *h, int32_t *pos_p, int32_t *pos_e, uint8_t *gone, uint8_t *term_p, uint8_t *term_e, int32_t *map_id,
                  uint32_t *tick);
}

namespace {

using namespace madrl;

constexpr int64_t N = 64, ID_BASE = 500;
constexpr uint64_t SEED = 0x5EED0123C0FFEE42ull;
static_assert((uint32_t)SEED != 0u && (uint32_t)(SEED >> 32) != 0u, "both halves of the seed");

int failures = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond) && ++failures <= 20) {                       \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, "\n");                               \
        }                                                        \
    } while (0)

struct Seen {   // what a configuration's envs went through
    int rejected = 0, clamped = 0, below_cap = 0;
    std::set<int> maps;
    std::set<std::tuple<int, int, int, int>> windows;
};

struct Oracle {
    po_config c;
    po_handle *h;
    std::vector<float> obs;
    std::vector<int32_t> pos_p, pos_e, map_id;
    std::vector<uint8_t> gone, term_p, term_e;
    std::vector<uint32_t> tick;
    Oracle(const po_config &cfg, const std::vector<int8_t> &maps) : c(cfg), h(po_create(&c, maps.data(), N, SEED, ID_BASE)) {
        const size_t P = (size_t)c.n_pursuers, E = (size_t)c.n_evaders;
        obs.resize(N * P * (size_t)po_obs_dim_of(&c));
        pos_p.resize(N * P * 2); pos_e.resize(N * E * 2); map_id.resize(N);
        gone.resize(N * E); term_p.resize(N * P); term_e.resize(N * E); tick.resize(N);
    }
    ~Oracle() { po_destroy(h); }
    void reset() {
        po_reset(h, nullptr, nullptr, nullptr, obs.data());
        po_get_state(h, pos_p.data(), pos_e.data(), gone.data(), term_p.data(), term_e.data(), map_id.data(), tick.data());
    }
};

// one reset of every env from the header alone, at capacity (P, E) with live counts (np, ne), against the oracle `o` of an (np, ne) batch;
// `tick`: the oracle's tick before this reset
Seen check_reset(const char *name, const Oracle &o, const std::vector<int8_t> &maps, int P, int E, int np_pending, int ne_pending, uint32_t tick) {
    Seen seen;
    const po_config &c = o.c;
    const uint32_t k0 = (uint32_t)SEED, k1 = (uint32_t)(SEED >> 32);
    const pr::Counts live = pr::clamp_pending(np_pending, ne_pending, P, E);
    CHECK(live.np == c.n_pursuers && live.ne == c.n_evaders, "%s: live counts (%d, %d)", name, live.np, live.ne);
    for (int64_t n = 0; n < N; ++n) {
        const uint32_t gid = (uint32_t)(ID_BASE + n);
        const int map_id = c.sample_maps ? pr::reset_map_id(gid, tick, k0, k1, c.n_maps) : 0;
        const pr::Window w = pr::reset_window(gid, tick, k0, k1, c.constraint_window, c.xs, c.ys);
        int n_create = live.ne;
        if (c.max_opponents > 0) {
            n_create = pr::reset_n_create(gid, tick, k0, k1, c.max_opponents, live.ne);
            const int unclamped = pr::reset_n_create(gid, tick, k0, k1, c.max_opponents, 1 << 30);
            seen.clamped += unclamped > live.ne && n_create == live.ne;
            seen.below_cap += n_create < live.ne;
        }
        seen.maps.insert(map_id);
        seen.windows.insert(std::make_tuple(w.xlb, w.xub, w.ylb, w.yub));
        CHECK(map_id == o.map_id[n], "%s env %d: map %d, oracle %d", name, (int)n, map_id, o.map_id[n]);
        CHECK(o.tick[n] == tick + 1u, "%s env %d: oracle tick %u", name, (int)n, o.tick[n]);
        const int8_t *map = maps.data() + (size_t)map_id * c.xs * c.ys;
        int created = 0;
        for (int a = 0; a < live.np + live.ne; ++a) {
            const bool is_p = a < live.np;
            const int slot = is_p ? a : a - live.np;
            const int32_t *want = is_p ? &o.pos_p[(n * live.np + slot) * 2] : &o.pos_e[(n * live.ne + slot) * 2];
            if (!is_p && slot >= n_create) {   // not created: gone, reported at (-1, -1)
                CHECK(o.gone[n * live.ne + slot] == 1 && want[0] == -1 && want[1] == -1, "%s env %d evader %d: created by the oracle", name, (int)n, slot);
                continue;
            }
            created += !is_p;
            pr::Cell cell{0, 0};
            for (uint32_t att = 0; att < 1024u; ++att) {
                cell = pr::reset_cell(gid, tick, pr::live_agent_index(is_p ? slot : P + slot, P, live.np), att, k0, k1, w);
                if (cell.x < w.xlb || cell.x >= w.xub || cell.y < w.ylb || cell.y >= w.yub || w.xlb < 0 || w.xub > c.xs || w.ylb < 0 || w.yub > c.ys) {
                    CHECK(false, "%s env %d agent %d: (%d, %d) outside its window", name, (int)n, a, cell.x, cell.y);
                    return seen;
                }
                if (map[cell.x * c.ys + cell.y] != -1) break;
                seen.rejected += 1;
            }
            CHECK(cell.x == want[0] && cell.y == want[1], "%s env %d agent %d: (%d, %d), oracle (%d, %d)", name, (int)n, a, cell.x, cell.y, want[0], want[1]);
            if (!is_p) CHECK(o.gone[n * live.ne + slot] == 0, "%s env %d evader %d: gone in the oracle", name, (int)n, slot);
        }
        CHECK(created == n_create, "%s env %d: %d evaders created, n_create %d", name, (int)n, created, n_create);
    }
    return seen;
}

po_config config(int xs, int ys, int P, int E, int n_maps, double cw, int max_opponents) {
    po_config c{};
    c.xs = xs; c.ys = ys; c.n_pursuers = P; c.n_evaders = E;
    c.obs_range = 7; c.n_catch = 2; c.surround = 1; c.flatten = 1; c.include_id = 1; c.reward_global = 0;
    c.sample_maps = n_maps > 1; c.n_maps = n_maps; c.max_opponents = max_opponents; c.train_pursuit = 1;
    c.catchr = 0.01; c.term_pursuit = 5.0; c.urgency_reward = -0.1; c.layer_norm = 10.0; c.constraint_window = cw;
    return c;
}

// n_maps maps of xs x ys (0 free, -1 building), a bw x bw building block in each at its own place
std::vector<int8_t> block_maps(int xs, int ys, int n_maps, int bw, const int (*at)[2]) {
    std::vector<int8_t> m((size_t)n_maps * xs * ys, 0);
    for (int k = 0; k < n_maps; ++k)
        for (int i = 0; i < bw; ++i)
            for (int j = 0; j < bw; ++j) m[((size_t)k * xs + at[k][0] + i) * ys + at[k][1] + j] = -1;
    return m;
}

void check_step_rules() {
    struct { double catchr; int kpre; double term; bool sur; double urgency; } v[] = {
        {0.01, 3, 5.0, false, -0.1}, {0.01, 3, 5.0, true, -0.1}, {0.01, 0, 5.0, false, -0.1}, {0.01, 255, 5.0, true, 0.0},
        {0.1, 7, 1.0 / 3.0, true, -0.1}, {0.0, 3, 5.0, true, -0.1}};
    for (const auto &t : v) {
        volatile double r = t.catchr * (double)t.kpre;   // the reference's three float64 statements
        r = r + t.term * (t.sur ? 1.0 : 0.0);
        r = r + t.urgency;
        const double got = pr::pursuer_reward(t.catchr, t.kpre, t.term, t.sur, t.urgency);
        CHECK(got == r, "pursuer_reward(%g, %d, %g, %d, %g) = %.17g, want %.17g", t.catchr, t.kpre, t.term, (int)t.sur, t.urgency, got, (double)r);
    }
    CHECK(pr::done_bits(false, 0, 1000) == 0u, "done_bits: no time limit");
    CHECK(pr::done_bits(true, 0, 1) == 1u, "done_bits: all gone");
    CHECK(pr::done_bits(false, 7, 6) == 0u, "done_bits: below the limit");
    CHECK(pr::done_bits(false, 7, 7) == 2u, "done_bits: at the limit");
    CHECK(pr::done_bits(true, 7, 8) == 3u, "done_bits: both");
    CHECK(pr::done_bits(true, -1, 8) == 1u, "done_bits: a negative limit is none");
}

}  // namespace

int main() {
    static const int at3[3][2] = {{2, 3}, {8, 1}, {5, 9}};
    const std::vector<int8_t> maps3 = block_maps(16, 16, 3, 6, at3);
    {
        Oracle a(config(16, 16, 8, 30, 3, 0.5, 10), maps3);
        a.reset();
        const Seen s = check_reset("a", a, maps3, 8, 30, 8, 30, 0u);
        CHECK(s.rejected >= 1, "a: no position needed a second attempt");
        CHECK(s.maps.size() >= 2, "a: %d distinct map ids", (int)s.maps.size());
        CHECK(s.windows.size() >= 2, "a: %d distinct windows", (int)s.windows.size());
        printf("a rejected=%d maps=%d windows=%d\n", s.rejected, (int)s.maps.size(), (int)s.windows.size());
        a.reset();   // e: the same handle again
        const Seen e = check_reset("e", a, maps3, 8, 30, 8, 30, 1u);
        printf("e rejected=%d maps=%d windows=%d\n", e.rejected, (int)e.maps.size(), (int)e.windows.size());
    }
    {
        Oracle b(config(16, 16, 8, 4, 3, 0.5, 10), maps3);
        b.reset();
        const Seen s = check_reset("b", b, maps3, 8, 4, 8, 4, 0u);
        CHECK(s.clamped >= 1, "b: the clamp never binds");
        CHECK(s.below_cap >= 1, "b: no env with n_create < E");
        printf("b clamped=%d below=%d\n", s.clamped, s.below_cap);
    }
    {
        static const int at1[1][2] = {{1, 4}};
        const std::vector<int8_t> maps1 = block_maps(5, 10, 1, 2, at1);
        Oracle c(config(5, 10, 16, 7, 1, 1.0, 0), maps1);
        c.reset();
        const Seen s = check_reset("c", c, maps1, 16, 7, 16, 7, 0u);
        CHECK(s.windows.size() == 1 && *s.windows.begin() == std::make_tuple(0, 5, 0, 10), "c: the window is not the map");
        printf("c rejected=%d\n", s.rejected);
    }
    {
        Oracle d(config(16, 16, 5, 12, 3, 0.5, 10), maps3);   // the fixed 5 v 12 batch; the rules run at capacity 8 v 30, live (5, 12)
        d.reset();
        const Seen s = check_reset("d", d, maps3, 8, 30, 5, 12, 0u);
        printf("d rejected=%d clamped=%d\n", s.rejected, s.clamped);
        const pr::Counts lo = pr::clamp_pending(0, -3, 8, 30), hi = pr::clamp_pending(99, 99, 8, 30);
        CHECK(lo.np == 1 && lo.ne == 0 && hi.np == 8 && hi.ne == 30, "clamp_pending at its bounds");
        CHECK(pr::live_agent_index(4, 8, 5) == 4u && pr::live_agent_index(8, 8, 5) == 5u && pr::live_agent_index(19, 8, 5) == 16u, "live_agent_index");
    }
    check_step_rules();
    if (failures) fprintf(stderr, "%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
