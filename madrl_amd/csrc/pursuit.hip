// pursuit.hip -- batched PursuitEvade for MI355X (gfx950 / CDNA4).
//
// One workgroup owns one env instance at a time (workgroups stride over envs).  All of an
// env's mutable state -- agent positions, alive/terminal bitmasks, the three observation
// layers (map / pursuer counts / evader counts) as PADDED byte grids -- is staged in LDS;
// HBM sees exactly one packed state record in, one record out, the action row in, and the
// observation / reward / done rows out.  There is no dense contraction anywhere: this kernel
// is HBM-write bound (the observation row is 94 % of the bytes), so the design
// goals are (1) fully coalesced observation stores, (2) few instructions per stored dword,
// (3) enough resident waves (64-thread workgroups, <4 KB LDS) to cover store latency.
//
// Reference semantics (file:line under /root/reference/madrl_environments/pursuit):
//   step order ............... pursuit_evade.py:209-262      (A.1 in SURVEY.md)
//   pre-move proximity reward  pursuit_evade.py:359-381
//   agent motion ............. utils/DiscreteAgent.py:69-97
//   catch resolution ......... pursuit_evade.py:463-521, need_to_surround :523-540
//   observations ............. pursuit_evade.py:418-461 (stale out-of-map cells kept: the
//                              obs buffer is IN/OUT and those cells are simply not stored)
//   reset .................... pursuit_evade.py:173-207, utils/agent_utils.py:12-47
//
// Host side: the configuration's layout(), PursuitDev and the host-built tables (both formats, and the rules that make a configuration
// eligible for its fast line) are pure functions in pursuit_tables.hpp; this file holds the handle, the dispatch tables and the one launch().
#include "common.hpp"
#include "pursuit_tables.hpp"
#include "pursuit_wave.hpp"
#include "pursuit_group.hpp"
#include "pursuit_crowd.hpp"

#include <memory>
#include <new>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

namespace {

using namespace madrl;

enum { OBS_F32 = 0, OBS_F16 = 1 };   // the element format of an observation buffer (launch(), madrl_pursuit::zmask_fmt)
constexpr int MAX_CELL_COUNT = 253;  // byte grids: the agents of one layer on ONE cell must stay < PAD_MAP (checked where they are counted)
constexpr int NOT_HERE = 0xFF;       // position byte of a slot that does not exist (per-env agent counts; no coordinate is 255)
constexpr int MAX_COUNT = 1023;      // agents per layer.  The authors' largest launch line runs 100 pursuers / 300 evaders
                                     // (runners/old/rllab/pursuit_cnn.sh:1); more than 253 of one kind on one cell raises the overflow bit

struct PursuitIO {
    const uint8_t *mask;       // reset mode
    const int32_t *inj_pos;    // reset mode
    const int32_t *inj_map;    // reset mode
    const int32_t *actions;    // step mode
    const int32_t *inj_eact;   // step mode
    float *obs;
    float *rew;
    uint8_t *done;
    int32_t *removed;
};

static_assert(SENT == pw::SENT, "pursuit_tables.hpp builds the count template the wave / group kernels read");

// `ovf`: set when the cell already held MAX_CELL_COUNT agents -- its count leaves the byte's usable range (254 / 255 are the padding
// sentinels, one more would carry into the neighbouring cell).  The env's results are void from there on: sticky word 3 of its
// record, reported as bit 7 of the done byte (BatchedPursuitEvade raises for it); a new episode clears it.
__device__ __forceinline__ void lds_byte_add(uint8_t *grid, int idx, uint32_t *ovf) {
    const unsigned sh = 8u * (unsigned)(idx & 3);
    const unsigned old = atomicAdd(reinterpret_cast<unsigned *>(grid + (idx & ~3)), 1u << sh);
    if (((old >> sh) & 0xFFu) >= (unsigned)MAX_CELL_COUNT) *ovf = 1u;
}
__device__ __forceinline__ void lds_byte_sub(uint8_t *grid, int idx) {
    atomicSub(reinterpret_cast<unsigned *>(grid + (idx & ~3)), 1u << (8 * (idx & 3)));
}

// numpy float64 add.reduce order (pairwise, 8-way unrolled base case), used by
// `rewards.mean()` at pursuit_evade.py:261.  Base case: 8 <= n <= 128 (or n < 8).
__device__ __forceinline__ double np_pairwise_base(const double *a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}
// numpy's recursive split above 128 elements (pairwise_sum in numpy/core/src/umath/loops_utils.h).  The halves are uneven (n2 = n / 2 rounded
// down to a multiple of 8, the rest goes right): 1 023 -> 504 + 519 -> ... 263 -> 128 + 135, and 135 splits once more -- four levels for
// n <= 1 024 (three left the 49 counts 969 .. 1 023 with a flat sum over more than 128 elements at the bottom: another order of additions)
template <int DEPTH>
__device__ __forceinline__ double np_pairwise_sum_t(const double *a, int n) {
    if (n <= 128) return np_pairwise_base(a, n);
    if constexpr (DEPTH == 0) return np_pairwise_base(a, n);   // (not reached: MAX_COUNT <= 1024, tests/test_advice_regressions.py)
    else {
        int n2 = n / 2;
        n2 -= n2 % 8;
        return np_pairwise_sum_t<DEPTH - 1>(a, n2) + np_pairwise_sum_t<DEPTH - 1>(a + n2, n - n2);
    }
}
__device__ __forceinline__ double np_pairwise_sum(const double *a, int n) { return np_pairwise_sum_t<4>(a, n); }
static_assert(MAX_COUNT <= 1024, "np_pairwise_sum: four levels of numpy's split");

// mode 0: reset(mask)   mode 1: step (+ fused auto-reset)
// LIVE (pursuit_live_kernel) = per-env agent counts (madrl_pursuit_set_agent_counts): d.P / d.E are a capacity, the env's live
// (np, ne) are its leading slots whose position byte is not NOT_HERE; a reset takes them from pending [n_envs][2].  Pursuers >= np
// do not move, are not counted and get no observation row and a 0 reward; evader slots >= ne are gone; draws number the agents in
// the live layout (evader i = agent np + i), as a fixed (np, ne) batch does.
template <int NT>
__global__ void pursuit_kernel(const PursuitDev d, const PursuitIO io, const int mode) {
    constexpr bool LIVE = false;
    constexpr bool TO = false;
    constexpr bool H16 = false;
    const int32_t *const pending = nullptr;
    [[maybe_unused]] const float *const obs_prev = nullptr;
#include "pursuit_generic.inc"
}

template <int NT>
__global__ void pursuit_live_kernel(const PursuitDev d, const PursuitIO io, const int mode, const int32_t *pending) {
    constexpr bool LIVE = true;
    constexpr bool TO = false;
    constexpr bool H16 = false;
    [[maybe_unused]] const float *const obs_prev = nullptr;
#include "pursuit_generic.inc"
}

// The two-buffer step (madrl_pursuit_step_to) of every handle that has no two-buffer fast kernel: the step's rows go to io.obs, and what
// an in-place step leaves alone comes from obs_prev (write_obs in the body).
template <int NT, bool LIVE_>
__global__ void pursuit_to_kernel(const PursuitDev d, const PursuitIO io, [[maybe_unused]] const int32_t *pending, const float *const obs_prev) {
    constexpr bool LIVE = LIVE_;
    constexpr bool TO = true;
    constexpr bool H16 = false;
    const int mode = 1;
#include "pursuit_generic.inc"
}

// The same over binary16 observation buffers (madrl_pursuit_step_to_f16): io.obs and obs_prev16 point at 2-byte elements (io.obs is the
// half pointer, cast: PursuitIO does not grow), every shape and mode -- evader control and the handles whose fast kernel has no half form.
template <int NT, bool LIVE_>
__global__ void pursuit_to_f16_kernel(const PursuitDev d, const PursuitIO io, [[maybe_unused]] const int32_t *pending, const uint16_t *const obs_prev16) {
    constexpr bool LIVE = LIVE_;
    constexpr bool TO = true;
    constexpr bool H16 = true;
    const int mode = 1;
    const float *const obs_prev = reinterpret_cast<const float *>(obs_prev16);   // (write_obs reads it as the 2-byte elements it holds)
#include "pursuit_generic.inc"
}

// ------------------------------------------------------------------ state (un)packing
__global__ void pursuit_get_state_kernel(const PursuitDev d, int32_t *pos_p, int32_t *pos_e, uint8_t *gone,
                                         uint8_t *term_p, uint8_t *term_e, int32_t *map_id, uint32_t *tick,
                                         int32_t *t) {
    const int64_t env = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (env >= d.n_envs) return;
    const uint8_t *rec = d.state + env * (int64_t)d.rec_bytes;
    const uint32_t *h = reinterpret_cast<const uint32_t *>(rec);
    const uint8_t *xy = rec + HDR_BYTES;
    const uint32_t *gw = reinterpret_cast<const uint32_t *>(rec + d.off_gone);
    const uint32_t *tw = reinterpret_cast<const uint32_t *>(rec + d.off_term);
    if (tick) tick[env] = h[0];
    if (t) t[env] = (int32_t)h[1];
    if (map_id) map_id[env] = (int32_t)h[2];
    for (int p = 0; p < d.P; ++p) {
        if (pos_p) {
            pos_p[(env * d.P + p) * 2] = xy[2 * p];
            pos_p[(env * d.P + p) * 2 + 1] = xy[2 * p + 1];
        }
        if (term_p) term_p[env * d.P + p] = (tw[p >> 5] >> (p & 31)) & 1u;
    }
    for (int i = 0; i < d.E; ++i) {
        const uint32_t g = (gw[i >> 5] >> (i & 31)) & 1u;
        const int a = d.P + i;
        if (gone) gone[env * d.E + i] = (uint8_t)g;
        if (pos_e) {
            pos_e[(env * d.E + i) * 2] = g ? -1 : (int32_t)xy[2 * a];
            pos_e[(env * d.E + i) * 2 + 1] = g ? -1 : (int32_t)xy[2 * a + 1];
        }
        if (term_e) term_e[env * d.E + i] = g ? 0 : (uint8_t)((tw[a >> 5] >> (a & 31)) & 1u);
    }
}

__global__ void pursuit_set_state_kernel(const PursuitDev d, const int32_t *pos_p, const int32_t *pos_e,
                                         const uint8_t *gone, const uint8_t *term_p, const uint8_t *term_e,
                                         const int32_t *map_id, const uint32_t *tick, const int32_t *t) {
    const int64_t env = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (env >= d.n_envs) return;
    uint8_t *rec = d.state + env * (int64_t)d.rec_bytes;
    uint32_t *h = reinterpret_cast<uint32_t *>(rec);
    uint8_t *xy = rec + HDR_BYTES;
    uint32_t *gw = reinterpret_cast<uint32_t *>(rec + d.off_gone);
    uint32_t *tw = reinterpret_cast<uint32_t *>(rec + d.off_term);
    if (tick) h[0] = tick[env];
    if (t) h[1] = (uint32_t)t[env];
    if (map_id) h[2] = (uint32_t)map_id[env];
    for (int p = 0; p < d.P; ++p) {
        if (pos_p) {
            xy[2 * p] = (uint8_t)pos_p[(env * d.P + p) * 2];
            xy[2 * p + 1] = (uint8_t)pos_p[(env * d.P + p) * 2 + 1];
        }
        if (term_p) {
            if (term_p[env * d.P + p]) tw[p >> 5] |= 1u << (p & 31);
            else tw[p >> 5] &= ~(1u << (p & 31));
        }
    }
    for (int i = 0; i < d.E; ++i) {
        const int a = d.P + i;
        bool g = (gw[i >> 5] >> (i & 31)) & 1u;
        if (gone) {
            g = gone[env * d.E + i] != 0;
            if (g) gw[i >> 5] |= 1u << (i & 31);
            else gw[i >> 5] &= ~(1u << (i & 31));
        }
        if (pos_e && !g) {
            xy[2 * a] = (uint8_t)pos_e[(env * d.E + i) * 2];
            xy[2 * a + 1] = (uint8_t)pos_e[(env * d.E + i) * 2 + 1];
        }
        if (term_e) {
            if (term_e[env * d.E + i] && !g) tw[a >> 5] |= 1u << (a & 31);
            else tw[a >> 5] &= ~(1u << (a & 31));
        }
    }
}

// Per-env agent counts in the records (madrl_pursuit_get_live_counts / set_live_counts, madrl_pursuit_get_state).  in != nullptr: env n gets
// live counts (in[n][0], in[n][1]) -- slots past them do not exist (NOT_HERE, evaders gone), a slot that exists again is at (0, 0) and,
// for an evader, gone (not created) until the next reset.  out: the live counts; pos_p: pursuers that do not exist read (-1, -1).
__global__ void pursuit_live_counts_kernel(const PursuitDev d, int32_t *pos_p, int32_t *out, const int32_t *in) {
    const int64_t env = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (env >= d.n_envs) return;
    uint8_t *rec = d.state + env * (int64_t)d.rec_bytes;
    uint8_t *xy = rec + HDR_BYTES;
    uint32_t *gw = reinterpret_cast<uint32_t *>(rec + d.off_gone);
    uint32_t *tw = reinterpret_cast<uint32_t *>(rec + d.off_term);
    if (in) {
        const int np = min(max(in[2 * env], 1), d.P), ne = min(max(in[2 * env + 1], 0), d.E);
        for (int a = 0; a < d.A; ++a) {
            const bool is_p = a < d.P;
            const int i = a - d.P;
            if (is_p ? a >= np : i >= ne) {
                xy[2 * a] = xy[2 * a + 1] = (uint8_t)NOT_HERE;
                tw[a >> 5] &= ~(1u << (a & 31));
                if (!is_p) gw[i >> 5] |= 1u << (i & 31);
            } else if (xy[2 * a] == NOT_HERE) {
                xy[2 * a] = xy[2 * a + 1] = 0;
                if (!is_p) gw[i >> 5] |= 1u << (i & 31);
            }
        }
    }
    int np = 0, ne = 0;
    while (np < d.P && xy[2 * np] != NOT_HERE) ++np;
    while (ne < d.E && xy[2 * (d.P + ne)] != NOT_HERE) ++ne;
    if (out) {
        out[2 * env] = np;
        out[2 * env + 1] = ne;
    }
    if (pos_p)
        for (int p = 0; p < d.P; ++p)
            if (xy[2 * p] == NOT_HERE) pos_p[(env * d.P + p) * 2] = pos_p[(env * d.P + p) * 2 + 1] = -1;
}

}  // namespace

// =================================================================== host side / C ABI
namespace {
struct Line;  // one line of the specialisation lists with every kernel compiled for it (below)
}

struct madrl_pursuit {
    madrl_pursuit_config cfg{};
    PursuitDev dev{};
    int device = 0;
    int threads = 0;
    int nt = 0;
    int64_t max_blocks = 0;
    size_t lds_bytes = 0;
    void *tables = nullptr;  // one device allocation holding maps | cnt_tmpl | vtab | codes
    // the fast path: the line of this shape (find_line), when there is one and the configuration is eligible for it -- one wavefront per
    // env or a group of them (pursuit_wave.hpp, pursuit_group.hpp: wdev, wtables) or the crowd kernel (pursuit_crowd.hpp: cdev; it shares
    // the generic kernel's tables).  Which of the line's kernels a launch runs: runs_fast() and takes_fixed() below
    const Line *line = nullptr;
    bool fixed_on = false;   // the line's fixed-constants step kernel is not switched off (MADRL_PURSUIT_FIXED=0 at create)
    int last_step_entry = MADRL_STEP_ENTRY_NONE;   // which kernel the last step launch ran on (madrl_pursuit_last_step_entry)
    madrl::pw::WaveDev wdev{};
    madrl::pc::CrowdDev cdev{};
    void *zmask = nullptr;          // what the fast path remembers about the observation buffer (zmask_len): the stale-zero masks,
                                    // [n_envs][64 * waves] dwords per mask word (pursuit_wave.hpp), or the crowd kernel's one word per env,
                                    // "channel 3 of the env's rows is not known to hold +0.0".  The tail of the caller's state buffer
                                    // (madrl_pursuit_state_bytes), not a library allocation
    const void *zmask_obs = nullptr; // the observation buffer the masks describe; another buffer, a generic-kernel launch,
                                    // set_state or madrl_pursuit_invalidate_obs resets them to "nothing known"
    int zmask_fmt = OBS_F32;   // ... and the element format it was read in: the same address in the other format is an unknown buffer
    uint64_t step_count = 0;  // step launches so far (parity of the walk direction, see launch())
    int walk_mode = 0;        // 0 auto (alternate above ~375 MB per launch), 1 always alternate, 2 always forward; fixed at create
    void *wtables = nullptr;  // the wave / group kernels' device allocation (build_wave_tables)
    int kernel_kind = MADRL_KERNEL_AUTO;  // MADRL_KERNEL_AUTO / _GENERIC / _WAVE (requested)
    const int32_t *pending = nullptr;      // per-env agent counts (madrl_pursuit_set_agent_counts): caller-owned int32 [n_envs][2], or off
    hipEvent_t ev_fork = nullptr, ev_done = nullptr;   // madrl_pursuit_step_sharded: made by madrl_pursuit_create on the handle's device, destroyed with the handle

    madrl_pursuit() = default;
    madrl_pursuit(const madrl_pursuit &) = delete;
    madrl_pursuit &operator=(const madrl_pursuit &) = delete;
    ~madrl_pursuit() {   // the one place that frees: madrl_pursuit_destroy, and every error path of madrl_pursuit_create
        if (tables) (void)hipFree(tables);
        if (wtables) (void)hipFree(wtables);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_done) (void)hipEventDestroy(ev_done);
    }
};

namespace {

// ------------------------------------------------------------------ fast-path dispatch (DESIGN.md §4.3 "Host dispatch")
struct ShapeKey {
    int xs, ys, P, E, R, flatten;
    constexpr bool operator==(const ShapeKey &o) const {
        return xs == o.xs && ys == o.ys && P == o.P && E == o.E && R == o.R && flatten == o.flatten;
    }
};
ShapeKey key_of(const madrl_pursuit_config *c) { return {c->xs, c->ys, c->n_pursuers, c->n_evaders, c->obs_range, c->flatten ? 1 : 0}; }

using WaveLaunch = void (*)(const pw::WaveDev &, const pw::WaveIO &, int mode, int64_t blocks, hipStream_t s);
using CrowdLaunch = void (*)(const pc::CrowdDev &, const pc::CrowdIO &, const int32_t *pending, int mode, int64_t blocks, hipStream_t s);
using WaveFixedLaunch = void (*)(const pw::WaveDev &, const pw::WaveIO &, int64_t blocks, hipStream_t s);
using WaveToLaunch = void (*)(const pw::WaveDev &, const pw::WaveIO &, int64_t blocks, hipStream_t s);
using CrowdToLaunch = void (*)(const pc::CrowdDev &, const pc::CrowdIO &, const int32_t *pending, const float *obs_prev, int64_t blocks, hipStream_t s);

// The kernels of one line in one count mode, by role; nullptr: no list gives the line that role.  A wave / group line has wave
// launchers, a crowd line crowd ones (and no half form).
struct Kernels {
    WaveLaunch wave;            // in place: reset and step (mode)
    CrowdLaunch crowd;
    WaveToLaunch wave_to;       // two buffers (madrl_pursuit_step_to)
    CrowdToLaunch crowd_to;
    WaveToLaunch wave_to_f16;   // two buffers of binary16 elements (madrl_pursuit_step_to_f16)
    constexpr bool has(bool two_buffer, int fmt) const {
        return !two_buffer ? (wave || crowd) : fmt == OBS_F16 ? wave_to_f16 != nullptr : (wave_to || crowd_to);
    }
};

// One X / XG / XC line of pursuit_specializations.def / pursuit_crowd_specializations.def with what the other four lists compile for it.
struct Line {
    ShapeKey key;
    bool crowd;      // the family: the crowd kernel, or one wavefront / a group of them per env
    WaveGeom g;      // the compiled geometry (pursuit_tables.hpp).  g.nw, wavefronts per env: 1 = pursuit_wave_kernel, > 1 = pursuit_group_kernel; the
                     // crowd kernel's workgroup.  g.mwords: 1 = one bit per float4 slot in each byte, up to 8 slots per lane; the row-loop kernel: NS / 8
    int mask_bytes;  // per env, of `zmask`
    int resident;    // workgroups of one launch: exactly the resident capacity of the 256 CUs
    Kernels k[2];    // [0] the configuration's counts, [1] per-env agent counts (madrl_pursuit_set_agent_counts)
    WaveFixedLaunch fixed;   // the step with its launch constants folded in (pw::FShape), taken launch by launch: takes_fixed()
};

template <class S>
void wave_launch(const pw::WaveDev &d, const pw::WaveIO &io, int mode, int64_t blocks, hipStream_t s) {
    if constexpr (S::E >= S::P && !S::LIVE) {
        if (io.control_evaders) {   // train_pursuit=False: the evader-control instantiations (reset, flexible step)
            if (mode == 0) hipLaunchKernelGGL((pw::pursuit_wave_kernel<S, 0, false, true>), dim3((unsigned)blocks), dim3(64), 0, s, d, io);
            else hipLaunchKernelGGL((pw::pursuit_wave_kernel<S, 1, true, true>), dim3((unsigned)blocks), dim3(64), 0, s, d, io);
            return;
        }
    }
    if (mode == 0)
        hipLaunchKernelGGL((pw::pursuit_wave_kernel<S, 0, false>), dim3((unsigned)blocks), dim3(64), 0, s, d, io);
    else if (io.flex)
        hipLaunchKernelGGL((pw::pursuit_wave_kernel<S, 1, true>), dim3((unsigned)blocks), dim3(64), 0, s, d, io);
    else
        hipLaunchKernelGGL((pw::pursuit_wave_kernel<S, 1, false>), dim3((unsigned)blocks), dim3(64), 0, s, d, io);
}

template <class S>
void group_launch(const pw::WaveDev &d, const pw::WaveIO &io, int mode, int64_t blocks, hipStream_t s) {
    if (mode == 0)
        hipLaunchKernelGGL((pw::pursuit_group_kernel<S, 0, false>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
    else if (io.flex)
        hipLaunchKernelGGL((pw::pursuit_group_kernel<S, 1, true>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
    else
        hipLaunchKernelGGL((pw::pursuit_group_kernel<S, 1, false>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
}

// resident: 4 SIMDs of S::OCC wavefronts (the occupancy the kernel's registers are allocated for) on each CU
template <class S, int NW>
constexpr Line wave_entry(WaveLaunch launch) {
    constexpr WaveGeom g{NW, S::GSZ, S::GW, S::PAD, S::X_ID, S::X_SKIP, S::MWORDS, S::D, S::REC_BYTES, S::OFF_GONE, S::OFF_TERM};
    static_assert(g == wave_geom(S::XS, S::YS, S::P, S::E, S::R, S::FLATTEN, NW), "wave_geom() of pursuit_tables.hpp is not this kernel's geometry");
    return Line{{S::XS, S::YS, S::P, S::E, S::R, S::FLATTEN}, false, g, 256 * NW * S::MWORDS, 256 * 4 * S::OCC / NW, {{launch}}, nullptr};
}

// resident: what the LDS of a workgroup and 24 wavefronts per CU allow (at most 85 registers per lane; a 16-wavefront workgroup may use
// 128 and is alone on its CU anyway)
template <class S>
constexpr Line crowd_entry(CrowdLaunch launch) {
    constexpr int by_lds = 160 * 1024 / (S::LDS_DWORDS * 4), by_waves = 24 / S::NW > 0 ? 24 / S::NW : 1;
    return Line{{S::XS, S::YS, S::P, S::E, S::R, S::FLATTEN}, true, WaveGeom{S::NW, S::GSZ, 0, 0, 0, 0, 0, S::D, S::REC_BYTES, S::OFF_GONE, S::OFF_TERM},
                4, 256 * (by_lds < by_waves ? by_lds : by_waves), {{nullptr, launch}}, nullptr};
}

// The lines: the X / XG lines, then the XC lines -- a shape that has an X / XG line keeps the kernel of that line.  The *.local.def lists
// are the lines added on this machine by `python -m madrl_amd.build --pursuit-shape / --pursuit-crowd-shape ...` (git-ignored).
#define X(XS, YS, NP, NE, R, FL) wave_entry<pw::Shape<XS, YS, NP, NE, R, FL>, 1>(wave_launch<pw::Shape<XS, YS, NP, NE, R, FL>>),
#define XG(XS, YS, NP, NE, R, FL, NW) wave_entry<pw::GShape<XS, YS, NP, NE, R, FL, NW>, NW>(group_launch<pw::GShape<XS, YS, NP, NE, R, FL, NW>>),
#define XC(XS, YS, NP, NE, R, FL, NW) crowd_entry<pc::CShape<XS, YS, NP, NE, R, FL, NW>>(pc::crowd_launch<pc::CShape<XS, YS, NP, NE, R, FL, NW>>),
constexpr Line BASE_LINES[] = {
#include "pursuit_specializations.def"
#if __has_include("pursuit_specializations.local.def")
#include "pursuit_specializations.local.def"
#endif
#include "pursuit_crowd_specializations.def"
#if __has_include("pursuit_crowd_specializations.local.def")
#include "pursuit_crowd_specializations.local.def"
#endif
};
#undef X
#undef XG
#undef XC

// The lines with the kernels of the other four lists attached, each to the first line of its key, family and NW.  A line of those lists
// that finds no line to stand on would compile a kernel that no handle can use: its list is noted in `orphans`, which stops the compile.
enum Orphan : unsigned { LIVE_WAVE = 1, LIVE_CROWD = 2, LIVE_GEOMETRY = 4, FIXED_LIST = 8, TO_LIST = 16, TO_F16_GROUP_LIST = 32 };
struct LineTable {
    Line line[sizeof(BASE_LINES) / sizeof(BASE_LINES[0])];
    unsigned orphans;

    constexpr Line *stand(const ShapeKey &key, bool crowd, int nw) {
        for (Line &b : line)
            if (b.key == key && b.crowd == crowd && b.g.nw == nw) return &b;
        return nullptr;
    }
    // the roles of `add` go to count mode `live` of line `b` (the first line of a list that names a role keeps it); no line: an orphan
    constexpr void attach(Line *b, bool live, const Kernels &add, Orphan list) {
        if (!b) { orphans |= list; return; }
        Kernels &k = b->k[live];
        if (!k.wave) k.wave = add.wave;
        if (!k.crowd) k.crowd = add.crowd;
        if (!k.wave_to) k.wave_to = add.wave_to;
        if (!k.crowd_to) k.crowd_to = add.crowd_to;
        if (!k.wave_to_f16) k.wave_to_f16 = add.wave_to_f16;
    }
    // a per-env-count instantiation (wave_entry / crowd_entry of an LShape / LGShape / LCShape): it is launched with the tables, masks and
    // block count of the line it stands on, so its compiled geometry must be that line's
    constexpr void attach_live(const Line &l) {
        Line *b = stand(l.key, l.crowd, l.g.nw);
        if (b && !(b->g == l.g && b->mask_bytes == l.mask_bytes)) orphans |= LIVE_GEOMETRY;
        attach(b, true, l.k[0], l.crowd ? LIVE_CROWD : LIVE_WAVE);
    }
    constexpr void attach_fixed(const ShapeKey &key, WaveFixedLaunch launch) {
        Line *b = stand(key, false, 1);
        if (!b) orphans |= FIXED_LIST;
        else if (!b->fixed) b->fixed = launch;
    }
    // a half line of the multi-wavefront family stands on the XG line of its shape, a live one (HLG) also on its XLG line
    constexpr void attach_half_group(const ShapeKey &key, int nw, bool live, WaveToLaunch launch) {
        Line *b = nw > 1 ? stand(key, false, nw) : nullptr;
        attach(b && (!live || b->k[1].wave) ? b : nullptr, live, Kernels{nullptr, nullptr, nullptr, nullptr, launch}, TO_F16_GROUP_LIST);
    }
};

constexpr LineTable resolve_lines() {
    LineTable t{};
    for (size_t i = 0; i < sizeof(BASE_LINES) / sizeof(BASE_LINES[0]); ++i) t.line[i] = BASE_LINES[i];
    // Per-env agent counts: same geometry, same tables.  (wave_launch of an LShape: no evader-control instantiations,
    // madrl_pursuit_set_agent_counts refuses control_evaders; the XLG and XLC kernels are compiled in pursuit_live_group.hip and
    // pursuit_live_crowd.hip.)  The .local.def list: `python -m madrl_amd.build --pursuit-live-shape / --pursuit-live-crowd-shape ...`,
    // which appends the fixed line too.
#define XL(XS, YS, NP, NE, R, FL) t.attach_live(wave_entry<pw::LShape<XS, YS, NP, NE, R, FL>, 1>(wave_launch<pw::LShape<XS, YS, NP, NE, R, FL>>));
#define XLG(XS, YS, NP, NE, R, FL, NW) t.attach_live(wave_entry<pw::LGShape<XS, YS, NP, NE, R, FL, NW>, NW>(pw::live_group_launch<pw::LGShape<XS, YS, NP, NE, R, FL, NW>>));
#define XLC(XS, YS, NP, NE, R, FL, NW) t.attach_live(crowd_entry<pc::LCShape<XS, YS, NP, NE, R, FL, NW>>(pc::live_crowd_launch<pc::LCShape<XS, YS, NP, NE, R, FL, NW>>));
#include "pursuit_live_specializations.def"
#if __has_include("pursuit_live_specializations.local.def")
#include "pursuit_live_specializations.local.def"
#endif
#undef XL
#undef XLG
#undef XLC
    // The step kernels with their launch constants folded in (pw::FShape, pursuit_fixed.hip), of one-wavefront lines: the masks and the
    // record are the X line's.
#define XF(XS, YS, NP, NE, R, FL) t.attach_fixed({XS, YS, NP, NE, R, FL}, pw::wave_fixed_launch<pw::FShape<XS, YS, NP, NE, R, FL>>);
#include "pursuit_fixed_specializations.def"
#if __has_include("pursuit_fixed_specializations.local.def")
#include "pursuit_fixed_specializations.local.def"
#endif
#undef XF
    // The two-buffer step kernels (pursuit_to.hip, pursuit_to_group.hip); an XL / XLG / XLC line is used by handles whose capacity also
    // has its line in the live list.  The X / XL lines come with their binary16 form (pursuit_to_f16.hip).
#define TO(XS, YS, NP, NE, R, FL, CROWD, NW, LIVE, ...) t.attach(t.stand({XS, YS, NP, NE, R, FL}, CROWD, NW), LIVE, Kernels{nullptr, nullptr, __VA_ARGS__}, TO_LIST);
#define X(XS, YS, NP, NE, R, FL) TO(XS, YS, NP, NE, R, FL, false, 1, false, pw::wave_to_launch<pw::TShape<XS, YS, NP, NE, R, FL>>, nullptr, pw::wave_to_f16_launch<pw::THShape<XS, YS, NP, NE, R, FL>>)
#define XL(XS, YS, NP, NE, R, FL) TO(XS, YS, NP, NE, R, FL, false, 1, true, pw::wave_to_launch<pw::TLShape<XS, YS, NP, NE, R, FL>>, nullptr, pw::wave_to_f16_launch<pw::TLHShape<XS, YS, NP, NE, R, FL>>)
#define XC(XS, YS, NP, NE, R, FL, NW) TO(XS, YS, NP, NE, R, FL, true, NW, false, nullptr, pc::crowd_to_launch<pc::CShape<XS, YS, NP, NE, R, FL, NW>>, nullptr)
#define XLC(XS, YS, NP, NE, R, FL, NW) TO(XS, YS, NP, NE, R, FL, true, NW, true, nullptr, pc::crowd_to_launch<pc::LCShape<XS, YS, NP, NE, R, FL, NW>>, nullptr)
#define XG(XS, YS, NP, NE, R, FL, NW) TO(XS, YS, NP, NE, R, FL, false, NW, false, pw::group_to_launch<pw::TGShape<XS, YS, NP, NE, R, FL, NW>>, nullptr, nullptr)
#define XLG(XS, YS, NP, NE, R, FL, NW) TO(XS, YS, NP, NE, R, FL, false, NW, true, pw::group_to_launch<pw::TLGShape<XS, YS, NP, NE, R, FL, NW>>, nullptr, nullptr)
#include "pursuit_to_specializations.def"
#if __has_include("pursuit_to_specializations.local.def")
#include "pursuit_to_specializations.local.def"
#endif
#undef X
#undef XL
#undef XC
#undef XLC
#undef XG
#undef XLG
#undef TO
    // The half-precision two-buffer step kernels of the multi-wavefront family (pursuit_to_group_f16.hip, pursuit_to_group_f16_live.hip):
    // a list of its own; a half line does not need a float32 two-buffer line.
#define HG(XS, YS, NP, NE, R, FL, NW) t.attach_half_group({XS, YS, NP, NE, R, FL}, NW, false, pw::group_to_f16_launch<pw::THGShape<XS, YS, NP, NE, R, FL, NW>>);
#define HLG(XS, YS, NP, NE, R, FL, NW) t.attach_half_group({XS, YS, NP, NE, R, FL}, NW, true, pw::group_to_f16_launch<pw::TLHGShape<XS, YS, NP, NE, R, FL, NW>>);
#include "pursuit_to_f16_group_specializations.def"
#if __has_include("pursuit_to_f16_group_specializations.local.def")
#include "pursuit_to_f16_group_specializations.local.def"
#endif
#undef HG
#undef HLG
    return t;
}
constexpr LineTable LINES = resolve_lines();
static_assert(!(LINES.orphans & LIVE_WAVE), "an XL / XLG line needs the X / XG line of the same capacity with the same NW");
static_assert(!(LINES.orphans & LIVE_CROWD), "an XLC line needs the XC line of the same capacity with the same NW");
static_assert(!(LINES.orphans & LIVE_GEOMETRY), "an XL / XLG / XLC kernel's compiled geometry or mask bytes are not those of the X / XG / XC line it is launched with");
static_assert(!(LINES.orphans & FIXED_LIST), "an XF line of pursuit_fixed_specializations.def needs the X line of its shape in pursuit_specializations.def");
static_assert(!(LINES.orphans & TO_LIST), "a line of pursuit_to_specializations.def needs the X line (X / XL), the XG line with the same NW (XG / XLG) or the XC line with the same NW (XC / XLC) of its shape");
static_assert(!(LINES.orphans & TO_F16_GROUP_LIST), "a line of pursuit_to_f16_group_specializations.def needs the XG line of its shape with the same NW in pursuit_specializations.def, an HLG line also the XLG line in pursuit_live_specializations.def");

// The line a configuration runs on, by the configuration alone (madrl_pursuit_state_bytes sizes the caller's buffer by it): the first of
// its shape.  A flatten row without the id is not a whole number of float4; evader control has the one-wavefront kernel or the generic one.
// A line that madrl_pursuit_create then finds not eligible leaves the handle on the generic kernel, not on a later line.
const Line *find_line(const madrl_pursuit_config *c) {
    if (c->flatten && !c->include_id) return nullptr;
    const ShapeKey k = key_of(c);
    for (const Line &e : LINES.line) {
        if (c->control_evaders && (e.g.nw > 1 || e.crowd)) continue;
        if (e.key == k) return &e;
    }
    return nullptr;
}

// MADRL_PURSUIT_FIXED=0 in the environment keeps every handle created from then on off the fixed-constants kernels (A/B runs, twin tests)
bool fixed_enabled() {
    const char *v = getenv("MADRL_PURSUIT_FIXED");
    return !(v && v[0] == '0' && v[1] == 0);
}
// What of a launch decides between the two kernels of a line, and the FShape contract (pursuit_wave.hpp) over it and the handle's
// constants: pure, so that madrl_pursuit_fixed_choice answers without a device exactly what launch() does.
struct LaunchAsk {
    bool step;        // mode 1 (resets run on the plain kernel)
    bool two_buffer;  // step_to / step_to_f16
    bool pending;     // per-env agent counts
    bool inj_eact;    // injected evader actions
    bool alternate;   // the walk alternates its direction (set_walk, or automatic above the threshold)
};
bool walk_alternates(const PursuitDev &d, int walk_mode) {
    if (walk_mode != 0) return walk_mode == 1;
    return (double)d.n_envs * (4.0 * d.P * d.D + 2.0 * d.rec_bytes) > 375e6;
}
bool fixed_contract(const PursuitDev &d, const LaunchAsk &a) {
    return a.step && !a.two_buffer && !a.pending && !a.inj_eact && !a.alternate && d.surround && !d.reward_global && d.train_pursuit &&
           d.n_maps == 1 && !d.sample_maps && d.max_opponents == 0 && d.cw_env == nullptr && d.catchr_env == nullptr;
}
// a fast launch on line `l` runs the line's fixed-constants kernel (on: MADRL_PURSUIT_FIXED as read at create)
bool takes_fixed(const Line *l, bool on, const PursuitDev &d, const LaunchAsk &a) { return on && l && l->fixed && fixed_contract(d, a); }

int validate(const madrl_pursuit_config *c) {
    if (!c) return fail(MADRL_EINVAL, "config is NULL");
    if (c->struct_size != (int32_t)sizeof(madrl_pursuit_config))
        return fail(MADRL_EINVAL, "madrl_pursuit_config.struct_size=%d, library expects %d", c->struct_size,
                    (int)sizeof(madrl_pursuit_config));
    if (c->xs < 1 || c->ys < 1 || c->xs > 255 || c->ys > 255)
        return fail(MADRL_EINVAL, "map size %dx%d unsupported (1..255)", c->xs, c->ys);
    if (c->n_pursuers < 1 || c->n_evaders < 0 || c->n_pursuers > MAX_COUNT || c->n_evaders > MAX_COUNT)
        return fail(MADRL_EINVAL, "n_pursuers=%d n_evaders=%d unsupported (pursuers 1..%d, evaders 0..%d: "
                    "byte count grids)", c->n_pursuers, c->n_evaders, MAX_COUNT, MAX_COUNT);
    if (c->obs_range < 1 || c->obs_range > 63) return fail(MADRL_EINVAL, "obs_range=%d unsupported", c->obs_range);
    if (c->n_maps < 1) return fail(MADRL_EINVAL, "n_maps must be >= 1");
    if (!(c->layer_norm > 0.0)) return fail(MADRL_EINVAL, "layer_norm must be > 0");
    if (!(c->constraint_window > 0.0 && c->constraint_window <= 1.0))
        return fail(MADRL_EINVAL, "constraint_window must be in (0,1]");
    if (c->control_evaders != 0 && c->control_evaders != 1) return fail(MADRL_EINVAL, "control_evaders must be 0 or 1");
    if (c->control_evaders && c->n_evaders < c->n_pursuers)
        return fail(MADRL_EINVAL, "control_evaders=1 (train_pursuit=False): collect_obs walks range(n_pursuers) over evaders_gone (pursuit_evade.py:418-428): n_evaders=%d must be >= n_pursuers=%d",
                    c->n_evaders, c->n_pursuers);
    if (c->control_evaders && c->max_opponents != 0)
        return fail(MADRL_EINVAL, "control_evaders=1 (train_pursuit=False) with random_opponents (a per-reset number of pursuers, :180-181) is not supported");
    if (c->max_opponents != 0 && c->max_opponents < 2) return fail(MADRL_EINVAL, "max_opponents=%d: random_opponents draws randint(1, max_opponents)", c->max_opponents);
    return MADRL_OK;
}

size_t lds_bytes_for(const PursuitDev &d) {
    size_t b = 1024 + 4 * (size_t)d.GSZ;
    b += 2 * align_up((size_t)d.A, 16);
    b += 4 * align_up((size_t)d.ngw, 4) + 4 * align_up((size_t)d.ntw, 4) + 32;
    b += 4 * align_up((size_t)d.P, 4);
    b = align_up(b, 8);
    b += 8 * align_up((size_t)d.P, 2);
    b += 4 * align_up((size_t)d.D, 4);  // slot codes
    b += 2 * align_up((size_t)d.P, 16);  // observer positions (evader control)
    return align_up(b, 16);
}

// The generic kernels' slots per thread, a template argument NT in 1..8, from the handle's nt: fn(std::integral_constant<int, NT>) is called
// for NT == nt -- the one place that spells the instantiations out.
template <int NT = 1, class F>
int with_nt(int nt, F &&fn) {
    if constexpr (NT > 8) return fail(MADRL_EINVAL, "internal: nt=%d", nt);
    else {
        if (nt != NT) return with_nt<NT + 1>(nt, fn);
        fn(std::integral_constant<int, NT>{});
        return MADRL_OK;
    }
}

// The kernels of this handle's line in count mode `live` (per-env agent counts: the live-count instantiations), when it has a fast path
// there at all: a line, and that line's in-place kernel.
const Kernels *fast_kernels(const madrl_pursuit *h, bool live) {
    return h->line && h->line->k[live].has(false, OBS_F32) ? &h->line->k[live] : nullptr;
}
// Which launch runs a kernel of the line -- every other one runs the generic kernel: in place, a handle with a fast path in its count mode
// that is not switched to the generic kernel; with two buffers it also needs the line's two-buffer kernel of that mode and element format
// (shapes without a line in pursuit_to_specializations.def have none; a half form have the X / XL lines of that list and the HG / HLG
// lines of pursuit_to_f16_group_specializations.def), and evader control runs in place only.
bool runs_fast(const madrl_pursuit *h, bool two_buffer = false, int fmt = OBS_F32) {
    const Kernels *k = fast_kernels(h, h->pending != nullptr);
    if (!k || h->kernel_kind == MADRL_KERNEL_GENERIC) return false;
    return !two_buffer || (h->dev.train_pursuit && k->has(true, fmt));
}

// bytes of what the fast path of line `f` remembers about the observation buffer (behind the records in the caller's state buffer)
size_t zmask_len(const Line *f, int64_t n_envs) { return f ? (size_t)n_envs * (size_t)f->mask_bytes : 0; }

template <class IO>
IO io_of(const PursuitIO &io) {
    IO o{};
    o.mask = io.mask; o.inj_pos = io.inj_pos; o.inj_map = io.inj_map; o.actions = io.actions;
    o.inj_eact = io.inj_eact; o.obs = io.obs; o.rew = io.rew; o.done = io.done; o.removed = io.removed;
    return o;
}

// the arguments of a step launch (madrl_pursuit_step, _step_to, _step_sharded)
PursuitIO step_io(const int32_t *actions, const int32_t *inj_eact, float *obs, float *rew, uint8_t *done, int32_t *removed) {
    PursuitIO io{};
    io.actions = actions; io.inj_eact = inj_eact; io.obs = obs; io.rew = rew; io.done = done; io.removed = removed;
    return io;
}

// the fast path's launch constants as madrl_pursuit_create made them, with the curriculum of this launch
template <class Dev>
Dev dev_now(Dev d, const PursuitDev &now) {
    d.catchr = now.catchr; d.cw = now.cw; d.cw_env = now.cw_env; d.catchr_env = now.catchr_env;
    return d;
}

// mode 0: reset, 1: step.  obs_prev == nullptr: in place, io.obs is read and written.  Otherwise madrl_pursuit_step_to: the step's rows go to
// io.obs and the kept cells come from obs_prev.  fmt: the element format of both buffers -- OBS_F16 (two buffers only): io.obs and
// obs_prev point at binary16 elements, cast.
int launch(madrl_pursuit *h, const PursuitIO &io, int mode, const float *obs_prev, void *stream, int fmt = OBS_F32) {
    hipStream_t s = (hipStream_t)stream;
    const bool to = obs_prev != nullptr;   // two buffers
    if (runs_fast(h, to, fmt)) {
        const Line *l = h->line;
        const Kernels &k = l->k[h->pending != nullptr];
        int64_t blocks = h->max_blocks > 0 ? h->max_blocks : l->resident;   // persistent workgroups, as many as are resident
        if (blocks > h->dev.n_envs) blocks = h->dev.n_envs;
        // The masks describe the buffer the kept cells are read from; another one has unknown contents: every cell "not known to be zero".
        // After this launch they describe the buffer it wrote (two buffers: obs_prev is an unknown buffer from here on).
        // "Known zero" is "all bits zero" in either format, but the masks are per element: the same address read in the other format is an
        // unknown buffer too.
        if (h->zmask_obs != (obs_prev ? (const void *)obs_prev : (const void *)io.obs) || h->zmask_fmt != fmt)
            MADRL_HIP_TRY(hipMemsetAsync(h->zmask, 0xFF, zmask_len(l, h->dev.n_envs), s));
        h->zmask_obs = io.obs;
        h->zmask_fmt = fmt;
        if (mode == 1) h->last_step_entry = MADRL_STEP_ENTRY_WAVE;
        if (l->crowd) {
            const pc::CrowdDev cd = dev_now(h->cdev, h->dev);
            if (to) k.crowd_to(cd, io_of<pc::CrowdIO>(io), h->pending, obs_prev, blocks, s);
            else k.crowd(cd, io_of<pc::CrowdIO>(io), h->pending, mode, blocks, s);
        } else {
            pw::WaveIO w = io_of<pw::WaveIO>(io);
            w.flex = (to || io.inj_eact != nullptr || h->dev.catchr_env != nullptr) ? 1 : 0;
            w.control_evaders = (to || h->dev.train_pursuit) ? 0 : 1;   // (in place only: runs_fast)
            w.obs_prev = obs_prev;
            // Large batches: successive step launches walk the env range in opposite directions, so the rows written last by
            // one step are the first ones touched by the next while they are still in the 256 MB memory-side cache.  Measured
            // (scripts/sweep_wave.py, C2 shape): forward-only holds 7.2e8 env-steps/s up to 73 728 envs and collapses beyond
            // (98 304: 4.7e8, 131 072: 4.5e8); alternating holds 6.4-6.7e8 from 81 920 to 131 072 but costs 6 % below.  Hence
            // the switch at ~375 MB of rows + records per launch.  Env results do not depend on the processing order.
            pw::WaveDev wd = dev_now(h->wdev, h->dev);
            const bool alternate = mode == 1 && walk_alternates(h->dev, h->walk_mode);
            if (alternate) wd.reverse = (int32_t)(h->step_count++ & 1);
            wd.pending = h->pending;
            // the fixed-constants kernel of the line, when this launch meets its contract (the same masks and record: interchangeable)
            const bool fixed = takes_fixed(l, h->fixed_on, h->dev, LaunchAsk{mode == 1, to, h->pending != nullptr, io.inj_eact != nullptr, alternate});
            if (fixed) h->last_step_entry = MADRL_STEP_ENTRY_FIXED;
            if (to) (fmt == OBS_F16 ? k.wave_to_f16 : k.wave_to)(wd, w, blocks, s);
            else if (fixed) l->fixed(wd, w, blocks, s);
            else k.wave(wd, w, mode, blocks, s);
        }
        MADRL_HIP_TRY(hipGetLastError());
        return MADRL_OK;
    }
    if (mode == 1) h->last_step_entry = MADRL_STEP_ENTRY_GENERIC;
    h->zmask_obs = nullptr;  // the generic kernel does not maintain the fast path's stale-zero masks
    int64_t blocks = h->dev.n_envs;
    if (h->max_blocks > 0 && blocks > h->max_blocks) blocks = h->max_blocks;
    const dim3 grid((unsigned)blocks), block((unsigned)h->threads);
    const int rc = with_nt(h->nt, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        const uint16_t *const prev16 = reinterpret_cast<const uint16_t *>(obs_prev);
        if (obs_prev && fmt == OBS_F16 && h->pending) hipLaunchKernelGGL((pursuit_to_f16_kernel<NT, true>), grid, block, h->lds_bytes, s, h->dev, io, h->pending, prev16);
        else if (obs_prev && fmt == OBS_F16) hipLaunchKernelGGL((pursuit_to_f16_kernel<NT, false>), grid, block, h->lds_bytes, s, h->dev, io, h->pending, prev16);
        else if (obs_prev && h->pending) hipLaunchKernelGGL((pursuit_to_kernel<NT, true>), grid, block, h->lds_bytes, s, h->dev, io, h->pending, obs_prev);
        else if (obs_prev) hipLaunchKernelGGL((pursuit_to_kernel<NT, false>), grid, block, h->lds_bytes, s, h->dev, io, h->pending, obs_prev);
        else if (h->pending) hipLaunchKernelGGL(pursuit_live_kernel<NT>, grid, block, h->lds_bytes, s, h->dev, io, mode, h->pending);
        else hipLaunchKernelGGL(pursuit_kernel<NT>, grid, block, h->lds_bytes, s, h->dev, io, mode);
    });
    if (rc) return rc;
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}

// caller-owned state buffer = [n_envs packed records][pad to 256 B][what the configuration's fast path remembers about the observation
// buffer (Line::mask_bytes per env): stale-zero masks, 256 B per wavefront and mask word, or the crowd kernel's one word][flag plane,
// one dword per env].  The one-wavefront kernels of a pw::Shape with ZM16 (pursuit_zm16.hpp: 16 mask bits per lane) read and write only the
// first n_envs * 128 bytes of the mask region, [n_envs][32] dwords; the region keeps its 256 B per env -- sizes and offsets are part of the
// ABI -- and the memsets below (0xFF = nothing known, 0 = known zero: the same polarity in both forms) keep covering all of it.
uint64_t zmask_offset(int rec_bytes, int64_t n_envs) { return align_up((uint64_t)rec_bytes * (uint64_t)n_envs, 256); }
uint64_t flags_offset(const madrl_pursuit_config *cfg, int rec_bytes, int64_t n_envs) { return zmask_offset(rec_bytes, n_envs) + zmask_len(find_line(cfg), n_envs); }

// the launch constants WaveDev and CrowdDev share with the generic kernel's
template <class Dev>
void fill_common(Dev &w, const PursuitDev &d) {
    memset(&w, 0, sizeof(w));
    w.n_catch = d.n_catch; w.surround = d.surround; w.reward_global = d.reward_global; w.sample_maps = d.sample_maps;
    w.n_maps = d.n_maps; w.max_steps = d.max_steps; w.auto_reset = d.auto_reset; w.max_opponents = d.max_opponents;
    w.k0 = d.k0; w.k1 = d.k1; w.gid_base = d.gid_base;
    w.catchr = d.catchr; w.term_pursuit = d.term_pursuit; w.urgency = d.urgency; w.cw = d.cw;
    w.n_envs = d.n_envs;
    w.vtab = d.vtab;
    w.state = d.state;
    w.flags = d.flags;
}

int pick_threads(const PursuitDev &d, int requested) {
    int thr = requested;
    if (thr <= 0) {
        // one wavefront unless the observation row needs more than 8 slots per lane: agents loop over
        // lanes (measured at C5, 76 agents: 64 threads 171 us, 128 threads 253 us, 256 threads 388 us)
        thr = 64;
        while (thr < 1024 && (d.D + thr - 1) / thr > 8) thr += 64;
    }
    return thr;
}

}  // namespace

extern "C" {

int madrl_pursuit_obs_dim(const madrl_pursuit_config *cfg, int32_t *out_dim) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!out_dim) return fail(MADRL_EINVAL, "out_dim is NULL");
    *out_dim = obs_dim_of(cfg);
    return MADRL_OK;
}

int madrl_pursuit_state_bytes(const madrl_pursuit_config *cfg, int64_t n_envs, uint64_t *out_bytes) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (n_envs < 1 || !out_bytes) return fail(MADRL_EINVAL, "n_envs must be >= 1 and out_bytes non-NULL");
    PursuitDev d;
    layout(cfg, &d);
    *out_bytes = flags_offset(cfg, d.rec_bytes, n_envs) + 4u * (uint64_t)n_envs;
    return MADRL_OK;
}

int madrl_pursuit_flags_offset(const madrl_pursuit_config *cfg, int64_t n_envs, uint64_t *out_offset) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (n_envs < 1 || !out_offset) return fail(MADRL_EINVAL, "n_envs must be >= 1 and out_offset non-NULL");
    PursuitDev d;
    layout(cfg, &d);
    *out_offset = flags_offset(cfg, d.rec_bytes, n_envs);
    return MADRL_OK;
}

int madrl_pursuit_record_bytes(const madrl_pursuit_config *cfg, int32_t *out_bytes) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!out_bytes) return fail(MADRL_EINVAL, "out_bytes is NULL");
    PursuitDev d;
    layout(cfg, &d);
    *out_bytes = d.rec_bytes;
    return MADRL_OK;
}

int madrl_pursuit_create(const madrl_pursuit_config *cfg, const int8_t *map_pool_host, int64_t n_envs,
                         int32_t device, void *state_dev, madrl_pursuit **out) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!map_pool_host || !state_dev || !out || n_envs < 1)
        return fail(MADRL_EINVAL, "create: NULL argument or n_envs < 1");
    rc = check_env_ids(n_envs, cfg->env_id_base);
    if (rc) return rc;
    MADRL_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<madrl_pursuit> h(new (std::nothrow) madrl_pursuit());   // ~madrl_pursuit frees whatever an early return leaves behind
    if (!h) return fail(MADRL_ENOMEM, "out of host memory");
    h->cfg = *cfg;
    h->device = device;
    layout(cfg, &h->dev);
    PursuitDev &d = h->dev;
    d.n_envs = n_envs;
    d.state = (uint8_t *)state_dev;
    d.flags = reinterpret_cast<uint32_t *>((uint8_t *)state_dev + flags_offset(cfg, d.rec_bytes, n_envs));

    // ---- the generic kernel's tables
    const GenericTables gt = build_generic_tables(cfg, d, map_pool_host);
    if (gt.bad_map >= 0) return fail(MADRL_EINVAL, "map %d cell (%d,%d) = %d, expected 0 or -1", gt.bad_map, gt.bad_x, gt.bad_y, gt.bad_v);
    const size_t total = gt.host.size();
    hipError_t e = hipMalloc(&h->tables, total);
    if (e != hipSuccess) return fail(MADRL_EHIP, "hipMalloc(%zu) failed: %s", total, hipGetErrorString(e));
    e = hipMemcpy(h->tables, gt.host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(MADRL_EHIP, "hipMemcpy tables failed: %s", hipGetErrorString(e));
    const uint8_t *tb = (const uint8_t *)h->tables;
    d.maps = tb + gt.maps;
    d.cnt_tmpl = tb + gt.cnt;
    d.vtab = reinterpret_cast<const float *>(tb + gt.vtab);
    d.codes = reinterpret_cast<const uint32_t *>(tb + gt.codes);

    // ---- the fast path of this shape, if the configuration is eligible for its line
    h->line = find_line(cfg);
    void *const zmask = (uint8_t *)state_dev + zmask_offset(d.rec_bytes, n_envs);  // caller-owned, like the records
    if (h->line && !h->line->crowd) {
        // one wavefront or a group of them per env: its own tables (pursuit_wave.hpp)
        const WaveTables wt = build_wave_tables(cfg, d, h->line->g, n_envs, map_pool_host);
        if (wt.eligible) {
            const size_t wbytes = wt.host.size() * sizeof(uint32_t);
            e = hipMalloc(&h->wtables, wbytes);
            if (e == hipSuccess) e = hipMemcpy(h->wtables, wt.host.data(), wbytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) return fail(MADRL_EHIP, "wave tables: %s", hipGetErrorString(e));
            h->zmask = zmask;
            pw::WaveDev &w = h->wdev;
            fill_common(w, d);
            w.fmap_stride = wt.fstride;
            w.fmaps = reinterpret_cast<const uint32_t *>(h->wtables);
            w.cnt_tmpl = w.fmaps + wt.w_tmpl;
            w.slot_tab = w.fmaps + wt.w_slots;
            w.zmask = reinterpret_cast<uint32_t *>(zmask);
        } else {
            h->line = nullptr;
        }
    } else if (h->line && h->line->g.GSZ == d.GSZ && same_record(h->line->g, d)) {
        // the crowd kernel: the generic kernel's tables and record, when the compiled geometry is this configuration's
        h->zmask = zmask;
        pc::CrowdDev &c = h->cdev;
        fill_common(c, d);
        c.map_stride = d.map_stride;
        c.maps = d.maps;
        c.ch3 = reinterpret_cast<const uint32_t *>(zmask);
    } else {
        h->line = nullptr;
    }
    h->fixed_on = fixed_enabled();

    rc = madrl_pursuit_set_launch(h.get(), 0, 0);
    if (rc) return rc;
    // the fork / join events of madrl_pursuit_step_sharded, on this handle's device (hipSetDevice above), each checked on its own
    if (hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess)
        return fail(MADRL_EHIP, "create: hipEventCreateWithFlags failed");
    *out = h.release();
    return MADRL_OK;
}

int madrl_pursuit_last_step_entry(const madrl_pursuit *h, int32_t *out) {
    if (!h || !out) return fail(MADRL_EINVAL, "last_step_entry: NULL argument");
    *out = h->last_step_entry;
    return MADRL_OK;
}

int madrl_pursuit_fixed_choice(const madrl_pursuit_config *cfg, int64_t n_envs, uint32_t launch_bits, int32_t *out) {
    if (!out) return fail(MADRL_EINVAL, "fixed_choice: out is NULL");
    const int rc = validate(cfg);
    if (rc) return rc;
    if (n_envs < 1 || launch_bits >= 2u * MADRL_LAUNCH_KERNEL_GENERIC) return fail(MADRL_EINVAL, "fixed_choice: n_envs < 1 or unknown launch bits");
    PursuitDev d;
    layout(cfg, &d);
    d.n_envs = n_envs;
    static const double some = 0.0;   // (per-env curriculum arrays: bound or not is all the contract asks)
    if (launch_bits & MADRL_LAUNCH_CURRICULUM_ARRAYS) d.cw_env = d.catchr_env = &some;
    const int walk = (launch_bits & MADRL_LAUNCH_WALK_ALTERNATE) ? 1 : (launch_bits & MADRL_LAUNCH_WALK_FORWARD) ? 2 : 0;
    const LaunchAsk a{!(launch_bits & MADRL_LAUNCH_RESET), (launch_bits & (MADRL_LAUNCH_STEP_TO | MADRL_LAUNCH_HALF)) != 0,
                      (launch_bits & MADRL_LAUNCH_PER_ENV_COUNTS) != 0, (launch_bits & MADRL_LAUNCH_INJECTED_ACTIONS) != 0, walk_alternates(d, walk)};
    const bool fixed = !(launch_bits & MADRL_LAUNCH_KERNEL_GENERIC) && takes_fixed(find_line(cfg), fixed_enabled(), d, a);
    *out = fixed ? 1 : 0;
    return MADRL_OK;
}

int madrl_pursuit_set_walk(madrl_pursuit *h, int32_t mode) {
    if (!h || mode < 0 || mode > 2) return fail(MADRL_EINVAL, "set_walk: mode must be 0 (auto), 1 (alternate) or 2 (forward)");
    h->walk_mode = mode;
    return MADRL_OK;
}

int madrl_pursuit_set_launch(madrl_pursuit *h, int32_t threads, int64_t max_blocks) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    const int thr = pick_threads(h->dev, threads);
    if (thr % 64 != 0 || thr < 64 || thr > 1024) return fail(MADRL_EINVAL, "threads=%d must be a multiple of 64 in 64..1024", thr);
    const int nt = (h->dev.D + thr - 1) / thr;
    if (nt > 8) return fail(MADRL_EINVAL, "obs_dim=%d needs more than 8 slots per thread at %d threads", h->dev.D, thr);
    const size_t lds = lds_bytes_for(h->dev);
    if (lds > 160 * 1024) return fail(MADRL_EINVAL, "configuration needs %zu B of LDS (> 160 KiB)", lds);
    if (max_blocks < 0) return fail(MADRL_EINVAL, "max_blocks < 0");
    h->threads = thr;
    h->nt = nt;
    h->lds_bytes = lds;
    h->max_blocks = max_blocks;
    if (lds > 64 * 1024) {
        // opt in to large dynamic LDS for every instantiation we may launch
        const int bytes = (int)lds;
        for (int k = 1; k <= 8; ++k)
            (void)with_nt(k, [&](auto nt_c) {
                constexpr int NT = decltype(nt_c)::value;
                (void)hipFuncSetAttribute((const void *)pursuit_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
                (void)hipFuncSetAttribute((const void *)pursuit_live_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
                (void)hipFuncSetAttribute((const void *)pursuit_to_kernel<NT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
                (void)hipFuncSetAttribute((const void *)pursuit_to_kernel<NT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
                (void)hipFuncSetAttribute((const void *)pursuit_to_f16_kernel<NT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
                (void)hipFuncSetAttribute((const void *)pursuit_to_f16_kernel<NT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
            });
    }
    return MADRL_OK;
}

void madrl_pursuit_destroy(madrl_pursuit *h) { delete h; }   // (~madrl_pursuit)

int madrl_pursuit_set_kernel(madrl_pursuit *h, int32_t kind) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    if (kind != MADRL_KERNEL_AUTO && kind != MADRL_KERNEL_GENERIC && kind != MADRL_KERNEL_WAVE)
        return fail(MADRL_EINVAL, "unknown kernel kind %d", kind);
    if (kind == MADRL_KERNEL_WAVE && h->pending && !fast_kernels(h, true))
        return fail(MADRL_EINVAL, "per-env agent counts: no live-count specialisation was compiled for this capacity "
                    "(see madrl_amd/csrc/pursuit_live_specializations.def)");
    if (kind == MADRL_KERNEL_WAVE && !fast_kernels(h, false))
        return fail(MADRL_EINVAL, "no one-wavefront-per-env specialisation was compiled for this configuration "
                    "(see madrl_amd/csrc/pursuit_specializations.def)");
    h->kernel_kind = kind;
    return MADRL_OK;
}

int madrl_pursuit_kernel_kind(const madrl_pursuit *h, int32_t *out_kind) {
    if (!h || !out_kind) return fail(MADRL_EINVAL, "NULL argument");
    *out_kind = runs_fast(h) ? MADRL_KERNEL_WAVE : MADRL_KERNEL_GENERIC;
    return MADRL_OK;
}

int madrl_pursuit_reset(madrl_pursuit *h, const uint8_t *mask_dev, const int32_t *inj_pos_dev,
                        const int32_t *inj_map_dev, float *obs_dev, void *stream) {
    if (!h || !obs_dev) return fail(MADRL_EINVAL, "reset: handle/obs is NULL");
    PursuitIO io;
    memset(&io, 0, sizeof(io));
    io.mask = mask_dev;
    io.inj_pos = inj_pos_dev;
    io.inj_map = inj_map_dev;
    io.obs = obs_dev;
    return launch(h, io, 0, nullptr, stream);
}

int madrl_pursuit_step(madrl_pursuit *h, const int32_t *actions_dev, const int32_t *inj_evader_actions_dev,
                       float *obs_dev, float *rew_dev, uint8_t *done_dev, int32_t *removed_dev, void *stream) {
    if (!h || !actions_dev || !obs_dev || !rew_dev || !done_dev || !removed_dev)
        return fail(MADRL_EINVAL, "step: NULL argument");
    return launch(h, step_io(actions_dev, inj_evader_actions_dev, obs_dev, rew_dev, done_dev, removed_dev), 1, nullptr, stream);
}

int madrl_pursuit_step_to(madrl_pursuit *h, const int32_t *actions_dev, const int32_t *inj_evader_actions_dev, const float *obs_prev_dev,
                          float *obs_next_dev, float *rew_dev, uint8_t *done_dev, int32_t *removed_dev, void *stream) {
    if (!h || !actions_dev || !obs_prev_dev || !obs_next_dev || !rew_dev || !done_dev || !removed_dev)
        return fail(MADRL_EINVAL, "step_to: NULL argument");
    if (obs_prev_dev == obs_next_dev)
        return madrl_pursuit_step(h, actions_dev, inj_evader_actions_dev, obs_next_dev, rew_dev, done_dev, removed_dev, stream);
    const uint64_t bytes = 4ull * (uint64_t)h->dev.n_envs * (uint64_t)h->dev.P * (uint64_t)h->dev.D;
    const uint64_t a = (uint64_t)obs_prev_dev, b = (uint64_t)obs_next_dev;
    if (a < b + bytes && b < a + bytes) return fail(MADRL_EINVAL, "step_to: obs_prev and obs_next overlap (the same buffer is madrl_pursuit_step; two buffers must be disjoint)");
    if ((a | b) & 15u) return fail(MADRL_EINVAL, "step_to: observation buffers must be 16-byte aligned");
    return launch(h, step_io(actions_dev, inj_evader_actions_dev, obs_next_dev, rew_dev, done_dev, removed_dev), 1, obs_prev_dev, stream);
}

int madrl_pursuit_step_to_kernel_kind(madrl_pursuit *h, int32_t *out) {
    if (!h || !out) return fail(MADRL_EINVAL, "NULL argument");
    *out = runs_fast(h, true) ? MADRL_KERNEL_WAVE : MADRL_KERNEL_GENERIC;
    return MADRL_OK;
}

int madrl_pursuit_step_to_f16(madrl_pursuit *h, const int32_t *actions_dev, const int32_t *inj_evader_actions_dev, const uint16_t *obs_prev_dev,
                              uint16_t *obs_next_dev, float *rew_dev, uint8_t *done_dev, int32_t *removed_dev, void *stream) {
    if (!h || !actions_dev || !obs_prev_dev || !obs_next_dev || !rew_dev || !done_dev || !removed_dev)
        return fail(MADRL_EINVAL, "step_to_f16: NULL argument");
    const uint64_t bytes = 2ull * (uint64_t)h->dev.n_envs * (uint64_t)h->dev.P * (uint64_t)h->dev.D;
    const uint64_t a = (uint64_t)obs_prev_dev, b = (uint64_t)obs_next_dev;
    if (a < b + bytes && b < a + bytes) return fail(MADRL_EINVAL, "step_to_f16: obs_prev and obs_next overlap (there is no in-place half step; two buffers must be disjoint)");
    if ((a | b) & 15u) return fail(MADRL_EINVAL, "step_to_f16: observation buffers must be 16-byte aligned");
    // (the half pointers travel in the float fields of the launch structures, cast: no structure grows)
    return launch(h, step_io(actions_dev, inj_evader_actions_dev, reinterpret_cast<float *>(obs_next_dev), rew_dev, done_dev, removed_dev), 1,
                  reinterpret_cast<const float *>(obs_prev_dev), stream, OBS_F16);
}

int madrl_pursuit_step_to_f16_kernel_kind(madrl_pursuit *h, int32_t *out) {
    if (!h || !out) return fail(MADRL_EINVAL, "NULL argument");
    *out = runs_fast(h, true, OBS_F16) ? MADRL_KERNEL_WAVE : MADRL_KERNEL_GENERIC;
    return MADRL_OK;
}

int madrl_pursuit_step_sharded(madrl_pursuit *const *hs, const madrl_pursuit_shard_io *io, int32_t n_shards, void *caller_stream,
                               int32_t fork, int32_t join) {
    if (!hs || !io || n_shards < 1) return fail(MADRL_EINVAL, "step_sharded: NULL argument or n_shards < 1");
    for (int j = 0; j < n_shards; ++j) {
        if (!hs[j] || !io[j].actions || !io[j].obs || !io[j].rew || !io[j].done || !io[j].removed) return fail(MADRL_EINVAL, "step_sharded: shard %d has a NULL argument", j);
        if (!hs[j]->ev_done || !hs[j]->ev_fork) return fail(MADRL_EINVAL, "step_sharded: shard %d's handle has no events (madrl_pursuit_create makes them)", j);
    }
    hipStream_t cs = (hipStream_t)caller_stream;
    if (fork) {   // every sub-batch stream waits for what the caller's stream holds so far (the actions)
        MADRL_HIP_TRY(hipEventRecord(hs[0]->ev_fork, cs));
        for (int j = 0; j < n_shards; ++j) if ((hipStream_t)io[j].stream != cs) MADRL_HIP_TRY(hipStreamWaitEvent((hipStream_t)io[j].stream, hs[0]->ev_fork, 0));
    }
    int rc = MADRL_OK, launched = 0;
    for (; launched < n_shards && rc == MADRL_OK; ++launched) {
        const int j = launched;
        rc = launch(hs[j], step_io(io[j].actions, io[j].inj_evader_actions, io[j].obs, io[j].rew, io[j].done, io[j].removed), 1, nullptr, io[j].stream);
        if (rc) break;
    }
    // ... and the caller's stream waits for every sub-batch -- also when a launch failed half way: the shards launched before it are
    // running, and the caller's stream must not be left unordered against them
    if (join || rc != MADRL_OK)
        for (int j = 0; j < launched; ++j) {
            if ((hipStream_t)io[j].stream == cs) continue;
            if (hipEventRecord(hs[j]->ev_done, (hipStream_t)io[j].stream) != hipSuccess || hipStreamWaitEvent(cs, hs[j]->ev_done, 0) != hipSuccess) {
                if (rc == MADRL_OK) rc = fail(MADRL_EHIP, "step_sharded: joining shard %d failed", j);
            }
        }
    return rc;
}

int madrl_pursuit_get_state(madrl_pursuit *h, int32_t *pos_p, int32_t *pos_e, uint8_t *gone, uint8_t *term_p,
                            uint8_t *term_e, int32_t *map_id, uint32_t *tick, int32_t *t, void *stream) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    const unsigned blocks = (unsigned)((h->dev.n_envs + 127) / 128);
    hipLaunchKernelGGL(pursuit_get_state_kernel, dim3(blocks), dim3(128), 0, (hipStream_t)stream, h->dev, pos_p,
                       pos_e, gone, term_p, term_e, map_id, tick, t);
    MADRL_HIP_TRY(hipGetLastError());
    if (h->pending && pos_p) {  // pursuer slots that do not exist: (-1, -1)
        hipLaunchKernelGGL(pursuit_live_counts_kernel, dim3(blocks), dim3(128), 0, (hipStream_t)stream, h->dev, pos_p, nullptr, nullptr);
        MADRL_HIP_TRY(hipGetLastError());
    }
    return MADRL_OK;
}

int madrl_pursuit_set_state(madrl_pursuit *h, const int32_t *pos_p, const int32_t *pos_e, const uint8_t *gone,
                            const uint8_t *term_p, const uint8_t *term_e, const int32_t *map_id,
                            const uint32_t *tick, const int32_t *t, void *stream) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    const unsigned blocks = (unsigned)((h->dev.n_envs + 127) / 128);
    hipLaunchKernelGGL(pursuit_set_state_kernel, dim3(blocks), dim3(128), 0, (hipStream_t)stream, h->dev, pos_p,
                       pos_e, gone, term_p, term_e, map_id, tick, t);
    MADRL_HIP_TRY(hipGetLastError());
    // agents put somewhere else usually come with an observation buffer written from outside (a checkpoint restored): forget what is known
    // about it.  Episode clocks and RNG ticks alone (t, tick) say nothing about the buffer.
    if (pos_p || pos_e || gone || term_p || term_e || map_id) h->zmask_obs = nullptr;
    return MADRL_OK;
}

int madrl_pursuit_invalidate_obs(madrl_pursuit *h) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    h->zmask_obs = nullptr;  // the next fast-path launch starts from "no cell is known to be zero"
    return MADRL_OK;
}

int madrl_pursuit_declare_obs_zero(madrl_pursuit *h, const float *obs_dev, void *stream) {
    if (!h || !obs_dev) return fail(MADRL_EINVAL, "declare_obs_zero: NULL argument");
    if (h->zmask) {   // every cell of that buffer is known to hold +0.0f: no stale cell can need protecting
        MADRL_HIP_TRY(hipMemsetAsync(h->zmask, 0, zmask_len(h->line, h->dev.n_envs), (hipStream_t)stream));
        h->zmask_obs = obs_dev;
        h->zmask_fmt = OBS_F32;
    }
    return MADRL_OK;
}

int madrl_pursuit_set_params(madrl_pursuit *h, double catchr, double constraint_window) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    if (!(constraint_window > 0.0 && constraint_window <= 1.0)) return fail(MADRL_EINVAL, "constraint_window must be in (0,1]");
    h->cfg.catchr = catchr; h->cfg.constraint_window = constraint_window;
    h->dev.catchr = catchr; h->dev.cw = constraint_window;
    return MADRL_OK;
}

int madrl_pursuit_set_curriculum(madrl_pursuit *h, const double *constraint_window_dev, const double *catchr_dev) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    h->dev.cw_env = constraint_window_dev;
    h->dev.catchr_env = catchr_dev;
    return MADRL_OK;
}

int madrl_pursuit_set_agent_counts(madrl_pursuit *h, const int32_t *pending_dev) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    if (pending_dev && !h->dev.train_pursuit)
        return fail(MADRL_EINVAL, "per-env agent counts with control_evaders=1 (train_pursuit=False) are not supported");
    if (pending_dev && h->kernel_kind == MADRL_KERNEL_WAVE && !fast_kernels(h, true))
        return fail(MADRL_EINVAL, "per-env agent counts: kernel WAVE was requested and no live-count specialisation was compiled for this "
                    "capacity (see madrl_amd/csrc/pursuit_live_specializations.def)");
    h->pending = pending_dev;
    return MADRL_OK;
}

int madrl_pursuit_get_live_counts(madrl_pursuit *h, int32_t *live_dev, void *stream) {
    if (!h || !live_dev) return fail(MADRL_EINVAL, "get_live_counts: NULL argument");
    const unsigned blocks = (unsigned)((h->dev.n_envs + 127) / 128);
    hipLaunchKernelGGL(pursuit_live_counts_kernel, dim3(blocks), dim3(128), 0, (hipStream_t)stream, h->dev, nullptr, live_dev, nullptr);
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}

int madrl_pursuit_set_live_counts(madrl_pursuit *h, const int32_t *live_dev, void *stream) {
    if (!h || !live_dev) return fail(MADRL_EINVAL, "set_live_counts: NULL argument");
    if (!h->pending) return fail(MADRL_EINVAL, "set_live_counts: the handle has no per-env agent counts (madrl_pursuit_set_agent_counts)");
    const unsigned blocks = (unsigned)((h->dev.n_envs + 127) / 128);
    hipLaunchKernelGGL(pursuit_live_counts_kernel, dim3(blocks), dim3(128), 0, (hipStream_t)stream, h->dev, nullptr, nullptr, live_dev);
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}

}  // extern "C"
