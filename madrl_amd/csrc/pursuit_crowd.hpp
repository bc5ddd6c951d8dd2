// pursuit_crowd.hpp -- compile-time-specialised PursuitEvade kernel for CROWDS: more than 64 pursuers or evaders.
//
// The one-wavefront and the group kernel (pursuit_wave.hpp, pursuit_group.hpp) keep one agent per lane, the evaders' alive mask in one
// 64-bit scalar, the record in 64 dwords and three dword layers in LDS.  This kernel gives all of that up so that the shapes those two
// refuse -- up to 1 023 agents of a kind, maps up to 128 x 128 with obs_range 21, records of any length (the authors' CNN launch line,
// runners/old/rllab/pursuit_cnn.sh:1: 100 v 300, obs_range 21, (R, R, 4) rows, a 912-byte record) -- have a specialised kernel too.
// The shapes are the XC lines of pursuit_crowd_specializations.def; the kernels are instantiated in pursuit_crowd.hip.  Per-env agent
// counts within such a shape as a capacity: LCShape / pursuit_live_crowd_kernel below, the XLC lines of pursuit_live_specializations.def,
// instantiated in pursuit_live_crowd.hip.
//
// Design (DESIGN.md "pursuit_crowd_kernel"):
//   * One workgroup of NW wavefronts per env, persistent over envs.  Agents are LOOPED over the threads; positions, the gone / terminal
//     bit words and the window origins live in LDS.  An evader's index in the evader layer is a popcount over the gone words, as in
//     the generic kernel (pursuit_generic.inc), whose packed record and whose tables (padded byte maps, need_to_surround, value table)
//     this kernel reads as they are: the two are interchangeable step by step on one state buffer.
//   * LDS holds ONE PACKED DWORD PER CELL of the padded grid: byte 0 the map (0 free, 1 building, 0xFE outside the map), byte 1 the
//     pursuer count, byte 2 the evader count, byte 3 the catch credit (purs_sur).  One LDS read feeds one (R, R, 4) float4.  Counts
//     are placed with one ds_add per agent and taken away again after the row pass (the dword arithmetic is modular, so even a count
//     that leaves its byte -- the overflow mark -- leaves the cells as they were); the cells are rewritten only when the env's map
//     differs from the previous env's, expanded from the 4x smaller byte map.
//   * Row pass: float4 slot q of the env's P*D/4 goes to thread q % NT, a rolled loop: every store instruction writes consecutive
//     float4 from consecutive lanes.  (R, R, 4) rows: a cell inside the map is one non-temporal float4 when channel 3 of the env's rows
//     is known to hold +0.0 (one word per env behind the records, CrowdDev::ch3: madrl_pursuit_declare_obs_zero sets it, every event
//     after which the buffer is unknown clears it -- the kernel never stores anything but +0.0 there, so the knowledge never expires
//     by itself), else three dwords; a cell outside the map is one dword (channel 0).  The centre cell always is a whole float4.
//     Flatten rows: a float4 whose four elements are all stored (channel 0, the id, count cells inside the map) is whole, one that
//     holds a count cell outside the map falls back to dword stores.
//   * Barriers are LDS-only (group_sync): no wavefront waits for its row stores at a barrier.
#pragma once

#include "common.hpp"
#include "pursuit_rules.hpp"

namespace madrl {
namespace pc {

constexpr uint32_t PAD_MAP = 0xFEu;    // map byte outside the map (value table entry: 1 / layer_norm)
constexpr int MAX_CELL_COUNT = 253;    // as in the generic kernel: one more agent of a kind on a cell raises the overflow mark
constexpr int HDR_BYTES = 16;

struct CrowdDev {
    int32_t n_catch, surround, reward_global, sample_maps, n_maps, max_steps, auto_reset;
    int32_t max_opponents;   // > 0: random_opponents (pursuit_evade.py:177-181)
    int32_t map_stride;      // bytes per map entry in `maps`
    uint32_t k0, k1, gid_base;
    double catchr, term_pursuit, urgency, cw;
    int64_t n_envs;
    const uint8_t *maps;     // the generic kernel's table: per map the padded wall layer [GSZ bytes], then need_to_surround [XS*YS]
    const float *vtab;       // 256 floats: fl32(k / layer_norm), [0xFE] = fl32(1.0 / layer_norm)
    const double *cw_env;    // per-env constraint_window / catchr (curriculum) or nullptr: the scalars above
    const double *catchr_env;
    uint8_t *state;
    uint32_t *flags;         // [n_envs] flag words of the step launches (done_flag_word, common.hpp)
    const uint32_t *ch3;     // [n_envs] 0: channel 3 of the env's (R, R, 4) rows holds +0.0 off the centre; anything else: not known
};

struct CrowdIO {
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

template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_, int NW_>
struct CShape {
    static constexpr int XS = XS_, YS = YS_, P = P_, E = E_, A = P_ + E_, R = R_, FLATTEN = FLATTEN_, NW = NW_, NT = 64 * NW_;
    static constexpr int OFF = (R - 1) / 2;
    static constexpr int PAD = OFF > 1 ? OFF : 1;
    static constexpr int GW = YS + 2 * PAD;
    static constexpr int GH = XS + 2 * PAD;
    static constexpr int GSZ = (GH * GW + 15) / 16 * 16;           // cells: the generic kernel's bytes per layer
    static constexpr int D = FLATTEN ? 3 * R * R + 1 : 4 * R * R;  // include_id is implied
    static constexpr int DV = D / 4;                               // float4 per pursuer row
    static constexpr int NQ = P * DV;                              // float4 slots per env
    // packed state record, identical to the generic kernel's layout() (pursuit_tables.hpp)
    static constexpr int NGW = (E + 31) / 32 > 0 ? (E + 31) / 32 : 1;
    static constexpr int NTW = (A + 31) / 32;
    static constexpr int OFF_GONE = (HDR_BYTES + 2 * A + 3) / 4 * 4;
    static constexpr int OFF_TERM = OFF_GONE + 4 * NGW;
    static constexpr int REC_BYTES = (OFF_TERM + 4 * NTW + 15) / 16 * 16;
    // LDS, in dwords
    static constexpr int X_CELL = 0;
    static constexpr int X_VTAB = GSZ;                                       // 256 floats
    static constexpr int X_CODE = X_VTAB + 256;                              // flatten: D element codes
    static constexpr int X_REW = X_CODE + (FLATTEN ? (D + 3) / 4 * 4 : 0);   // P doubles (global reward)
    static constexpr int X_BASE = X_REW + 2 * ((P + 1) / 2 * 2);             // P window origins
    static constexpr int X_KPRE = X_BASE + (P + 3) / 4 * 4;                  // P pre-move counts
    static constexpr int X_GONE = X_KPRE + (P + 3) / 4 * 4;
    static constexpr int X_PLACED = X_GONE + (NGW + 3) / 4 * 4;              // evaders whose count is in the cells
    static constexpr int X_TERM = X_PLACED + (NGW + 3) / 4 * 4;
    // [0..3] header, [4] removed, LCShape: [5] / [6] the first pursuer / evader slot that does not exist (ds_min over the record's
    // x bytes while it is loaded) -- they must hold (P, E) whenever a load begins: set before the env loop and by every record store
    static constexpr int X_MISC = X_TERM + (NTW + 3) / 4 * 4;
    static constexpr int X_XY = X_MISC + 8;                                  // u8 x[A16], y[A16]
    static constexpr int A16 = (A + 15) / 16 * 16;
    static constexpr int LDS_DWORDS = X_XY + 2 * A16 / 4;
    static constexpr int CENTRE = (R / 2) * R + R / 2;                       // (R, R, 4) rows: the float4 that holds the id
    static_assert(NW >= 1 && NW <= 16, "1 .. 16 wavefronts per workgroup");
    static_assert(P >= 1 && P <= 1023 && E >= 0 && E <= 1023, "agent counts up to the generic kernel's MAX_COUNT");
    static_assert(XS >= 1 && YS >= 1 && XS <= 255 && YS <= 255, "coordinates are bytes of the record");
    static_assert(R % 2 == 1, "odd obs_range only (even ranges run on the generic kernel)");
    static_assert(D % 4 == 0, "observation row must be a whole number of float4");
    static_assert(LDS_DWORDS * 4 <= 160 * 1024, "LDS budget: one workgroup may declare 160 KiB");
    static_assert(X_REW % 2 == 0, "the reward doubles are 8-byte aligned");
    static constexpr bool LIVE = false;
};

// Per-env agent counts (madrl_pursuit_set_agent_counts): the same geometry with P and E as a capacity.  The env's live (np, ne) are the
// leading pursuer / evader slots of its record whose x byte is not NOT_HERE -- the generic kernel's marks (pursuit_generic.inc), whose
// LIVE branches pursuit_live_crowd_kernel follows line for line.  The XLC lines of pursuit_live_specializations.def, instantiated in
// pursuit_live_crowd.hip.
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_, int NW_>
struct LCShape : CShape<XS_, YS_, P_, E_, R_, FLATTEN_, NW_> {
    static constexpr bool LIVE = true;
};

constexpr uint32_t NOT_HERE = 0xFFu;   // position byte of a slot that does not exist (no coordinate is 255)

// ds_add of one agent to byte `sh / 8` of a cell; *ovf as in the generic kernel's lds_byte_add
__device__ __forceinline__ void cell_add(uint32_t *cell, int idx, unsigned sh, uint32_t *ovf) {
    const unsigned old = atomicAdd(&cell[idx], 1u << sh);
    if (((old >> sh) & 0xFFu) >= (unsigned)MAX_CELL_COUNT) *ovf = 1u;
}

// numpy float64 add.reduce order (pairwise, 8-way unrolled base case; the recursive split above 128 elements): see pursuit.hip
__device__ __forceinline__ double np_base(const double *a, int n) {
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
template <int N>
__device__ __forceinline__ double np_sum(const double *a) {
    if constexpr (N <= 128) return np_base(a, N);
    else {
        constexpr int N2 = N / 2 - (N / 2) % 8;
        return np_sum<N2>(a) + np_sum<N - N2>(a + N2);
    }
}

// the same order over a run-time count (LCShape: the live pursuers): np_pairwise_sum of pursuit.hip, numpy's uneven split (n2 = n / 2 rounded
// down to a multiple of 8) above 128 elements, four levels for every count up to 1 024.  A loop instead of the recursion (one copy of
// np_base in the code, not sixteen): the up to sixteen leaves in order, each found by walking its path bits down from the root (a leaf
// above the bottom level is taken on its all-zero path only), and a partial sum per level that is added when its right sibling arrives.
__device__ __forceinline__ double np_sum_n(const double *a, int n) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t has = 0u;
    double v = 0.0;
#pragma unroll 1
    for (int leaf = 0; leaf < 16; ++leaf) {
        int off = 0, len = n, depth = 0;
        bool first = true;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const bool right = (leaf >> (3 - l)) & 1;
            if (len <= 128) {
                if (right) first = false;
            } else {
                int n2 = len / 2;
                n2 -= n2 % 8;
                if (right) { off += n2; len -= n2; }
                else len = n2;
                depth = l + 1;
            }
        }
        if (!first) continue;
        v = np_base(a + off, len);
#pragma unroll
        for (int d = 4; d >= 1; --d) {
            if (d != depth) continue;
            if (has & (1u << (d - 1))) { v = acc[d - 1] + v; has &= ~(1u << (d - 1)); --depth; }
            else { acc[d - 1] = v; has |= 1u << (d - 1); }
        }
    }
    return v;
}

// workgroup barrier that waits for LDS traffic only (a wavefront does not wait for its row stores here)
__device__ __forceinline__ void group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef float v4f __attribute__((ext_vector_type(4)));

// MODE 0: reset(mask)   MODE 1: step (+ fused auto-reset)
// The body (pursuit_crowd_body.inc) is included in both kernels rather than called, as pursuit_generic.inc is: the fixed-shape kernels'
// code stays what it was, and the live kernels get the caller's pending counts as an argument of their own -- CrowdDev and CrowdIO, and
// with them the fixed kernels' argument loads, are untouched.
template <class S, int MODE>
__global__ __launch_bounds__(S::NT) void pursuit_crowd_kernel(const CrowdDev d, const CrowdIO io) {
    [[maybe_unused]] const int32_t *const pending = nullptr;
    constexpr bool TO = false;
    [[maybe_unused]] const float *const obs_prev = nullptr;
#include "pursuit_crowd_body.inc"
}

// S = LCShape: pending = the caller's int32 [n_envs][2] (pursuers, evaders), read by resets only
template <class S, int MODE>
__global__ __launch_bounds__(S::NT) void pursuit_live_crowd_kernel(const CrowdDev d, const CrowdIO io, const int32_t *const pending) {
    constexpr bool TO = false;
    [[maybe_unused]] const float *const obs_prev = nullptr;
#include "pursuit_crowd_body.inc"
}

// The two-buffer step (madrl_pursuit_step_to) of a CShape or an LCShape: the step's rows go to io.obs, whole float4s, and what an in-place
// step leaves alone comes from obs_prev (write_obs in the body).  The XC / XLC lines of pursuit_to_specializations.def, instantiated in
// pursuit_to.hip.
template <class S>
__global__ __launch_bounds__(S::NT) void pursuit_crowd_to_kernel(const CrowdDev d, const CrowdIO io, [[maybe_unused]] const int32_t *const pending,
                                                                 const float *const obs_prev) {
    constexpr int MODE = 1;
    constexpr bool TO = true;
#include "pursuit_crowd_body.inc"
}

// host side: launches the instantiation of shape S (defined and instantiated for every XC line in pursuit_crowd.hip; `pending` is not
// used: one signature for both launchers, Kernels in pursuit.hip)
template <class S>
void crowd_launch(const CrowdDev &d, const CrowdIO &io, const int32_t *pending, int mode, int64_t blocks, hipStream_t s);
// ... of an LCShape (for every XLC line in pursuit_live_crowd.hip)
template <class S>
void live_crowd_launch(const CrowdDev &d, const CrowdIO &io, const int32_t *pending, int mode, int64_t blocks, hipStream_t s);
// ... of the two-buffer step of a CShape / LCShape (for every XC / XLC line of pursuit_to_specializations.def in pursuit_to.hip)
template <class S>
void crowd_to_launch(const CrowdDev &d, const CrowdIO &io, const int32_t *pending, const float *obs_prev, int64_t blocks, hipStream_t s);

}  // namespace pc
}  // namespace madrl
