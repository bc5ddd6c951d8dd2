// pursuit_group.hpp -- compile-time-specialised PursuitEvade kernel for shapes with MORE THAN 64 AGENTS:
// one workgroup of NW wavefronts = one env (BASELINE configs[4]: 32x32, 16 pursuers / 60 evaders).
//
// The scheme is pursuit_wave.hpp's (read that header first) and the environment's rules are pursuit_rules.hpp's, where calling them
// leaves the kernels bench.py runs as they were.  What changes when the agents of an env no longer fit one wavefront:
//   * thread t = agent t (pursuers first): the agents occupy the first NAW = ceil(A / 64) wavefronts; the
//     observation row is dealt over ALL NW wavefronts (slot q -> thread q % (64 NW)), so a wavefront without
//     agents still carries its share of the row;
//   * phases are separated by `s_waitcnt lgkmcnt(0); s_barrier` (LDS traffic only -- unlike __syncthreads()
//     no vmcnt(0): a wavefront never waits for its observation stores to reach HBM);
//   * wave-wide ballots (caught evaders, evaders not created by a reset) are combined through two LDS words
//     per wavefront; the alive mask of the <= 64 evaders stays ONE 64-bit scalar in every wavefront, the
//     terminal flags are one 64-bit scalar per wavefront for its own lanes;
//   * window origins come from LDS (written by the pursuer lanes) instead of ds_bpermute, since the pursuers
//     live in wavefront 0 only;
//   * every wavefront loads the whole record (dword k in lane k) and stores the dwords it owns.
// Requirements: n_pursuers <= 64, n_evaders <= 64, record <= 64 dwords, odd obs_range, row length % 4 == 0.
//
// LONG ROWS (round 6; the authors' own training shapes, runners/old/rllab/pursuit.sh:1 -- 30 pursuers, obs_range 11: 2 730 float4 per
// env, 11 slots per thread of four wavefronts, two mask words): with more than 8 slots per thread of two wavefronts the per-slot
// constants no longer live in registers (6 VGPRs per slot), and four wavefronts carry the rows.
// Such a shape is TABLED: slot q = tid + NT s still belongs to thread tid (every store instruction writes NT consecutive float4, whole
// 64-byte chunks), but its constants come from a table in LDS indexed by the float4's position f = q mod DV inside its row -- four
// 15-bit dword offsets relative to the window origin, packed in two dwords, identical for every pursuer -- and (pursuer, f) advance
// from slot to slot by constants.  The stale-zero mask grows to MWORDS = ceil(NS / 8) dwords per thread (one bit per slot in each byte).
// The authors' shapes have two mask words; three and four (17 to 32 slots), words that hold 1, 5 and 7 slots and the 9-slot threshold
// run in the `// tests:` lines of pursuit_specializations.def.
//
// PER-ENV AGENT COUNTS (LGShape, pursuit_live_specializations.def XLG lines): the LShape contract of pursuit_wave.hpp carried over.  The
// agents span wavefronts, so the live (np, ne) are counted from the record that EVERY wavefront holds whole (dword k in lane k), not from
// a ballot of the agent lanes: all NW wavefronts agree on them without a barrier.  Rows k >= np are not stored (their store branches stay,
// taken by no lane), and their stale-zero mask bits are kept.
//
// TWO BUFFERS (TGShape / TLGShape, madrl_pursuit_step_to) and HALF-PRECISION SLOTS (THGShape / TLHGShape, madrl_pursuit_step_to_f16; the
// HG / HLG lines of pursuit_to_f16_group_specializations.def): see the comments at those shapes below.  A half shape differs from its
// float32 two-buffer twin in the row pass only -- 8-byte slots, converted values, kept halves carried over as bits, a load-blend-store
// second pass -- and in the S::LEAN_REGS form of the global reward's sum; dynamics, rewards, done bits, records and the masks'
// equilibrium are the shared kernel text.
#pragma once

#include "pursuit_wave.hpp"

namespace madrl {
namespace pw {

// resident wavefronts per SIMD the group kernel's registers are allocated for
#ifndef MADRL_PG_WAVES
#define MADRL_PG_WAVES 4
#endif
#ifndef MADRL_PG_UNROLL
#define MADRL_PG_UNROLL 2   // LONG ROWS: slots of one mask word in flight together (their LDS reads issued side by side)
#endif

template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_, int NW_>
struct GShape {
    static constexpr int XS = XS_, YS = YS_, P = P_, E = E_, A = P_ + E_, R = R_, FLATTEN = FLATTEN_, NW = NW_;
    static constexpr int NT = 64 * NW;
    static constexpr int NAW = (A + 63) / 64;                    // wavefronts that hold agents
    static constexpr int OFF = (R - 1) / 2;
    static constexpr int PAD = OFF > 1 ? OFF : 1;
    static constexpr int GW = YS + 2 * PAD;
    static constexpr int GH = XS + 2 * PAD;
    static constexpr int GSZ = (GH * GW + 3) / 4 * 4;
    static constexpr int D = FLATTEN ? 3 * R * R + 1 : 4 * R * R;
    static constexpr int DV = D / 4;
    static constexpr int NQ = P * DV;
    static constexpr int NS = (NQ + NT - 1) / NT;                // float4 slots per thread
    static constexpr int MWORDS = (NS + 7) / 8;                  // stale-zero mask dwords per thread: one bit per slot in each byte, 8 slots per dword
    static constexpr bool TABLED = NS > 8;                       // slot constants from an LDS table indexed by the position in the row (see above)
    static constexpr int X_FILL = 3 * GSZ;
    static constexpr int X_SKIP = 3 * GSZ + 1;
    static constexpr int X_ID = 3 * GSZ + 2;
    static constexpr int X_VTAB = (X_ID + P + 3) / 4 * 4;
    static constexpr int NVT = 72;
    static constexpr int X_NEED = X_VTAB + NVT;
    static constexpr int X_ORG = X_NEED + (XS * YS + 3) / 4;     // P window origins
    static constexpr int X_XCH = (X_ORG + P + 3) / 4 * 4;        // 2 dwords per wavefront: ballot exchange
    static constexpr int X_TAB = (X_XCH + 2 * NW + 3) / 4 * 4;   // TABLED: DV entries of two dwords (8-byte aligned)
    static constexpr int LDS_DWORDS = X_TAB + (TABLED ? 2 * DV : 0);
    static constexpr int NGW = (E + 31) / 32 > 0 ? (E + 31) / 32 : 1;
    static constexpr int NTW = (A + 31) / 32;
    static constexpr int OFF_GONE = (16 + 2 * A + 3) / 4 * 4;
    static constexpr int OFF_TERM = OFF_GONE + 4 * NGW;
    static constexpr int REC_BYTES = (OFF_TERM + 4 * NTW + 15) / 16 * 16;
    static constexpr int REC_DW = REC_BYTES / 4;
    static_assert(NAW <= NW, "not enough wavefronts for the agents");
    static_assert(P <= 64 && E <= 64, "pursuers must fit wavefront 0, the evader alive mask one 64-bit scalar");
    static_assert(REC_DW <= 64, "the whole record must fit one dword per lane");
    static_assert(R % 2 == 1, "odd obs_range only");
    static_assert(D % 4 == 0, "observation row must be a whole number of float4");
    static_assert(LDS_DWORDS * 4 <= 64 * 1024, "LDS budget");
    // resident wavefronts per SIMD: what the registers are allocated for, capped by what the LDS of a CU (160 KB) admits
    static constexpr int OCC_LDS = (160 * 1024 / (LDS_DWORDS * 4)) * NW / 4;
    static constexpr int OCC = OCC_LDS < MADRL_PG_WAVES ? (OCC_LDS < 1 ? 1 : OCC_LDS) : MADRL_PG_WAVES;
    static_assert(MWORDS <= 4, "at most 32 float4 slots per thread");
    static_assert(!TABLED || 3 * GSZ + 2 + P < 32768, "TABLED: dword offsets of the layers must fit 15 bits");
    static constexpr bool LIVE = false;
    static constexpr bool TO = false;
    static constexpr bool H16 = false;                           // (THGShape / TLHGShape: binary16 observation buffers)
    static constexpr bool LEAN_REGS = false;                     // register-pressure measures no float32 shape takes (see THGShape)
};

// Per-env agent counts on the group kernel: the same geometry with P and E as a capacity (see LShape in pursuit_wave.hpp).
// pursuit_group_kernel<LGShape<...>, ...> is a kernel of its own, instantiated in pursuit_live_group.hip.
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_, int NW_>
struct LGShape : GShape<XS_, YS_, P_, E_, R_, FLATTEN_, NW_> {
    static constexpr bool LIVE = true;
};

// The two-buffer step on the group kernel (madrl_pursuit_step_to; see TShape in pursuit_wave.hpp): the step's observation pass stores
// every valid float4 of the env's rows to io.obs, whole and non-temporal; the elements the in-place pass leaves alone come from the same
// place of io.obs_prev, loaded only by the lanes that keep one.  The second pass of a fused auto-reset is the in-place pass on io.obs.
// Only the flexible step kernel <S, 1, true> is instantiated (group_to_launch, pursuit_to_group.hip); the shapes are the XG / XLG lines
// of pursuit_to_specializations.def.
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_, int NW_>
struct TGShape : GShape<XS_, YS_, P_, E_, R_, FLATTEN_, NW_> {
    static constexpr bool TO = true;
};
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_, int NW_>
struct TLGShape : LGShape<XS_, YS_, P_, E_, R_, FLATTEN_, NW_> {
    static constexpr bool TO = true;
};
// The two-buffer step over binary16 buffers on the group kernel (madrl_pursuit_step_to_f16; the contract is THShape's in pursuit_wave.hpp):
// io.obs and io.obs_prev point at 2-byte elements (cast: WaveDev / WaveIO do not grow), an env's rows are P * D * 2 bytes, and a slot -- the
// same four elements, thread tid keeps slot q = tid + NT s -- is 8 bytes at q * 8.  The stale-zero mask words, the TABLED slot table and
// the batch sizes keep their meaning.  Part 1 of the two-buffer pass (need_of) is the float32 kernel's; part 2 loads an old slot as one
// 8-byte word (lanes that keep nothing load nothing), converts the four new values (half_bits: round to nearest even; SENT / outside and
// known zero becomes +0.0), carries the kept halves over as the 16 bits they are -- their mask bit: "the loaded half is non-zero by its
// bits" -- and stores the slot as ONE non-temporal 8-byte store.  The old values of a batch cost two registers per slot instead of four.
// The second pass of a fused auto-reset is a load-blend-store of whole 8-byte slots of io.obs (half_slot_in_place, pursuit_wave.hpp): the
// thread that wrote a slot in pass 0 reads it back, after its stores have been acknowledged, with an agent-scope load; the float32
// in-place stores are float32 geometry and refuse to compile for these shapes (float32_slots_only below).
// Only the flexible step kernel <S, 1, true> is instantiated (group_to_f16_launch; pursuit_to_group_f16.hip the HG lines,
// pursuit_to_group_f16_live.hip the HLG lines of pursuit_to_f16_group_specializations.def).
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_, int NW_>
struct THGShape : GShape<XS_, YS_, P_, E_, R_, FLATTEN_, NW_> {
    static constexpr bool TO = true;
    static constexpr bool H16 = true;
    static constexpr bool LEAN_REGS = true;
};
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_, int NW_>
struct TLHGShape : LGShape<XS_, YS_, P_, E_, R_, FLATTEN_, NW_> {
    static constexpr bool TO = true;
    static constexpr bool H16 = true;
    static constexpr bool LEAN_REGS = true;
};
// slots of the two-buffer pass whose old float4s are in flight together: all loads of a batch are issued before its first store (vmcnt
// retires in order: a wait for a load is a wait for every store issued before it).  Four registers per slot and lane; the live forms
// of the long-row shapes compile to the 128 registers of their occupancy with no room to spare (eight slots spill 76 - 80 registers).
// Measured at the authors' 30 v 50 shape, 16 384 envs, one launch per step round a ring of nine buffers: batches of 2 slots 311 us per
// launch, of 3 slots 295, of 4 slots 281 (profiles/r11_step_to_group): the waits bind, not the loads.
// The binary16 forms (THGShape / TLHGShape) keep these sizes: their old values are two registers per slot, but the unrolled body of a
// larger batch does not fit either -- at the authors' shapes batches of 5 / 6 / 8 slots compile to 13 / 17 / 55 VGPR spills (fixed) and
// 27 / 27 / 61 (live), batches of 4 to 105 and 108 registers without one.
#ifndef MADRL_PG_TO_BATCH
#define MADRL_PG_TO_BATCH 4    // long rows (the rolled loop)
#endif
#ifndef MADRL_PG_TO_RBATCH
#define MADRL_PG_TO_RBATCH 2   // short rows (slot constants in registers)
#endif

// host launcher of a TGShape / TLGShape kernel: explicitly instantiated in pursuit_to_group.hip, one per XG / XLG line of
// pursuit_to_specializations.def
template <class S>
void group_to_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s);

// ... and of a THGShape / TLHGShape kernel (binary16 buffers: io.obs and io.obs_prev are the half pointers, cast): explicitly instantiated
// in pursuit_to_group_f16.hip (HG lines) and pursuit_to_group_f16_live.hip (HLG lines of pursuit_to_f16_group_specializations.def)
template <class S>
void group_to_f16_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s);

// host launcher of an LGShape kernel: explicitly instantiated in pursuit_live_group.hip, one per XLG line, so that these kernels
// compile in a translation unit of their own
template <class S>
void live_group_launch(const WaveDev &d, const WaveIO &io, int mode, int64_t blocks, hipStream_t s);

// LDS-only workgroup barrier: the DS queue of this wavefront is drained, global stores stay in flight.
__device__ __forceinline__ void group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The global reward under S::LEAN_REGS: the sums of pursuit_wave.hpp over the lanes of wavefront 0 (lane k = pursuer k) instead of over an
// array of P doubles.  The same additions in the same order, but the values are fetched eight lanes at a time and the scheduler cannot
// gather all P of them -- 2 P registers -- before the first addition: at 46 and 64 pursuers the float32 kernels spill there.
// lane k's value by its constant byte address (two ds_bpermute; __shfl would keep `lane & 64` as a loop constant)
__device__ __forceinline__ double lane_val(double v, int k) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * k, (int)(uint32_t)b);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * k, (int)(uint32_t)(b >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// np_sum_regs over lanes 0 .. P - 1
template <int P>
__device__ __forceinline__ double np_sum_lanes(double v) {
    if constexpr (P < 8) {
        double res = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) res += lane_val(v, i);
        return res;
    } else {
        double r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = lane_val(v, k);
        constexpr int LIM = P - (P % 8);
#pragma unroll
        for (int i = 8; i < LIM; i += 8) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 8; ++k) r[k] += lane_val(v, i + k);
        }
        __builtin_amdgcn_sched_barrier(0);
        double res = pairwise8(r);
#pragma unroll
        for (int i = LIM; i < P; ++i) res += lane_val(v, i);
        return res;
    }
}
// np_sum_first over lanes 0 .. n - 1 (n <= P, wave-uniform): a block of eight below lim = n - n % 8 goes into the eight partial sums, the
// block at lim is kept and its first n % 8 values are added one by one after the pairwise step, as np_sum_first does
template <int P>
__device__ __forceinline__ double np_sum_first_lanes(double v, int n) {
    double res = 0.0;
    if (n < 8) {
#pragma unroll
        for (int i = 0; i < (P < 8 ? P : 7); ++i)
            if (i < n) res += lane_val(v, i);
        return res;
    }
    if constexpr (P >= 8) {
        double r[8], t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            r[k] = lane_val(v, k);
            t[k] = 0.0;
        }
        const int lim = n - (n % 8);
#pragma unroll
        for (int i = 8; i < P; i += 8) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (i + k < P) {
                    const double a = lane_val(v, i + k);
                    if (i < lim) r[k] += a;    // (then i + 8 <= lim <= P: a whole block)
                    if (i == lim) t[k] = a;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        res = pairwise8(r);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < n - lim) res += t[k];
    }
    return res;
}

// Stands where a row pass addresses float4 slots (16 bytes at q * 16, elements 4 bytes apart): float32 geometry, which would run past the
// end of a binary16 buffer.  H16: the caller's shape holds binary16 buffers -- refused here, wherever the call stands (as
// store_slot_masked does in pursuit_wave.hpp): an H16 shape runs its in-place pass through half_slot_in_place.
template <bool H16>
__device__ __forceinline__ constexpr void float32_slots_only() {
    static_assert(!H16, "float32 geometry: an H16 shape runs its in-place pass through half_slot_in_place");
}

template <class S, int MODE, bool INJECT>
__global__ __launch_bounds__(S::NT) __attribute__((amdgpu_waves_per_eu(S::OCC, S::OCC))) void pursuit_group_kernel(const WaveDev d, const WaveIO io) {
    constexpr int P = S::P, E = S::E, A = S::A, GW = S::GW, PAD = S::PAD, GSZ = S::GSZ, NS = S::NS, NT = S::NT;
    static_assert(!S::TO || (MODE == 1 && INJECT), "the two-buffer step: the flexible step kernel only");
    static_assert(!S::H16 || S::TO, "binary16 buffers: the two-buffer step only");
    // an env's rows in the float-sized units of io.obs / io.obs_prev (binary16 buffers, S::H16: half as many bytes)
    constexpr int64_t ROW = P * S::D / (S::H16 ? 2 : 1);
    __shared__ __attribute__((aligned(16))) uint32_t L[S::LDS_DWORDS];
    const int tid = threadIdx.x;            // = agent index for tid < A
    const int lane = tid & 63;
    const uint32_t utid = threadIdx.x, ulane = utid & 63u;  // unsigned 32-bit indices: SGPR base + VGPR offset addressing
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool is_p = tid < P;
    const int eslot = tid - P;

    // ---------------------------------------------------------------- once per workgroup
    // The tables, the slot constants and the first env's record, action and masks in one batch of loads with one wait ("table staging",
    // pursuit_wave.hpp; map 0 is staged with the tables as there) -- in two where they do not fit FILL_FIRST registers.  The
    // group_sync before the env loop publishes the LDS writes.  The per-env-counts kernels (LIVE) stage tables and slot constants the
    // same way and fetch their first env as a batch of its own after it: with that fetch in the first batch they compile to a 36-byte
    // stack frame at every batch size down to 4 trips (tests/test_live_counts_group_isa.py forbids one).
    using F = Fill<S, NT>;
    constexpr int NSR = S::TABLED ? 1 : NS;   // slots whose constants live in registers
    constexpr int NSL = S::TABLED ? 0 : NS;   // ... and are loaded here
    constexpr int MW = S::MWORDS;
    if (d.n_envs <= 0) return;   // (the batched start-up fetches an env unconditionally)
    const uint32_t *const vtab_u = reinterpret_cast<const uint32_t *>(d.vtab);   // (TABLED: d.slot_tab is the [DV][2] table of packed offsets, a fill of its own)
    constexpr int ROOM = FILL_FIRST - 6 * NSL - 2 - MW;
    constexpr int JF = F::J_END < (ROOM > 4 ? ROOM : 4) ? F::J_END : (ROOM > 4 ? ROOM : 4);
    int s_cst[NSR][4];
    int s_rel3[NSR];
    int s_org[NSR];    // LDS index of the owning pursuer's window origin
    uint32_t cur_rec = 0, cur_zm[MW];
#pragma unroll
    for (int w = 0; w < MW; ++w) cur_zm[w] = 0xFFFFFFFFu;
    int cur_act = 4;
    {
        uint32_t st[JF], sraw[6 * NSL + 1];
        static_for<0, JF>([&](auto jc) { st[decltype(jc)::value] = fill_load<S, NT, decltype(jc)::value>(utid, d.cnt_tmpl, d.fmaps, vtab_u, d.slot_tab); });
#pragma unroll
        for (int k = 0; k < 6 * NSL; ++k) sraw[k] = d.slot_tab[(uint32_t)NT * k + utid];  // host-built (pursuit.hip), see WaveDev: [NS][6][NT]
        // the first env of this workgroup (a workgroup without one fetches the last env's and never looks at it); every thread loads, from
        // clamped offsets
        __builtin_amdgcn_sched_barrier(0);  // these stay the loads issued last
        if constexpr (!S::LIVE) {
            const int ne0 = (int)d.n_envs, e0 = (int)blockIdx.x < ne0 ? (int)blockIdx.x : ne0 - 1;
            const int64_t env0 = (int64_t)(d.reverse ? ne0 - 1 - e0 : e0);
            const uint32_t rec_off = (ulane < (uint32_t)S::REC_DW ? ulane : (uint32_t)S::REC_DW - 1u) * 4u;
            const uint32_t act_off = (utid < (uint32_t)P ? utid : (uint32_t)P - 1u) * 4u;
            cur_rec = *reinterpret_cast<const uint32_t *>(d.state + env0 * (int64_t)S::REC_BYTES + rec_off);
            if constexpr (MODE == 1) cur_act = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(io.actions + env0 * P) + act_off);
#pragma unroll
            for (int w = 0; w < MW; ++w) {
                if (w == MW - 1) __builtin_amdgcn_sched_barrier(0);
                cur_zm[w] = d.zmask[(env0 * MW + w) * NT + utid];
            }
        }
        if constexpr (!S::LIVE) {
            staged_wait<MW>(cur_zm);  // the loads issued last: the one wait, vmcnt(0), of the whole batch
            asm volatile("" : "+v"(cur_rec), "+v"(cur_act));
        }
        staged_wait<6 * NSL>(sraw);
        staged_wait<JF>(st);
        static_for<0, JF>([&](auto jc) { fill_store<S, NT, decltype(jc)::value, true>(L, utid, st[decltype(jc)::value]); });
        fill_trips<S, NT, JF, F::J_END, FILL_BATCH, true>(L, utid, d.cnt_tmpl, d.fmaps, vtab_u, d.slot_tab);
        if (tid < P) L[S::X_ID + tid] = __float_as_uint((float)((double)tid / (double)P));
        if constexpr (!S::LIVE) {
            if (ulane >= (uint32_t)S::REC_DW) cur_rec = 0u;
            if (!is_p) cur_act = 4;
        }
        if constexpr (!S::TABLED) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
#pragma unroll
                for (int k = 0; k < 4; ++k) s_cst[s][k] = (int)sraw[6 * s + k];
                s_rel3[s] = (int)sraw[6 * s + 4];
                s_org[s] = S::X_ORG + (int)sraw[6 * s + 5];
            }
        }
    }
    const int q0_p = tid / S::DV, q0_f = tid % S::DV;   // TABLED: (pursuer, float4 position in its row) of this thread's slot 0
    int cached_map = 0;
    int cached_np = P;  // LIVE: the pursuer count the id cells X_ID.. hold (k / np, :440-445)
    const uint8_t *need_tab = reinterpret_cast<const uint8_t *>(&L[S::X_NEED]);
    uint32_t *const layer = &L[is_p ? GSZ : 2 * GSZ];
    // record dword k (held by lane k of every wavefront) is STORED by one wavefront: the agent-pair dwords by the
    // wavefront that holds the two agents, the terminal words by the wavefront whose lanes they describe, the
    // rest (header, alive mask, padding) by wavefront 0
    constexpr int XY_END = 4 + (A + 1) / 2;
    const bool own_xy = lane >= 4 && lane < XY_END && (lane - 4) / 32 == wv;
    const bool own_term = lane >= S::OFF_TERM / 4 && lane < S::OFF_TERM / 4 + S::NTW && (lane - S::OFF_TERM / 4) / 2 == wv;
    const bool own_rest = wv == 0 && lane < S::REC_DW && !(lane >= 4 && lane < XY_END) &&
                          !(lane >= S::OFF_TERM / 4 && lane < S::OFF_TERM / 4 + S::NTW);
    const bool own_dw = own_xy || own_term || own_rest;
    const int rec_src0 = (own_xy ? 2 * (lane - 4) - 64 * wv : 0) * 4, rec_src1 = rec_src0 + 4;

    auto isP = [&]() { return fresh(tid) < P; };
    auto isE = [&]() { return (unsigned)(fresh(tid) - P) < (unsigned)E; };
    auto isAgent = [&]() { return fresh(tid) < A; };
    auto fetch_rec = [&](int64_t env) -> uint32_t {
        return (fresh(lane) < S::REC_DW) ? uniform_ptr(reinterpret_cast<const uint32_t *>(d.state + env * (int64_t)S::REC_BYTES))[ulane] : 0u;
    };
    auto fetch_act = [&](int64_t env) -> int {
        if constexpr (MODE == 1) return isP() ? uniform_ptr(io.actions + env * P)[utid] : 4;
        else return 4;
    };
    // evader-slot mask of a wave-wide predicate, combined over the wavefronts that hold agents and handed to EVERY wavefront of the group
    // -- also when one wavefront holds all agents (NAW == 1, long rows: 30 v 30 on four wavefronts): the others must learn of this step's
    // catches too, or they miss an episode that ends by its last catch, skip the fused reset's second pass and leave the group's barriers
    auto evader_mask = [&](bool pred) -> uint64_t {
        static_assert(S::NW >= 2 && S::NAW <= 2, "the exchange reads the words of wavefronts 0 and 1");
        const uint64_t b = __ballot(pred);
        // (64 pursuers: wavefront 0 holds no evader -- and a 64-bit shift by 64 is not defined)
        const uint64_t mine = (wv == 0) ? (P < 64 ? (b >> (P & 63)) : 0ull) : ((wv == 1) ? (b << ((64 - P) & 63)) : 0ull);
        if (lane == 0) {
            L[S::X_XCH + 2 * wv] = (uint32_t)mine;
            L[S::X_XCH + 2 * wv + 1] = (uint32_t)(mine >> 32);
        }
        group_sync();
        const uint32_t a0 = L[S::X_XCH], a1 = L[S::X_XCH + 1], b0 = L[S::X_XCH + 2], b1 = L[S::X_XCH + 3];
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(a0 | b0));
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(a1 | b1));
        return ((uint64_t)hi << 32) | lo;
    };
    auto fetch_zm = [&](int64_t env, uint32_t (&zmw)[MW]) {   // stale-zero masks, pursuit_wave.hpp: [env][MWORDS][NT]
#pragma unroll
        for (int w = 0; w < MW; ++w) zmw[w] = uniform_ptr(d.zmask + (env * MW + w) * NT)[utid];
    };
    // env indices are 32-bit (the fast path is not taken for n_envs >= 2^31 - 2^20), byte offsets 64-bit
    const int n_envs = (int)d.n_envs, stride = (int)gridDim.x;
    auto phys = [&](int e) -> int64_t { return (int64_t)(d.reverse ? n_envs - 1 - e : e); };
    if constexpr (S::LIVE) {   // the first env, a batch of its own (see the start-up above)
        if ((int)blockIdx.x < n_envs) {
            cur_rec = fetch_rec(phys(blockIdx.x));
            cur_act = fetch_act(phys(blockIdx.x));
            fetch_zm(phys(blockIdx.x), cur_zm);
        }
        asm volatile("" : "+v"(cur_rec), "+v"(cur_act));
#pragma unroll
        for (int w = 0; w < MW; ++w) asm volatile("" : "+v"(cur_zm[w]));
    }
    group_sync();

    for (int e = blockIdx.x; e < n_envs; e += stride) {
        const int64_t env = phys(e);
        const bool has_next = e + stride < n_envs;
        const int64_t nenv = phys(has_next ? e + stride : e);
        uint32_t nxt_rec = 0, nxt_zm[MW];
#pragma unroll
        for (int w = 0; w < MW; ++w) nxt_zm[w] = 0xFFFFFFFFu;
        int nxt_act = 4;
        if (has_next) {
            nxt_rec = fetch_rec(nenv);
            nxt_act = fetch_act(nenv);
            fetch_zm(nenv, nxt_zm);
        }
        bool skip = false;
        if constexpr (MODE == 0) skip = (io.mask != nullptr && io.mask[env] == 0);
        if (!skip) {
            // -------------------------------------------------------- unpack the record
            uint32_t tick = __builtin_amdgcn_readlane(cur_rec, 0);
            int32_t tstep = (int32_t)__builtin_amdgcn_readlane(cur_rec, 1);
            int32_t map_id = (int32_t)__builtin_amdgcn_readlane(cur_rec, 2);
            const uint32_t xyw = (uint32_t)__shfl((int)cur_rec, (4 + (tid >> 1)) & 63);
            const pr::Cell at = pr::unpack_xy(xyw, tid & 1);
            int x = at.x, y = at.y;
            if (!isAgent()) x = y = 0;  // threads past the last agent keep a harmless in-map cell
            uint64_t gone = (uint32_t)__builtin_amdgcn_readlane(cur_rec, S::OFF_GONE / 4);  // (uint32_t): readlane returns int, bit 31 must not sign-extend
            if constexpr (S::NGW > 1) gone |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane(cur_rec, S::OFF_GONE / 4 + 1) << 32;
            // terminal flags of THIS wavefront's lanes (record words 2 wv, 2 wv + 1)
            uint64_t term = 0ull;
            {
                const uint32_t tw = (uint32_t)__shfl((int)cur_rec, (S::OFF_TERM / 4 + 2 * wv + (lane & 1)) & 63);
                const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane(tw, 0), t1 = (uint32_t)__builtin_amdgcn_readlane(tw, 1);
                if (2 * wv < S::NTW) term = t0;
                if (2 * wv + 1 < S::NTW) term |= (uint64_t)t1 << 32;
            }
            const uint32_t gid = d.gid_base + (uint32_t)env;
            const uint32_t k0 = fresh_s(d.k0), k1 = fresh_s(d.k1);
            int np = P, ne = E;  // live pursuers / evader slots (LIVE; the capacity otherwise)
            if constexpr (S::LIVE) {
                // from the record, which every wavefront holds whole: dword 4 + j = agents 2j (low half) and 2j + 1 (high half)
                const int a0 = 2 * (lane - 4);
                const bool in_xy = lane >= 4 && lane < XY_END;
                const bool h0 = in_xy && (cur_rec & 0xFFu) != (uint32_t)NOT_HERE;
                const bool h1 = in_xy && a0 + 1 < A && ((cur_rec >> 16) & 0xFFu) != (uint32_t)NOT_HERE;
                np = __popcll(__builtin_amdgcn_ballot_w64(h0 && a0 < P)) + __popcll(__builtin_amdgcn_ballot_w64(h1 && a0 + 1 < P));
                ne = __popcll(__builtin_amdgcn_ballot_w64(h0 && a0 >= P)) + __popcll(__builtin_amdgcn_ballot_w64(h1 && a0 + 1 >= P));
                if (x == NOT_HERE) {  // a slot that does not exist computes on cell (0, 0) and never stores there
                    x = 0;
                    y = 0;
                }
            }
            // a pursuer of the running episode (LIVE: tid < np)
            auto isLP = [&]() {
                if constexpr (S::LIVE) return fresh(tid) < np;
                else return isP();
            };
            bool do_reset = (MODE == 0);
            uint32_t done_bits = 0;
            float rew_out = 0.0f;
            int n_removed = 0;
            bool alive = isLP() || (isE() && !((gone >> (eslot & 63)) & 1ull));
            int cell = (x + PAD) * GW + y + PAD;

            auto load_map = [&](int mid) {
                if (cached_map == mid) return;
                const KArgsPtr ka = cold_args();  // rare-path launch parameters come from the kernarg segment (pursuit_wave.hpp)
                // the map layer and its need bytes in batches of at most FILL_BATCH trips (the slot constants are live here): per batch all
                // loads, one wait to zero, then the LDS writes (table staging).  One batch up to 16 trips: 14 at C5 (32 x 32 on two
                // wavefronts), 8 at the authors' shape
                fill_trips<S, NT, F::J_MAP, F::J_VT, FILL_BATCH, false>(L, utid, nullptr, ka->d.fmaps + (int64_t)mid * ka->d.fmap_stride, nullptr, nullptr);
                cached_map = mid;
                group_sync();
            };
            load_map(map_id);

            if constexpr (MODE == 1) {
                const bool e_alive = alive && !isP();
                // ---------------------------------------------------- pre-move reward (:359-381)
                if (e_alive) atomicAdd(&layer[cell], 1u);
                group_sync();
                int kpre = 0;
                if (isP()) {
                    const pr::Clip4 n = pr::clipped_neighbours<GW, S::XS, S::YS>(x, y);
                    const uint32_t *ec = &L[2 * GSZ];
                    kpre = (int)(ec[cell - n.dxm] + ec[cell + n.dxp] + ec[cell + n.dyp] + ec[cell - n.dym]);
                }
                group_sync();
                if (e_alive) atomicSub(&layer[cell], 1u);
                // ---------------------------------------------------- moves (:229-241)
                const int kidx = __popcll((~gone) & ((1ull << (eslot & 63)) - 1ull));
                int act = cur_act;
                bool injected = false;
                if constexpr (INJECT) {   // the FLEX instantiation, see pursuit_wave.hpp
                    injected = io.inj_eact != nullptr;
                    if (injected && e_alive) act = io.inj_eact[env * E + kidx];
                }
                if (!injected) {
                    const u32x4 r = philox4x32_10(gid, tick, (uint32_t)kidx, TAG_EVADER_ACT, k0, k1);
                    if (!isP()) act = (int)__umulhi(r.x, 5u);
                }
                const int dcell = pr::move_dcell<GW>(act);
                const bool tflag = (term >> lane) & 1ull;
                const bool in_building = L[cell] != 0u;
                const bool target_free = L[cell + dcell] == 0u;
                const bool newterm = alive && !tflag && in_building;
                if (alive && !tflag && !in_building && target_free) {
                    cell += dcell;
                    x += pr::move_dx(act), y += pr::move_dy(act);
                }
                term |= __ballot(newterm);
                if (alive) atomicAdd(&layer[cell], 1u);
                group_sync();
                // ---------------------------------------------------- catch resolution (:463-521)
                bool caught = false;
                if (e_alive) {
                    const uint32_t *pc = &L[GSZ];
                    if (d.surround) caught = pr::cells_with_pursuers(pc[cell - GW], pc[cell + GW], pc[cell + 1], pc[cell - 1], SENT) == (int)need_tab[x * S::YS + y];  // :523-540
                    else caught = (int)pc[cell] >= d.n_catch;
                    if (caught) atomicAdd(&layer[cell], CAUGHT);
                }
                const uint64_t caught_mask = evader_mask(caught);  // contains the barrier for the CAUGHT marks
                gone |= caught_mask;
                // ---------------------------------------------------- rewards (:254-262)
                double r = 0.0;
                if (isLP()) {
                    const uint32_t *ec = &L[2 * GSZ];
                    bool sur;
                    if (d.surround) sur = pr::caught_beside(ec[cell - GW], ec[cell + GW], ec[cell + 1], ec[cell - 1], SENT, CAUGHT);
                    else sur = ec[cell] >= CAUGHT;
                    double catchr = d.catchr;
                    if constexpr (INJECT) { if (d.catchr_env != nullptr) catchr = sload_f64(d.catchr_env, env); }
                    r = pr::pursuer_reward(catchr, kpre, d.term_pursuit, sur, d.urgency);
                }
                if (d.reward_global && wv == 0) {
                    if constexpr (S::LEAN_REGS) {   // the same sums over the lanes, eight at a time (np_sum_lanes above)
                        if constexpr (S::LIVE) r = isLP() ? np_sum_first_lanes<P>(r, np) / (double)np : 0.0;
                        else r = np_sum_lanes<P>(r) / (double)P;
                    } else {
                    double all[P];
#pragma unroll
                    for (int k = 0; k < P; ++k) all[k] = __shfl(r, k);
                    if constexpr (S::LIVE) r = isLP() ? np_sum_first<P>(all, np) / (double)np : 0.0;
                    else r = np_sum_regs<P>(all) / (double)P;
                    }
                }
                tick += 1;
                tstep += 1;
                constexpr uint64_t all_e = E >= 64 ? ~0ull : ((1ull << (E & 63)) - 1ull);
                if ((gone & all_e) == all_e) done_bits |= 1u;
                if (d.max_steps > 0 && tstep >= d.max_steps) done_bits |= 2u;
                do_reset = d.auto_reset && done_bits != 0;
                rew_out = (float)r;
                n_removed = __popcll(caught_mask);
            }

            asm volatile("" : "+v"(nxt_rec), "+v"(nxt_act));  // pipeline hinge (pursuit_wave.hpp)
            uint32_t zm[MW];
#pragma unroll
            for (int w = 0; w < MW; ++w) {
                asm volatile("" : "+v"(nxt_zm[w]));
                zm[w] = cur_zm[w];
            }

            const int npass = (MODE == 1 && do_reset) ? 2 : 1;
            for (int pass = 0; pass < npass; ++pass) {
                if (do_reset && pass == npass - 1) {
                    // -------------------------------------------------- reset (:173-207)
                    gone = 0ull;
                    term = 0ull;
                    const KArgsPtr ka = cold_args();
                    const double cw = ka->d.cw_env != nullptr ? sload_f64(ka->d.cw_env, env) : ka->d.cw;
                    const int max_opponents = ka->d.max_opponents;
                    bool inj_map = false, inj_pos = false;
                    if constexpr (MODE == 0) {
                        inj_map = io.inj_map != nullptr;
                        inj_pos = io.inj_pos != nullptr;
                    }
                    if (inj_map) {
                        map_id = __builtin_amdgcn_readfirstlane(io.inj_map[env]);
                    } else if (ka->d.sample_maps) {
                        const u32x4 rm = philox4x32_10(gid, tick, 0u, TAG_RESET_ENV, k0, k1);
                        map_id = (int)__umulhi(rm.x, (uint32_t)ka->d.n_maps);
                    }
                    load_map(map_id);
                    const pr::Window win = pr::reset_window(gid, tick, k0, k1, cw, S::XS, S::YS);
                    int n_create = E;
                    if constexpr (S::LIVE) {  // the pending counts take effect
                        const pr::Counts live = pr::clamp_pending(pending_count(env, 0), pending_count(env, 1), P, E);
                        np = live.np, ne = n_create = live.ne;
                    }
                    if (max_opponents > 0 && !inj_pos) n_create = pr::reset_n_create(gid, tick, k0, k1, max_opponents, S::LIVE ? ne : E);
                    bool exists = false;
                    if (isAgent()) {
                        if constexpr (S::LIVE) exists = isLP() || (!isP() && eslot < n_create);
                        else exists = isP() || eslot < n_create;
                        if (inj_pos) {
                            x = io.inj_pos[(env * A + tid) * 2];
                            y = io.inj_pos[(env * A + tid) * 2 + 1];
                            if (!isP() && x < 0) exists = false;
                        } else {
                            for (uint32_t att = 0; att < 1024u; ++att) {
                                const uint32_t aidx = S::LIVE ? (uint32_t)(isP() ? tid : np + eslot) : (uint32_t)tid;
                                const pr::Cell c = pr::reset_cell(gid, tick, aidx, att, k0, k1, win);
                                x = c.x, y = c.y;
                                if (L[(x + PAD) * GW + y + PAD] == 0u) break;
                            }
                        }
                        if (exists) {
                            cell = (x + PAD) * GW + y + PAD;
                            atomicAdd(&layer[cell], 1u);
                        } else {
                            x = 0;
                            y = 0;
                        }
                    }
                    gone = evader_mask(isE() && !exists);
                    alive = exists;
                    tick += 1;
                    tstep = 0;
                }
                // ------------------------------------------------------ observations (:418-461)
                if constexpr (S::LIVE) {  // the id values k / np of this pass's pursuer count (np is the same in every wavefront; the
                    if (np != cached_np) {  // two barriers below publish the cells before the row pass reads them)
                        if (tid < P) L[S::X_ID + tid] = __float_as_uint((float)((double)tid / (double)np));
                        cached_np = np;
                    }
                }
                uint32_t cnt = 0;
                if (alive) cnt = layer[cell] & 0xFFFFu;
                group_sync();
                if (alive) layer[cell] = L[S::X_VTAB + cnt];
                // window origin of pursuer tid: a dword index into L (a byte offset for TABLED shapes)
                if (isP()) L[S::X_ORG + tid] = (uint32_t)((x - S::OFF + PAD) * GW + (y - S::OFF + PAD)) * (S::TABLED ? 4u : 1u);
                group_sync();
                bool in_place = true;   // the in-place row pass; false: this pass was the two-buffer pass below
                if constexpr (S::TO) {
                    if (pass == 0) {
                        // ------------------------------------------------ the two-buffer pass: every valid float4 leaves whole, into io.obs
                        in_place = false;
                        typedef float v4f __attribute__((ext_vector_type(4)));
                        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                        typedef uint32_t v2u __attribute__((ext_vector_type(2)));
                        // a slot in memory: a float4 -- binary16 buffers: four halves in one 8-byte word, two per dword
                        using old_t = std::conditional_t<S::H16, v2u, v4u>;
                        using slot_t = std::conditional_t<S::H16, v2u, v4f>;
                        slot_t *orow = reinterpret_cast<slot_t *>(io.obs + env * ROW);
                        const old_t *prow = reinterpret_cast<const old_t *>(io.obs_prev + env * ROW);
                        const old_t no_old = {};   // (zeros)
                        uint32_t acc[MW];
#pragma unroll
                        for (int w = 0; w < MW; ++w) acc[w] = 0u;
                        // the elements of a slot (one flag per byte) that come from io.obs_prev: what the in-place pass leaves alone -- outside
                        // cells not known to be zero, and the whole row of an absent pursuer (LIVE)
                        auto need_of = [&](auto wc, int sh, bool row_live, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) -> uint32_t {
                            constexpr int w = decltype(wc)::value;
                            const uint32_t top = __builtin_amdgcn_perm(v1, v0, 0x0C0C0703u) | __builtin_amdgcn_perm(v3, v2, 0x07030C0Cu);
                            const uint32_t dirty = (top >> 7) & (zm[w] >> sh) & 0x01010101u;
                            if constexpr (S::LIVE) return row_live ? dirty : 0x01010101u;
                            else return dirty;
                        };
                        // one slot: the kept elements from `oldv` (zeros in a lane that loaded nothing: it keeps nothing), the others from the
                        // layers -- outside cells known to be zero as +0.0 -- and the slot's new mask bits: a stored element as in the in-place
                        // pass, a kept one "the loaded value is non-zero"
                        auto emit = [&](auto wc, int sh, int q, bool valid, bool row_live, const old_t oldv, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
                            constexpr int w = decltype(wc)::value;
                            const uint32_t top = __builtin_amdgcn_perm(v1, v0, 0x0C0C0703u) | __builtin_amdgcn_perm(v3, v2, 0x07030C0Cu);
                            const uint32_t out4 = (top >> 7) & 0x01010101u;
                            const uint32_t nz4 = ((top >> 5) | (top >> 6)) & 0x01010101u;
                            const uint32_t old4 = (zm[w] >> sh) & 0x01010101u;
                            if constexpr (!S::LIVE) row_live = true;
                            const uint32_t need4 = row_live ? (out4 & old4) : 0x01010101u;
                            if constexpr (S::H16) {
                                // per half: "the loaded 16 bits are non-zero"
                                const uint32_t oldnz = ((oldv.x & 0xFFFFu) != 0u ? 0x00000001u : 0u) | ((oldv.x >> 16) != 0u ? 0x00000100u : 0u) |
                                                       ((oldv.y & 0xFFFFu) != 0u ? 0x00010000u : 0u) | ((oldv.y >> 16) != 0u ? 0x01000000u : 0u);
                                acc[w] = (acc[w] << 1) | (row_live ? (~out4 & nz4) : 0u) | (need4 & (valid ? oldnz : old4));
                                if (valid) {
                                    // converted and packed; the kept halves come from the old word, 16 bits as they are
                                    auto hb = [](uint32_t v) -> uint32_t { return half_bits(__uint_as_float((uint32_t)max((int)v, 0))); };
                                    uint32_t lo = hb(v0) | (hb(v1) << 16), hi = hb(v2) | (hb(v3) << 16);
                                    const uint32_t klo = ((need4 & 0x00000001u) ? 0x0000FFFFu : 0u) | ((need4 & 0x00000100u) ? 0xFFFF0000u : 0u);
                                    const uint32_t khi = ((need4 & 0x00010000u) ? 0x0000FFFFu : 0u) | ((need4 & 0x01000000u) ? 0xFFFF0000u : 0u);
                                    lo = (lo & ~klo) | (oldv.x & klo);
                                    hi = (hi & ~khi) | (oldv.y & khi);
                                    __builtin_nontemporal_store(v2u{lo, hi}, &orow[q]);
                                }
                            } else {
                            const uint32_t oldnz = (oldv.x != 0u ? 0x00000001u : 0u) | (oldv.y != 0u ? 0x00000100u : 0u) |
                                                   (oldv.z != 0u ? 0x00010000u : 0u) | (oldv.w != 0u ? 0x01000000u : 0u);
                            // (a thread past the end of the rows stores and loads nothing: its bits stay what the in-place pass makes them)
                            acc[w] = (acc[w] << 1) | (row_live ? (~out4 & nz4) : 0u) | (need4 & (valid ? oldnz : old4));
                            if (valid) {
                                uint32_t w0 = (uint32_t)max((int)v0, 0), w1 = (uint32_t)max((int)v1, 0);
                                uint32_t w2 = (uint32_t)max((int)v2, 0), w3 = (uint32_t)max((int)v3, 0);
                                if (need4 & 0x00000001u) w0 = oldv.x;
                                if (need4 & 0x00000100u) w1 = oldv.y;
                                if (need4 & 0x00010000u) w2 = oldv.z;
                                if (need4 & 0x01000000u) w3 = oldv.w;
                                const v4f val = {__uint_as_float(w0), __uint_as_float(w1), __uint_as_float(w2), __uint_as_float(w3)};
                                __builtin_nontemporal_store(val, &orow[q]);
                            }
                            }
                        };
                        // Batches of slots.  Part 1: which lanes keep an element of which slot (the values are read from LDS again in part 2:
                        // keeping them across the loads would cost four registers per slot).  Part 2: the batch's loads, all issued before
                        // its first store -- and none, and no wait, in a wavefront none of whose lanes keeps anything -- then its stores.
                        if constexpr (S::TABLED) {
                            int pq = q0_p, fq = q0_f, q = tid;
                            const char *Lb = reinterpret_cast<const char *>(L);
                            auto cell_b = [&](int byte_off) -> uint32_t { return *reinterpret_cast<const uint32_t *>(Lb + byte_off); };
                            auto read_slot = [&](int pp, int f, uint32_t &v0, uint32_t &v1, uint32_t &v2, uint32_t &v3) {   // as the in-place loop below
                                const uint2 t = *reinterpret_cast<const uint2 *>(&L[S::X_TAB + 2 * f]);
                                const int base = (int)L[S::X_ORG + pp];
                                v0 = cell_b(base + (int)((t.x & 0xFFFFu) << 2));
                                v1 = cell_b(base + (int)((t.x >> 16) << 2));
                                v2 = cell_b(base + (int)((t.y & 0x7FFFu) << 2));
                                const int b3 = ((int)t.y < 0) ? 0 : base;
                                const int id3 = (t.y & 0x8000u) ? pp : 0;
                                v3 = cell_b(b3 + (int)((((t.y >> 16) & 0x7FFFu) + (uint32_t)id3) << 2));
                            };
                            auto advance = [&](int &aq, int &af, int &ap) {
                                aq += NT;
                                af += NT % S::DV;
                                ap += NT / S::DV;
                                if (af >= S::DV) { af -= S::DV; ap += 1; }
                            };
                            static_for<0, MW>([&](auto wc) {
                                constexpr int w = decltype(wc)::value, nsw = (NS - 8 * w) < 8 ? (NS - 8 * w) : 8;
                                constexpr int B = MADRL_PG_TO_BATCH < nsw ? MADRL_PG_TO_BATCH : nsw;
                                auto batch = [&](auto nbc, int i0) {   // slots i0 .. i0 + nb - 1 of mask word w
                                    constexpr int nb = decltype(nbc)::value;
                                    uint32_t need[nb], any = 0u;
                                    {
                                        int bq = q, bf = fq, bp = pq;
#pragma unroll
                                        for (int j = 0; j < nb; ++j) {
                                            const bool valid = bq < S::NQ;
                                            const int pp = valid ? bp : 0;
                                            uint32_t v0, v1, v2, v3;
                                            read_slot(pp, bf, v0, v1, v2, v3);
                                            need[j] = valid ? need_of(wc, nsw - 1 - (i0 + j), pp < np, v0, v1, v2, v3) : 0u;
                                            any |= need[j];
                                            advance(bq, bf, bp);
                                        }
                                    }
                                    auto stores = [&](const old_t (&old)[nb]) {
#pragma unroll
                                        for (int j = 0; j < nb; ++j) {
                                            const bool valid = q < S::NQ;
                                            const int pp = valid ? pq : 0;
                                            uint32_t v0, v1, v2, v3;
                                            read_slot(pp, fq, v0, v1, v2, v3);
                                            emit(wc, nsw - 1 - (i0 + j), q, valid, pp < np, old[j], v0, v1, v2, v3);
                                            advance(q, fq, pq);
                                        }
                                    };
                                    old_t old[nb];
#pragma unroll
                                    for (int j = 0; j < nb; ++j) old[j] = no_old;
                                    if (__builtin_amdgcn_ballot_w64(any != 0u) != 0ull) {
#pragma unroll
                                        for (int j = 0; j < nb; ++j)
                                            if (need[j] != 0u) old[j] = prow[q + NT * j];
                                        stores(old);
                                    } else {
                                        stores(old);
                                    }
                                };
#pragma unroll 1
                                for (int i = 0; i + B <= nsw; i += B) batch(std::integral_constant<int, B>{}, i);
                                if constexpr (nsw % B != 0) batch(std::integral_constant<int, nsw % B>{}, nsw - nsw % B);
                            });
                        } else {
                            // (slot constants in registers: short rows.  The live form with five or more slots has no register to spare: one slot at a time)
                            constexpr int TG = (S::LIVE && NS > 4) ? 1 : (MADRL_PG_TO_RBATCH < NS ? MADRL_PG_TO_RBATCH : NS);
                            auto read_slot = [&](auto sc, uint32_t &v0, uint32_t &v1, uint32_t &v2, uint32_t &v3) {
                                constexpr int s = decltype(sc)::value;
                                const int base = (int)L[s_org[s]];
                                v0 = L[base + s_cst[s][0]];
                                v1 = L[base + s_cst[s][1]];
                                v2 = L[base + s_cst[s][2]];
                                v3 = L[(int)__umul24((uint32_t)base, (uint32_t)s_rel3[s]) + s_cst[s][3]];
                            };
                            auto valid_of = [&](auto sc) -> bool {
                                constexpr int s = decltype(sc)::value;
                                return (NT * (s + 1) <= S::NQ) ? true : (fresh(tid) + NT * s < S::NQ);
                            };
                            static_for<0, (NS + TG - 1) / TG>([&](auto gc) {
                                constexpr int g0 = decltype(gc)::value * TG, g1 = g0 + TG < NS ? g0 + TG : NS;
                                uint32_t need[TG], any = 0u;
                                static_for<g0, g1>([&](auto sc) {
                                    constexpr int s = decltype(sc)::value;
                                    uint32_t v0, v1, v2, v3;
                                    read_slot(sc, v0, v1, v2, v3);
                                    need[s - g0] = valid_of(sc) ? need_of(std::integral_constant<int, 0>{}, NS - 1 - s, s_org[s] - S::X_ORG < np, v0, v1, v2, v3) : 0u;
                                    any |= need[s - g0];
                                });
                                auto stores = [&](const old_t (&old)[TG]) {
                                    static_for<g0, g1>([&](auto sc) {
                                        constexpr int s = decltype(sc)::value;
                                        uint32_t v0, v1, v2, v3;
                                        read_slot(sc, v0, v1, v2, v3);
                                        emit(std::integral_constant<int, 0>{}, NS - 1 - s, tid + NT * s, valid_of(sc), s_org[s] - S::X_ORG < np, old[s - g0], v0, v1, v2, v3);
                                    });
                                };
                                old_t old[TG];
#pragma unroll
                                for (int j = 0; j < TG; ++j) old[j] = no_old;
                                if (__builtin_amdgcn_ballot_w64(any != 0u) != 0ull) {
                                    static_for<g0, g1>([&](auto sc) {
                                        constexpr int s = decltype(sc)::value;
                                        if (need[s - g0] != 0u) old[s - g0] = prow[tid + NT * s];
                                    });
                                    stores(old);
                                } else {
                                    stores(old);
                                }
                            });
                        }
#pragma unroll
                        for (int w = 0; w < MW; ++w) zm[w] = acc[w];
                    }
                }
                if (in_place) {
                    typedef float v4f __attribute__((ext_vector_type(4)));
                    v4f *orow = reinterpret_cast<v4f *>(io.obs + env * ROW);   // (binary16 buffers: the base of the env's rows, never indexed as float4s)
                    // binary16 buffers: this is the second pass of a fused auto-reset, and it reads back the slots this thread stored in the
                    // first (half_slot_in_place): they have all been acknowledged first
                    [[maybe_unused]] const auto orow_h = (__attribute__((address_space(1))) float *)(io.obs + env * ROW);
                    if constexpr (S::H16) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    uint32_t acc[MW];
#pragma unroll
                    for (int w = 0; w < MW; ++w) acc[w] = 0u;
                    // what happens to the four cells of one slot (stale-zero mask: see pursuit_wave.hpp).  Slot s = bit (slots of its word - 1 - s % 8)
                    // of every byte of mask word s / 8; `wc` is that word (a compile-time index: the words live in registers), `sh` the bit
                    // row_live (LIVE): the slot's pursuer is < np.  Rows of absent pursuers keep their contents -- and their mask bits
                    auto finish_slot = [&](auto wc, int sh, int q, bool valid, bool row_live, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
                        constexpr int w = decltype(wc)::value;
                        const uint32_t top = __builtin_amdgcn_perm(v1, v0, 0x0C0C0703u) | __builtin_amdgcn_perm(v3, v2, 0x07030C0Cu);
                        const uint32_t out4 = (top >> 7) & 0x01010101u;
                        const uint32_t nz4 = ((top >> 5) | (top >> 6)) & 0x01010101u;
                        const uint32_t old4 = (zm[w] >> sh) & 0x01010101u;
                        const uint32_t dirty = out4 & old4;
                        if constexpr (S::LIVE) {
                            acc[w] = (acc[w] << 1) | (row_live ? (dirty | (~out4 & nz4)) : old4);
                            valid = valid && row_live;
                        } else {
                            acc[w] = (acc[w] << 1) | (dirty | (~out4 & nz4));
                        }
                        if constexpr (S::H16) {
                            // binary16 buffer: the slot is 8 bytes of io.obs.  Whole slots, load-blend-store: a slot with a cell that must stay
                            // untouched reads the first pass's word back and keeps those halves; outside cells known to be zero are written as
                            // the zero bits they hold.  (Rows of absent pursuers, LIVE: `valid` is false, nothing is loaded or stored.)
                            half_slot_in_place(orow_h, (uint32_t)q, valid, dirty, v0, v1, v2, v3);
                        } else {
                        float32_slots_only<S::H16>();   // (refuses to compile for an H16 shape should this ever be restructured)
                        if (valid) {
                            if (dirty == 0u) {
                                if (out4 != 0x01010101u) {
                                    const v4f val = {__uint_as_float((uint32_t)max((int)v0, 0)), __uint_as_float((uint32_t)max((int)v1, 0)),
                                                     __uint_as_float((uint32_t)max((int)v2, 0)), __uint_as_float((uint32_t)max((int)v3, 0))};
                                    __builtin_nontemporal_store(val, &orow[q]);
                                }
                            } else {  // an outside cell with a non-zero stale value (Q2): plain stores that merge in L2
                                float *o = reinterpret_cast<float *>(orow + q);
                                if (v0 != SENT) o[0] = __uint_as_float(v0);
                                if (v1 != SENT) o[1] = __uint_as_float(v1);
                                if (v2 != SENT) o[2] = __uint_as_float(v2);
                                if (v3 != SENT) o[3] = __uint_as_float(v3);
                            }
                        }
                        }
                    };
                    if constexpr (S::TABLED) {
                        // a ROLLED loop per mask word (fully unrolled, the 22 slots the authors' shape had on two wavefronts cost 241 VGPRs: two wavefronts per SIMD)
                        int pq = q0_p, fq = q0_f, q = tid;   // (pursuer, position in its row) and index of the slot, advanced by constants
                        const char *Lb = reinterpret_cast<const char *>(L);
                        auto cell_b = [&](int byte_off) -> uint32_t { return *reinterpret_cast<const uint32_t *>(Lb + byte_off); };
                        static_for<0, MW>([&](auto wc) {
                            constexpr int w = decltype(wc)::value, nsw = (NS - 8 * w) < 8 ? (NS - 8 * w) : 8;
#pragma unroll MADRL_PG_UNROLL
                            for (int i = 0; i < nsw; ++i) {
                                const bool valid = q < S::NQ;
                                const int pp = valid ? pq : 0;                                   // threads past the end of the rows read harmless cells
                                const uint2 t = *reinterpret_cast<const uint2 *>(&L[S::X_TAB + 2 * fq]);
                                const int base = (int)L[S::X_ORG + pp];                          // byte offset of the window origin
                                const uint32_t v0 = cell_b(base + (int)((t.x & 0xFFFFu) << 2));
                                const uint32_t v1 = cell_b(base + (int)((t.x >> 16) << 2));
                                const uint32_t v2 = cell_b(base + (int)((t.y & 0x7FFFu) << 2));
                                // element 3: relative like the others, or absolute (bit 31: the skip cell / the id cells; bit 15: + pursuer)
                                const int b3 = ((int)t.y < 0) ? 0 : base;
                                const int id3 = (t.y & 0x8000u) ? pp : 0;
                                const uint32_t v3 = cell_b(b3 + (int)((((t.y >> 16) & 0x7FFFu) + (uint32_t)id3) << 2));
                                finish_slot(wc, nsw - 1 - i, q, valid, pp < np, v0, v1, v2, v3);
                                q += NT;
                                fq += NT % S::DV;
                                pq += NT / S::DV;
                                if (fq >= S::DV) { fq -= S::DV; pq += 1; }
                            }
                        });
                    } else {
                        static_for<0, NS>([&](auto sc) {
                            constexpr int s = decltype(sc)::value;
                            const int q = tid + NT * s;
                            const bool valid = (NT * (s + 1) <= S::NQ) ? true : (fresh(tid) + NT * s < S::NQ);
                            const int base = (int)L[s_org[s]];
                            const uint32_t v0 = L[base + s_cst[s][0]];
                            const uint32_t v1 = L[base + s_cst[s][1]];
                            const uint32_t v2 = L[base + s_cst[s][2]];
                            const uint32_t v3 = L[(int)__umul24((uint32_t)base, (uint32_t)s_rel3[s]) + s_cst[s][3]];
                            finish_slot(std::integral_constant<int, 0>{}, NS - 1 - s, q, valid, s_org[s] - S::X_ORG < np, v0, v1, v2, v3);
                        });
                    }
#pragma unroll
                    for (int w = 0; w < MW; ++w) zm[w] = acc[w];
                }
                group_sync();
                if (alive) layer[cell] = 0u;
                group_sync();
            }
            if constexpr (MODE == 1) {
                if (isP()) uniform_ptr(io.rew + env * P)[utid] = rew_out;
                if (fresh(tid) == 0) {
                    io.done[env] = (uint8_t)done_bits;
                    io.removed[env] = n_removed;
                    cold_args()->d.flags[env] = done_flag_word(done_bits);
                }
            }
            // ---------------------------------------------------------- registers -> state record
            {
                int myxy = x | (y << 8);
                if constexpr (S::LIVE) {
                    if (!(isP() ? isLP() : eslot < ne)) myxy = NOT_HERE | (NOT_HERE << 8);
                }
                const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(rec_src0, myxy);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(rec_src1, myxy);
                uint32_t w = (lo & 0xFFFFu) | (hi << 16);
                if (lane == 0) w = tick;
                if (lane == 1) w = (uint32_t)tstep;
                if (lane == 2) w = (uint32_t)map_id;
                if (lane == 3) w = 0u;
                if (lane == S::OFF_GONE / 4) w = (uint32_t)gone;
                if (S::NGW > 1 && lane == S::OFF_GONE / 4 + 1) w = (uint32_t)(gone >> 32);
                if (own_term) w = ((lane - S::OFF_TERM / 4) & 1) ? (uint32_t)(term >> 32) : (uint32_t)term;
                if (lane >= S::OFF_TERM / 4 + S::NTW) w = 0u;  // padding dwords
                if (own_dw) uniform_ptr(reinterpret_cast<uint32_t *>(d.state + env * (int64_t)S::REC_BYTES))[ulane] = w;
#pragma unroll
                for (int w = 0; w < MW; ++w) uniform_ptr(d.zmask + (env * MW + w) * NT)[utid] = zm[w];
            }
        }
        cur_rec = nxt_rec;
        cur_act = nxt_act;
#pragma unroll
        for (int w = 0; w < MW; ++w) cur_zm[w] = nxt_zm[w];
    }
}

}  // namespace pw
}  // namespace madrl
