// pursuit_wave.hpp -- compile-time-specialised PursuitEvade kernel: ONE WAVEFRONT = ONE ENV.
//
// Used when the configuration matches one of the instantiations listed in
// pursuit_specializations.def (n_pursuers + n_evaders <= 64 lanes, odd obs_range, observation
// row length divisible by 4); everything else runs on the generic kernel in pursuit.hip.
// Both kernels share the packed state record, so they are interchangeable step by step
// (tests/test_pursuit_gpu.py checks them against each other and against the oracle).
//
// Design (DESIGN.md "pursuit_wave_kernel"):
//   * 64-thread workgroups (__launch_bounds__(64)): lane a < P is pursuer a, lane P+i is evader
//     slot i; every barrier is wave-local.  Workgroups are persistent and stride over envs,
//     so the per-map tables and each lane's observation slot constants are built once.
//   * LDS holds three PADDED dword layers addressed as one array L[3*GSZ]:
//       layer 0  map as float bits (0 free, 1/norm building, 1/norm outside the map), static;
//       layer 1  pursuer counts, layer 2 evader counts: integers while the dynamics run
//                (ds_add atomics), overwritten IN PLACE by their float32 observation values
//                (count / layer_norm, table lookup) right before the observation pass;
//                cells outside the map hold the sentinel 0xFFFFFFFF = "do not store" (Q2).
//     Catch credit (purs_sur) needs no extra layer: a caught evader adds 0x10000 to its own
//     evader-count cell and pursuers look at their four neighbours.
//     After the observation pass each agent lane zeroes its own cell again, so no per-env
//     re-initialisation of the layers is needed.
//   * Observation row of an env = P*D floats = P*D/4 float4 slots, slot q -> lane q % 64:
//     every store instruction writes 64 consecutive float4 (1 KiB, fully coalesced).  Per
//     slot a lane keeps 4 LDS offsets relative to the owning pursuer's window origin; the
//     pursuer's origin comes from its lane by ds_bpermute.  A float4 that contains a stale
//     (out-of-map) cell falls back to per-dword conditional stores.
#pragma once

#include <type_traits>

#include "common.hpp"
#include "pursuit_rules.hpp"
#include "pursuit_zm16.hpp"

namespace madrl {
namespace pw {

// Register allocation for this many resident wavefronts per SIMD.  Measured at BASELINE C2 (scripts/sweep_wave.py): 4 waves (105
// VGPRs, 4 096 persistent workgroups) 87.8 us per launch, 5 waves (96 VGPRs, no scratch; 5 120 workgroups = exactly the resident
// capacity) 77.0 us, 6 waves (80 VGPRs, 32 B of scratch; 6 144 workgroups) 80.2 us.
#ifndef MADRL_PW_WAVES
#define MADRL_PW_WAVES 5
#endif
// Shapes with more than 5 float4 slots per lane keep 4 waves (at 96 VGPRs they would spill, and spill stores reach HBM).
#define MADRL_PW_OCC __attribute__((amdgpu_waves_per_eu(S::OCC, S::OCC)))

constexpr uint32_t SENT = 0xFFFFFFFFu;   // layer 1/2 outside the map: element is not stored
constexpr uint32_t CAUGHT = 0x10000u;    // added to an evader-count cell by a caught evader

struct WaveDev {
    int32_t n_catch, surround, reward_global, sample_maps, n_maps, max_steps, auto_reset;
    int32_t fmap_stride;  // dwords per map entry in fmaps
    int32_t max_opponents;  // > 0: random_opponents (pursuit_evade.py:177-181)
    int32_t reverse;      // 1: walk the envs from the last to the first (see launch() in pursuit.hip)
    uint32_t k0, k1, gid_base;
    double catchr, term_pursuit, urgency, cw;
    int64_t n_envs;
    const uint32_t *fmaps;   // per map: padded float layer [GSZ] then need_to_surround [XS*YS] as u32
    const float *vtab;       // fl32(k / layer_norm), k = 0..255
    const int32_t *pending;  // LShape kernels: the caller's pending agent counts [n_envs][2], read by resets (pending_count); unused otherwise
    // Host-built launch constants, so that the per-workgroup preamble is loads, not index arithmetic (every resident wavefront
    // runs it at the same moment, 2.8 us of a 78 us launch when it was computed in the kernel):
    const uint32_t *cnt_tmpl;  // [GSZ] an empty count layer: 0 inside the map, SENT outside
    const uint32_t *slot_tab;  // [NS][6][NT] per thread and float4 slot: 4 cell offsets, element-3-is-relative flag, owning pursuer
    const double *cw_env;      // per-env constraint_window / catchr (curriculum) or nullptr: the scalars above.  Read with scalar loads
    const double *catchr_env;  // (constant address space): written by the host or an earlier launch, never by these kernels
    uint8_t *state;
    uint32_t *flags;         // [n_envs] flag words of the step launches (done_flag_word, common.hpp)
    uint32_t *zmask;         // [n_envs][64]: per lane, which of its observation cells hold a NON-ZERO stale value (see "stale-zero mask");
                             // S::ZM16 shapes: [n_envs][32], 16 bits per lane (pursuit_zm16.hpp), the first half of the same region
};

struct WaveIO {
    const uint8_t *mask;
    const int32_t *inj_pos;
    const int32_t *inj_map;
    const int32_t *actions;
    const int32_t *inj_eact;
    float *obs;
    float *rew;
    uint8_t *done;
    int32_t *removed;
    int32_t flex;            // host side only: 1 = launch the FLEX instantiation (injected evader actions and / or per-env catchr)
    int32_t control_evaders; // host side only: 1 = launch the evader-control instantiations (madrl_pursuit_config::control_evaders)
    const float *obs_prev;   // TShape / TLShape kernels (madrl_pursuit_step_to): the buffer the kept cells come from; unused otherwise
};

// a wave-uniform float64 read through the scalar cache (s_load_dwordx2, counted by lgkmcnt -- not by the vmcnt the
// store pipeline of these kernels is scheduled around)
__device__ __forceinline__ double sload_f64(const double *p, int64_t index) {
    return ((const __attribute__((address_space(4))) double *)(uint64_t)p)[index];
}

// Launch parameters that only the rare paths read (episode reset, a change of map) come from the kernel-argument segment
// (kernargs, common.hpp) instead of SGPRs held across the env loop.
struct KArgs {
    WaveDev d;
    WaveIO io;
};
// The launch flags of WaveDev as the env loop reads them: the launch's values, or for an S::FIXED shape the constants of its contract
// (FShape) -- the branches on them, the code behind the untaken sides and the SGPRs that held the flags leave that kernel.
// MADRL_PW_FOLD=1 (a profiling aid like MADRL_ABLATE, scripts/variants.sh: never the shipped library) folds these three flags in EVERY
// kernel of this file: the cheapest stand-in for the FShape kernel in the benchmarked form (profiles/r23_fixed/pricing.txt).
#ifndef MADRL_PW_FOLD
#define MADRL_PW_FOLD 0
#endif
template <class S>
struct Launch {
    static constexpr bool FOLD = S::FIXED || MADRL_PW_FOLD;
    static __device__ __forceinline__ bool surround(const WaveDev &d) { if constexpr (FOLD) return true; else return d.surround; }
    static __device__ __forceinline__ bool reward_global(const WaveDev &d) { if constexpr (FOLD) return false; else return d.reward_global; }
    static __device__ __forceinline__ bool reverse(const WaveDev &d) { if constexpr (FOLD) return false; else return d.reverse; }
};
typedef const __attribute__((address_space(4))) KArgs *KArgsPtr;
__device__ __forceinline__ KArgsPtr cold_args() { return kernargs<KArgs>(); }
// pending count k (0 pursuers, 1 evaders) of an env (LShape kernels, resets only): a scalar load, like sload_f64
__device__ __forceinline__ int32_t pending_count(int64_t env, int k) {
    const int32_t *pend = cold_args()->d.pending;
    return ((const __attribute__((address_space(4))) int32_t *)(uint64_t)pend)[2 * env + k];
}

template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_>
struct Shape {
    static constexpr int XS = XS_, YS = YS_, P = P_, E = E_, A = P_ + E_, R = R_, FLATTEN = FLATTEN_;
    static constexpr int OFF = (R - 1) / 2;
    static constexpr int PAD = OFF > 1 ? OFF : 1;
    static constexpr int GW = YS + 2 * PAD;
    static constexpr int GH = XS + 2 * PAD;
    static constexpr int GSZ = (GH * GW + 3) / 4 * 4;           // dwords per layer
    static constexpr int D = FLATTEN ? 3 * R * R + 1 : 4 * R * R;  // include_id is implied
    static constexpr int DV = D / 4;                             // float4 per pursuer row
    static constexpr int NQ = P * DV;                            // float4 slots per env
    static constexpr int NS = (NQ + 63) / 64;                    // slots per lane
    static constexpr int MWORDS = 1;                             // stale-zero mask dwords per lane
    static constexpr bool ZM16 = zm16::eligible(P, R, FLATTEN);  // the masks are kept as 16 bits per lane (pursuit_zm16.hpp)
    static constexpr int ZMW = ZM16 ? 32 : 64;                   // mask dwords per env
    // the in-place float32 pass leaves out the float4 stores of a 64-byte chunk that would write zeros over zeros ("zeros over known
    // zeros" in the kernel).  Sound only where the pass stores into the buffer the masks describe and every mask position it trusts is a
    // true bit: the 16-bit form (the position a lane drops is forced to "unknown"), in place, float32 -- the two-buffer shapes switch it off
    static constexpr bool ZSKIP = ZM16;
    static constexpr int OCC = NS <= 5 ? MADRL_PW_WAVES : (MADRL_PW_WAVES < 4 ? MADRL_PW_WAVES : 4);  // resident wavefronts per SIMD aimed at
    static constexpr int X_FILL = 3 * GSZ;                       // extras after the layers
    static constexpr int X_SKIP = 3 * GSZ + 1;
    static constexpr int X_ID = 3 * GSZ + 2;                     // P id values
    static constexpr int X_VTAB = (X_ID + P + 3) / 4 * 4;        // 72 count values
    static constexpr int NVT = 72;
    static constexpr int X_NEED = X_VTAB + NVT;                  // XS*YS bytes, as dwords
    static constexpr int X_OBSV = X_NEED + (XS * YS + 3) / 4;    // evader control: window origin of the observer of row p (P dwords)
    static constexpr int LDS_DWORDS = X_OBSV + (P + 3) / 4 * 4;
    // packed state record, identical to the generic kernel's layout() (pursuit_tables.hpp)
    static constexpr int NGW = (E + 31) / 32 > 0 ? (E + 31) / 32 : 1;
    static constexpr int NTW = (A + 31) / 32;
    static constexpr int OFF_GONE = (16 + 2 * A + 3) / 4 * 4;
    static constexpr int OFF_TERM = OFF_GONE + 4 * NGW;
    static constexpr int REC_BYTES = (OFF_TERM + 4 * NTW + 15) / 16 * 16;
    static constexpr int REC_DW = REC_BYTES / 4;
    static_assert(REC_DW <= 64, "the whole record must fit one dword per lane");
    static_assert(A <= 64, "one wavefront per env: n_pursuers + n_evaders must fit 64 lanes");
    static_assert(R % 2 == 1, "odd obs_range only (even ranges run on the generic kernel)");
    static_assert(D % 4 == 0, "observation row must be a whole number of float4");
    static_assert(LDS_DWORDS * 4 <= 64 * 1024, "LDS budget");
    static_assert(NS <= 8, "stale-zero mask: one bit per slot in each byte of the lane's mask dword");
    static constexpr bool LIVE = false;
    static constexpr bool TO = false;
    static constexpr bool H16 = false;                           // (THShape / TLHShape: binary16 observation buffers)
    static constexpr bool LEAN_REGS = false;                     // loop constants worked out again at their uses (see THShape)
    static constexpr bool TABLED = false;                       // (pursuit_group.hpp: slot constants from an LDS table; never here)
    static constexpr int X_TAB = 0;
    static constexpr bool FIXED = false;                         // (FShape: the launch flags are compile-time constants)
};

// Per-env agent counts (madrl_pursuit_set_agent_counts): the same geometry, with P and E as a CAPACITY.  An env runs LIVE p <= P
// pursuers and e <= E evader slots; a slot that does not exist holds position byte 0xFF in the record (no coordinate is 255), so p
// and e are the numbers of leading slots without it.  pursuit_wave_kernel<LShape<...>, ...> is a kernel of its own (the fixed-shape
// instantiations keep their code and names); the shapes are listed in pursuit_live_specializations.def.
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_>
struct LShape : Shape<XS_, YS_, P_, E_, R_, FLATTEN_> {
    static constexpr bool LIVE = true;
};
constexpr int NOT_HERE = 0xFF;   // position byte of a slot that does not exist (live-count records)

// The step kernel specialised on its LAUNCH CONSTANTS as well: the same geometry, and every launch flag the env loop of the plain kernel
// tests per env is a constant of the shape (the accessors of `Launch` above).  The contract -- launch() in pursuit.hip takes this
// kernel only for a step launch that meets all of it, and the plain kernel of the same shape otherwise; both share record and masks,
// so they are interchangeable launch by launch:
//   surround catch, local reward, train_pursuit (no evader control), ONE map and no sample_maps (map_id is 0: the map staged with the
//   tables is the map of every env, load_map leaves the loop), forward walk, no per-env curriculum arrays (catchr_env == cw_env ==
//   nullptr), max_opponents == 0, no pending counts, no injected evader actions, in place, float32.
// max_steps, auto_reset, catchr, cw, urgency, term_pursuit and n_catch stay run-time values.  Only <FShape, 1, false, false> is
// instantiated (pursuit_fixed.hip, the XF lines of pursuit_fixed_specializations.def); resets run on the plain kernel.
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_>
struct FShape : Shape<XS_, YS_, P_, E_, R_, FLATTEN_> {
    static constexpr bool FIXED = true;
};

// The two-buffer step (madrl_pursuit_step_to): the step's observation pass stores every valid float4 of the env's rows to io.obs, whole
// and non-temporal; the cells the in-place pass leaves alone come from the same place of io.obs_prev -- loaded only in the slots whose
// `dirty` word is non-zero (a kept cell not known to be zero) and in the rows of absent observers, which are copied whole.  The mask bit
// of a kept cell becomes "the loaded value is non-zero".  The second pass of a fused auto-reset is the in-place pass on io.obs.
// Only the flexible step kernel <S, 1, true> is instantiated (to_wave_launch, pursuit_to.hip); the shapes are the X / XL lines of
// pursuit_to_specializations.def.
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_>
struct TShape : Shape<XS_, YS_, P_, E_, R_, FLATTEN_> {
    static constexpr bool TO = true;
    static constexpr bool ZSKIP = false;                         // (another buffer: never skips)
};
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_>
struct TLShape : LShape<XS_, YS_, P_, E_, R_, FLATTEN_> {
    static constexpr bool TO = true;
    static constexpr bool ZSKIP = false;                         // (another buffer: never skips)
};
// The two-buffer step over binary16 buffers (madrl_pursuit_step_to_f16): io.obs and io.obs_prev point at 2-byte elements (cast: WaveIO does
// not grow), so the env's rows are P * D * 2 bytes and a slot -- the same four elements -- is 8 bytes at (64 s + lane) * 8.  Part 1 of the
// pass is the float32 kernel's; part 2 loads the old slot as one 8-byte word, converts the four values (half_bits: round to nearest even),
// takes the kept halves from the old word and stores the slot as ONE non-temporal 8-byte store, 512 B per instruction and wavefront.  The
// second pass of a fused auto-reset is a load-blend-store of whole slots of io.obs itself (half_slot_in_place below): the in-place pass's
// masked stores are float32 geometry and cannot be reached from these shapes.
// LEAN_REGS has nothing to do with the storage format: it is a register-pressure trait these two shapes set.  At the 96 VGPRs of five
// wavefronts per SIMD the TLHShape kernel spilled three loop constants of the shared kernel text; with the trait the mask index of fetch_zm
// and the two lane indices of the record store are worked out again at their uses and the global reward reads lane k by two ds_bpermute at
// a constant address instead of __shfl (which keeps `lane & 64` live across the env loop).  No existing shape sets it: their code is the
// parent's.  Instantiated in pursuit_to_f16.hip (THShape) and
// pursuit_to_f16_live.hip (TLHShape).
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_>
struct THShape : Shape<XS_, YS_, P_, E_, R_, FLATTEN_> {
    static constexpr bool TO = true;
    static constexpr bool ZSKIP = false;                         // (another buffer: never skips)
    static constexpr bool H16 = true;
    static constexpr bool LEAN_REGS = true;
};
template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_>
struct TLHShape : LShape<XS_, YS_, P_, E_, R_, FLATTEN_> {
    static constexpr bool TO = true;
    static constexpr bool ZSKIP = false;                         // (another buffer: never skips)
    static constexpr bool H16 = true;
    static constexpr bool LEAN_REGS = true;
};

__device__ __forceinline__ double pairwise8(const double *r) {
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

// numpy's float64 add.reduce order over P values held in registers (see pursuit.hip)
template <int P>
__device__ __forceinline__ double np_sum_regs(const double (&a)[P]) {
    if constexpr (P < 8) {
        double res = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) res += a[i];
        return res;
    } else {
        double r[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = a[i];
        constexpr int LIM = P - (P % 8);
#pragma unroll
        for (int i = 8; i < LIM; i += 8) {
#pragma unroll
            for (int k = 0; k < 8; ++k) r[k] += a[i + k];
        }
        double res = pairwise8(r);
#pragma unroll
        for (int i = LIM; i < P; ++i) res += a[i];
        return res;
    }
}

// numpy's add.reduce order (np_sum_regs) over the first n <= P of P values in registers: the live-count kernel's global reward
template <int P>
__device__ __forceinline__ double np_sum_first(const double (&a)[P], int n) {
    double res = 0.0;
    if (n < 8) {
#pragma unroll
        for (int i = 0; i < (P < 8 ? P : 7); ++i)
            if (i < n) res += a[i];
        return res;
    }
    if constexpr (P >= 8) {
        double r[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = a[i];
        const int lim = n - (n % 8);
#pragma unroll
        for (int i = 8; i + 8 <= P; i += 8) {
            if (i < lim) {
#pragma unroll
                for (int k = 0; k < 8; ++k) r[k] += a[i + k];
            }
        }
        res = pairwise8(r);
#pragma unroll
        for (int i = 8; i < P; ++i)
            if (i >= lim && i < n) res += a[i];
    }
    return res;
}

// Masked global stores that are ALWAYS issued (exec narrowed inside the asm, no compiler-made skip branch around them): the
// number of vector-memory instructions per env iteration is then a compile-time constant, which is what lets the record
// prefetch wait with an exact s_waitcnt vmcnt(N) instead of vmcnt(0) (see "software pipeline").  base: wave-uniform pointer,
// voff: per-lane byte offset, OFF: immediate byte offset (< 4096).  The trailing s_nop covers the "store of more than 8 bytes,
// then a VALU write of its data registers" hazard that the compiler cannot see through inline asm.
typedef float v4f_t __attribute__((ext_vector_type(4)));
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
// One observation slot: the four elements under their own lane masks as plain (L2-merged) dword stores, then the float4 under its
// mask as one non-temporal store.  Each mask is the result of one v_cmp (inactive lanes compare to 0, so a mask never enables a lane
// that exec had off) and goes into exec with one s_mov: 7 scalar instructions per slot, no mask algebra on the scalar unit.
// H16: the caller's shape holds binary16 buffers -- refused here, wherever the call stands: the offsets below (a float4 at voff = lane * 16,
// elements 4 bytes apart, slots 1 KiB apart) are float32 geometry and would run past the end of a half buffer.
template <int OFF, bool H16 = false>
__device__ __forceinline__ void store_slot_masked(const void *base, uint32_t voff, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3,
                                                  v4f_t val, uint64_t m0, uint64_t m1, uint64_t m2, uint64_t m3, uint64_t m_nt) {
    static_assert(!H16, "store_slot_masked is float32 geometry: an H16 shape runs its in-place pass through half_slot_in_place");
    uint64_t sv;
    asm volatile("s_mov_b64 %0, exec\n\t"
                 "s_mov_b64 exec, %1\n\tglobal_store_dword %6, %7, %12 offset:%13\n\t"
                 "s_mov_b64 exec, %2\n\tglobal_store_dword %6, %8, %12 offset:%13+4\n\t"
                 "s_mov_b64 exec, %3\n\tglobal_store_dword %6, %9, %12 offset:%13+8\n\t"
                 "s_mov_b64 exec, %4\n\tglobal_store_dword %6, %10, %12 offset:%13+12\n\t"
                 "s_mov_b64 exec, %5\n\tglobal_store_dwordx4 %6, %11, %12 offset:%13 nt\n\t"
                 "s_mov_b64 exec, %0\n\ts_nop 0"
                 : "=&s"(sv) : "s"(m0), "s"(m1), "s"(m2), "s"(m3), "s"(m_nt), "v"(voff), "v"(v0), "v"(v1), "v"(v2), "v"(v3), "v"(val),
                   "s"(base), "n"(OFF));
}
// a + K for a loop constant a, computed where it stands (volatile: not hoisted out of the env loop into one more live register) in ONE instruction
template <uint32_t K>
__device__ __forceinline__ uint32_t add_here(uint32_t a) {
    uint32_t r;
    asm volatile("v_add_u32 %0, %1, %2" : "=v"(r) : "n"(K), "v"(a));
    return r;
}
// OR of a lane value over its aligned group of four lanes (a DPP quad): two quad_perm moves, no scalar instruction
__device__ __forceinline__ uint32_t quad_or(uint32_t v) {
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
    return v;
}

// Record prefetch with an exact wait (step kernel).  vmcnt counts loads and stores alike and retires them in issue order, and the
// compiler, which cannot know how many of the masked stores above were issued, would wait for a prefetched record with
// vmcnt(0): every wavefront then stalls until its previous env's observation stores have been acknowledged, half an iteration
// after issuing them.  Here the three loads of the next env are issued (inline asm, so the compiler inserts no wait of its own)
// at the top of an iteration and waited for at its END with s_waitcnt vmcnt(<stores per iteration>): only the stores of the
// PREVIOUS iteration -- a whole iteration old -- must have retired, this iteration's may all be in flight.
// Every lane loads (clamped offsets, no exec games); s_nop 4 covers a base pointer that a VALU instruction may have just written.
__device__ __forceinline__ void prefetch3(uint32_t &r0, uint32_t &r1, uint32_t &r2, const void *b0, uint32_t o0, const void *b1, uint32_t o1,
                                          const void *b2, uint32_t o2) {
    asm volatile("s_nop 4\n\tglobal_load_dword %0, %3, %4\n\tglobal_load_dword %1, %5, %6\n\tglobal_load_dword %2, %7, %8"
                 : "=&v"(r0), "=&v"(r1), "=&v"(r2) : "v"(o0), "s"(b0), "v"(o1), "s"(b1), "v"(o2), "s"(b2));
}
template <int N>
__device__ __forceinline__ void prefetch_wait(uint32_t &r0, uint32_t &r1, uint32_t &r2) {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(r0), "+v"(r1), "+v"(r2) : "n"(N) : "memory");
}

// One observation slot of a binary16 buffer, in place (the second pass of a fused auto-reset in the THShape / TLHShape kernels): `row` is
// the env's rows, `slot` the lane's 8-byte slot in them, v0..v3 the four cells as float32 bits (SENT outside the map: written as zero), keep4
// the cells that must stay untouched, one flag per byte.  A slot with such a cell is loaded -- from L2 (an agent-scope load: the word was
// stored by this lane earlier in the kernel, non-temporal) -- and keeps those halves; every valid slot leaves as one whole 8-byte store.
template <class RowPtr>
__device__ __forceinline__ void half_slot_in_place(RowPtr row, uint32_t slot, bool valid, uint32_t keep4, uint32_t v0, uint32_t v1, uint32_t v2,
                                                   uint32_t v3) {
    typedef __attribute__((address_space(1))) uint64_t gu64_t;
    if (!valid) return;
    auto hb = [](uint32_t v) -> uint64_t { return half_bits(__uint_as_float((uint32_t)max((int)v, 0))); };
    uint64_t w = hb(v0) | (hb(v1) << 16) | (hb(v2) << 32) | (hb(v3) << 48);
    gu64_t *const at = reinterpret_cast<gu64_t *>(row) + slot;
    if (keep4 != 0u) {
        const uint64_t old = __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t k = ((keep4 & 0x00000001u) ? 0x000000000000FFFFull : 0ull) | ((keep4 & 0x00000100u) ? 0x00000000FFFF0000ull : 0ull) |
                           ((keep4 & 0x00010000u) ? 0x0000FFFF00000000ull : 0ull) | ((keep4 & 0x01000000u) ? 0xFFFF000000000000ull : 0ull);
        w = (w & ~k) | (old & k);
    }
    *at = w;
}

// w[lane LN] = v for a wave-uniform v: one v_writelane_b32, no lane mask, no compare
template <int LN>
__device__ __forceinline__ void put_lane(uint32_t &w, uint32_t v) {
    const uint32_t sv = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    asm("v_writelane_b32 %0, %1, %2" : "+v"(w) : "s"(sv), "n"(LN));
}
template <int LN, int END>
__device__ __forceinline__ void put_zero_from(uint32_t &w) {
    if constexpr (LN < END) {
        put_lane<LN>(w, 0u);
        put_zero_from<LN + 1, END>(w);
    }
}

// ---------------------------------------------------------------- table staging (once per workgroup, and at a change of map)
// The per-workgroup tables go from global memory to LDS in strided TRIPS: trip j of a table moves elements [NT j, NT j + NT), one per
// thread.  Written as `for (k = tid; k < n; k += NT) L[k] = tab[k]` the compiler emits load -> s_waitcnt vmcnt(0) -> ds_write per
// trip, each next load behind a branch on the bounds test: one dependent round trip to L2 per trip, about twenty before a workgroup's
// first env, made by every workgroup of a launch at the same moment.  Here the trips have compile-time numbers, every thread loads
// unconditionally from an index CLAMPED to the table's last element (the host sizes the tables exactly: no read may pass their end;
// the bounds test stays on the LDS write alone), all loads of a batch are issued before its first value is used, and the batch is
// waited for ONCE (staged_wait).  Fill<S, NT> numbers the trips of all tables of a shape:
//   [0, J_MAP) empty count layer -> layers 1 and 2   [J_MAP, J_NEED) map layer   [J_NEED, J_VT) need_to_surround bytes
//   [J_VT, J_TAB) count values   [J_TAB, J_END) the long-row slot table of the multi-wavefront kernel (TABLED shapes)
template <class S, int NT>
struct Fill {
    static constexpr int NEEDW = (S::XS * S::YS + 3) / 4;
    static constexpr int TABW = S::TABLED ? 2 * S::DV : 0;
    static constexpr int J_MAP = (S::GSZ + NT - 1) / NT;
    static constexpr int J_NEED = 2 * J_MAP;
    static constexpr int J_VT = J_NEED + (NEEDW + NT - 1) / NT;
    static constexpr int J_TAB = J_VT + (S::NVT + NT - 1) / NT;
    static constexpr int J_END = J_TAB + (TABW + NT - 1) / NT;
    static constexpr int first(int j) { return j < J_MAP ? 0 : j < J_NEED ? J_MAP : j < J_VT ? J_NEED : j < J_TAB ? J_VT : J_TAB; }
    static constexpr int words(int j) { return j < J_NEED ? S::GSZ : j < J_VT ? NEEDW : j < J_TAB ? S::NVT : TABW; }
};
// (the sources: cnt = WaveDev::cnt_tmpl, map = the map's entry of WaveDev::fmaps -- layer, then the need bytes --, vtab, tab = the slot table)
template <class S, int NT, int J>
__device__ __forceinline__ uint32_t fill_load(uint32_t utid, const uint32_t *cnt, const uint32_t *map, const uint32_t *vtab, const uint32_t *tab) {
    using F = Fill<S, NT>;
    constexpr int t = J - F::first(J), n = F::words(J);
    const uint32_t k = utid + (uint32_t)(NT * t);
    const uint32_t kc = (NT * (t + 1) <= n) ? k : (k < (uint32_t)n ? k : (uint32_t)n - 1u);
    if constexpr (J < F::J_MAP) return cnt[kc];
    else if constexpr (J < F::J_NEED) return map[kc];
    else if constexpr (J < F::J_VT) return map[(uint32_t)S::GSZ + kc];
    else if constexpr (J < F::J_TAB) return vtab[kc];
    else return tab[kc];
}
// FIRST: the workgroup's first fill also sets the two cells the slot constants of absent elements point at
template <class S, int NT, int J, bool FIRST>
__device__ __forceinline__ void fill_store(uint32_t *L, uint32_t utid, uint32_t v) {
    using F = Fill<S, NT>;
    constexpr int t = J - F::first(J), n = F::words(J);
    const uint32_t k = utid + (uint32_t)(NT * t);
    if ((NT * (t + 1) <= n) || k < (uint32_t)n) {
        if constexpr (J < F::J_MAP) {
            L[S::GSZ + k] = v;
            L[2 * S::GSZ + k] = v;
        } else if constexpr (J < F::J_NEED) L[k] = v;
        else if constexpr (J < F::J_VT) L[S::X_NEED + k] = v;
        else if constexpr (J < F::J_TAB) L[S::X_VTAB + k] = v;
        else L[S::X_TAB + k] = v;
    }
    if constexpr (FIRST && J == F::J_MAP) {
        if (utid == 0u) {
            L[S::X_FILL] = v;   // element 0 of map 0: a corner of the padded map layer is always outside the map
            L[S::X_SKIP] = SENT;
        }
    }
}
// The one wait of a batch of N staged registers a[0 .. N): groups of empty-asm operands from the END of the array -- the loads issued
// last -- so that the first group makes the compiler wait with s_waitcnt vmcnt(0) and the others need no wait at all.  (Left to
// itself it waits before each LDS write with a counted vmcnt(k); correct, but one of them is then the vmcnt(VM_PER_ENV) that
// tests/test_wave_isa_budget.py wants to find in exactly one place.)
template <int N>
__device__ __forceinline__ void staged_wait(uint32_t *a) {
    if constexpr (N >= 8) {
        asm volatile("" : "+v"(a[N - 1]), "+v"(a[N - 2]), "+v"(a[N - 3]), "+v"(a[N - 4]), "+v"(a[N - 5]), "+v"(a[N - 6]), "+v"(a[N - 7]), "+v"(a[N - 8]));
        staged_wait<N - 8>(a);
    } else if constexpr (N >= 4) {
        asm volatile("" : "+v"(a[N - 1]), "+v"(a[N - 2]), "+v"(a[N - 3]), "+v"(a[N - 4]));
        staged_wait<N - 4>(a);
    } else if constexpr (N >= 2) {
        asm volatile("" : "+v"(a[N - 1]), "+v"(a[N - 2]));
        staged_wait<N - 2>(a);
    } else if constexpr (N == 1) {
        asm volatile("" : "+v"(a[0]));
    }
}
// trips [J0, J1) in batches of at most CAP: per batch all loads, one wait, the LDS writes
template <class S, int NT, int J0, int J1, int CAP, bool FIRST>
__device__ __forceinline__ void fill_trips(uint32_t *L, uint32_t utid, const uint32_t *cnt, const uint32_t *map, const uint32_t *vtab, const uint32_t *tab) {
    if constexpr (J0 < J1) {
        constexpr int JB = J0 + CAP < J1 ? J0 + CAP : J1;
        uint32_t st[JB - J0];
        static_for<J0, JB>([&](auto jc) {
            if constexpr (decltype(jc)::value == JB - 1) __builtin_amdgcn_sched_barrier(0);  // the load staged_wait looks at first stays the last one issued
            st[decltype(jc)::value - J0] = fill_load<S, NT, decltype(jc)::value>(utid, cnt, map, vtab, tab);
        });
        staged_wait<JB - J0>(st);
        static_for<J0, JB>([&](auto jc) { fill_store<S, NT, decltype(jc)::value, FIRST>(L, utid, st[decltype(jc)::value - J0]); });
        fill_trips<S, NT, JB, J1, CAP, FIRST>(L, utid, cnt, map, vtab, tab);
    }
}
// registers a workgroup's first batch may hold in flight (table trips + slot constants + the first env's fetch), and the table trips
// of every later batch (also of a change of map inside the env loop, where the slot constants are live as well)
constexpr int FILL_FIRST = 56, FILL_BATCH = 16;

// Profiling aid (scripts/variants.sh builds one library per value, never the shipped one):
//   1 no observation stores   2 store stale cells too (all float4 full, nt)   4 no Philox
//   8 no observation pass at all   16 no record / reward stores
//   64 no record prefetch (timing only, wrong results)   128 20 dependent SALU more per observation slot (results unchanged)
//   256 every env's stale-zero mask at the address of env & 255: the mask traffic stays in L2 (timing only, wrong results)
//   512 no mask traffic: the masks are read at env & 255 (never written: they stay in L2) and not stored, every float4 stored whole as
//       with 2 -- against 2 this prices the mask bytes alone (timing only, wrong results)
//   1024 S::ZSKIP shapes: no non-temporal float4 in a chunk whose clean slots get new values that are all zero or outside the map, whatever
//       the buffer holds -- more than "zeros over known zeros" can skip, its upper bound (timing only, wrong results)
#ifndef MADRL_ABLATE
#define MADRL_ABLATE 0
#endif
// Timing aids (same rules): 4 return at once (launch cost)   8 return after the per-workgroup preamble
#ifndef MADRL_PW_EXP
#define MADRL_PW_EXP 0
#endif

// Stale-zero mask (quirk Q2).  A cell of channel 1 / 2 outside the map is not written: it keeps the value of the last time it
// was inside.  A float4 slot that mixes written and unwritten cells becomes a partial store, which the memory side turns into
// a read-modify-write of the sector (about 20 us of the 90 us launch at BASELINE C2).  Most stale values are 0.0 -- counts of
// mostly empty cells -- and storing 0.0 over a stale 0.0 changes nothing.  So the kernel keeps, per lane, one bit per observation
// cell it owns (5 slots x 4 cells; dword [env][lane] of `zmask`, prefetched and written back with the state record):
// "the value this cell holds in the caller's observation buffer is not known to be zero".  A cell inside the map sets its bit to
// (value != 0), a cell outside keeps it.  A slot is stored as ONE non-temporal float4, zeros in its outside cells, unless an
// outside cell's bit is set; only those slots (about 3 % instead of 19 %) fall back to masked dword stores.  All bits set =
// "nothing known" is always correct: the library starts there and returns there whenever the caller hands it another buffer.
// S::ZM16 shapes keep the same dword in registers but 16 bits per lane in memory (pursuit_zm16.hpp): [env][32] dwords, lane l < 32 stores
// its own half and lane l + 32's, every lane loads dword l & 31 and unpacks its half -- 128 B read and written per env instead of 256 B.
//
// MODE 0: reset(mask)      MODE 1: step (+ fused auto-reset)
// INJECT (step only) = the FLEXIBLE instantiation: evader actions come from io.inj_eact when it is given (parity harness)
// instead of Philox, and the catch reward is d.catchr_env[env] when per-env curriculum arrays are bound.
// It is a template parameter because a conditional global load in the hot loop makes the
// compiler's s_waitcnt pass put a vmcnt(0) on the common path (see "pipeline hinge" below).
// CTRL = evader control (train_pursuit=False, pursuit_evade.py:105-112, :204-241, :418-428): the P actions drive the first P REMAINING
// evaders of the layer, the pursuers move by their controller (io.inj_eact [n_envs][P] or Philox, TAG_PURSUER_ACT), observation row k
// shows the window of the k-th remaining evader among slots 0..P-1 and the rows past the last one stay untouched; rewards stay the
// pursuers'.  Only instantiated for the FLEX step kernel and the reset kernel of shapes with E >= P.
// S::LIVE (LShape) = per-env agent counts: the env's live (np, ne) come from its record (NOT_HERE slots);
// pursuer lanes >= np do not move, are not counted, write no observation row (their stores stay issued, exec-masked, so that
// VM_PER_ENV holds) and a 0 reward; evader slots >= ne are gone; a reset takes (np, ne) from the caller's pending counts and
// numbers its draws in the live layout (pursuit_rules.hpp).
template <class S, int MODE, bool INJECT, bool CTRL = false>
__global__ __launch_bounds__(64) MADRL_PW_OCC void pursuit_wave_kernel(const WaveDev d, const WaveIO io) {
    static_assert(!CTRL || (S::E >= S::P && (MODE == 0 || INJECT)), "evader control: n_evaders >= n_pursuers, flexible instantiation");
    static_assert(!CTRL || !S::LIVE, "evader control has no per-env agent counts");
    static_assert(!S::TO || (MODE == 1 && INJECT && !CTRL), "the two-buffer step: the flexible step kernel only");
    static_assert(!S::H16 || S::TO, "binary16 buffers: the two-buffer step only");
    static_assert(!S::ZSKIP || (S::ZM16 && !S::TO && !S::H16), "zeros over known zeros: the in-place float32 pass of a 16-bit-mask shape only");
    static_assert(!S::FIXED || (MODE == 1 && !INJECT && !CTRL && !S::LIVE && !S::TO), "launch constants folded in: the plain in-place step kernel only");
    using LC = Launch<S>;
    constexpr int P = S::P, E = S::E, A = S::A, GW = S::GW, PAD = S::PAD, GSZ = S::GSZ, NS = S::NS;
    __shared__ __attribute__((aligned(16))) uint32_t L[S::LDS_DWORDS];
    const int lane = threadIdx.x;
    const uint32_t ulane = threadIdx.x;  // as an unsigned 32-bit index: zero-extends into the VGPR-offset addressing form
    const bool is_p = lane < P;
    const int eslot = lane - P;

#if MADRL_PW_EXP & 4
    if (d.n_envs > 0) return;
#endif
    // ---------------------------------------------------------------- once per workgroup
    // Everything a workgroup needs before its first env comes in ONE batch of loads with one wait (see "table staging"): the empty
    // count layer, map 0, its need_to_surround bytes, the count values, the observation slot constants and the first env's record,
    // action and mask.  Map 0 is staged with the tables: with a single map -- every BASELINE config -- the first env then needs no
    // second round trip to HBM for a map chosen by its record, at a moment when every wavefront of the launch waits for the same
    // thing.  With a map pool the first env may reload (load_map below).  (Shapes whose tables do not fit FILL_FIRST registers
    // beside their slot constants stage the rest in further batches.)
    using F = Fill<S, 64>;
    const int n_envs = (int)d.n_envs;  // env indices are 32-bit (the C ABI caps n_envs below 2^31); only byte offsets are 64-bit
    int stride = (int)gridDim.x;
    // (FIXED: a value made here, held in an SGPR the flags left -- as a plain kernel argument the plain kernel loads it again at the top
    // of every env iteration and waits for it before it can form the next env's prefetch addresses)
    if constexpr (S::FIXED) asm volatile("" : "+s"(stride));
    uint64_t urgency_bits = __builtin_bit_cast(uint64_t, d.urgency);   // (FIXED: likewise -- the plain kernel loads it in every env's reward block)
    if constexpr (S::FIXED) asm volatile("" : "+s"(urgency_bits));
    const double urgency = __builtin_bit_cast(double, urgency_bits);
    if (n_envs <= 0) return;
    auto phys = [&](int e) -> int64_t { return (int64_t)(LC::reverse(d) ? n_envs - 1 - e : e); };
    // the env whose mask words an env reads and writes: its own
    auto zm_env = [](int64_t env) -> int64_t { return (MADRL_ABLATE & (256 | 512)) ? (env & 255) : env; };
    // the dword of an env's masks a lane loads: its own -- or, 16 bits per lane, the one it shares with lane +- 32
    const uint32_t zm_lane = S::ZM16 ? (ulane & 31u) : ulane;
    [[maybe_unused]] const uint32_t zm_keep = S::ZM16 ? zm16::keep_low(P, S::R, lane) : 0u;   // which bit position the lane's 16 bits leave out
    const uint32_t *const vtab_u = reinterpret_cast<const uint32_t *>(d.vtab);
    constexpr int ROOM = FILL_FIRST - 6 * NS - 3;
    constexpr int JF = F::J_END < (ROOM > 4 ? ROOM : 4) ? F::J_END : (ROOM > 4 ? ROOM : 4);
    const uint32_t rec_off = (ulane < (uint32_t)S::REC_DW ? ulane : (uint32_t)S::REC_DW - 1u) * 4u;
    const uint32_t act_off = (ulane < (uint32_t)P ? ulane : (uint32_t)P - 1u) * 4u;
    uint32_t st[JF], sraw[6 * NS];
    static_for<0, JF>([&](auto jc) { st[decltype(jc)::value] = fill_load<S, 64, decltype(jc)::value>(ulane, d.cnt_tmpl, d.fmaps, vtab_u, nullptr); });
#pragma unroll
    for (int k = 0; k < 6 * NS; ++k) sraw[k] = d.slot_tab[64u * k + ulane];  // [NS][6][64]; slots past the end of the row read harmless cells and are never stored
    // the first env of this workgroup (a workgroup without one fetches the last env's and never looks at it: every lane loads, from
    // clamped offsets, like the prefetch of the env loop)
    uint32_t cur_rec, cur_zm;
    int cur_act = 4;
    __builtin_amdgcn_sched_barrier(0);  // these three stay the loads issued last
    {
        const int64_t env0 = phys((int)blockIdx.x < n_envs ? (int)blockIdx.x : n_envs - 1);
        cur_rec = *reinterpret_cast<const uint32_t *>(d.state + env0 * (int64_t)S::REC_BYTES + rec_off);
        if constexpr (MODE == 1) cur_act = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(io.actions + env0 * P) + act_off);
        cur_zm = d.zmask[zm_env(env0) * S::ZMW + zm_lane];
    }
    asm volatile("" : "+v"(cur_rec), "+v"(cur_act), "+v"(cur_zm));  // the loads issued last: the one wait, vmcnt(0), of the whole batch
    staged_wait<6 * NS>(sraw);
    staged_wait<JF>(st);
    static_for<0, JF>([&](auto jc) { fill_store<S, 64, decltype(jc)::value, true>(L, ulane, st[decltype(jc)::value]); });
    fill_trips<S, 64, JF, F::J_END, FILL_BATCH, true>(L, ulane, d.cnt_tmpl, d.fmaps, vtab_u, nullptr);
    if (lane < P) L[S::X_ID + lane] = __float_as_uint((float)((double)lane / (double)P));  // :440-445
    if (ulane >= (uint32_t)S::REC_DW) cur_rec = 0u;
    if (!is_p) cur_act = 4;
    // observation slot constants (registers, live across the env loop)
    int s_cst[NS][4];
    int s_rel3[NS];   // 1: element 3 is window-relative, 0: absolute (id / skip cell)
    int s_src[NS];    // ds_bpermute byte address of the owning pursuer's lane
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_cst[s][k] = (int)sraw[6 * s + k] * 4;  // byte offsets into L
        s_rel3[s] = (int)sraw[6 * s + 4];
        s_src[s] = (int)sraw[6 * s + 5] * 4;
    }
    int cached_map = 0;
    int cached_np = P;  // live-count kernel: the pursuer count the id cells X_ID.. hold (k / np, :440-445)
    const uint8_t *need_tab = reinterpret_cast<const uint8_t *>(&L[S::X_NEED]);
    uint32_t *const layer = &L[is_p ? GSZ : 2 * GSZ];  // this lane's count layer
    // which lanes feed my dword of the packed state record (agents 2j and 2j+1 for dword 4+j)
    const int rec_src0 = (lane >= 4 ? 2 * (lane - 4) : 0) * 4, rec_src1 = rec_src0 + 4;

    // ---------------------------------------------------------------- software pipeline
    // The whole packed state record (S::REC_DW dwords) is fetched by ONE coalesced load, lane k
    // holding dword k, together with the pursuer action of the same env; both are issued one
    // env ahead so their HBM latency hides behind the current env's work.
    auto isP = [&]() { return fresh(lane) < P; };
    auto isE = [&]() { return (unsigned)(fresh(lane) - P) < (unsigned)E; };
    auto isAgent = [&]() { return fresh(lane) < A; };
    auto fetch_rec = [&](int64_t env) -> uint32_t {
        return (fresh(lane) < S::REC_DW) ? uniform_ptr(reinterpret_cast<const uint32_t *>(d.state + env * (int64_t)S::REC_BYTES))[ulane] : 0u;
    };
    auto fetch_act = [&](int64_t env) -> int {
        if constexpr (MODE == 1) return isP() ? uniform_ptr(io.actions + env * P)[ulane] : 4;
        else return 4;
    };
    auto fetch_zm = [&](int64_t env) -> uint32_t {
        // (S::LEAN_REGS: the lane's index worked out again at each use -- one loop constant fewer in kernels that sit at their register limit)
        if constexpr (S::LEAN_REGS) return uniform_ptr(d.zmask + zm_env(env) * S::ZMW)[S::ZM16 ? ((uint32_t)fresh(lane) & 31u) : (uint32_t)fresh(lane)];
        else return uniform_ptr(d.zmask + zm_env(env) * S::ZMW)[zm_lane];
    };
    wave_sync();
#if MADRL_PW_EXP & 8
    if (d.n_envs > 0) { if (s_cst[0][0] + s_cst[NS - 1][3] + s_rel3[0] + s_src[NS - 1] + (int)cur_rec == 0x12345) io.rew[0] = 1.f; return; }
#endif

    // PIPE: the exact-wait prefetch above (production step kernel); the reset kernel (envs may be skipped) and the parity
    // harness variant keep compiler-managed loads and the mid-iteration hinge.
    constexpr bool PIPE = (MODE == 1) && !INJECT && !(MADRL_ABLATE & (1 | 8 | 16 | 64));
    constexpr int VM_PER_ENV = 5 * NS + 6 - ((MADRL_ABLATE & 512) ? 1 : 0);  // stores every step iteration issues: NS x (4 dword + 1 float4), reward, done, removed, flag word, record, mask
    static_assert(!PIPE || VM_PER_ENV < 64, "vmcnt range");
    for (int e = blockIdx.x; e < n_envs; e += stride) {
        const int64_t env = phys(e);
        const bool has_next = e + stride < n_envs;  // n_envs + number of workgroups < 2^31
        const int64_t nenv = phys(has_next ? e + stride : e);
        uint32_t nxt_rec = 0, nxt_zm = 0xFFFFFFFFu;
        int nxt_act = 4;
        uint32_t pf_rec, pf_act, pf_zm;
        if constexpr (PIPE) {
            prefetch3(pf_rec, pf_act, pf_zm, d.state + nenv * (int64_t)S::REC_BYTES, rec_off, io.actions + nenv * P, act_off,
                      d.zmask + zm_env(nenv) * S::ZMW, (S::ZSKIP ? ((uint32_t)fresh(lane) & 31u) : zm_lane) * 4u);   // (ZSKIP: worked out again, as S::LEAN_REGS does in fetch_zm -- the rule's values take the register)
        } else {
#if MADRL_ABLATE & 64
            nxt_rec = cur_rec ^ (uint32_t)(fresh(lane) == 0);  // no loads in the loop: is the in-order vmcnt drain what serialises a wave?
            nxt_act = cur_act;
#else
            if (has_next) {
                nxt_rec = fetch_rec(nenv);
                nxt_act = fetch_act(nenv);
                nxt_zm = fetch_zm(nenv);
            }
#endif
        }
        bool skip = false;
        if constexpr (MODE == 0) skip = (io.mask != nullptr && io.mask[env] == 0);
        if (!skip) {
            // -------------------------------------------------------- unpack the record
            uint32_t tick = __builtin_amdgcn_readlane(cur_rec, 0);
            int32_t tstep = (int32_t)__builtin_amdgcn_readlane(cur_rec, 1);
            int32_t map_id = S::FIXED ? 0 : (int32_t)__builtin_amdgcn_readlane(cur_rec, 2);   // (FIXED: one map)
            const uint32_t xyw = (uint32_t)__shfl((int)cur_rec, 4 + (lane >> 1));
            const pr::Cell at = pr::unpack_xy(xyw, lane & 1);
            int x = at.x, y = at.y;
            uint64_t gone = (uint32_t)__builtin_amdgcn_readlane(cur_rec, S::OFF_GONE / 4);  // (uint32_t): readlane returns int, bit 31 must not sign-extend
            if constexpr (S::NGW > 1) gone |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane(cur_rec, S::OFF_GONE / 4 + 1) << 32;
            uint64_t term = (uint32_t)__builtin_amdgcn_readlane(cur_rec, S::OFF_TERM / 4);
            if constexpr (S::NTW > 1) term |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane(cur_rec, S::OFF_TERM / 4 + 1) << 32;
            const uint32_t gid = d.gid_base + (uint32_t)env;
            // round keys recomputed on the SALU, not kept live (FIXED too: holding the twenty keys takes more SGPRs than the flags left -- 8
            // scalars parked in VGPR lanes and read back in the evader draw; holding k0's ten alone: 2)
            const uint32_t k0 = fresh_s(d.k0), k1 = fresh_s(d.k1);
            int np = P, ne = E;  // live pursuers / evader slots (LIVE; the capacity otherwise)
            if constexpr (S::LIVE) {
                const bool here = x != NOT_HERE;
                np = __popcll(__builtin_amdgcn_ballot_w64(isP() && here));
                ne = __popcll(__builtin_amdgcn_ballot_w64(isE() && here));
                if (!here) {  // a slot that does not exist computes on cell (0, 0) and never stores there
                    x = 0;
                    y = 0;
                }
            }
            // a pursuer of the running episode (LIVE: lane < np)
            auto isLP = [&]() {
                if constexpr (S::LIVE) return fresh(lane) < np;
                else return isP();
            };
            bool do_reset = (MODE == 0);
            uint32_t done_bits = 0;
            float rew_out = 0.0f;
            int n_removed = 0;
            bool alive = isLP() || (isE() && !((gone >> eslot) & 1ull));
            int cell = (x + PAD) * GW + y + PAD;

            auto load_map = [&](int mid) {
                if (cached_map == mid) return;
                const KArgsPtr ka = cold_args();
                // the map layer and its need bytes in batches of at most FILL_BATCH trips (the slot constants are live here): per batch all
                // loads, one wait to zero, then the LDS writes (table staging).  One batch up to 16 trips -- 9 at 16 x 16, obs_range 7;
                // a 32 x 32 map on one wavefront has 27 and reloads in two
                fill_trips<S, 64, F::J_MAP, F::J_VT, FILL_BATCH, false>(L, ulane, nullptr, ka->d.fmaps + (int64_t)mid * ka->d.fmap_stride, nullptr, nullptr);
                cached_map = mid;
                wave_sync();
            };
            if constexpr (!S::FIXED) load_map(map_id);

            if constexpr (MODE == 1) {
                const bool e_alive = alive && !isP();
                // ---------------------------------------------------- pre-move reward (:359-381)
                if (e_alive) atomicAdd(&layer[cell], 1u);
                wave_sync();
                int kpre = 0;
                if (isP()) {  // np.clip keeps a border pursuer on its own cell (:374-380)
                    const pr::Clip4 n = pr::clipped_neighbours<GW, S::XS, S::YS>(x, y);
                    const uint32_t *ec = &L[2 * GSZ];
                    kpre = (int)(ec[cell - n.dxm] + ec[cell + n.dxp] + ec[cell + n.dyp] + ec[cell - n.dym]);
                }
                wave_sync();
                if (e_alive) atomicSub(&layer[cell], 1u);
                // ---------------------------------------------------- moves (:229-241), branch-free
                // evader draw: index in the evader layer = alive evaders in lower slots
                const int kidx = __popcll((~gone) & ((1ull << (eslot & 63)) - 1ull));
                int act = cur_act;
                bool injected = false;
                if constexpr (CTRL) {
                    // action k belongs to the k-th remaining evader (:229-230 with agent_layer = evader_layer); evaders past the first P of
                    // the layer stay; every pursuer moves by one pursuer_controller.act() (:238-241)
                    const int from_k = __builtin_amdgcn_ds_bpermute((kidx < P ? kidx : 0) * 4, cur_act);   // lane k holds action k
                    injected = io.inj_eact != nullptr;
                    int pact;
                    if (injected) pact = isP() ? io.inj_eact[env * P + lane] : 4;
                    else pact = pr::pursuer_action(gid, tick, (uint32_t)lane, k0, k1);
                    act = isP() ? pact : (kidx < P ? from_k : 4);
                    injected = true;   // (nothing below draws evader moves)
                } else if constexpr (INJECT) {
                    injected = io.inj_eact != nullptr;
                    if (injected && e_alive) act = io.inj_eact[env * E + kidx];
                }
                if (!injected) {
#if MADRL_ABLATE & 4
                    u32x4 r; r.x = (gid * 2654435761u + tick * 40503u + (uint32_t)kidx * 2246822519u) ^ k0 ^ k1;
#else
                    const u32x4 r = philox4x32_10(gid, tick, (uint32_t)kidx, TAG_EVADER_ACT, k0, k1);
#endif
                    if (!isP()) act = (int)__umulhi(r.x, 5u);  // RandomPolicy.act, Controllers.py:15-16
                }
                // DiscreteAgent.step, DiscreteAgent.py:69-97
                const int dcell = pr::move_dcell<GW>(act);
                const bool tflag = (term >> lane) & 1ull;
                const bool in_building = L[cell] != 0u;          // layer 0 is +0.0f only on free in-map cells
                const bool target_free = L[cell + dcell] == 0u;  // building or outside the map otherwise
                const bool newterm = alive && !tflag && in_building;
                if (alive && !tflag && !in_building && target_free) {
                    cell += dcell;
                    x += pr::move_dx(act), y += pr::move_dy(act);
                }
                term |= __ballot(newterm);
                if (alive) atomicAdd(&layer[cell], 1u);  // :244-246
                wave_sync();
                // ---------------------------------------------------- catch resolution (:463-521)
                bool caught = false;
                if (e_alive) {
                    const uint32_t *pc = &L[GSZ];
                    if (LC::surround(d)) caught = pr::cells_with_pursuers(pc[cell - GW], pc[cell + GW], pc[cell + 1], pc[cell - 1], SENT) == (int)need_tab[x * S::YS + y];  // :523-540
                    else caught = (int)pc[cell] >= d.n_catch;  // :498
                    if (caught) atomicAdd(&layer[cell], CAUGHT);
                }
                const uint64_t caught_mask = __ballot(caught) >> P;
                gone |= caught_mask;
                wave_sync();
                // ---------------------------------------------------- rewards (:254-262)
                double r = 0.0;
                if (isLP()) {
                    const uint32_t *ec = &L[2 * GSZ];
                    bool sur;
                    if (LC::surround(d)) sur = pr::caught_beside(ec[cell - GW], ec[cell + GW], ec[cell + 1], ec[cell - 1], SENT, CAUGHT);
                    else sur = ec[cell] >= CAUGHT;  // :503-506
                    double catchr = d.catchr;
                    if constexpr (INJECT) { if (d.catchr_env != nullptr) catchr = sload_f64(d.catchr_env, env); }
                    r = pr::pursuer_reward(catchr, kpre, d.term_pursuit, sur, urgency);
                }
                if (LC::reward_global(d)) {  // [rewards.mean()] * n_pursuers, numpy summation order
                    double all[P];
#pragma unroll
                    for (int k = 0; k < P; ++k) {
                        if constexpr (S::LEAN_REGS) {   // lane k's value by its constant byte address: __shfl keeps `lane & 64` as a loop constant
                            const uint64_t rb = __builtin_bit_cast(uint64_t, r);
                            const uint32_t rl = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * k, (int)(uint32_t)rb);
                            const uint32_t rh = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * k, (int)(uint32_t)(rb >> 32));
                            all[k] = __builtin_bit_cast(double, ((uint64_t)rh << 32) | rl);
                        } else {
                            all[k] = __shfl(r, k);
                        }
                    }
                    if constexpr (S::LIVE) r = isLP() ? np_sum_first<P>(all, np) / (double)np : 0.0;
                    else r = np_sum_regs<P>(all) / (double)P;
                }
                tick += 1;
                tstep += 1;
                constexpr uint64_t all_e = (1ull << E) - 1ull;
                if ((gone & all_e) == all_e) done_bits |= 1u;  // :383-389
                if (d.max_steps > 0 && tstep >= d.max_steps) done_bits |= 2u;
                do_reset = d.auto_reset && done_bits != 0;
                rew_out = (float)r;
                n_removed = __popcll(caught_mask);
            }

            // Pipeline hinge: everything above only LOADS from HBM (issued one env ago), everything
            // below only STORES.  Touching the prefetched registers here makes the compiler wait
            // for the next env's record now -- when only loads and the previous env's long-issued
            // stores are outstanding -- instead of at the loop back-edge, where an in-order
            // vmcnt(0) would also wait for this env's observation stores to reach HBM.
            if constexpr (!PIPE) asm volatile("" : "+v"(nxt_rec), "+v"(nxt_act), "+v"(nxt_zm));
            uint32_t zm = cur_zm;  // stale-zero mask of this env: byte k, bit (4 - s) = cell k of slot s
            if constexpr (S::ZM16) zm = zm16::unpack(fresh(lane) < 32 ? cur_zm : cur_zm >> 16, zm_keep);  // (cur_zm: as loaded, two lanes' halves)
            // (S::ZSKIP: the position the lane's 16 bits leave out reads "unknown" -- unpack fills it with its neighbour's bit, which only
            // `out4 & old4` may consult, never the rule that trusts a zero; pack drops the position again)
            if constexpr (S::ZSKIP) zm |= add_here<0x01010101u>(zm_keep);

            // One observation pass normally.  On auto-reset two: the reference sequence is step()
            // then reset(), both write the persistent observation buffer and the cells the second
            // write skips keep the first one's values.  `alive` is the PRE-catch set in the first
            // pass: a just-caught evader is still drawn in channel 2 (Q6) and its cell (count +
            // CAUGHT mark) is zeroed with the others.
            const int npass = (MODE == 1 && do_reset) ? 2 : 1;
            for (int pass = 0; pass < npass; ++pass) {
                if (do_reset && pass == npass - 1) {
                    // -------------------------------------------------- reset (:173-207)
                    gone = 0ull;
                    term = 0ull;
                    const KArgsPtr ka = cold_args();
                    double cw;
                    if constexpr (S::FIXED) cw = ka->d.cw;
                    else cw = ka->d.cw_env != nullptr ? sload_f64(ka->d.cw_env, env) : ka->d.cw;
                    const int max_opponents = S::FIXED ? 0 : ka->d.max_opponents;
                    // (FIXED: the draws below see their inputs as values made HERE, so that their lane-uniform first Philox rounds cannot
                    // be hoisted out of the branch into every env's straight-line code -- 1 env in 500 resets)
                    uint32_t rgid = gid, rk0 = k0, rk1 = k1;
                    if constexpr (S::FIXED) asm volatile("" : "+s"(rgid), "+s"(tick), "+s"(rk0), "+s"(rk1));
                    bool inj_map = false, inj_pos = false;
                    if constexpr (MODE == 0) {
                        inj_map = io.inj_map != nullptr;
                        inj_pos = io.inj_pos != nullptr;
                    }
                    if (inj_map) {
                        map_id = __builtin_amdgcn_readfirstlane(io.inj_map[env]);
                    } else if (!S::FIXED && ka->d.sample_maps) {  // :182-183
                        const u32x4 rm = philox4x32_10(rgid, tick, 0u, TAG_RESET_ENV, rk0, rk1);
                        map_id = (int)__umulhi(rm.x, (uint32_t)ka->d.n_maps);
                    }
                    if constexpr (!S::FIXED) load_map(map_id);
                    const pr::Window win = pr::reset_window(rgid, tick, rk0, rk1, cw, S::XS, S::YS);
                    int n_create = E;   // (an injected position with x < 0 marks an evader slot that is not created)
                    if constexpr (S::LIVE) {  // the pending counts take effect
                        const pr::Counts live = pr::clamp_pending(pending_count(env, 0), pending_count(env, 1), P, E);
                        np = live.np, ne = n_create = live.ne;
                    }
                    if (max_opponents > 0 && !inj_pos) n_create = pr::reset_n_create(rgid, tick, rk0, rk1, max_opponents, S::LIVE ? ne : E);
                    bool exists = false;
                    if (isAgent()) {  // create_agents / feasible_position, agent_utils.py:12-47
                        if constexpr (S::LIVE) exists = isLP() || (!isP() && eslot < n_create);
                        else exists = isP() || eslot < n_create;
                        if (inj_pos) {
                            x = io.inj_pos[(env * A + lane) * 2];
                            y = io.inj_pos[(env * A + lane) * 2 + 1];
                            if (!isP() && x < 0) exists = false;
                        } else {
                            for (uint32_t att = 0; att < 1024u; ++att) {
                                const uint32_t aidx = S::LIVE ? (uint32_t)(isP() ? lane : np + eslot) : (uint32_t)lane;
                                const u32x4 rp = philox4x32_10(rgid, tick, aidx, TAG_RESET_POS | (att << 8), rk0, rk1);
                                x = win.xlb + (int)__umulhi(rp.x, (uint32_t)(win.xub - win.xlb));   // (pr::reset_cell's text: the helper
                                y = win.ylb + (int)__umulhi(rp.y, (uint32_t)(win.yub - win.ylb));   // changes the headline step kernel)
                                // building cells hold fl32(1/norm) != 0; window cells are inside the map
                                if (L[(x + PAD) * GW + y + PAD] == 0u) break;
                            }
                        }
                        if (exists) {
                            cell = (x + PAD) * GW + y + PAD;
                            atomicAdd(&layer[cell], 1u);  // :201-203
                        } else {
                            x = 0;
                            y = 0;
                        }
                    }
                    gone = __ballot(isE() && !exists) >> P;
                    alive = exists;
                    tick += 1;
                    tstep = 0;
                    wave_sync();
                }
                // ------------------------------------------------------ observations (:418-461)
                // integer counts -> float32 observation values, in place (a wave executes the
                // ds_read of every lane before the ds_write of any lane)
                if constexpr (S::LIVE) {  // the id values k / np of this pass's pursuer count
                    if (np != cached_np) {
                        if (lane < P) L[S::X_ID + lane] = __float_as_uint((float)((double)lane / (double)np));
                        cached_np = np;
                        wave_sync();
                    }
                }
                uint32_t cnt = 0;
                if (alive) cnt = layer[cell] & 0xFFFFu;
                wave_sync();
                if (alive) layer[cell] = L[S::X_VTAB + cnt];
                wave_sync();
#if MADRL_ABLATE & 8
                if (d.n_envs < 0)
#endif
                {
                    // byte offset of this pursuer's window origin in L; the slot constants are byte offsets too, so a cell address is one add
                    int origin = isP() ? ((x - S::OFF + PAD) * GW + (y - S::OFF + PAD)) * 4 : 0;
                    int n_rows = P;
                    if constexpr (CTRL) {
                        // observers (collect_obs walks range(n_pursuers) over evaders_gone, :418-428): the remaining evaders of slots
                        // 0..P-1 in slot order; row k = the k-th of them.  Each tells lane k its window origin through LDS.
                        const uint64_t obsv = ~gone & ((1ull << P) - 1ull);
                        n_rows = __popcll(obsv);
                        const bool is_obs = isE() && eslot < P && ((obsv >> (eslot & 63)) & 1ull);
                        if (is_obs) L[S::X_OBSV + __popcll(obsv & ((1ull << (eslot & 63)) - 1ull))] = (uint32_t)(((x - S::OFF + PAD) * GW + (y - S::OFF + PAD)) * 4);
                        wave_sync();
                        origin = (isP() && lane < n_rows) ? (int)L[S::X_OBSV + lane] : 0;
                    }
                    if constexpr (S::LIVE) n_rows = np;
                    // SGPR base + one loop-invariant 32-bit VGPR offset (+ immediate) for every store of the row
                    const char *orow_u = (const char *)uniform_ptr(io.obs + env * (int64_t)(P * S::D));
                    // if that base came through v_readfirstlane (a VALU write of an SGPR), a vector-memory instruction may read it as its
                    // scalar address only 5 wait states later; the compiler cannot see the stores inside the asm blocks below
                    asm volatile("s_nop 4" : "+s"(orow_u));
                    const uint32_t voff = ulane * 16u;
                    // (orow_u and voff are float32 geometry and feed store_slot_masked alone, which an S::H16 kernel cannot reach -- see the
                    // static_assert in it: in those kernels they are values nothing dereferences)
                    // (the two-buffer pass: both rows as global pointers of their own, its loads and stores are the compiler's)
                    // (binary16 buffers, S::H16: the rows hold half as many bytes -- P * D / 2 of the pointers' float-sized units)
                    [[maybe_unused]] const auto prow_g = uniform_ptr(S::TO ? io.obs_prev + env * (int64_t)(P * S::D / (S::H16 ? 2 : 1)) : io.obs);
                    [[maybe_unused]] const auto orow_g = uniform_ptr(io.obs + env * (int64_t)(P * S::D / (S::H16 ? 2 : 1)));
                    const char *Lb = reinterpret_cast<const char *>(L);
                    auto cell_at = [&](int off) -> uint32_t { return *reinterpret_cast<const uint32_t *>(Lb + off); };
                    uint32_t acc = 0u;  // the new mask, slot by slot
                    if constexpr (S::H16) {
                        // the second pass of a fused auto-reset reads back the slots the first pass stored (half_slot_in_place): they have
                        // all been acknowledged first
                        if (pass == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                    // the two-buffer pass (S::TO, the step's pass): per slot the elements that come from the previous buffer (one flag per byte)
                    // and the new mask bits
                    [[maybe_unused]] uint32_t to_need[S::TO ? NS : 1], to_bits[S::TO && !S::H16 ? NS : 1];
                    static_for<0, NS>([&](auto sc) {
                        constexpr int s = decltype(sc)::value;
                        const int base = __builtin_amdgcn_ds_bpermute(s_src[s], origin);
                        const uint32_t v0 = cell_at(base + s_cst[s][0]);
                        const uint32_t v1 = cell_at(base + s_cst[s][1]);
                        const uint32_t v2 = cell_at(base + s_cst[s][2]);
                        const uint32_t v3 = cell_at((int)__umul24((uint32_t)base, (uint32_t)s_rel3[s]) + s_cst[s][3]);
                        // flags of the four cells, one per byte (bit 0).  The top byte of a value is 0x00 for +0.0f, 0x3D..0x41 for the
                        // positive observation values and 0xFF for SENT (outside the map).
                        const uint32_t top = __builtin_amdgcn_perm(v1, v0, 0x0C0C0703u) | __builtin_amdgcn_perm(v3, v2, 0x07030C0Cu);
                        const uint32_t out4 = (top >> 7) & 0x01010101u;                    // outside the map: not written
                        const uint32_t nz4 = ((top >> 5) | (top >> 6)) & 0x01010101u;      // value != 0 (meaningful where inside)
                        const uint32_t old4 = (zm >> (NS - 1 - s)) & 0x01010101u;          // holds a value not known to be zero
                        const uint32_t dirty = out4 & old4;                                 // outside AND possibly non-zero: must stay untouched
                        if constexpr (S::TO) {
                            if (pass == 0) {   // the two-buffer pass, part 1: this slot's values and which of them come from io.obs_prev
                                bool row_live = true;
                                if constexpr (S::LIVE) row_live = (s_src[s] >> 2) < n_rows;
                                const bool in_row = (64 * (s + 1) <= S::NQ) ? true : (fresh(lane) + 64 * s < S::NQ);
                                const uint32_t need4 = in_row ? (row_live ? dirty : 0x01010101u) : 0u;
                                to_need[s] = need4;
                                if constexpr (S::H16) {   // the new mask bits of all slots in ONE register, slot s at bit s of each byte (as in acc)
                                    if constexpr (s == 0) to_bits[0] = ~need4 & ~out4 & nz4;
                                    else to_bits[0] |= (~need4 & ~out4 & nz4) << s;
                                } else {
                                    to_bits[s] = ~need4 & ~out4 & nz4;
                                }
                                return;
                            }
                        }
                        bool valid = (64 * (s + 1) <= S::NQ) ? true : (fresh(lane) + 64 * s < S::NQ);
                        uint32_t new4 = (out4 & old4) | (~out4 & nz4);   // the slot's new mask bits
                        if constexpr (CTRL || S::LIVE) {
                            const bool row_live = (s_src[s] >> 2) < n_rows;   // rows of absent observers keep their contents -- and their flags
                            new4 = row_live ? new4 : old4;
                            valid = valid && row_live;
                        }
                        acc = (acc << 1) | new4;
                        bool clean = dirty == 0u;
#if MADRL_ABLATE & 1
                        valid = d.n_envs < 0;
#endif
#if MADRL_ABLATE & (2 | 512)
                        clean = true;
#endif
                        // The lane's part of the slot as one integer, so that every store mask below is ONE vector compare (a lane mask
                        // built from two compares would be an s_and_b64 on the scalar unit, which all four SIMDs of a CU share):
                        //   0 = one float4 (clean), 1 .. 0x01010101 = dword stores of the inside cells (dirty), 0x80000000 = nothing (past the row)
                        const uint32_t st = valid ? (clean ? 0u : dirty) : 0x80000000u;
#if MADRL_ABLATE & 32
                        // what a scheme that REMEMBERS small stale values (two bits per cell: 0, 0.1, 0.2, other) and rebuilds them would add to
                        // this pass: about twenty vector instructions per slot (second byte of the four values, two flag planes, byte-to-float
                        // conversions, one fused multiply-add per cell).  With `& 2` (every float4 stored whole) this prices the scheme:
                        // its stores at their best, its instructions at their count (Pursuit fast path, "stale values remembered").
                        {
                            uint32_t burn = acc;
                            asm volatile("v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n"
                                         "v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n"
                                         "v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n"
                                         "v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1\n v_xor_b32 %0, %0, %1"
                                         : "+v"(burn) : "v"(v0));
                            acc = burn;   // (an even number of XORs with the same value: unchanged)
                        }
#endif
#if MADRL_ABLATE & 128
                        // the price of one scalar instruction per env: 20 dependent SALU per slot (100 per env at NS = 5) on a dummy SGPR
                        // that feeds nothing observable ("what a SALU costs")
                        {
                            uint32_t sburn = fresh_s(0u);
                            asm volatile("s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n"
                                         "s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n"
                                         "s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n"
                                         "s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1\n s_add_u32 %0, %0, 1"
                                         : "+s"(sburn) : : "scc");
                        }
#endif
                        if constexpr (S::H16) {
                            // binary16 buffer: the slot is 8 bytes of io.obs.  Whole slots, load-blend-store: a slot with a cell that must
                            // stay untouched reads the first pass's word back (the same lane stored it, and it has been waited for) and
                            // keeps those halves; outside cells known to be zero are written as the zero bits they hold.
                            half_slot_in_place(orow_g, 64u * s + ulane, valid, clean ? 0u : dirty, v0, v1, v2, v3);
                        } else {
                            // (float32 geometry from here on: orow_u + 4096 (s / 4), voff = lane * 16.  The `if constexpr` keeps it out of an H16
                            // kernel; store_slot_masked<.., S::H16> refuses to compile for one should this ever be restructured)
                            const void *sb = orow_u + 4096 * (s / 4);
                            // dirty: element k is stored iff it is inside the map, i.e. v_k != SENT, i.e. v_k < lim (unsigned); other lanes: lim = 0.
                            // (fresh(): kept as a value, or the compiler splits `v_k < select` back into two lane masks and an s_and_b64)
                            const uint32_t lim = (uint32_t)fresh((st - 1u < 0x01010101u) ? (int)SENT : 0);
                            // One non-temporal float4 unless a cell must stay untouched; nothing if all four are outside and known zero.
                            // Outside cells (SENT = -1 as an integer) are written as the +0.0f they already hold.
                            // Whole 64-byte chunks: a slot that lies ENTIRELY outside the map and whose cells are known to hold zero normally
                            // stores nothing -- but when another slot of its aligned group of four lanes is written, it is written too (as the
                            // zeros it already holds), so that the group's 64 bytes leave the CU as one full chunk instead of a partial one the
                            // memory side has to merge.  Round 4, mask equilibrium, 65 536 envs: 80.0 -> 71.6 us per launch (groups of two:
                            // 74.0, of eight: 75.8; scripts/zmask_drift.py).  (The two-wavefront kernel, whose 32 x 32 map leaves far fewer cells outside, loses
                            // with the same rule -- 86.5 against 80.4 us per 32 768-env launch -- and does not apply it.)
                            // The group of four lanes is a DPP quad: a clean lane stores iff a clean lane of its quad has a cell inside the map.
                            uint32_t nt;
                            if constexpr (S::ZSKIP) {
                                // Zeros over known zeros: `x` = the cells of this lane's slot that are NOT "known to hold +0.0f before this
                                // pass and holding it after": an old bit set, or a non-zero value stored now.  A clean lane without one would
                                // overwrite sixteen bytes of zeros with zeros (its outside cells are known zeros too, or it would be dirty),
                                // so leaving its store out is exact lane by lane; the quad decides together only to keep chunks whole: the
                                // clean lanes of a quad store iff one of them has an x.  That implies the condition of the rule above (a clean
                                // lane's old bits and new values sit on cells inside the map) and costs what it cost: x takes the place of
                                // the inside flags in the same quad_or and the same single compare.  Dirty lanes, lanes past the row and
                                // lanes in an absent observer's row (st != 0) say nothing; a dirty lane stores its inside cells one by one
                                // whatever its quad does.
#if MADRL_ABLATE & 1024
                                const uint32_t x = ~out4 & nz4;
#else
                                const uint32_t x = old4 | new4;   // (= old4 | (~out4 & nz4): the kept bits of new4 are old bits)
#endif
                                const uint32_t grp = quad_or(st == 0u ? x : 0u);
                                nt = (uint32_t)fresh(st == 0u ? (int)grp : 0);
                            } else {
                                const uint32_t grp = quad_or(st == 0u ? (out4 ^ 0x01010101u) : 0u);
                                nt = (uint32_t)fresh(st == 0u ? (int)grp : 0);
                            }
                            const v4f_t val = {__uint_as_float((uint32_t)max((int)v0, 0)), __uint_as_float((uint32_t)max((int)v1, 0)),
                                               __uint_as_float((uint32_t)max((int)v2, 0)), __uint_as_float((uint32_t)max((int)v3, 0))};
                            // An outside cell with a non-zero stale value: leave it alone (Q2), store the inside cells one by one.  Plain
                            // (L2-cached) stores: partial lines must merge in L2 -- nontemporal partial writes cost a read-modify-write
                            // at the memory side (3x slower).  They are issued BEFORE the non-temporal store of the slot's other lanes: the
                            // line is then in L2 when the streaming store arrives and leaves as one write (the other order: 175 us, not 77).
                            store_slot_masked<1024 * (s % 4), S::H16>(sb, voff, v0, v1, v2, v3, val, __builtin_amdgcn_ballot_w64(v0 < lim),
                                                              __builtin_amdgcn_ballot_w64(v1 < lim), __builtin_amdgcn_ballot_w64(v2 < lim),
                                                              __builtin_amdgcn_ballot_w64(v3 < lim), __builtin_amdgcn_ballot_w64(nt != 0u));
                        }
                    });
                    if constexpr (S::TO) {
                        if (pass == 0) {
                            // part 2, in groups of up to TG slots: the group's loads, all issued before the one wait -- and none, and no wait, in
                            // a wavefront none of whose lanes needs one (vmcnt retires in order: a wait for a load is also a wait for every
                            // store issued before it) -- then every float4 of the group leaves whole (the values are read from LDS again:
                            // keeping them across the loads would cost four registers per slot)
                            typedef uint32_t v4u_t __attribute__((ext_vector_type(4)));
                            typedef __attribute__((address_space(1))) v4u_t gv4u_t;
                            typedef __attribute__((address_space(1))) v4f_t gv4f_t;
                            constexpr int TG = NS <= 5 ? NS : 4;
                            // (binary16 buffers: the old slot is one 8-byte word, two halves per dword)
                            typedef uint32_t v2u_t __attribute__((ext_vector_type(2)));
                            typedef __attribute__((address_space(1))) v2u_t gv2u_t;
                            using old_t = std::conditional_t<S::H16, uint64_t, v4u_t>;
                            using gold_t = std::conditional_t<S::H16, __attribute__((address_space(1))) uint64_t, gv4u_t>;
                            auto emit = [&](auto sc, const old_t oldv) {
                                constexpr int s = decltype(sc)::value;
                                const int base = __builtin_amdgcn_ds_bpermute(s_src[s], origin);
                                const uint32_t need4 = to_need[s];
                                uint32_t w0 = (uint32_t)max((int)cell_at(base + s_cst[s][0]), 0);
                                uint32_t w1 = (uint32_t)max((int)cell_at(base + s_cst[s][1]), 0);
                                uint32_t w2 = (uint32_t)max((int)cell_at(base + s_cst[s][2]), 0);
                                uint32_t w3 = (uint32_t)max((int)cell_at((int)__umul24((uint32_t)base, (uint32_t)s_rel3[s]) + s_cst[s][3]), 0);
                                if constexpr (S::H16) {
                                    const bool in_row = (64 * (s + 1) <= S::NQ) ? true : (fresh(lane) + 64 * s < S::NQ);
                                    // converted and packed; the kept halves come from the old word, 16 bits as they are
                                    const uint32_t oldx = (uint32_t)oldv, oldy = (uint32_t)(oldv >> 32);
                                    uint32_t lo = (uint32_t)half_bits(__uint_as_float(w0)) | ((uint32_t)half_bits(__uint_as_float(w1)) << 16);
                                    uint32_t hi = (uint32_t)half_bits(__uint_as_float(w2)) | ((uint32_t)half_bits(__uint_as_float(w3)) << 16);
                                    const uint32_t klo = ((need4 & 0x00000001u) ? 0x0000FFFFu : 0u) | ((need4 & 0x00000100u) ? 0xFFFF0000u : 0u);
                                    const uint32_t khi = ((need4 & 0x00010000u) ? 0x0000FFFFu : 0u) | ((need4 & 0x01000000u) ? 0xFFFF0000u : 0u);
                                    lo = (lo & ~klo) | (oldx & klo);
                                    hi = (hi & ~khi) | (oldy & khi);
                                    const uint32_t oldnz = ((oldx & 0xFFFFu) != 0u ? 0x00000001u : 0u) | ((oldx >> 16) != 0u ? 0x00000100u : 0u) |
                                                           ((oldy & 0xFFFFu) != 0u ? 0x00010000u : 0u) | ((oldy >> 16) != 0u ? 0x01000000u : 0u);
                                    acc = (acc << 1) | ((to_bits[0] >> s) & 0x01010101u) | (need4 & oldnz);   // per half: "the loaded 16 bits are non-zero"
                                    if (in_row) __builtin_nontemporal_store(v2u_t{lo, hi}, reinterpret_cast<gv2u_t *>(orow_g) + (64u * s + ulane));
                                } else {
                                    if (need4 & 0x00000001u) w0 = oldv.x;
                                    if (need4 & 0x00000100u) w1 = oldv.y;
                                    if (need4 & 0x00010000u) w2 = oldv.z;
                                    if (need4 & 0x01000000u) w3 = oldv.w;
                                    const uint32_t oldnz = (oldv.x != 0u ? 0x00000001u : 0u) | (oldv.y != 0u ? 0x00000100u : 0u) |
                                                           (oldv.z != 0u ? 0x00010000u : 0u) | (oldv.w != 0u ? 0x01000000u : 0u);
                                    acc = (acc << 1) | to_bits[s] | (need4 & oldnz);   // the mask bit of a kept cell: "the loaded value is non-zero"
                                    const bool in_row = (64 * (s + 1) <= S::NQ) ? true : (fresh(lane) + 64 * s < S::NQ);
                                    if (in_row) {
                                        const v4f_t wv = {__uint_as_float(w0), __uint_as_float(w1), __uint_as_float(w2), __uint_as_float(w3)};
                                        __builtin_nontemporal_store(wv, reinterpret_cast<gv4f_t *>(orow_g) + (64u * s + ulane));
                                    }
                                }
                            };
                            static_for<0, (NS + TG - 1) / TG>([&](auto gc) {
                                constexpr int g0 = decltype(gc)::value * TG, g1 = g0 + TG < NS ? g0 + TG : NS;
                                uint32_t any = 0u;
#pragma unroll
                                for (int s = g0; s < g1; ++s) any |= to_need[s];
                                if (__builtin_amdgcn_ballot_w64(any != 0u) != 0ull) {
                                    old_t old[TG];
#pragma unroll
                                    for (int s = g0; s < g1; ++s) {
                                        old[s - g0] = old_t{};
                                        if (to_need[s] != 0u) old[s - g0] = reinterpret_cast<const gold_t *>(prow_g)[64u * s + ulane];
                                    }
                                    static_for<g0, g1>([&](auto sc) { emit(sc, old[decltype(sc)::value - g0]); });
                                } else {
                                    static_for<g0, g1>([&](auto sc) { emit(sc, old_t{}); });
                                }
                            });
                        }
                    }
                    zm = acc;
                    if constexpr (S::ZSKIP) zm |= add_here<0x01010101u>(zm_keep);   // (the second pass of a fused auto-reset: as above)
                }
                wave_sync();
                if (alive) layer[cell] = 0u;  // restore the count layers for the next pass / env
                wave_sync();
            }
#if MADRL_ABLATE & 16
            if (d.n_envs < 0)
#endif
            if constexpr (MODE == 1) {
                if (isP()) uniform_ptr(io.rew + env * P)[ulane] = rew_out;
                if (fresh(lane) == 0) {
                    io.done[env] = (uint8_t)done_bits;
                    io.removed[env] = n_removed;
                    if constexpr (S::FIXED) d.flags[env] = done_flag_word(done_bits);
                    else cold_args()->d.flags[env] = done_flag_word(done_bits);   // (the pointer is not kept in SGPRs across the env loop)
                }
            }
            // ---------------------------------------------------------- registers -> state record
            // one coalesced dword store: lane k writes dword k of the record
            {
                int myxy = x | (y << 8);
                if constexpr (S::LIVE) {
                    if (!(isP() ? isLP() : eslot < ne)) myxy = NOT_HERE | (NOT_HERE << 8);
                }
                // (S::LEAN_REGS: worked out again, like the mask index in fetch_zm -- two loop constants fewer)
                [[maybe_unused]] auto src_of = [&](auto kc) -> int {
                    if constexpr (S::LEAN_REGS) return ((fresh(lane) >= 4 ? 2 * (fresh(lane) - 4) : 0) + decltype(kc)::value) * 4;
                    else return decltype(kc)::value ? rec_src1 : rec_src0;
                };
                const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src_of(std::integral_constant<int, 0>{}), myxy);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src_of(std::integral_constant<int, 1>{}), myxy);
                uint32_t w = (lo & 0xFFFFu) | (hi << 16);
                // the uniform header / bit-set dwords go in with v_writelane (one VALU op each, no lane mask)
                put_lane<0>(w, tick);
                put_lane<1>(w, (uint32_t)tstep);
                put_lane<2>(w, (uint32_t)map_id);
                put_lane<3>(w, 0u);
                put_lane<S::OFF_GONE / 4>(w, (uint32_t)gone);
                if constexpr (S::NGW > 1) put_lane<S::OFF_GONE / 4 + 1>(w, (uint32_t)(gone >> 32));
                put_lane<S::OFF_TERM / 4>(w, (uint32_t)term);
                if constexpr (S::NTW > 1) put_lane<S::OFF_TERM / 4 + 1>(w, (uint32_t)(term >> 32));
                put_zero_from<S::OFF_TERM / 4 + S::NTW, S::REC_DW>(w);  // padding dwords
#if MADRL_ABLATE & 16
                if (d.n_envs < 0)
#endif
                if (fresh(lane) < S::REC_DW)
                    uniform_ptr(reinterpret_cast<uint32_t *>(d.state + env * (int64_t)S::REC_BYTES))[ulane] = w;
#if MADRL_ABLATE & 16
                if (d.n_envs < 0)
#endif
#if !(MADRL_ABLATE & 512)
                if constexpr (S::ZM16) {
                    // 16 bits per lane: lane l < 32 stores its own half and lane l + 32's, ONE 128-byte line per env
                    const uint32_t h = zm16::pack(zm, zm_keep);
                    const uint32_t other = __builtin_amdgcn_permlane32_swap(h, h, false, false)[1];   // lanes 0..31: lane + 32's h
                    if (fresh(lane) < 32) uniform_ptr(d.zmask + zm_env(env) * S::ZMW)[ulane] = h | (other << 16);
                } else {
                    uniform_ptr(d.zmask + zm_env(env) * 64)[ulane] = zm;
                }
#endif
            }
        }
        if constexpr (PIPE) {
            prefetch_wait<VM_PER_ENV>(pf_rec, pf_act, pf_zm);
            nxt_rec = (fresh(lane) < S::REC_DW) ? pf_rec : 0u;
            nxt_act = (int)pf_act;  // lanes that are not pursuers never read it
            nxt_zm = pf_zm;
        }
        cur_rec = nxt_rec;
        cur_act = nxt_act;
        cur_zm = nxt_zm;
    }
}

// host side: launches the two-buffer step kernel <S, 1, true> of a TShape / TLShape (defined and instantiated for every X / XL line of
// pursuit_to_specializations.def in pursuit_to.hip)
template <class S>
void wave_to_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s);
// ... and of a THShape / TLHShape: binary16 buffers, io.obs and io.obs_prev are the half pointers, cast (pursuit_to_f16.hip, pursuit_to_f16_live.hip)
template <class S>
void wave_to_f16_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s);
// ... and the fixed-constants step kernel <S, 1, false> of an FShape (defined and instantiated for every XF line of
// pursuit_fixed_specializations.def in pursuit_fixed.hip)
template <class S>
void wave_fixed_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s);

}  // namespace pw
}  // namespace madrl
