// hostage_crowd.hip -- ContinuousHostageWorld for envs beyond one wavefront's worth of particles (gfx950 / CDNA4), float32: hw_crowd_kernel,
// one workgroup of NW wavefronts per env.  The scheme (phases, sensing passes, the ordered reach walk) and the code it shares with
// ww_crowd_kernel are in particle_crowd.hpp; this file is the oracle's hw_step_env in its order.  Limits:
//   n_good <= 128            a thread owns at most one rescuer
//   n_hostages <= 64         the saved mask is one 64-bit word in the record, in get_state and in the oracle (64 itself works: "all saved" is ~0)
//   at most 1 023 particles, n_sensors in 1..256, n_coop_save >= 1
// The record is the one hostage_kernel reads and writes (the two kernels are interchangeable on one state buffer).
//
// LDS (dynamic, hw_crowd_lds_bytes; about 35 KB at the limits, 2 KB at 20 / 30 / 40):
//   S     the packed state record  X[NP][2] | V[NP][2] | key[2] | bomb[2] | saved_lo saved_hi | flags | t | tick     (<= 16 KB)
//   SEN   sensor unit vectors [K][2]
//   ACT   the scaled actions [Nr][2]: the global control penalty sums them row-major
//   COL   collision bits, per rescuer one 64-bit word for the hostages and one per chunk of 64 criminals   (<= 14 KB)
//   CAU / ENC   ho_caught | cr_caught bits per chunk / ho_enc bits;  KEB / BOB   key / bomb contact bit per rescuer
// The observation row is NOT staged.  Reference lines (:n) are hostage.py's, as in hostage.hip.  What the processing of :365-383 decides
// (saved mask, gate, bombed, done) is known after B2, before anything reads it.
// The kernel's text is hostage_crowd_body.inc, included inside the two __global__ entries below (as waterworld_crowd_body.inc is): the
// fixed-shape entry keeps its two arguments, its name and its code, the live-count entry has the count arrays as a third argument.
#include "particle_crowd.hpp"
#include "hostage_dev.hpp"

// wavefronts per workgroup (a profiling variant builds the other value: scripts/hostage_crowd_time.py)
#ifndef MADRL_HWC_NW
#define MADRL_HWC_NW 4
#endif

namespace {

using namespace madrl;

// MODE 0: reset(mask)   MODE 1: step (+ fused auto-reset)
// LIVE (hw_crowd_kernel_live, madrl_hostage_set_particle_counts): d.Nr / d.Nh / d.Nc are a CAPACITY (Rc, Hc, Cc) and every env runs its own
// counts (cn.live).  Whatever a caller sees stays at the capacity, slotted by class: rescuer i at slot i, hostage m at Rc + m, criminal m
// at Rc + Hc + m in the record; criminal m at row m of inj_resp (stride Cc); the action / reward / observation rows (stride Rc).  The
// record is compacted into packed arrays of the live counts on its way into LDS and scattered back on its way out ((-1, -1) / 0 into the
// slots that do not exist), so the phases between run on the live counts as they stand: the reset's draw indices (bomb at 1 + NP), "all
// saved" (all_h), the not_saved_reward term and the control penalty are those of a fixed-shape batch of those counts, and bit m of the
// saved mask stays hostage m.  The counts are per env: every branch on them is uniform over the workgroup.  The nine tail words and the
// LDS parts keep their offsets at the capacity (hw_crowd_lds_bytes of the capacity bounds every live triple).
template <int MODE, int NW>
__global__ __launch_bounds__(64 * NW) void hw_crowd_kernel(const HwDev d, const HwIO io) {
    constexpr bool LIVE = false;
    constexpr ParticleCounts cn{nullptr, nullptr};
#include "hostage_crowd_body.inc"
}

template <int MODE, int NW>
__global__ __launch_bounds__(64 * NW) void hw_crowd_kernel_live(const HwDev d, const HwIO io, const ParticleCounts cn) {
    constexpr bool LIVE = true;
#include "hostage_crowd_body.inc"
}

}  // namespace

namespace madrl {

size_t hw_crowd_lds_bytes(int Nr, int Nh, int Nc, int K, int rec_dw) {
    (void)Nh;  // at most 64: one word per rescuer
    const size_t W = 1 + ((size_t)Nc + 63) / 64;
    return ((size_t)up4(rec_dw) + up4(2 * K) + up4(2 * Nr)) * 4 + ((size_t)Nr * W + W + 1 + 2 + 2) * 8;
}

int hw_crowd_launch(const void *dev, const void *io, int mode, int64_t max_blocks, size_t lds_bytes, const int32_t *pending, int32_t *live,
                    void *stream) {
    if (live != nullptr)  // per-env particle counts
        return crowd_launch<HwDev, HwIO>(mode == 0 ? hw_crowd_kernel_live<0, MADRL_HWC_NW> : hw_crowd_kernel_live<1, MADRL_HWC_NW>, MADRL_HWC_NW,
                                         dev, io, ParticleCounts{pending, live}, max_blocks, lds_bytes, stream);
    return crowd_launch<HwDev, HwIO>(mode == 0 ? hw_crowd_kernel<0, MADRL_HWC_NW> : hw_crowd_kernel<1, MADRL_HWC_NW>, MADRL_HWC_NW, dev, io,
                                     max_blocks, lds_bytes, stream);
}

}  // namespace madrl
