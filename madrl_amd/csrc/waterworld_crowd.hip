// waterworld_crowd.hip -- MAWaterWorld for envs beyond one wavefront's worth of particles (gfx950 / CDNA4), float32: ww_crowd_kernel, one
// workgroup of NW wavefronts per env.  The scheme (phases, sensing passes, the ordered reach walk) and the code it shares with
// hw_crowd_kernel are in particle_crowd.hpp; this file is the oracle's Waterworld step in its order.  Limits: 1 023 particles, 128 pursuers,
// n_sensors in 1..256.
//
// LDS (dynamic, ww_crowd_lds_bytes; about 35 KB at the limits, 3 KB at 20 / 60 / 40):
//   S     the packed state record  X[NP][2] | V[NP][2] | obst[2] | t | tick     (<= 16 KB)
//   SEN   sensor unit vectors [K][2]
//   ACT   the scaled actions [Np][2]: the global control penalty sums them row-major
//   COL   collision bits, one 64-bit word per (pursuer, chunk of 64 evaders | chunk of 64 poisons)   (<= 15 KB)
//   CAU / ENC   caught / encountered bits per chunk
// The observation row is NOT staged (40 pursuers x 200 sensors would be 224 KB).  Reference lines (:n) are waterworld.py's, as in waterworld.hip.
// The kernel's text is waterworld_crowd_body.inc, included inside the two __global__ entries below (as pursuit_crowd_body.inc is): the
// fixed-shape entry keeps its two arguments, its name and its code, the live-count entry has the count arrays as a third argument.
#include "particle_crowd.hpp"
#include "waterworld_dev.hpp"

// wavefronts per workgroup (a profiling variant builds the other value: scripts/ww_crowd_time.py)
#ifndef MADRL_WWC_NW
#define MADRL_WWC_NW 4
#endif

namespace {

using namespace madrl;

// MODE 0: reset(mask)   MODE 1: step (+ fused auto-reset)
// LIVE (ww_crowd_kernel_live): d.Np / d.Ne / d.Npo are a CAPACITY and every env runs its own counts (cn.live).  Whatever a caller sees stays at the capacity,
// slotted by class: pursuer i at slot i, evader m at Pc + m, poison m at Pc + Ec + m -- the record, the rows of inj_resp, the action /
// reward / observation rows (stride Pc).  The record is compacted into packed arrays of the live counts on its way into LDS and scattered
// back on its way out ((-1, -1) / 0 into the slots that do not exist), so the phases between run on the live counts as they stand and the
// Philox particle index is the one of a fixed-shape batch of those counts.  The counts are per env: every branch on them is uniform over
// the workgroup.  The LDS parts keep their offsets at the capacity (ww_crowd_lds_bytes of the capacity bounds every live triple).
template <int MODE, int NW>
__global__ __launch_bounds__(64 * NW) void ww_crowd_kernel(const WwDev d, const WwIO io) {
    constexpr bool LIVE = false, RANGES = false;
    constexpr ParticleCounts cn{nullptr, nullptr};
#include "waterworld_crowd_body.inc"
}

template <int MODE, int NW>
__global__ __launch_bounds__(64 * NW) void ww_crowd_kernel_live(const WwDev d, const WwIO io, const ParticleCounts cn) {
    constexpr bool LIVE = true, RANGES = false;
#include "waterworld_crowd_body.inc"
}

// The ranged entry (madrl_waterworld_set_sensor_ranges): the fixed-shape text with a sensor range per pursuer; d.sensors holds the ranges
// behind the sensor vectors and the workgroup's LDS up4(Np) floats more.
template <int MODE, int NW>
__global__ __launch_bounds__(64 * NW) void ww_crowd_kernel_ranges(const WwDev d, const WwIO io) {
    constexpr bool LIVE = false, RANGES = true;
    constexpr ParticleCounts cn{nullptr, nullptr};
#include "waterworld_crowd_body.inc"
}

}  // namespace

namespace madrl {

size_t ww_crowd_lds_bytes(int Np, int Ne, int Npo, int K, int rec_dw) {
    const size_t WE = ((size_t)Ne + 63) / 64, WP = ((size_t)Npo + 63) / 64;
    return ((size_t)up4(rec_dw) + up4(2 * K) + up4(2 * Np)) * 4 + ((size_t)Np * (WE + WP) + (WE + WP) + WE) * 8;
}

int ww_crowd_launch(const void *dev, const void *io, int mode, int64_t max_blocks, size_t lds_bytes, const int32_t *pending, int32_t *live,
                    bool ranged, void *stream) {
    if (ranged)  // per-pursuer sensor ranges (never together with per-env counts: the two calls refuse each other)
        return crowd_launch<WwDev, WwIO>(mode == 0 ? ww_crowd_kernel_ranges<0, MADRL_WWC_NW> : ww_crowd_kernel_ranges<1, MADRL_WWC_NW>, MADRL_WWC_NW,
                                         dev, io, max_blocks, lds_bytes, stream);
    if (live != nullptr)  // per-env particle counts
        return crowd_launch<WwDev, WwIO>(mode == 0 ? ww_crowd_kernel_live<0, MADRL_WWC_NW> : ww_crowd_kernel_live<1, MADRL_WWC_NW>, MADRL_WWC_NW,
                                         dev, io, ParticleCounts{pending, live}, max_blocks, lds_bytes, stream);
    return crowd_launch<WwDev, WwIO>(mode == 0 ? ww_crowd_kernel<0, MADRL_WWC_NW> : ww_crowd_kernel<1, MADRL_WWC_NW>, MADRL_WWC_NW, dev, io,
                                     max_blocks, lds_bytes, stream);
}

}  // namespace madrl
