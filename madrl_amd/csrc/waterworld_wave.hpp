// waterworld_wave.hpp -- what the __global__ entries around waterworld_wave_body.inc have in common: waterworld_kernel, waterworld_kernel_live,
// waterworld_kernel_ranges (waterworld.hip) and waterworld_kernel_f16 (waterworld_f16.hip).  The views of the kernel-argument segment and the
// occupancy the specialised shapes' registers are allocated for.  Like the structs of waterworld_dev.hpp the views stay in the unnamed
// namespace: every translation unit has its own (identical) copy.
#pragma once

#include "waterworld_dev.hpp"   // WwDev, WwIO, the RNG tags
#include "particle_wave.hpp"    // the device code the body shares with hostage_wave_body.inc

namespace {

using namespace madrl;

// The launch parameters as read from the kernel-argument segment (kernargs(), common.hpp) at the phase that needs them.
struct WwKArgs {
    WwDev d;
    WwIO io;
};
// ... and of waterworld_kernel_live, whose third argument follows the two (all three are 8-byte aligned)
struct WwKArgsLive {
    WwDev d;
    WwIO io;
    ParticleCounts cn;
};
static_assert(sizeof(WwKArgs) % 8 == 0 && sizeof(WwKArgsLive) == sizeof(WwKArgs) + sizeof(ParticleCounts), "the third argument follows the two without padding");

}  // namespace

// Profiling aid (scripts/variants.sh, never the shipped library): 1 no sensing loop, 2 no observation store, 4 no collisions
#ifndef MADRL_WW_ABLATE
#define MADRL_WW_ABLATE 0
#endif

// Resident wavefronts per SIMD the SPECIALISED kernel's registers are allocated for (the generic one is left to the compiler).
// Measured at BASELINE C3, 32 768 envs: 4 waves (104 VGPRs) 77 us, 5 waves (86) 60.4 us, 6 waves (80, no scratch) 57.2 us, 7 waves
// (72 + 32 B of scratch) 57.4 us.
#ifndef MADRL_WW_WAVES
#define MADRL_WW_WAVES 6
#endif
// (the fused-wrapper variant holds float64 statistics: one wave fewer, or it spills)
#define MADRL_WW_OCC_N (TNp > 0 ? (FUSED ? MADRL_WW_WAVES - 1 : MADRL_WW_WAVES) - (TNp > 6 ? 1 : 0) : 0)  // (> 6 pursuers: two words per collision matrix, more live pass state)
#define MADRL_WW_OCC __attribute__((amdgpu_waves_per_eu(MADRL_WW_OCC_N > 0 ? MADRL_WW_OCC_N : 1, MADRL_WW_OCC_N > 0 ? MADRL_WW_OCC_N : 8)))
