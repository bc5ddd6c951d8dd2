// waterworld_f16.hip -- the one-wavefront Waterworld kernel with half-precision observation rows (madrl_waterworld_reset_f16,
// madrl_waterworld_step_f16; BatchedMAWaterWorld(obs_dtype=torch.float16)), gfx950 / CDNA4.
//
// waterworld_kernel_f16<MODE, ...> is waterworld_wave_body.inc once more, with MADRL_WW_BODY_HALF set: the step is waterworld_kernel's,
// float32 from the record to the staged rows in LDS, and the one thing that differs is how the rows leave -- as the round-to-nearest-even
// binary16 of each staged value (half_bits, common.hpp; store_rows_half, particle_wave.hpp), to a destination that is 2-byte aligned.
// Rewards, done bytes, info counters and the state record are the float32 kernel's, bit for bit.  The half pointer travels in io.obs, cast.
// One specialised instantiation per line of waterworld_specializations.def, reset and step, with the float32 kernel's occupancy; every other
// shape runs the generic one.  No fused StandardizedEnv, no live counts, no per-pursuer ranges: the C entries refuse such a handle
// (waterworld.hip).  An own translation unit so that it compiles beside waterworld.hip.
#include "waterworld_wave.hpp"

#include <math.h>

namespace {

using namespace madrl;

// the template parameters of waterworld_kernel, FUSED among them: the occupancy rule (MADRL_WW_OCC) reads it
template <int MODE, int TNp, int TNe, int TNpo, int TK, bool FUSED = false, int TD = 0>
__global__ __launch_bounds__(64) MADRL_WW_OCC void waterworld_kernel_f16(const WwDev d, const WwIO io) {
    static_assert(!FUSED, "the half entries have no fused StandardizedEnv");
#define MADRL_WW_BODY_LIVE 0
#define MADRL_WW_BODY_RANGES 0
#define MADRL_WW_BODY_HALF 1
#include "waterworld_wave_body.inc"
#undef MADRL_WW_BODY_HALF
#undef MADRL_WW_BODY_RANGES
#undef MADRL_WW_BODY_LIVE
}
#undef DA
#undef IOA
#undef LANE_LT
#undef LANE_EQ

struct WwSpecF16 {
    int Np, Ne, Npo, K, D;
    void (*launch)(const WwDev &, const WwIO &, int mode, dim3 g, hipStream_t s);
};

template <int TNp, int TNe, int TNpo, int TK, int TD>
void ww_launch_spec_f16(const WwDev &d, const WwIO &io, int mode, dim3 g, hipStream_t s) {
    const dim3 b(64);  // static LDS layout: 0 dynamic bytes
    if (mode == 0) hipLaunchKernelGGL((waterworld_kernel_f16<0, TNp, TNe, TNpo, TK, false, TD>), g, b, 0, s, d, io);
    else hipLaunchKernelGGL((waterworld_kernel_f16<1, TNp, TNe, TNpo, TK, false, TD>), g, b, 0, s, d, io);
}

#define X(NP_, NE_, NPO_, K_, D_) {NP_, NE_, NPO_, K_, D_, ww_launch_spec_f16<NP_, NE_, NPO_, K_, D_>},
const WwSpecF16 WW_SPECS_F16[] = {
#include "waterworld_specializations.def"
#if __has_include("waterworld_specializations.local.def")   // shapes added on this machine by `python -m madrl_amd.build --waterworld-shape ...` (git-ignored)
#include "waterworld_specializations.local.def"
#endif
};
#undef X

}  // namespace

namespace madrl {

int ww_f16_launch(const void *dev, const void *io_, int mode, int64_t max_blocks, size_t lds_bytes, void *stream, int *specialised) {
    hipStream_t s = (hipStream_t)stream;
    const WwDev &d = *static_cast<const WwDev *>(dev);
    const WwIO &io = *static_cast<const WwIO *>(io_);
    const dim3 g = particle_grid(max_blocks, d.n_envs), b(64);
    const WwSpecF16 *spec = nullptr;
    for (const WwSpecF16 &w : WW_SPECS_F16)
        if (d.Np == w.Np && d.Ne == w.Ne && d.Npo == w.Npo && d.K == w.K && d.D == w.D) spec = &w;
    if (spec) spec->launch(d, io, mode, g, s);
    else if (mode == 0) hipLaunchKernelGGL((waterworld_kernel_f16<0, 0, 0, 0, 0>), g, b, lds_bytes, s, d, io);
    else hipLaunchKernelGGL((waterworld_kernel_f16<1, 0, 0, 0, 0>), g, b, lds_bytes, s, d, io);
    MADRL_HIP_TRY(hipGetLastError());
    *specialised = spec != nullptr;
    return MADRL_OK;
}

}  // namespace madrl
