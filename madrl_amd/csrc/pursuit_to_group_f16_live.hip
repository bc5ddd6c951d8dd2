// pursuit_to_group_f16_live.hip -- the half-precision two-buffer step kernels of the multi-wavefront family with per-env agent counts:
// pursuit_group_kernel<S, 1, true> over a TLHGShape (pursuit_group.hpp), one for every HLG line of
// pursuit_to_f16_group_specializations.def (the HG lines: pursuit_to_group_f16.hip).  A translation unit of its own: the live long-row
// kernels compile slowest of all, and the build compiles its objects side by side.
#include "common.hpp"
#include "pursuit_group.hpp"

namespace madrl {
namespace pw {

template <class S>
void group_to_f16_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s) {
    static_assert(S::TO && S::H16 && S::LIVE, "a TLHGShape");
    hipLaunchKernelGGL((pursuit_group_kernel<S, 1, true>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
}

#define HG(XS, YS, NP, NE, R, FL, NW)
#define HLG(XS, YS, NP, NE, R, FL, NW) template void group_to_f16_launch<TLHGShape<XS, YS, NP, NE, R, FL, NW>>(const WaveDev &, const WaveIO &, int64_t, hipStream_t);
#include "pursuit_to_f16_group_specializations.def"
#if __has_include("pursuit_to_f16_group_specializations.local.def")   // shapes added locally by `python -m madrl_amd.build --pursuit-to-group-f16-shape ... 1` (git-ignored)
#include "pursuit_to_f16_group_specializations.local.def"
#endif
#undef HG
#undef HLG

}  // namespace pw
}  // namespace madrl
