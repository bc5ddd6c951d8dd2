// pursuit_to_group_f16.hip -- the half-precision two-buffer step kernels (madrl_pursuit_step_to_f16) of the multi-wavefront family: the
// flexible step kernel pursuit_group_kernel<S, 1, true> over a THGShape (pursuit_group.hpp), one for every HG line of
// pursuit_to_f16_group_specializations.def (the HLG lines, over a TLHGShape: pursuit_to_group_f16_live.hip).  A translation unit of its
// own: the long-row kernels are the slowest of the list to compile, and the build compiles its objects side by side.
// pursuit.hip's table of lines reaches these kernels through group_to_f16_launch<S>.
#include "common.hpp"
#include "pursuit_group.hpp"

namespace madrl {
namespace pw {

template <class S>
void group_to_f16_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s) {
    static_assert(S::TO && S::H16 && !S::LIVE, "a THGShape");
    hipLaunchKernelGGL((pursuit_group_kernel<S, 1, true>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
}

#define HG(XS, YS, NP, NE, R, FL, NW) template void group_to_f16_launch<THGShape<XS, YS, NP, NE, R, FL, NW>>(const WaveDev &, const WaveIO &, int64_t, hipStream_t);
#define HLG(XS, YS, NP, NE, R, FL, NW)
#include "pursuit_to_f16_group_specializations.def"
#if __has_include("pursuit_to_f16_group_specializations.local.def")   // shapes added locally by `python -m madrl_amd.build --pursuit-to-group-f16-shape ...` (git-ignored)
#include "pursuit_to_f16_group_specializations.local.def"
#endif
#undef HG
#undef HLG

}  // namespace pw
}  // namespace madrl
