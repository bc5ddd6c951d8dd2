// pursuit_live_group.hip -- the per-env agent-count instantiations of the group kernel (pursuit_group_kernel<LGShape<...>>, the XLG lines
// of pursuit_live_specializations.def).  A translation unit of their own: the build compiles it side by side with pursuit.hip, whose
// table of lines reaches these kernels through live_group_launch<S>.
#include "common.hpp"
#include "pursuit_group.hpp"

namespace madrl {
namespace pw {

template <class S>
void live_group_launch(const WaveDev &d, const WaveIO &io, int mode, int64_t blocks, hipStream_t s) {
    if (mode == 0)
        hipLaunchKernelGGL((pursuit_group_kernel<S, 0, false>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
    else if (io.flex)
        hipLaunchKernelGGL((pursuit_group_kernel<S, 1, true>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
    else
        hipLaunchKernelGGL((pursuit_group_kernel<S, 1, false>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
}

#define XL(XS, YS, NP, NE, R, FL)
#define XLC(XS, YS, NP, NE, R, FL, NW)
#define XLG(XS, YS, NP, NE, R, FL, NW) \
    template void live_group_launch<LGShape<XS, YS, NP, NE, R, FL, NW>>(const WaveDev &, const WaveIO &, int, int64_t, hipStream_t);
#include "pursuit_live_specializations.def"
#if __has_include("pursuit_live_specializations.local.def")   // capacities added on this machine by `python -m madrl_amd.build --pursuit-live-shape ...` (git-ignored)
#include "pursuit_live_specializations.local.def"
#endif
#undef XL
#undef XLG
#undef XLC

}  // namespace pw
}  // namespace madrl
