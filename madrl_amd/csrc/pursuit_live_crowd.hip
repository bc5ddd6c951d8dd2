// pursuit_live_crowd.hip -- the per-env agent-count instantiations of the crowd kernel (pursuit_live_crowd_kernel<LCShape<...>, MODE>, the XLC
// lines of pursuit_live_specializations.def).  A translation unit of their own: the build compiles it side by side with pursuit.hip, whose
// table of lines reaches these kernels through live_crowd_launch<S>.
#include "common.hpp"
#include "pursuit_crowd.hpp"

namespace madrl {
namespace pc {

template <class S>
void live_crowd_launch(const CrowdDev &d, const CrowdIO &io, const int32_t *pending, int mode, int64_t blocks, hipStream_t s) {
    if (mode == 0)
        hipLaunchKernelGGL((pursuit_live_crowd_kernel<S, 0>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io, pending);
    else
        hipLaunchKernelGGL((pursuit_live_crowd_kernel<S, 1>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io, pending);
}

#define XL(XS, YS, NP, NE, R, FL)
#define XLG(XS, YS, NP, NE, R, FL, NW)
#define XLC(XS, YS, NP, NE, R, FL, NW) \
    template void live_crowd_launch<LCShape<XS, YS, NP, NE, R, FL, NW>>(const CrowdDev &, const CrowdIO &, const int32_t *, int, int64_t, hipStream_t);
#include "pursuit_live_specializations.def"
#if __has_include("pursuit_live_specializations.local.def")   // capacities added on this machine by `python -m madrl_amd.build --pursuit-live-crowd-shape ...` (git-ignored)
#include "pursuit_live_specializations.local.def"
#endif
#undef XL
#undef XLG
#undef XLC

}  // namespace pc
}  // namespace madrl
