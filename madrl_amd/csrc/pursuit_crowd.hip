// pursuit_crowd.hip -- the instantiations of the crowd kernel (pursuit_crowd_kernel<CShape<...>, MODE>, the XC lines of
// pursuit_crowd_specializations.def).  A translation unit of their own: the build compiles it side by side with pursuit.hip, whose
// table of lines reaches these kernels through crowd_launch<S>.
#include "common.hpp"
#include "pursuit_crowd.hpp"

namespace madrl {
namespace pc {

template <class S>
void crowd_launch(const CrowdDev &d, const CrowdIO &io, const int32_t *, int mode, int64_t blocks, hipStream_t s) {
    if (mode == 0)
        hipLaunchKernelGGL((pursuit_crowd_kernel<S, 0>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
    else
        hipLaunchKernelGGL((pursuit_crowd_kernel<S, 1>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
}

#define XC(XS, YS, NP, NE, R, FL, NW) \
    template void crowd_launch<CShape<XS, YS, NP, NE, R, FL, NW>>(const CrowdDev &, const CrowdIO &, const int32_t *, int, int64_t, hipStream_t);
#include "pursuit_crowd_specializations.def"
#if __has_include("pursuit_crowd_specializations.local.def")   // shapes added on this machine by `python -m madrl_amd.build --pursuit-crowd-shape ...` (git-ignored)
#include "pursuit_crowd_specializations.local.def"
#endif
#undef XC

}  // namespace pc
}  // namespace madrl
