// pursuit_to_group.hip -- the two-buffer step kernels of the multi-wavefront family (the XG / XLG lines of pursuit_to_specializations.def):
// the flexible step kernel pursuit_group_kernel<S, 1, true> over a TGShape / TLGShape.  A translation unit of its own rather than a part of
// pursuit_to.hip: the long-row kernels are the slowest of the two-buffer list to compile, and the build compiles its objects side by side.
// pursuit.hip's table of lines reaches these kernels through group_to_launch<S>.
#include "common.hpp"
#include "pursuit_group.hpp"

namespace madrl {
namespace pw {

template <class S>
void group_to_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s) {
    hipLaunchKernelGGL((pursuit_group_kernel<S, 1, true>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io);
}

#define X(XS, YS, NP, NE, R, FL)
#define XL(XS, YS, NP, NE, R, FL)
#define XC(XS, YS, NP, NE, R, FL, NW)
#define XLC(XS, YS, NP, NE, R, FL, NW)
#define XG(XS, YS, NP, NE, R, FL, NW) template void group_to_launch<TGShape<XS, YS, NP, NE, R, FL, NW>>(const WaveDev &, const WaveIO &, int64_t, hipStream_t);
#define XLG(XS, YS, NP, NE, R, FL, NW) template void group_to_launch<TLGShape<XS, YS, NP, NE, R, FL, NW>>(const WaveDev &, const WaveIO &, int64_t, hipStream_t);
#include "pursuit_to_specializations.def"
#if __has_include("pursuit_to_specializations.local.def")   // shapes added on this machine by `python -m madrl_amd.build --pursuit-to-group-shape ...` (git-ignored)
#include "pursuit_to_specializations.local.def"
#endif
#undef X
#undef XL
#undef XC
#undef XLC
#undef XG
#undef XLG

}  // namespace pw
}  // namespace madrl
