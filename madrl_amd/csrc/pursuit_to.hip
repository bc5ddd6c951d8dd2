// pursuit_to.hip -- the two-buffer step kernels of madrl_pursuit_step_to (the lines of pursuit_to_specializations.def): the flexible step
// kernel of the one-wavefront family over a TShape / TLShape, and pursuit_crowd_to_kernel over a CShape / LCShape (the XG / XLG lines, the
// multi-wavefront family, are compiled in pursuit_to_group.hip).  A translation unit of its own: the build compiles it side by side with pursuit.hip, whose table of lines reaches these kernels through wave_to_launch<S> and
// crowd_to_launch<S>.
#include "common.hpp"
#include "pursuit_wave.hpp"
#include "pursuit_crowd.hpp"

namespace madrl {
namespace pw {

template <class S>
void wave_to_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s) {
    hipLaunchKernelGGL((pursuit_wave_kernel<S, 1, true>), dim3((unsigned)blocks), dim3(64), 0, s, d, io);
}

#define X(XS, YS, NP, NE, R, FL) template void wave_to_launch<TShape<XS, YS, NP, NE, R, FL>>(const WaveDev &, const WaveIO &, int64_t, hipStream_t);
#define XL(XS, YS, NP, NE, R, FL) template void wave_to_launch<TLShape<XS, YS, NP, NE, R, FL>>(const WaveDev &, const WaveIO &, int64_t, hipStream_t);
#define XC(XS, YS, NP, NE, R, FL, NW)
#define XLC(XS, YS, NP, NE, R, FL, NW)
#define XG(XS, YS, NP, NE, R, FL, NW)
#define XLG(XS, YS, NP, NE, R, FL, NW)
#include "pursuit_to_specializations.def"
#if __has_include("pursuit_to_specializations.local.def")   // shapes added on this machine by `python -m madrl_amd.build --pursuit-to-shape ...` (git-ignored)
#include "pursuit_to_specializations.local.def"
#endif
#undef X
#undef XL
#undef XC
#undef XLC
#undef XG
#undef XLG

}  // namespace pw

namespace pc {

template <class S>
void crowd_to_launch(const CrowdDev &d, const CrowdIO &io, const int32_t *pending, const float *obs_prev, int64_t blocks, hipStream_t s) {
    hipLaunchKernelGGL((pursuit_crowd_to_kernel<S>), dim3((unsigned)blocks), dim3(S::NT), 0, s, d, io, pending, obs_prev);
}

#define X(XS, YS, NP, NE, R, FL)
#define XL(XS, YS, NP, NE, R, FL)
#define XG(XS, YS, NP, NE, R, FL, NW)
#define XLG(XS, YS, NP, NE, R, FL, NW)
#define XC(XS, YS, NP, NE, R, FL, NW) \
    template void crowd_to_launch<CShape<XS, YS, NP, NE, R, FL, NW>>(const CrowdDev &, const CrowdIO &, const int32_t *, const float *, int64_t, hipStream_t);
#define XLC(XS, YS, NP, NE, R, FL, NW) \
    template void crowd_to_launch<LCShape<XS, YS, NP, NE, R, FL, NW>>(const CrowdDev &, const CrowdIO &, const int32_t *, const float *, int64_t, hipStream_t);
#include "pursuit_to_specializations.def"
#if __has_include("pursuit_to_specializations.local.def")
#include "pursuit_to_specializations.local.def"
#endif
#undef X
#undef XL
#undef XC
#undef XLC
#undef XG
#undef XLG

}  // namespace pc
}  // namespace madrl
