// pursuit_to_f16.hip -- the half-precision two-buffer step kernels of madrl_pursuit_step_to_f16: the flexible step kernel of the
// one-wavefront family over a THShape (pursuit_wave.hpp), one for every X line of pursuit_to_specializations.def (the XL lines, over a
// TLHShape: pursuit_to_f16_live.hip, which is compiled with another scalar register allocator).  The half kernels of the multi-wavefront
// family have a list of their own, pursuit_to_f16_group_specializations.def (HG / HLG lines over a THGShape / TLHGShape of
// pursuit_group.hpp: pursuit_to_group_f16.hip, pursuit_to_group_f16_live.hip).  The XC / XLC (crowd) lines and the multi-wavefront
// shapes not listed there have no half form: their handles run the half step on the generic kernel
// (pursuit_to_f16_kernel, pursuit.hip).  A translation unit of its own, compiled side by side with pursuit.hip, whose table of lines reaches these
// kernels through wave_to_f16_launch<S>.
#include "common.hpp"
#include "pursuit_wave.hpp"

namespace madrl {
namespace pw {

template <class S>
void wave_to_f16_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s) {
    static_assert(S::TO && S::H16 && !S::LIVE, "a THShape");
    hipLaunchKernelGGL((pursuit_wave_kernel<S, 1, true>), dim3((unsigned)blocks), dim3(64), 0, s, d, io);
}

#define X(XS, YS, NP, NE, R, FL) template void wave_to_f16_launch<THShape<XS, YS, NP, NE, R, FL>>(const WaveDev &, const WaveIO &, int64_t, hipStream_t);
#define XL(XS, YS, NP, NE, R, FL)
#define XC(XS, YS, NP, NE, R, FL, NW)
#define XLC(XS, YS, NP, NE, R, FL, NW)
#define XG(XS, YS, NP, NE, R, FL, NW)
#define XLG(XS, YS, NP, NE, R, FL, NW)
#include "pursuit_to_specializations.def"
#if __has_include("pursuit_to_specializations.local.def")   // shapes added locally by `python -m madrl_amd.build --pursuit-to-shape ...` (git-ignored)
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
