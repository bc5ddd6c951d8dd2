// pursuit_fixed.hip -- the one-wavefront step kernels with their launch constants folded in: pursuit_wave_kernel<FShape<...>, 1, false, false>
// for the XF lines of pursuit_fixed_specializations.def.  A translation unit of its own: the build compiles it side by side with pursuit.hip,
// whose table of lines reaches these kernels through wave_fixed_launch<S>.
#include "common.hpp"
#include "pursuit_wave.hpp"

namespace madrl {
namespace pw {

template <class S>
void wave_fixed_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s) {
    hipLaunchKernelGGL((pursuit_wave_kernel<S, 1, false, false>), dim3((unsigned)blocks), dim3(64), 0, s, d, io);
}

#define XF(XS, YS, NP, NE, R, FL) template void wave_fixed_launch<FShape<XS, YS, NP, NE, R, FL>>(const WaveDev &, const WaveIO &, int64_t, hipStream_t);
#include "pursuit_fixed_specializations.def"
#if __has_include("pursuit_fixed_specializations.local.def")
#include "pursuit_fixed_specializations.local.def"
#endif
#undef XF

}  // namespace pw
}  // namespace madrl
