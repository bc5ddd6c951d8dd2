// pursuit_to_f16_live.hip -- the half-precision two-buffer step kernels with per-env agent counts: pursuit_wave_kernel over a TLHShape
// (pursuit_wave.hpp), one for every XL line of pursuit_to_specializations.def (the X lines: pursuit_to_f16.hip).  A translation unit of
// its own because it is compiled with -mllvm -sgpr-regalloc=basic (EXTRA_FLAGS, madrl_amd/build.py): under the default (greedy) scalar
// register allocator this kernel is left with a 20-byte private segment that no instruction touches -- a 16-byte spill slot the allocator
// assigns to a kernel-argument load and then rematerialises instead, plus the emergency slot any stack object brings with it -- and a
// private segment costs every dispatch its scratch set-up.  The basic allocator leaves none (and no VGPR spill either).
#include "common.hpp"
#include "pursuit_wave.hpp"

namespace madrl {
namespace pw {

template <class S>
void wave_to_f16_launch(const WaveDev &d, const WaveIO &io, int64_t blocks, hipStream_t s) {
    static_assert(S::TO && S::H16 && S::LIVE, "a TLHShape");
    hipLaunchKernelGGL((pursuit_wave_kernel<S, 1, true>), dim3((unsigned)blocks), dim3(64), 0, s, d, io);
}

#define X(XS, YS, NP, NE, R, FL)
#define XL(XS, YS, NP, NE, R, FL) template void wave_to_f16_launch<TLHShape<XS, YS, NP, NE, R, FL>>(const WaveDev &, const WaveIO &, int64_t, hipStream_t);
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
