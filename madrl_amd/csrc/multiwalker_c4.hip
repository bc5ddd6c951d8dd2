// multiwalker_c4.hip -- the MultiWalker kernels for up to 4 walkers per env, 4 lanes of a wavefront per env (16 envs per wavefront).
// One of the three capacity classes of multiwalker_impl.hpp (see there, and multiwalker.hip for how the C ABI picks one).
#define MW_CAPW 4
#define MW_NLANES 4
#include "multiwalker_impl.hpp"

#if defined(MADRL_MW_TIMING)
// measurement build of THIS unit alone (SRC=multiwalker_c4 MACRO=MADRL_MW_TIMING EXTRA=-fno-slp-vectorize scripts/variants.sh 1, never the
// shipped library): what the stamps and counters of multiwalker_impl.hpp's MW_TSTAMP / MW_TVAL / MW_TACC hold, read back by scripts/mw_timing.py
extern "C" int madrl_multiwalker_debug_read(unsigned long long *stamps_host, int *vals_host) {   // [2][4096][8], [2][4096][16][4]
    MADRL_HIP_TRY(hipDeviceSynchronize());
    MADRL_HIP_TRY(hipMemcpyFromSymbol(stamps_host, HIP_SYMBOL(g_mw_stamp), sizeof(g_mw_stamp)));
    MADRL_HIP_TRY(hipMemcpyFromSymbol(vals_host, HIP_SYMBOL(g_mw_val), sizeof(g_mw_val)));
    return MADRL_OK;
}
extern "C" int madrl_multiwalker_debug_read_acc(unsigned long long *acc_host, int reset) {   // [4096][8]; reset != 0: zero the accumulators afterwards
    MADRL_HIP_TRY(hipDeviceSynchronize());
    MADRL_HIP_TRY(hipMemcpyFromSymbol(acc_host, HIP_SYMBOL(g_mw_acc), sizeof(g_mw_acc)));
    if (reset) { static unsigned long long zero[MW_DBG_BLOCKS][8]; MADRL_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_mw_acc), zero, sizeof(zero))); }
    return MADRL_OK;
}
#endif
