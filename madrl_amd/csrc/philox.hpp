// philox.hpp -- the counter-based generator and the RNG contract's tags, for device code and for a plain host compiler:
// no HIP include.  common.hpp includes it for every kernel; pursuit_rules.hpp includes it alone.
#pragma once

#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)   // a host compiler that knows no execution-space attributes: empty inside this header only
#define __host__
#define __device__
#define MADRL_PHILOX_OWN_ATTRS
#endif

namespace madrl {

// ---------------------------------------------------------------- Philox4x32-10
// Counter-based generator (Salmon, Moraes, Dror, Shaw, SC'11).  One call = 4 x 32 random
// bits addressed by (counter, key); no state to carry, so every (env, tick, agent) draw is
// independent of launch shape and of the number of GPUs.
struct u32x4 {
    uint32_t x, y, z, w;
};

__host__ __device__ inline uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

#ifndef MADRL_PHILOX_VARIANT
#define MADRL_PHILOX_VARIANT 0
#endif
// a ^ b ^ c: one v_bitop3_b32 on gfx950 (truth table 0x96)
__host__ __device__ inline uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

// Each round is two 32 x 32 -> 64 products (one v_mad_u64_u32 each on the device, instead of a v_mul_hi_u32 / v_mul_lo_u32
// pair) and two three-way XORs: 4 VALU ops per round for per-lane counters.
__host__ __device__ inline u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                               uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
#if MADRL_PHILOX_VARIANT == 1   // separate high / low products
        const uint32_t hi0 = mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = xor3(hi1, c1, k0); c1 = lo1; c2 = xor3(hi0, c3, k1); c3 = lo0;
#elif MADRL_PHILOX_VARIANT == 2  // and two-way XORs (round 1)
        const uint32_t hi0 = mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
#else
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        c0 = xor3((uint32_t)(p1 >> 32), c1, k0);
        c1 = (uint32_t)p1;
        c2 = xor3((uint32_t)(p0 >> 32), c3, k1);
        c3 = (uint32_t)p0;
#endif
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

// RNG contract tags: counter = (global env id, tick, index, tag | attempt << 8)
enum : uint32_t { TAG_EVADER_ACT = 0, TAG_RESET_POS = 1, TAG_RESET_ENV = 2, TAG_PURSUER_ACT = 3 };

// uniform double in [0,1) from 53 random bits
__host__ __device__ inline double u53(uint32_t hi, uint32_t lo) {
    return (double)(((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6)) * (1.0 / 9007199254740992.0);
}

}  // namespace madrl

#ifdef MADRL_PHILOX_OWN_ATTRS
#undef __host__
#undef __device__
#undef MADRL_PHILOX_OWN_ATTRS
#endif
