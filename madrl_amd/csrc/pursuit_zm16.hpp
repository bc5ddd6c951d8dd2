// pursuit_zm16.hpp -- the 16-bit-per-lane form of the one-wavefront Pursuit kernel's stale-zero masks (pursuit_wave.hpp, "stale-zero mask").
//
// In registers a lane's mask is one dword: byte k = cell k of a float4 slot, bit NS - 1 - s of each byte = the lane's slot s (NS <= 8 slots
// per lane).  A bit is only ever consulted as `out4 & old4`, and a cell can only be "outside the map" in channels 1 and 2: the bits of a
// slot that holds channel-0 cells and the id alone, or lies past the end of the env's rows, are dead weight.  Where every lane owns at
// most FOUR slots with a channel-1 or channel-2 cell (and at most five slots at all), a nibble per cell is enough: 16 bits per lane, two
// lanes per dword, 128 B per env instead of 256 B -- one aligned 128-byte line, stored by lanes 0..31 (lane l holds lane l + 32's half in its
// upper 16 bits).  With five slots each lane drops ONE bit position of its bytes, a slot without such a cell (`drop_slot`); with four or
// fewer nothing is dropped.  Polarity is that of the dword form: all ones = nothing known, all zeros = every cell known to hold zero.
//
// Everything here is pure and runs on the host as well (tests/host/pursuit_zm16_check.cpp): the predicate, the per-lane constants and
// pack / unpack; the kernel adds the exchange between lanes l and l + 32 and the load / store.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MADRL_ZM16_HD __host__ __device__
#else
#define MADRL_ZM16_HD
#endif

namespace madrl {
namespace zm16 {

constexpr int LANES = 64;

// float4 slots of a pursuer's row / of a lane, as pw::Shape has them
constexpr int row_slots(int R, int flatten) { return (flatten ? 3 * R * R + 1 : 4 * R * R) / 4; }
constexpr int lane_slots(int P, int R, int flatten) { return (P * row_slots(R, flatten) + LANES - 1) / LANES; }

// does float4 slot q of a FLATTENED env (P rows of 3 R^2 + 1 floats) exist and hold a cell of channel 1 or 2 (row elements [R^2, 3 R^2))?
MADRL_ZM16_HD constexpr bool useful(int P, int R, int q) {
    const int dv = row_slots(R, 1), m = q % dv;
    return q < P * dv && 4 * m + 3 >= R * R && 4 * m < 3 * R * R;
}
MADRL_ZM16_HD constexpr int useful_slots(int P, int R, int lane) {
    int n = 0;
    for (int s = 0; s < lane_slots(P, R, 1); ++s) n += useful(P, R, lane + LANES * s) ? 1 : 0;
    return n;
}
// the shapes that use the 16-bit form
constexpr bool eligible(int P, int R, int flatten) {
    if (flatten != 1 || lane_slots(P, R, 1) > 5) return false;
    for (int lane = 0; lane < LANES; ++lane)
        if (useful_slots(P, R, lane) > 4) return false;
    return true;
}
// the slot whose bit position a lane drops: the last one that is not useful; -1 with four or fewer slots per lane (nothing is dropped)
MADRL_ZM16_HD constexpr int drop_slot(int P, int R, int lane) {
    const int ns = lane_slots(P, R, 1);
    int d = -1;
    for (int s = 0; s < (ns == 5 ? ns : 0); ++s)
        if (!useful(P, R, lane + LANES * s)) d = s;
    return d;
}
// the lane's constant: in every byte the bit positions BELOW the dropped one (all four nibble bits when nothing is dropped)
MADRL_ZM16_HD constexpr uint32_t keep_low(int P, int R, int lane) {
    const int ns = lane_slots(P, R, 1);
    if (ns != 5) return 0x0F0F0F0Fu;
    return 0x01010101u * ((1u << (ns - 1 - drop_slot(P, R, lane))) - 1u);
}
// the bits of the in-register dword that belong to the lane's useful slots
MADRL_ZM16_HD constexpr uint32_t useful_bits(int P, int R, int lane) {
    const int ns = lane_slots(P, R, 1);
    uint32_t u = 0u;
    for (int s = 0; s < ns; ++s)
        if (useful(P, R, lane + LANES * s)) u |= 0x01010101u << (ns - 1 - s);
    return u;
}

// v_perm_b32 for the selectors used below (0..3: a byte of `lo`, 4..7: a byte of `hi`, 0x0C: 0x00)
MADRL_ZM16_HD inline uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    uint32_t r = 0u;
    for (int k = 0; k < 4; ++k) {
        const uint32_t c = (sel >> (8 * k)) & 0xFFu;
        const uint32_t b = c < 4u ? (lo >> (8 * c)) & 0xFFu : c < 8u ? (hi >> (8 * (c - 4u))) & 0xFFu : 0u;
        r |= b << (8 * k);
    }
    return r;
#endif
}
// (a & m) | (b & ~m), a bit select
MADRL_ZM16_HD inline uint32_t bfi(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }

// in-register dword -> the lane's 16 bits (cell k in nibble k).  keep = keep_low of the lane.
MADRL_ZM16_HD inline uint32_t pack(uint32_t x, uint32_t keep) {
    const uint32_t n = bfi(keep, x, x >> 1) & 0x0F0F0F0Fu;   // the dropped position deleted from all four bytes
    const uint32_t t = n | (n >> 4);                         // byte 0 = cells 1:0, byte 2 = cells 3:2
    return perm(0u, t, 0x0C0C0200u);
}
// the lane's 16 bits (upper 16 bits of h: ignored) -> in-register dword; the dropped position takes the bit below it (never consulted)
MADRL_ZM16_HD inline uint32_t unpack(uint32_t h, uint32_t keep) {
    const uint32_t t = perm(0u, h, 0x0C010C00u);             // byte 0 = cells 1:0, byte 2 = cells 3:2
    const uint32_t n = (t | (t << 4)) & 0x0F0F0F0Fu;
    return bfi(keep, n, n << 1);
}

}  // namespace zm16
}  // namespace madrl
