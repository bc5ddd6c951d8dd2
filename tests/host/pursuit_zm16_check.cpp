// pursuit_zm16_check.cpp -- the 16-bit-per-lane stale-zero mask format (madrl_amd/csrc/pursuit_zm16.hpp) on a CPU.
// tests/test_pursuit_zm16_cpu.py compiles this with -fsanitize=address,undefined and runs it.  Per X line of pursuit_specializations.def it
// prints the predicate (compared with tests/fixtures/pursuit_zm16_shapes.txt); for every line that has the format and every lane it checks
//   unpack(pack(x)) & U == x & U   for every subset x of the lane's useful bits U when |U| <= 16, and in any case for each single bit, all
//                                  ones, all zeros and 4 096 seeded random words (random words also carry bits outside U),
//   pack(0xFFFFFFFF) == 0xFFFF and pack(0) == 0,
// and the format's premises: at most four useful slots, the dropped slot not useful, U inside the bits pack keeps.
// Exit status 1 and a line on stderr per failure.
#include <stdio.h>

#include "../../madrl_amd/csrc/pursuit_zm16.hpp"

namespace {

using namespace madrl::zm16;

int failures = 0;
void fail(const char *what, int P, int R, int lane, uint32_t x, uint32_t got) {
    if (++failures <= 20) fprintf(stderr, "FAIL %s P=%d R=%d lane=%d x=%08x got=%08x\n", what, P, R, lane, x, got);
}

uint64_t rng = 0x9E3779B97F4A7C15ull;
uint32_t draw() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng >> 32);
}

void round_trip(int P, int R, int lane, uint32_t keep, uint32_t U, uint32_t x) {
    const uint32_t h = pack(x, keep);
    if (h >> 16) fail("pack: bits above 16", P, R, lane, x, h);
    // the kernel hands unpack a dword whose other half is another lane's: those bits must not matter
    const uint32_t y = unpack(h | 0xA5C30000u, keep);
    if ((y & U) != (x & U)) fail("round trip", P, R, lane, x, y);
}

long check_shape(int P, int R) {
    const int ns = lane_slots(P, R, 1);
    long words = 0;
    for (int lane = 0; lane < LANES; ++lane) {
        const uint32_t keep = keep_low(P, R, lane), U = useful_bits(P, R, lane);
        const int drop = drop_slot(P, R, lane);
        if (useful_slots(P, R, lane) > 4) fail("more than four useful slots", P, R, lane, U, 0);
        if (ns == 5 && (drop < 0 || useful(P, R, lane + LANES * drop))) fail("dropped slot", P, R, lane, U, (uint32_t)drop);
        if (ns != 5 && drop != -1) fail("a slot dropped with four or fewer", P, R, lane, U, (uint32_t)drop);
        if (ns == 5 && (U & (0x01010101u << (ns - 1 - drop)))) fail("useful bit at the dropped position", P, R, lane, U, (uint32_t)drop);
        if (pack(0xFFFFFFFFu, keep) != 0xFFFFu) fail("pack(all ones)", P, R, lane, 0xFFFFFFFFu, pack(0xFFFFFFFFu, keep));
        if (pack(0u, keep) != 0u) fail("pack(0)", P, R, lane, 0u, pack(0u, keep));
        int bits[32], nb = 0;
        for (int b = 0; b < 32; ++b)
            if (U >> b & 1u) bits[nb++] = b;
        if (nb <= 16) {   // every subset of U
            for (uint32_t sub = 0; sub < (1u << nb); ++sub, ++words) {
                uint32_t x = 0u;
                for (int k = 0; k < nb; ++k)
                    if (sub >> k & 1u) x |= 1u << bits[k];
                round_trip(P, R, lane, keep, U, x);
            }
        }
        for (int k = 0; k < nb; ++k, ++words) round_trip(P, R, lane, keep, U, 1u << bits[k]);
        round_trip(P, R, lane, keep, U, 0xFFFFFFFFu);
        round_trip(P, R, lane, keep, U, 0u);
        round_trip(P, R, lane, keep, U, U);
        for (int k = 0; k < 4096; ++k, ++words) round_trip(P, R, lane, keep, U, draw());
    }
    return words;
}

}  // namespace

int main() {
    struct Line { int xs, ys, P, E, R, flatten; };
    const Line lines[] = {
#define X(XS, YS, NP, NE, R, FL) {XS, YS, NP, NE, R, FL},
#define XG(XS, YS, NP, NE, R, FL, NW)
#include "../../madrl_amd/csrc/pursuit_specializations.def"
#undef X
#undef XG
    };
    for (const Line &l : lines) {
        const bool z = eligible(l.P, l.R, l.flatten);
        int most = 0;
        if (l.flatten)
            for (int lane = 0; lane < LANES; ++lane) most = useful_slots(l.P, l.R, lane) > most ? useful_slots(l.P, l.R, lane) : most;
        printf("X(%d,%d,%d,%d,%d,%d) slots=%d useful=%d zm16=%d", l.xs, l.ys, l.P, l.E, l.R, l.flatten, lane_slots(l.P, l.R, l.flatten), most, z ? 1 : 0);
        if (z) printf(" words=%ld", check_shape(l.P, l.R));
        printf("\n");
    }
    return failures ? 1 : 0;
}
