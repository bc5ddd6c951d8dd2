// pursuit_wide_check.cpp -- pursuit_rules_check.cpp's comparison at the 32-bit edges of the two Philox counter words: the device side's
// statement of the reset rules (madrl_amd/csrc/pursuit_rules.hpp) against the oracle's independent one (oracle/pursuit_oracle.c, linked in;
// it does not include the header), for global env indices on both sides of 2^31 and up to 2^32 - 2, and ticks that cross 2^31 and wrap
// at 2^32.  The GPU tests at these values (tests/test_wide_counters_gpu.py) trust the oracle there; this pins it without a GPU.
// tests/test_wide_counters_cpu.py compiles both with -fsanitize=address,undefined and runs this.
//
// 64 envs, 16 x 16, 8 v 30, three maps, sample_maps, constraint_window 0.5, max_opponents 10 (every reset rule draws).  The oracle's tick is
// set through po_set_state, then two resets follow; every env's map id, evader count and every agent's position are recomputed from the
// header alone with gid = (uint32_t)(env_id_base + n) and the tick of that reset:
//   f  env_id_base 2^31 - 32 (the batch straddles bit 31), ticks 2^31 - 1 and 2^31
//   g  env_id_base 2^32 - 1 - 64 (the largest the library accepts for 64 envs), ticks 2^32 - 1 and 0: the tick wraps
//   h  env_id_base 2^31 + 5, tick 2^31 + 7 and the next: both words with bit 31 set
// The program also checks that bit 31 matters: the same draws with bit 31 of gid, or of tick, cleared must place agents elsewhere.
// Exit status 1 and a line on stderr per failure; one line on stdout per case.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../madrl_amd/csrc/pursuit_rules.hpp"

extern "C" {
struct po_config {   // as oracle/pursuit_oracle.c declares it
    int32_t xs, ys, n_pursuers, n_evaders, obs_range, n_catch, surround, flatten, include_id, reward_global, sample_maps, n_maps, max_opponents,
        train_pursuit;
    double catchr, term_pursuit, urgency_reward, layer_norm, constraint_window;
};
struct po_handle;
int po_obs_dim_of(const po_config *c);
po_handle *po_create(const po_config *cfg, const int8_t *maps, int64_t n_envs, uint64_t seed, int64_t env_id_base);
void po_destroy(po_handle *h);
void po_reset(po_handle *h, const uint8_t *mask, const int32_t *inj_pos, const int32_t *inj_map, float *obs);
void po_get_state(const po_handle *h, int32_t *pos_p, int32_t *pos_e, uint8_t *gone, uint8_t *term_p, uint8_t *term_e, int32_t *map_id,
                  uint32_t *tick);
void po_set_state(po_handle *h, const int32_t *pos_p, const int32_t *pos_e, const uint8_t *gone, const uint8_t *term_p, const uint8_t *term_e,
                  const int32_t *map_id, const uint32_t *tick);
}

namespace {

using namespace madrl;

constexpr int64_t N = 64;
constexpr int XS = 16, YS = 16, P = 8, E = 30, N_MAPS = 3, MAX_OPP = 10;
constexpr double CW = 0.5;
constexpr uint64_t SEED = 0x5EED0123C0FFEE42ull;

int failures = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond) && ++failures <= 20) {                       \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, "\n");                               \
        }                                                        \
    } while (0)

struct State {
    std::vector<int32_t> pos_p = std::vector<int32_t>(N * P * 2), pos_e = std::vector<int32_t>(N * E * 2), map_id = std::vector<int32_t>(N);
    std::vector<uint8_t> gone = std::vector<uint8_t>(N * E), term_p = std::vector<uint8_t>(N * P), term_e = std::vector<uint8_t>(N * E);
    std::vector<uint32_t> tick = std::vector<uint32_t>(N);
    void get(const po_handle *h) { po_get_state(h, pos_p.data(), pos_e.data(), gone.data(), term_p.data(), term_e.data(), map_id.data(), tick.data()); }
    void set(po_handle *h) const { po_set_state(h, pos_p.data(), pos_e.data(), gone.data(), term_p.data(), term_e.data(), map_id.data(), tick.data()); }
};

// the position the header gives agent `aidx` of env `gid` at `tick`: draws until a free cell of the map comes up
pr::Cell place(const int8_t *map, uint32_t gid, uint32_t tick, uint32_t aidx, uint32_t k0, uint32_t k1, const pr::Window &w) {
    pr::Cell cell{0, 0};
    for (uint32_t att = 0; att < 1024u; ++att) {
        cell = pr::reset_cell(gid, tick, aidx, att, k0, k1, w);
        if (map[cell.x * YS + cell.y] != -1) break;
    }
    return cell;
}

// one reset of every env from the header alone against the oracle's state after that reset; -> agents that bit 31 of gid / of tick moves
void check_reset(const char *name, const State &o, const std::vector<int8_t> &maps, int64_t id_base, uint32_t tick, int *moved_gid, int *moved_tick) {
    const uint32_t k0 = (uint32_t)SEED, k1 = (uint32_t)(SEED >> 32);
    for (int64_t n = 0; n < N; ++n) {
        const uint32_t gid = (uint32_t)(id_base + n);
        const int map_id = pr::reset_map_id(gid, tick, k0, k1, N_MAPS);
        const pr::Window w = pr::reset_window(gid, tick, k0, k1, CW, XS, YS);
        const int n_create = pr::reset_n_create(gid, tick, k0, k1, MAX_OPP, E);
        CHECK(map_id == o.map_id[n], "%s env %d (gid %u, tick %u): map %d, oracle %d", name, (int)n, gid, tick, map_id, o.map_id[n]);
        CHECK(o.tick[n] == tick + 1u, "%s env %d: oracle tick %u after the reset at %u", name, (int)n, o.tick[n], tick);
        const int8_t *map = maps.data() + (size_t)map_id * XS * YS;
        for (int a = 0; a < P + E; ++a) {
            const bool is_p = a < P;
            const int slot = is_p ? a : a - P;
            const int32_t *want = is_p ? &o.pos_p[(n * P + slot) * 2] : &o.pos_e[(n * E + slot) * 2];
            if (!is_p && slot >= n_create) {
                CHECK(o.gone[n * E + slot] == 1 && want[0] == -1 && want[1] == -1, "%s env %d evader %d: created by the oracle", name, (int)n, slot);
                continue;
            }
            const pr::Cell cell = place(map, gid, tick, (uint32_t)a, k0, k1, w);
            CHECK(cell.x == want[0] && cell.y == want[1], "%s env %d (gid %u, tick %u) agent %d: (%d, %d), oracle (%d, %d)", name, (int)n, gid, tick, a, cell.x,
                  cell.y, want[0], want[1]);
            const pr::Cell g31 = place(map, gid ^ 0x80000000u, tick, (uint32_t)a, k0, k1, w), t31 = place(map, gid, tick ^ 0x80000000u, (uint32_t)a, k0, k1, w);
            *moved_gid += g31.x != cell.x || g31.y != cell.y;
            *moved_tick += t31.x != cell.x || t31.y != cell.y;
        }
    }
}

void run_case(const char *name, int64_t id_base, uint32_t first_tick, const std::vector<int8_t> &maps) {
    po_config c{};
    c.xs = XS; c.ys = YS; c.n_pursuers = P; c.n_evaders = E;
    c.obs_range = 7; c.n_catch = 2; c.surround = 1; c.flatten = 1; c.include_id = 1; c.reward_global = 0;
    c.sample_maps = 1; c.n_maps = N_MAPS; c.max_opponents = MAX_OPP; c.train_pursuit = 1;
    c.catchr = 0.01; c.term_pursuit = 5.0; c.urgency_reward = -0.1; c.layer_norm = 10.0; c.constraint_window = CW;
    CHECK(id_base + N <= 0xFFFFFFFFll, "%s: the library refuses this base", name);
    po_handle *h = po_create(&c, maps.data(), N, SEED, id_base);
    std::vector<float> obs((size_t)N * P * (size_t)po_obs_dim_of(&c));
    State st;
    po_reset(h, nullptr, nullptr, nullptr, obs.data());   // a state po_set_state can hand back
    st.get(h);
    for (auto &t : st.tick) t = first_tick;
    st.set(h);
    int moved_gid = 0, moved_tick = 0;
    uint32_t tick = first_tick;
    for (int k = 0; k < 2; ++k, tick += 1u) {   // (uint32_t: 2^32 - 1 is followed by 0)
        po_reset(h, nullptr, nullptr, nullptr, obs.data());
        st.get(h);
        check_reset(name, st, maps, id_base, tick, &moved_gid, &moved_tick);
    }
    CHECK(moved_gid > N && moved_tick > N, "%s: clearing bit 31 moves %d (gid) and %d (tick) agents -- does it reach the counter?", name, moved_gid, moved_tick);
    printf("%s base=%lld ticks=%u,%u moved_by_gid_bit31=%d moved_by_tick_bit31=%d\n", name, (long long)id_base, first_tick, first_tick + 1u, moved_gid, moved_tick);
    po_destroy(h);
}

}  // namespace

int main() {
    static const int at3[3][2] = {{2, 3}, {8, 1}, {5, 9}};
    std::vector<int8_t> maps((size_t)N_MAPS * XS * YS, 0);   // a 6 x 6 building block in each map, at its own place
    for (int k = 0; k < N_MAPS; ++k)
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) maps[((size_t)k * XS + at3[k][0] + i) * YS + at3[k][1] + j] = -1;
    run_case("f", (1ll << 31) - 32, 0x7FFFFFFFu, maps);
    run_case("g", (1ll << 32) - 1 - N, 0xFFFFFFFFu, maps);
    run_case("h", (1ll << 31) + 5, 0x80000007u, maps);
    if (failures) fprintf(stderr, "%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
