// pursuit_tables_check.cpp -- the Pursuit table builders (madrl_amd/csrc/pursuit_tables.hpp) on a CPU: both builders over a fixed list of
// configurations, one line each with the images' sizes, offsets, fstride, the eligibility verdict and a 64-bit FNV-1a hash of each image.
// tests/test_pursuit_tables_cpu.py compiles this with -fsanitize=address,undefined, runs it and compares the output with
// tests/fixtures/pursuit_tables_expected.txt (recorded from the table code as it stood inside madrl_pursuit_create).
#include <stdio.h>

#include "../../madrl_amd/csrc/pursuit_tables.hpp"

namespace {

uint64_t fnv1a(const void *p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t k = 0; k < n; ++k) h = (h ^ static_cast<const uint8_t *>(p)[k]) * 0x100000001b3ull;
    return h;
}

// n_maps maps from a fixed seed, about 20 % walls, with walls in row 0 and column 0 (need_to_surround skips those neighbours, "sic")
std::vector<int8_t> draw_maps(int xs, int ys, int n_maps) {
    std::vector<int8_t> m((size_t)n_maps * xs * ys, 0);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int8_t &v : m) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        v = ((s >> 33) % 5 == 0) ? -1 : 0;
    }
    for (int k = 0; k < n_maps; ++k) {
        int8_t *map = m.data() + (size_t)k * xs * ys;
        map[0 * ys + ys / 2] = -1;
        map[(xs / 2) * ys + 0] = -1;
    }
    return m;
}

struct Case {
    const char *name;
    int xs, ys, P, E, R, flatten;
    int nw;  // wavefronts per env of the case's X / XG line, 0: the generic tables only
    int include_id = 1, n_maps = 1;
    double layer_norm = 10.0;
    int64_t n_envs = 64;
    int bad_cell = 0;  // 1: the last map's cell (1, 2) holds a 1
};

void run(const Case &k) {
    madrl_pursuit_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = (int32_t)sizeof(cfg);
    cfg.xs = k.xs; cfg.ys = k.ys; cfg.n_pursuers = k.P; cfg.n_evaders = k.E; cfg.obs_range = k.R; cfg.flatten = k.flatten;
    cfg.include_id = k.include_id; cfg.n_maps = k.n_maps; cfg.n_catch = 2; cfg.layer_norm = k.layer_norm; cfg.constraint_window = 1.0;
    PursuitDev d;
    layout(&cfg, &d);
    std::vector<int8_t> maps = draw_maps(k.xs, k.ys, k.n_maps);
    if (k.bad_cell) maps[(size_t)(k.n_maps - 1) * k.xs * k.ys + 1 * k.ys + 2] = 1;
    printf("%s (%d,%d,%d,%d,%d,%d) id=%d maps=%d norm=%g envs=%lld:", k.name, k.xs, k.ys, k.P, k.E, k.R, k.flatten, k.include_id, k.n_maps,
           k.layer_norm, (long long)k.n_envs);
    const GenericTables t = build_generic_tables(&cfg, d, maps.data());
    if (t.bad_map >= 0) {
        printf(" bad cell map=%d x=%d y=%d value=%d\n", t.bad_map, t.bad_x, t.bad_y, t.bad_v);
        return;
    }
    printf(" generic bytes=%zu maps=%zu cnt=%zu vtab=%zu codes=%zu hash=%016llx", t.host.size(), t.maps, t.cnt, t.vtab, t.codes,
           (unsigned long long)fnv1a(t.host.data(), t.host.size()));
    if (k.nw) {
        const WaveGeom g = wave_geom(k.xs, k.ys, k.P, k.E, k.R, k.flatten, k.nw);
        const WaveTables w = build_wave_tables(&cfg, d, g, k.n_envs, maps.data());
        printf(" | wave nw=%d eligible=%d", k.nw, w.eligible ? 1 : 0);
        if (w.eligible)
            printf(" dwords=%zu w_codes=%zu w_tmpl=%zu w_slots=%zu fstride=%d hash=%016llx", w.host.size(), w.w_codes, w.w_tmpl, w.w_slots,
                   w.fstride, (unsigned long long)fnv1a(w.host.data(), w.host.size() * sizeof(uint32_t)));
    }
    printf("\n");
}

}  // namespace

int main() {
    const Case cases[] = {
    // every committed X / XG line, with its line's geometry
#define X(XS, YS, NP, NE, R, FL) {"X", XS, YS, NP, NE, R, FL, 1},
#define XG(XS, YS, NP, NE, R, FL, NW) {"XG", XS, YS, NP, NE, R, FL, NW},
#include "../../madrl_amd/csrc/pursuit_specializations.def"
#undef X
#undef XG
        // the generic tables only
        {"even-R", 7, 9, 3, 4, 4, 1, 0},          // K_FILL / K_SKIP at the window's last row and column
        {"even-R-hwc", 7, 9, 3, 4, 4, 0, 0},
        {"no-id", 16, 16, 8, 30, 7, 1, 0, /*include_id*/ 0},
        {"pad-1", 5, 5, 1, 0, 1, 1, 0},           // obs_range 1: pad clamps to 1; no evaders
        {"three-maps", 13, 14, 3, 27, 7, 0, 1, 1, /*n_maps*/ 3},   // (on its X line: fstride, one float map after the other)
        // not eligible, on the smallest flatten line
        {"norm-1e30", 10, 10, 2, 2, 3, 1, 1, 1, 1, /*layer_norm*/ 1e30},   // top byte of 1 / layer_norm below 0x20
        {"envs-2^31", 10, 10, 2, 2, 3, 1, 1, 1, 1, 10.0, /*n_envs*/ 0x7FF00000ll},
        // a map cell that is neither 0 nor -1
        {"bad-cell", 10, 10, 2, 2, 3, 1, 1, 1, /*n_maps*/ 2, 10.0, 64, /*bad_cell*/ 1},
    };
    for (const Case &k : cases) run(k);
    return 0;
}
