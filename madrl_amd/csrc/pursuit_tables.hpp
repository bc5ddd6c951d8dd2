// pursuit_tables.hpp -- the host-built tables of the Pursuit kernels (pursuit.hip), as pure host functions: the configuration's layout,
// the generic kernel's byte image (maps | count template | value table | slot codes) and the wave / group kernels' dword image (float maps |
// slot codes | count template | slot table), with the rules that make a configuration eligible for its fast line.  No HIP call, no handle,
// no device pointer is touched here, so tests/host/pursuit_tables_check.cpp runs all of it under the sanitizers on a machine without a GPU.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/madrl_hip.h"

namespace {   // internal linkage, like the rest of pursuit.hip's host side (PursuitDev is a kernel argument: its name is part of theirs)

// slot-code kinds (one code per element of an agent's observation row, built on the host)
enum : uint32_t { K_GRID = 0, K_ID = 1, K_FILL = 2, K_SKIP = 3 };

constexpr uint32_t PAD_MAP = 0xFEu;  // map layer outside the map  -> vtab[0xFE] = 1/layer_norm
constexpr uint32_t PAD_CNT = 0xFFu;  // count layers outside the map -> "do not store" (Q2)
constexpr uint32_t SENT = 0xFFFFFFFFu;  // the wave / group kernels' count layers outside the map (pw::SENT, pursuit_wave.hpp)

struct PursuitDev {
    int32_t xs, ys, P, E, A, R, D;
    int32_t pad, GW, GSZ;  // padded grid: width (y extent), bytes per layer (multiple of 16)
    int32_t n_catch, surround, reward_global, sample_maps, n_maps, max_steps, auto_reset;
    int32_t max_opponents;  // > 0: random_opponents (pursuit_evade.py:177-181)
    int32_t train_pursuit;  // 0: the ACTIONS drive the evaders, the pursuers move by their controller (pursuit_evade.py:215-224)
    int32_t rec_bytes, off_gone, off_term, ngw, ntw;  // state record layout (byte offsets)
    int32_t map_stride;                               // bytes per map entry in `maps`
    uint32_t k0, k1, gid_base;
    float fill32;
    double catchr, term_pursuit, urgency, cw;
    int64_t n_envs;
    const uint8_t *maps;     // per map: padded wall layer [GSZ] then need_to_surround [xs*ys]
    const uint8_t *cnt_tmpl; // padded count-layer template [GSZ]: 0 inside, 0xFF outside
    const float *vtab;       // 256 floats: fl32(k / layer_norm), [0xFE] = fl32(1.0 / layer_norm)
    const uint32_t *codes;   // D slot codes
    const double *cw_env;     // per-env constraint_window / catchr (curriculum, pursuit_evade.py:264-272) or nullptr: the scalars above
    const double *catchr_env;
    uint8_t *state;
    uint32_t *flags;         // [n_envs] flag words (done_flag_word, common.hpp): in the caller's state buffer, behind the stale-zero masks
};

// state record: [u32 tick][u32 t][u32 map_id][u32 spare][u8 xy[2A]][u32 gone[ngw]][u32 term[ntw]]
constexpr int HDR_BYTES = 16;

constexpr size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int obs_dim_of(const madrl_pursuit_config *c) {
    const int R = c->obs_range;
    return c->flatten ? 3 * R * R + (c->include_id ? 1 : 0) : 4 * R * R;
}

void layout(const madrl_pursuit_config *c, PursuitDev *d) {
    memset(d, 0, sizeof(*d));
    d->xs = c->xs; d->ys = c->ys; d->P = c->n_pursuers; d->E = c->n_evaders; d->A = d->P + d->E;
    d->R = c->obs_range; d->D = obs_dim_of(c);
    const int off = (c->obs_range - 1) / 2;
    d->pad = off > 1 ? off : 1;
    d->GW = c->ys + 2 * d->pad;
    d->GSZ = (int)round_up((size_t)(c->xs + 2 * d->pad) * d->GW, 16);
    d->n_catch = c->n_catch; d->surround = c->surround; d->reward_global = c->reward_global;
    d->sample_maps = c->sample_maps; d->n_maps = c->n_maps; d->max_steps = c->max_steps;
    d->auto_reset = c->auto_reset;
    d->max_opponents = c->max_opponents;
    d->train_pursuit = !c->control_evaders;
    d->ngw = (d->E + 31) / 32; if (d->ngw < 1) d->ngw = 1;
    d->ntw = (d->A + 31) / 32;
    d->off_gone = (int)round_up(HDR_BYTES + 2 * (size_t)d->A, 4);
    d->off_term = d->off_gone + 4 * d->ngw;
    d->rec_bytes = (int)round_up((size_t)d->off_term + 4 * d->ntw, 16);
    d->map_stride = (int)round_up((size_t)d->GSZ + (size_t)c->xs * c->ys, 16);
    d->k0 = (uint32_t)c->seed; d->k1 = (uint32_t)(c->seed >> 32);
    d->gid_base = (uint32_t)c->env_id_base;
    d->catchr = c->catchr; d->term_pursuit = c->term_pursuit; d->urgency = c->urgency_reward;
    d->cw = c->constraint_window;
    d->fill32 = (float)(1.0 / c->layer_norm);  // local_obs[..][0].fill(1.0 / layer_norm), :433
}

// need_to_surround(x, y), pursuit_evade.py:523-540, tabulated per map cell
int need_to_surround(const int8_t *map, int xs, int ys, int x, int y) {
    static const int mx[4] = {-1, 1, 0, 0}, my[4] = {0, 0, 1, -1};
    int tosur = 4;
    if (x == 0 || x == xs - 1) tosur -= 1;
    if (y == 0 || y == ys - 1) tosur -= 1;
    for (int m = 0; m < 4; ++m) {
        const int xn = x + mx[m], yn = y + my[m];
        if (!(0 < xn && xn < xs) || !(0 < yn && yn < ys)) continue;  // sic: row/col 0 skipped
        if (map[xn * ys + yn] == -1) tosur -= 1;
    }
    return tosur;
}

// one map's need_to_surround table [xs * ys]
void fill_need(uint8_t *need, const int8_t *map, int xs, int ys) {
    for (int x = 0; x < xs; ++x)
        for (int y = 0; y < ys; ++y) need[x * ys + y] = (uint8_t)need_to_surround(map, xs, ys, x, y);
}

// Element r of an observation row: the cell (i, j) of layer c of the observer's window (K_GRID) -- or the agent's id (K_ID: the last element
// of a flatten row, :444-445, the centre of channel 3 of an (R, R, 4) row) or nothing at all (K_SKIP: the rest of channel 3, :440-441: only
// its centre is ever written)
struct RowElem {
    uint32_t kind;
    int c, i, j;
};
RowElem decode_row_elem(bool flatten, int R, int r) {
    if (flatten) {
        if (r == 3 * R * R) return {K_ID, 0, 0, 0};
        return {K_GRID, r / (R * R), (r % (R * R)) / R, r % R};
    }
    const int c = r % 4, i = (r / 4) / R, j = (r / 4) % R;  // rollaxis -> (R,R,4), :449
    if (c == 3) return {(i == R / 2 && j == R / 2) ? K_ID : K_SKIP, c, i, j};
    return {K_GRID, c, i, j};
}

// ------------------------------------------------------------------ the generic kernel's tables
struct GenericTables {
    std::vector<uint8_t> host;                          // the image of the device allocation
    size_t maps = 0, cnt = 0, vtab = 0, codes = 0;      // byte offsets in it
    int bad_map = -1, bad_x = 0, bad_y = 0, bad_v = 0;  // bad_map >= 0: that cell is neither 0 nor -1, and `host` is not to be used
};

GenericTables build_generic_tables(const madrl_pursuit_config *cfg, const PursuitDev &d, const int8_t *map_pool_host) {
    GenericTables t;
    const int xs = d.xs, ys = d.ys, pad = d.pad, GW = d.GW;
    t.cnt = round_up((size_t)d.map_stride * d.n_maps, 16);
    t.vtab = round_up(t.cnt + d.GSZ, 16);
    t.codes = t.vtab + 256 * sizeof(float);
    t.host.assign(round_up(t.codes + sizeof(uint32_t) * d.D, 16), 0);
    uint8_t *ct = t.host.data() + t.cnt;
    memset(ct, PAD_CNT, d.GSZ);
    for (int m = 0; m < d.n_maps; ++m) {
        const int8_t *map = map_pool_host + (size_t)m * xs * ys;
        uint8_t *wall = t.host.data() + (size_t)m * d.map_stride;
        memset(wall, PAD_MAP, d.GSZ);
        for (int x = 0; x < xs; ++x)
            for (int y = 0; y < ys; ++y) {
                const int8_t v = map[x * ys + y];
                if (v != 0 && v != -1) {
                    t.bad_map = m; t.bad_x = x; t.bad_y = y; t.bad_v = (int)v;
                    return t;
                }
                wall[(x + pad) * GW + y + pad] = (v == -1) ? 1 : 0;
                ct[(x + pad) * GW + y + pad] = 0;
            }
        fill_need(wall + d.GSZ, map, xs, ys);
    }
    // np.abs(model_state) / layer_norm is float32 / weak python scalar -> float32 (:438-439)
    float *vt = reinterpret_cast<float *>(t.host.data() + t.vtab);
    const float norm32 = (float)cfg->layer_norm;
    for (int k = 0; k < 256; ++k) vt[k] = (float)k / norm32;
    vt[PAD_MAP] = d.fill32;
    vt[PAD_CNT] = 0.0f;
    // slot codes: which padded-grid byte (relative to the window origin) feeds element r
    uint32_t *codes = reinterpret_cast<uint32_t *>(t.host.data() + t.codes);
    const int W = 2 * ((d.R - 1) / 2) + 1;  // copied window width (:451-461)
    for (int r = 0; r < d.D; ++r) {
        const RowElem e = decode_row_elem(cfg->flatten != 0, d.R, r);
        if (e.kind != K_GRID) codes[r] = e.kind << 24;
        else if (e.i < W && e.j < W) codes[r] = (K_GRID << 24) | (uint32_t)(e.c * d.GSZ + e.i * GW + e.j);
        else codes[r] = (e.c == 0 ? K_FILL : K_SKIP) << 24;  // even obs_range (Q11)
    }
    return t;
}

// ------------------------------------------------------------------ the wave / group kernels' tables (pursuit_wave.hpp, pursuit_group.hpp)
// the compiled geometry of an X / XG line that its tables are built to (of an XC line: nw, GSZ and the last four)
struct WaveGeom {
    int nw;  // wavefronts per env
    int GSZ, GW, PAD, X_ID, X_SKIP;
    int mwords;  // stale-zero mask dwords per lane
    int D, rec_bytes, off_gone, off_term;  // madrl_pursuit_create holds these against layout() (same_record)
    constexpr bool operator==(const WaveGeom &o) const {
        return nw == o.nw && GSZ == o.GSZ && GW == o.GW && PAD == o.PAD && X_ID == o.X_ID && X_SKIP == o.X_SKIP && mwords == o.mwords &&
               D == o.D && rec_bytes == o.rec_bytes && off_gone == o.off_gone && off_term == o.off_term;
    }
};

// ... of the line X(xs, ys, P, E, R, flatten) (nw = 1) / XG(..., nw), as pw::Shape / pw::GShape have it (a static_assert of pursuit.hip)
constexpr WaveGeom wave_geom(int xs, int ys, int P, int E, int R, int flatten, int nw) {
    const int pad = (R - 1) / 2 > 1 ? (R - 1) / 2 : 1, GW = ys + 2 * pad, GSZ = ((xs + 2 * pad) * GW + 3) / 4 * 4;
    const int D = flatten ? 3 * R * R + 1 : 4 * R * R, NS = (P * (D / 4) + 64 * nw - 1) / (64 * nw);
    const int ngw = (E + 31) / 32 > 0 ? (E + 31) / 32 : 1, off_gone = (HDR_BYTES + 2 * (P + E) + 3) / 4 * 4, off_term = off_gone + 4 * ngw;
    return WaveGeom{nw, GSZ, GW, pad, 3 * GSZ + 2, 3 * GSZ + 1, nw == 1 ? 1 : (NS + 7) / 8,
                    D, (off_term + 4 * ((P + E + 31) / 32) + 15) / 16 * 16, off_gone, off_term};
}

// what madrl_pursuit_create holds a line's compiled geometry against: the configuration's record and row (layout())
bool same_record(const WaveGeom &g, const PursuitDev &d) {
    return g.rec_bytes == d.rec_bytes && g.off_gone == d.off_gone && g.off_term == d.off_term && g.D == d.D;
}

// float4 slots per thread of the line's workgroup; more than 8: the slot constants are one packed table (pursuit_group.hpp, LONG ROWS)
int slots_per_thread(const PursuitDev &d, const WaveGeom &g) { return (d.P * (d.D / 4) + 64 * g.nw - 1) / (64 * g.nw); }

// May this configuration run on its line's kernel?  wc: its D slot codes in the wave format (build_wave_tables).  One rule per line.
bool wave_eligible(const madrl_pursuit_config *cfg, const PursuitDev &d, const WaveGeom &g, int64_t n_envs, const uint32_t *wc) {
    // the fast path tells 0.0f, observation values and its "outside the map" marker apart by the top byte of the value: every non-zero
    // observation value must be a positive float >= 2^-63 (top byte 0x20..0x7F) -- the wall value |-1| / layer_norm in float32, and the fill
    const float unit = (float)1 / (float)cfg->layer_norm;
    uint32_t unit_bits, fill_bits;
    memcpy(&unit_bits, &unit, 4);
    memcpy(&fill_bits, &d.fill32, 4);
    if ((unit_bits >> 24) < 0x20u || (unit_bits >> 24) >= 0x80u || (fill_bits >> 24) < 0x20u || (fill_bits >> 24) >= 0x80u) return false;
    if (!same_record(g, d)) return false;    // the compiled record and row are the configuration's
    if (n_envs >= 0x7FF00000ll) return false;  // the fast kernels index envs with 32-bit integers (index + workgroup count < 2^31)
    for (int r = 0; r < d.D; ++r)            // the kernels assume only element 3 of a float4 can be absolute
        if ((r & 3) != 3 && !(wc[r] >> 31)) return false;
    const int NS = slots_per_thread(d, g);
    if (NS > 8) {                            // the packed table: 15-bit dword offsets, and the mask words of the row-loop kernel
        if (3 * g.GSZ + 2 + d.P >= 32768) return false;
        for (int r = 0; r < d.D; ++r)
            if ((wc[r] & 0x7FFFFFFFu) >= 32768u) return false;
        if (g.mwords != (NS + 7) / 8) return false;
    }
    return true;
}

struct WaveTables {
    std::vector<uint32_t> host;                   // the image of the device allocation; empty when not eligible
    size_t w_codes = 0, w_tmpl = 0, w_slots = 0;  // dword offsets in it
    int fstride = 0;                              // dwords per map entry
    bool eligible = false;
};

// the image: per map the padded float layer [GSZ] and need_to_surround [xs * ys bytes] | slot codes [D] | empty count layer [GSZ] | per-thread
// slot table [NS][6][NT] -- or, for shapes with more than 8 slots per thread, one packed entry of two dwords per float4 of a pursuer's row [DV][2]
WaveTables build_wave_tables(const madrl_pursuit_config *cfg, const PursuitDev &d, const WaveGeom &g, int64_t n_envs, const int8_t *map_pool_host) {
    WaveTables t;
    const int xs = d.xs, ys = d.ys;
    const int NT = 64 * g.nw, DV = d.D / 4, NQ = d.P * DV, NS = slots_per_thread(d, g);
    const bool tabled = NS > 8;
    t.fstride = g.GSZ + (xs * ys + 3) / 4;
    t.w_codes = (size_t)t.fstride * d.n_maps;
    t.w_tmpl = t.w_codes + (size_t)d.D;
    t.w_slots = t.w_tmpl + (size_t)g.GSZ;
    std::vector<uint32_t> wh(t.w_slots + (tabled ? (size_t)2 * DV : (size_t)NS * 6 * NT), 0u);
    uint32_t *wc = wh.data() + t.w_codes;
    for (int r = 0; r < d.D; ++r) {
        const RowElem e = decode_row_elem(cfg->flatten != 0, d.R, r);
        wc[r] = e.kind == K_ID ? (uint32_t)g.X_ID : e.kind == K_SKIP ? (uint32_t)g.X_SKIP : 0x80000000u | (uint32_t)(e.c * g.GSZ + e.i * g.GW + e.j);
    }
    if (!wave_eligible(cfg, d, g, n_envs, wc)) return t;
    const float wallv = (float)1 / (float)cfg->layer_norm;  // |-1| / layer_norm in float32
    uint32_t wall_bits, fill_bits;
    memcpy(&wall_bits, &wallv, 4);
    memcpy(&fill_bits, &d.fill32, 4);
    for (int m = 0; m < d.n_maps; ++m) {
        const int8_t *map = map_pool_host + (size_t)m * xs * ys;
        uint32_t *fm = wh.data() + (size_t)m * t.fstride;
        for (int k = 0; k < g.GSZ; ++k) fm[k] = fill_bits;
        for (int x = 0; x < xs; ++x)
            for (int y = 0; y < ys; ++y) fm[(x + g.PAD) * g.GW + y + g.PAD] = (map[x * ys + y] == -1) ? wall_bits : 0u;
        fill_need(reinterpret_cast<uint8_t *>(fm + g.GSZ), map, xs, ys);
    }
    for (int k = 0; k < g.GSZ; ++k) {
        const int gx = k / g.GW - g.PAD, gy = k % g.GW - g.PAD;
        wh[t.w_tmpl + k] = (gx >= 0 && gx < xs && gy >= 0 && gy < ys) ? 0u : SENT;
    }
    // the packed table, entry f: dword 0 = off0 | off1 << 16, dword 1 = off2 | id3 << 15 | off3 << 16 | abs3 << 31 -- dword offsets into the LDS
    // array, relative to the window origin unless abs3 (element 3 only: the skip cell, or with id3 the id cell of pursuer 0 + pursuer)
    for (int f = 0; f < (tabled ? DV : 0); ++f) {
        const uint32_t *c = wc + 4 * f, abs3 = c[3] >> 31 ? 0u : 1u, id3 = (abs3 && (int)c[3] == g.X_ID) ? 1u : 0u;
        wh[t.w_slots + 2 * (size_t)f] = (c[0] & 0x7FFFu) | ((c[1] & 0x7FFFu) << 16);
        wh[t.w_slots + 2 * (size_t)f + 1] = (c[2] & 0x7FFFu) | (id3 << 15) | ((c[3] & 0x7FFFu) << 16) | (abs3 << 31);
    }
    for (int sl = 0; sl < (tabled ? 0 : NS); ++sl)
        for (int th = 0; th < NT; ++th) {
            const int q = th + NT * sl, pidx = q / DV, f = q % DV;
            uint32_t *row = wh.data() + t.w_slots + (size_t)sl * 6 * NT + th;
            for (int k = 0; k < 4; ++k) {
                const uint32_t c = (q < NQ) ? wc[4 * f + k] : (k == 3 ? (uint32_t)g.X_SKIP : 0u);
                uint32_t cst = c & 0x7FFFFFFFu;
                if ((int)cst >= g.X_ID && (int)cst < g.X_ID + d.P) cst = (uint32_t)(g.X_ID + pidx);  // this pursuer's id cell
                row[(size_t)NT * k] = cst;
                if (k == 3) row[(size_t)NT * 4] = c >> 31;
            }
            row[(size_t)NT * 5] = (uint32_t)(q < NQ ? pidx : 0);
        }
    t.host.swap(wh);
    t.eligible = true;
    return t;
}

}  // namespace
