// pursuit_crowd.hpp -- compile-time-specialised PursuitEvade kernel for CROWDS: more than 64 pursuers or evaders.
//
// The one-wavefront and the group kernel (pursuit_wave.hpp, pursuit_group.hpp) keep one agent per lane, the evaders' alive mask in one
// 64-bit scalar, the record in 64 dwords and three dword layers in LDS.  This kernel gives all of that up so that the shapes those two
// refuse -- up to 1 023 agents of a kind, maps up to 128 x 128 with obs_range 21, records of any length (the authors' CNN launch line,
// runners/old/rllab/pursuit_cnn.sh:1: 100 v 300, obs_range 21, (R, R, 4) rows, a 912-byte record) -- have a specialised kernel too.
// The shapes are the XC lines of pursuit_crowd_specializations.def; the kernels are instantiated in pursuit_crowd.hip.
//
// Design (DESIGN.md "pursuit_crowd_kernel"):
//   * One workgroup of NW wavefronts per env, persistent over envs.  Agents are LOOPED over the threads; positions, the gone / terminal
//     bit words and the window origins live in LDS.  An evader's index in the evader layer is a popcount over the gone words, as in
//     the generic kernel (pursuit_generic.inc), whose packed record and whose tables (padded byte maps, need_to_surround, value table)
//     this kernel reads as they are: the two are interchangeable step by step on one state buffer.
//   * LDS holds ONE PACKED DWORD PER CELL of the padded grid: byte 0 the map (0 free, 1 building, 0xFE outside the map), byte 1 the
//     pursuer count, byte 2 the evader count, byte 3 the catch credit (purs_sur).  One LDS read feeds one (R, R, 4) float4.  Counts
//     are placed with one ds_add per agent and taken away again after the row pass (the dword arithmetic is modular, so even a count
//     that leaves its byte -- the overflow mark -- leaves the cells as they were); the cells are rewritten only when the env's map
//     differs from the previous env's, expanded from the 4x smaller byte map.
//   * Row pass: float4 slot q of the env's P*D/4 goes to thread q % NT, a rolled loop: every store instruction writes consecutive
//     float4 from consecutive lanes.  (R, R, 4) rows: a cell inside the map is one non-temporal float4 when channel 3 of the env's rows
//     is known to hold +0.0 (one word per env behind the records, CrowdDev::ch3: madrl_pursuit_declare_obs_zero sets it, every event
//     after which the buffer is unknown clears it -- the kernel never stores anything but +0.0 there, so the knowledge never expires
//     by itself), else three dwords; a cell outside the map is one dword (channel 0).  The centre cell always is a whole float4.
//     Flatten rows: a float4 whose four elements are all stored (channel 0, the id, count cells inside the map) is whole, one that
//     holds a count cell outside the map falls back to dword stores.
//   * Barriers are LDS-only (group_sync): no wavefront waits for its row stores at a barrier.
#pragma once

#include "common.hpp"

namespace madrl {
namespace pc {

constexpr uint32_t PAD_MAP = 0xFEu;    // map byte outside the map (value table entry: 1 / layer_norm)
constexpr int MAX_CELL_COUNT = 253;    // as in the generic kernel: one more agent of a kind on a cell raises the overflow mark
constexpr int HDR_BYTES = 16;

struct CrowdDev {
    int32_t n_catch, surround, reward_global, sample_maps, n_maps, max_steps, auto_reset;
    int32_t max_opponents;   // > 0: random_opponents (pursuit_evade.py:177-181)
    int32_t map_stride;      // bytes per map entry in `maps`
    uint32_t k0, k1, gid_base;
    double catchr, term_pursuit, urgency, cw;
    int64_t n_envs;
    const uint8_t *maps;     // the generic kernel's table: per map the padded wall layer [GSZ bytes], then need_to_surround [XS*YS]
    const float *vtab;       // 256 floats: fl32(k / layer_norm), [0xFE] = fl32(1.0 / layer_norm)
    const double *cw_env;    // per-env constraint_window / catchr (curriculum) or nullptr: the scalars above
    const double *catchr_env;
    uint8_t *state;
    uint32_t *flags;         // [n_envs] flag words of the step launches (done_flag_word, common.hpp)
    const uint32_t *ch3;     // [n_envs] 0: channel 3 of the env's (R, R, 4) rows holds +0.0 off the centre; anything else: not known
};

struct CrowdIO {
    const uint8_t *mask;       // reset mode
    const int32_t *inj_pos;    // reset mode
    const int32_t *inj_map;    // reset mode
    const int32_t *actions;    // step mode
    const int32_t *inj_eact;   // step mode
    float *obs;
    float *rew;
    uint8_t *done;
    int32_t *removed;
};

template <int XS_, int YS_, int P_, int E_, int R_, int FLATTEN_, int NW_>
struct CShape {
    static constexpr int XS = XS_, YS = YS_, P = P_, E = E_, A = P_ + E_, R = R_, FLATTEN = FLATTEN_, NW = NW_, NT = 64 * NW_;
    static constexpr int OFF = (R - 1) / 2;
    static constexpr int PAD = OFF > 1 ? OFF : 1;
    static constexpr int GW = YS + 2 * PAD;
    static constexpr int GH = XS + 2 * PAD;
    static constexpr int GSZ = (GH * GW + 15) / 16 * 16;           // cells: the generic kernel's bytes per layer
    static constexpr int D = FLATTEN ? 3 * R * R + 1 : 4 * R * R;  // include_id is implied
    static constexpr int DV = D / 4;                               // float4 per pursuer row
    static constexpr int NQ = P * DV;                              // float4 slots per env
    // packed state record, identical to the generic kernel's layout() in pursuit.hip
    static constexpr int NGW = (E + 31) / 32 > 0 ? (E + 31) / 32 : 1;
    static constexpr int NTW = (A + 31) / 32;
    static constexpr int OFF_GONE = (HDR_BYTES + 2 * A + 3) / 4 * 4;
    static constexpr int OFF_TERM = OFF_GONE + 4 * NGW;
    static constexpr int REC_BYTES = (OFF_TERM + 4 * NTW + 15) / 16 * 16;
    // LDS, in dwords
    static constexpr int X_CELL = 0;
    static constexpr int X_VTAB = GSZ;                                       // 256 floats
    static constexpr int X_CODE = X_VTAB + 256;                              // flatten: D element codes
    static constexpr int X_REW = X_CODE + (FLATTEN ? (D + 3) / 4 * 4 : 0);   // P doubles (global reward)
    static constexpr int X_BASE = X_REW + 2 * ((P + 1) / 2 * 2);             // P window origins
    static constexpr int X_KPRE = X_BASE + (P + 3) / 4 * 4;                  // P pre-move counts
    static constexpr int X_GONE = X_KPRE + (P + 3) / 4 * 4;
    static constexpr int X_PLACED = X_GONE + (NGW + 3) / 4 * 4;              // evaders whose count is in the cells
    static constexpr int X_TERM = X_PLACED + (NGW + 3) / 4 * 4;
    static constexpr int X_MISC = X_TERM + (NTW + 3) / 4 * 4;                // [0..3] header, [4] removed
    static constexpr int X_XY = X_MISC + 8;                                  // u8 x[A16], y[A16]
    static constexpr int A16 = (A + 15) / 16 * 16;
    static constexpr int LDS_DWORDS = X_XY + 2 * A16 / 4;
    static constexpr int CENTRE = (R / 2) * R + R / 2;                       // (R, R, 4) rows: the float4 that holds the id
    static_assert(NW >= 1 && NW <= 16, "1 .. 16 wavefronts per workgroup");
    static_assert(P >= 1 && P <= 1023 && E >= 0 && E <= 1023, "agent counts up to the generic kernel's MAX_COUNT");
    static_assert(XS >= 1 && YS >= 1 && XS <= 255 && YS <= 255, "coordinates are bytes of the record");
    static_assert(R % 2 == 1, "odd obs_range only (even ranges run on the generic kernel)");
    static_assert(D % 4 == 0, "observation row must be a whole number of float4");
    static_assert(LDS_DWORDS * 4 <= 160 * 1024, "LDS budget: one workgroup may declare 160 KiB");
    static_assert(X_REW % 2 == 0, "the reward doubles are 8-byte aligned");
};

// ds_add of one agent to byte `sh / 8` of a cell; *ovf as in the generic kernel's lds_byte_add
__device__ __forceinline__ void cell_add(uint32_t *cell, int idx, unsigned sh, uint32_t *ovf) {
    const unsigned old = atomicAdd(&cell[idx], 1u << sh);
    if (((old >> sh) & 0xFFu) >= (unsigned)MAX_CELL_COUNT) *ovf = 1u;
}

// numpy float64 add.reduce order (pairwise, 8-way unrolled base case; the recursive split above 128 elements): see pursuit.hip
__device__ __forceinline__ double np_base(const double *a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}
template <int N>
__device__ __forceinline__ double np_sum(const double *a) {
    if constexpr (N <= 128) return np_base(a, N);
    else {
        constexpr int N2 = N / 2 - (N / 2) % 8;
        return np_sum<N2>(a) + np_sum<N - N2>(a + N2);
    }
}

// workgroup barrier that waits for LDS traffic only (a wavefront does not wait for its row stores here)
__device__ __forceinline__ void group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef float v4f __attribute__((ext_vector_type(4)));

// MODE 0: reset(mask)   MODE 1: step (+ fused auto-reset)
template <class S, int MODE>
__global__ __launch_bounds__(S::NT) void pursuit_crowd_kernel(const CrowdDev d, const CrowdIO io) {
    constexpr int P = S::P, E = S::E, A = S::A, GW = S::GW, PAD = S::PAD, GSZ = S::GSZ, NT = S::NT, D = S::D, DV = S::DV, NQ = S::NQ;
    constexpr int R = S::R, OFF = S::OFF, NGW = S::NGW, NTW = S::NTW;
    __shared__ __attribute__((aligned(16))) uint32_t L[S::LDS_DWORDS];
    const int tid0 = threadIdx.x;
    uint32_t *const cell = &L[S::X_CELL];
    float *const s_vtab = reinterpret_cast<float *>(&L[S::X_VTAB]);
    uint32_t *const s_code = &L[S::X_CODE];
    double *const s_rew = reinterpret_cast<double *>(&L[S::X_REW]);
    int32_t *const s_base = reinterpret_cast<int32_t *>(&L[S::X_BASE]);
    int32_t *const s_kpre = reinterpret_cast<int32_t *>(&L[S::X_KPRE]);
    uint32_t *const s_gone = &L[S::X_GONE];
    uint32_t *const s_placed = &L[S::X_PLACED];
    uint32_t *const s_term = &L[S::X_TERM];
    uint32_t *const s_misc = &L[S::X_MISC];
    uint8_t *const s_ax = reinterpret_cast<uint8_t *>(&L[S::X_XY]);
    uint8_t *const s_ay = s_ax + S::A16;

    // ---- once per workgroup: the value table and (flatten) the element codes: channel << 24 | cell offset in the window; channel 3 = the id
    for (int k = tid0; k < 256; k += NT) s_vtab[k] = d.vtab[k];
    if constexpr (S::FLATTEN) {
        for (int r = tid0; r < D; r += NT) {
            const int c = r / (R * R), rr = r - c * (R * R), i = rr / R, j = rr - i * R;
            s_code[r] = c == 3 ? (3u << 24) : (((uint32_t)c << 24) | (uint32_t)(i * GW + j));
        }
    }
    int cached_map = -1;   // the map whose bytes the cells hold; the count and credit bytes are zero between envs

    for (int64_t env = blockIdx.x; env < d.n_envs; env += gridDim.x) {
        if (MODE == 0 && io.mask != nullptr && io.mask[env] == 0) continue;  // block-uniform
        // (a fresh copy per env: what is derived from the thread index -- LDS addresses, lane predicates -- is then computed where it is
        // used instead of being held in registers across the env loop, which the 128 registers of a 16-wavefront workgroup cannot afford)
        const int tid = fresh(tid0);
        uint8_t *rec = d.state + env * (int64_t)S::REC_BYTES;
        group_sync();  // the previous env's LDS traffic is finished
        // ------------------------------------------------------------ load state record
        if (tid < 4) s_misc[tid] = reinterpret_cast<const uint32_t *>(rec)[tid];
        if (tid == 4) s_misc[4] = 0;
        for (int a = tid; a < A; a += NT) {
            const uint32_t xy = reinterpret_cast<const uint16_t *>(rec + HDR_BYTES)[a];
            s_ax[a] = (uint8_t)(xy & 0xFF);
            s_ay[a] = (uint8_t)(xy >> 8);
        }
        for (int w = tid; w < NGW; w += NT) {
            const uint32_t g = reinterpret_cast<const uint32_t *>(rec + S::OFF_GONE)[w];
            s_gone[w] = g;
            s_placed[w] = ~g;   // step mode: the evaders the pre-move pass counts
        }
        for (int w = tid; w < NTW; w += NT) s_term[w] = reinterpret_cast<const uint32_t *>(rec + S::OFF_TERM)[w];
        const bool ch3_zero = !S::FLATTEN && d.ch3[env] == 0u;
        group_sync();
        uint32_t tick = s_misc[0];
        int32_t tstep = (int32_t)s_misc[1];
        int32_t map_id = (int32_t)s_misc[2];
        const uint32_t gid = d.gid_base + (uint32_t)env;
        bool do_reset = (MODE == 0);
        uint32_t done_bits = 0;

        // the cells take the map's bytes (count and credit bytes: zero).  Only called while no agent is placed.
        auto load_map = [&](int m) {
            if (cached_map == m) return;
            const uint32_t *mt = reinterpret_cast<const uint32_t *>(d.maps + (int64_t)m * d.map_stride);
            for (int k = tid; k < GSZ / 4; k += NT) {
                const uint32_t w = mt[k];
                reinterpret_cast<uint4 *>(cell)[k] = make_uint4(w & 0xFFu, (w >> 8) & 0xFFu, (w >> 16) & 0xFFu, w >> 24);
            }
            cached_map = m;
        };

        // -------------------------------------------------------------- observations (:418-461)
        auto write_obs = [&]() {
            // (the env's rows through a wave-uniform base and 32-bit offsets: P * D floats are far below 4 GB)
            typedef __attribute__((address_space(1))) float gfloat;
            typedef __attribute__((address_space(1))) v4f gv4f;
            gfloat *const orow = uniform_ptr(io.obs + env * (int64_t)P * D);
            int p = tid / DV, f = tid - p * DV;
            constexpr int dp = NT / DV, df = NT - dp * DV;
#pragma unroll 2
            for (uint32_t q = (uint32_t)tid; q < (uint32_t)NQ; q += (uint32_t)NT) {
                const int base = s_base[p];
                gfloat *const o = orow + 4u * q;
                if constexpr (S::FLATTEN) {
                    const uint4 cd = reinterpret_cast<const uint4 *>(s_code)[f];
                    const uint32_t code[4] = {cd.x, cd.y, cd.z, cd.w};
                    float val[4];
                    bool keep[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t ch = code[k] >> 24;
                        if (ch == 3u) {
                            val[k] = (float)((double)p / (double)P);  // :440-445
                            keep[k] = true;
                        } else {
                            const uint32_t c = cell[base + (int)(code[k] & 0xFFFFFFu)];
                            val[k] = s_vtab[(c >> (8u * ch)) & 0xFFu];
                            keep[k] = ch == 0u || (c & 0xFFu) != PAD_MAP;  // count cells outside the map keep their old contents
                        }
                    }
                    if (keep[0] & keep[1] & keep[2] & keep[3]) {
                        const v4f v = {val[0], val[1], val[2], val[3]};
                        __builtin_nontemporal_store(v, reinterpret_cast<gv4f *>(o));
                    } else {
                        if (keep[0]) o[0] = val[0];
                        if (keep[1]) o[1] = val[1];
                        if (keep[2]) o[2] = val[2];
                        if (keep[3]) o[3] = val[3];
                    }
                } else {
                    const int i = f / R, j = f - i * R;
                    const uint32_t c = cell[base + i * GW + j];
                    const float v0 = s_vtab[c & 0xFFu];
                    if ((c & 0xFFu) == PAD_MAP) {
                        o[0] = v0;   // outside the map: the fill value in channel 0, the counts keep their old contents
                    } else {
                        const float v1 = s_vtab[(c >> 8) & 0xFFu], v2 = s_vtab[(c >> 16) & 0xFFu];
                        if (f == S::CENTRE) {
                            const v4f v = {v0, v1, v2, (float)((double)p / (double)P)};  // :440-445
                            __builtin_nontemporal_store(v, reinterpret_cast<gv4f *>(o));
                        } else if (ch3_zero) {
                            const v4f v = {v0, v1, v2, 0.0f};
                            __builtin_nontemporal_store(v, reinterpret_cast<gv4f *>(o));
                        } else {   // channel 3 off the centre is never written (:440-441)
                            o[0] = v0;
                            o[1] = v1;
                            o[2] = v2;
                        }
                    }
                }
                f += df; p += dp;
                if (f >= DV) { f -= DV; ++p; }
            }
        };

        // the placed agents leave the cells: counts first, then (behind a barrier: a count that left its byte may have carried into the
        // credit bit) the credit of the evaders caught in this step
        auto undo = [&]() {
            group_sync();  // the row pass has read the cells
            for (int a = tid; a < A; a += NT) {
                const int idx = (s_ax[a] + PAD) * GW + s_ay[a] + PAD;
                if (a < P) atomicSub(&cell[idx], 1u << 8);
                else if ((s_placed[(a - P) >> 5] >> ((a - P) & 31)) & 1u) atomicSub(&cell[idx], 1u << 16);
            }
            group_sync();
            for (int i = tid; i < E; i += NT) {
                if (!((s_placed[i >> 5] & s_gone[i >> 5]) >> (i & 31) & 1u)) continue;
                const int c0 = (s_ax[P + i] + PAD) * GW + s_ay[P + i] + PAD;
                atomicAnd(&cell[c0], 0x00FFFFFFu);
                atomicAnd(&cell[c0 - GW], 0x00FFFFFFu);
                atomicAnd(&cell[c0 + GW], 0x00FFFFFFu);
                atomicAnd(&cell[c0 + 1], 0x00FFFFFFu);
                atomicAnd(&cell[c0 - 1], 0x00FFFFFFu);
            }
        };

        if constexpr (MODE == 1) {
            load_map(map_id);
            group_sync();
            // -------------------------------------------------------- pre-move evader counts (:364-365)
            for (int i = tid; i < E; i += NT) {
                if (!((s_gone[i >> 5] >> (i & 31)) & 1u)) cell_add(cell, (s_ax[P + i] + PAD) * GW + s_ay[P + i] + PAD, 16u, &s_misc[3]);
            }
            group_sync();
            // proximity reward on the PRE-move state, np.clip keeps border pursuers on their own cell (:374-380)
            for (int p = tid; p < P; p += NT) {
                const int x = s_ax[p], y = s_ay[p];
                const int xm = max(x - 1, 0), xp = min(x + 1, S::XS - 1);
                const int ym = max(y - 1, 0), yp = min(y + 1, S::YS - 1);
                s_kpre[p] = (int)((cell[(xm + PAD) * GW + y + PAD] >> 16) & 0xFFu) + (int)((cell[(xp + PAD) * GW + y + PAD] >> 16) & 0xFFu) +
                            (int)((cell[(x + PAD) * GW + yp + PAD] >> 16) & 0xFFu) + (int)((cell[(x + PAD) * GW + ym + PAD] >> 16) & 0xFFu);
            }
            group_sync();
            // -------------------------------------------------------- moves (:229-241)
            for (int a = tid; a < A; a += NT) {
                const bool is_p = a < P;
                const int i = a - P;
                if (!is_p && ((s_gone[i >> 5] >> (i & 31)) & 1u)) continue;
                int x = s_ax[a], y = s_ay[a];
                int act;
                if (is_p) {
                    act = io.actions[env * P + a];
                } else {
                    atomicSub(&cell[(x + PAD) * GW + y + PAD], 1u << 16);  // undo the pre-move count
                    int k = 0;  // index in the evader LAYER = alive evaders in slots below i
                    for (int w = 0; w < (i >> 5); ++w) k += 32 - __popc(s_gone[w]);
                    k += (i & 31) - __popc(s_gone[i >> 5] & ((1u << (i & 31)) - 1u));
                    if (io.inj_eact != nullptr) {
                        act = io.inj_eact[env * E + k];
                    } else {
                        const u32x4 r = philox4x32_10(gid, tick, (uint32_t)k, TAG_EVADER_ACT, d.k0, d.k1);
                        act = (int)__umulhi(r.x, 5u);  // RandomPolicy.act, Controllers.py:15-16
                    }
                }
                // DiscreteAgent.step, DiscreteAgent.py:69-97
                const bool term = (s_term[a >> 5] >> (a & 31)) & 1u;
                if (!term) {
                    if ((cell[(x + PAD) * GW + y + PAD] & 0xFFu) == 1u) {
                        atomicOr(&s_term[a >> 5], 1u << (a & 31));  // standing in a building
                    } else {
                        int nx = x, ny = y;
                        if (act == 0) nx = x - 1;
                        else if (act == 1) nx = x + 1;
                        else if (act == 2) ny = y + 1;
                        else if (act == 3) ny = y - 1;
                        if ((cell[(nx + PAD) * GW + ny + PAD] & 0xFFu) == 0u) {  // 0 = free, 1 = building, 0xFE = outside the map
                            x = nx;
                            y = ny;
                        }
                    }
                }
                s_ax[a] = (uint8_t)x;
                s_ay[a] = (uint8_t)y;
                if (is_p) s_base[a] = (x - OFF + PAD) * GW + (y - OFF + PAD);
                cell_add(cell, (x + PAD) * GW + y + PAD, is_p ? 8u : 16u, &s_misc[3]);  // :244-246
            }
            group_sync();
            // -------------------------------------------------------- catch resolution (:463-521)
            const uint8_t *need_tab = d.maps + (int64_t)map_id * d.map_stride + GSZ;
            for (int i = tid; i < E; i += NT) {
                if ((s_gone[i >> 5] >> (i & 31)) & 1u) continue;
                const int x = s_ax[P + i], y = s_ay[P + i];
                const int c0 = (x + PAD) * GW + y + PAD;
                bool caught;
                // a neighbour holds pursuers: its count byte is 1 .. 254 (cells outside the map never hold any)
                auto hit = [&](int c) { return (uint8_t)(((cell[c] >> 8) & 0xFFu) - 1u) < 0xFEu; };
                if (d.surround) {
                    const bool h0 = hit(c0 - GW), h1 = hit(c0 + GW), h2 = hit(c0 + 1), h3 = hit(c0 - 1);  // neighbour order of surround_mask (:150)
                    const int cnt = (int)h0 + (int)h1 + (int)h2 + (int)h3;
                    caught = (cnt == (int)need_tab[x * S::YS + y]);  // need_to_surround :523-540
                    if (caught) {  // pursuers standing on a matched neighbour get credit (:489-495)
                        if (h0) atomicOr(&cell[c0 - GW], 1u << 24);
                        if (h1) atomicOr(&cell[c0 + GW], 1u << 24);
                        if (h2) atomicOr(&cell[c0 + 1], 1u << 24);
                        if (h3) atomicOr(&cell[c0 - 1], 1u << 24);
                    }
                } else {
                    caught = (int)((cell[c0] >> 8) & 0xFFu) >= d.n_catch;  // :498
                    if (caught) atomicOr(&cell[c0], 1u << 24);             // :503-506
                }
                if (caught) {
                    atomicOr(&s_gone[i >> 5], 1u << (i & 31));
                    atomicAdd(&s_misc[4], 1u);
                }
            }
            group_sync();
            // -------------------------------------------------------- rewards (:254-262)
            int n_alive = E;
            for (int w = 0; w < NGW; ++w) n_alive -= __popc(s_gone[w]);
            const double catchr = d.catchr_env ? d.catchr_env[env] : d.catchr;
            for (int p = tid; p < P; p += NT) {
                const uint32_t sur = (cell[(s_ax[p] + PAD) * GW + s_ay[p] + PAD] >> 24) & 1u;
                double r = catchr * (double)s_kpre[p];
                r += d.term_pursuit * (sur ? 1.0 : 0.0);
                r += d.urgency;
                if (d.reward_global) s_rew[p] = r;
                else io.rew[env * P + p] = (float)r;
            }
            if (d.reward_global) {
                group_sync();
                if (tid < P) {
                    const double m = np_sum<P>(s_rew) / (double)P;
                    for (int p = tid; p < P; p += NT) io.rew[env * P + p] = (float)m;
                }
            }
            tick += 1;
            tstep += 1;
            if (n_alive == 0) done_bits |= 1u;                               // :383-389
            if (d.max_steps > 0 && tstep >= d.max_steps) done_bits |= 2u;
            const uint32_t overflow = s_misc[3] ? 0x80u : 0u;                // a cell's count left the byte range: results void
            if (tid == 0) {
                io.done[env] = (uint8_t)(done_bits | overflow);
                io.removed[env] = (int32_t)s_misc[4];
                d.flags[env] = done_flag_word(done_bits | overflow);
            }
            do_reset = d.auto_reset && done_bits != 0;
        }
        // a step: the rows of the step; with auto-reset the reference sequence is step() then reset(), both write the persistent observation
        // buffer, and cells the second write skips keep the first one's values.  A reset launch: the reset, then its rows.
        for (int pass = MODE == 0 ? 1 : 0;; ++pass) {
            if (pass == 1) {
                // ---------------------------------------------------------- reset (:173-207)
                group_sync();
                if (tid == 0) s_misc[3] = 0u;                         // a new episode: the overflow mark goes
                for (int w = tid; w < NGW; w += NT) s_gone[w] = 0u;   // :175-176
                for (int w = tid; w < NTW; w += NT) s_term[w] = 0u;   // fresh agents
                if (io.inj_map != nullptr && MODE == 0) {
                    map_id = io.inj_map[env];
                } else if (d.sample_maps) {  // :182-183
                    const u32x4 r = philox4x32_10(gid, tick, 0u, TAG_RESET_ENV, d.k0, d.k1);
                    map_id = (int)__umulhi(r.x, (uint32_t)d.n_maps);
                }
                load_map(map_id);
                // constraint window (:185-191), float64 like the reference
                const u32x4 rw = philox4x32_10(gid, tick, 1u, TAG_RESET_ENV, d.k0, d.k1);
                const double cw = d.cw_env ? d.cw_env[env] : d.cw;
                const double sx = u53(rw.x, rw.y) * (1.0 - cw);
                const double sy = u53(rw.z, rw.w) * (1.0 - cw);
                const int xlb = (int)(S::XS * sx), xub = (int)(S::XS * (sx + cw));
                const int ylb = (int)(S::YS * sy), yub = (int)(S::YS * (sy + cw));
                // random_opponents (:177-181): this episode has n_create <= E evaders; the slots above are not created and count as gone.
                // An injected position with x < 0 marks a slot that is not created.
                const bool inj = io.inj_pos != nullptr && MODE == 0;
                int n_create = E;
                if (d.max_opponents > 0 && !inj) {
                    const u32x4 r3 = philox4x32_10(gid, tick, 2u, TAG_RESET_ENV, d.k0, d.k1);
                    n_create = min(1 + (int)__umulhi(r3.x, (uint32_t)(d.max_opponents - 1)), E);
                }
                group_sync();
                for (int a = tid; a < A; a += NT) {  // create_agents, agent_utils.py:12-28
                    int x = 0, y = 0;
                    if (a >= P && (a - P >= n_create || (inj && io.inj_pos[(env * A + a) * 2] < 0))) {
                        atomicOr(&s_gone[(a - P) >> 5], 1u << ((a - P) & 31));
                        s_ax[a] = 0;
                        s_ay[a] = 0;
                        continue;
                    }
                    if (inj) {
                        x = io.inj_pos[(env * A + a) * 2];
                        y = io.inj_pos[(env * A + a) * 2 + 1];
                        // (an injected position is the caller's word, as in the generic kernel; only the LDS index is kept inside the grid)
                        x = min(max(x, 0), S::XS - 1);
                        y = min(max(y, 0), S::YS - 1);
                    } else {
                        // feasible_position: rejection sampling (agent_utils.py:37-47); bounded
                        for (uint32_t att = 0; att < 1024u; ++att) {
                            const u32x4 r = philox4x32_10(gid, tick, (uint32_t)a, TAG_RESET_POS | (att << 8), d.k0, d.k1);
                            x = xlb + (int)__umulhi(r.x, (uint32_t)(xub - xlb));
                            y = ylb + (int)__umulhi(r.y, (uint32_t)(yub - ylb));
                            if ((cell[(x + PAD) * GW + y + PAD] & 0xFFu) != 1u) break;
                        }
                    }
                    s_ax[a] = (uint8_t)x;
                    s_ay[a] = (uint8_t)y;
                    if (a < P) s_base[a] = (x - OFF + PAD) * GW + (y - OFF + PAD);
                    cell_add(cell, (x + PAD) * GW + y + PAD, a < P ? 8u : 16u, &s_misc[3]);  // :201-203
                }
                tick += 1;
                tstep = 0;
                group_sync();
                for (int w = tid; w < NGW; w += NT) s_placed[w] = ~s_gone[w];
                group_sync();
            }
            write_obs();   // (a step: the barrier after the catches published everything the rows read)
            if (pass == 1 || !do_reset) break;
            undo();
        }
        // -------------------------------------------------------------- store state record
        for (int a = tid; a < A; a += NT)
            reinterpret_cast<uint16_t *>(rec + HDR_BYTES)[a] = (uint16_t)(s_ax[a] | (s_ay[a] << 8));
        for (int w = tid; w < NGW; w += NT) reinterpret_cast<uint32_t *>(rec + S::OFF_GONE)[w] = s_gone[w];
        for (int w = tid; w < NTW; w += NT) reinterpret_cast<uint32_t *>(rec + S::OFF_TERM)[w] = s_term[w];
        if (tid == 0) {
            uint32_t *h = reinterpret_cast<uint32_t *>(rec);
            h[0] = tick;
            h[1] = (uint32_t)tstep;
            h[2] = (uint32_t)map_id;
            h[3] = s_misc[3];   // sticky count-overflow mark of the episode
        }
        undo();
    }
}

// host side: launches the instantiation of shape S (defined and instantiated for every XC line in pursuit_crowd.hip)
template <class S>
void crowd_launch(const CrowdDev &d, const CrowdIO &io, int mode, int64_t blocks, hipStream_t s);

}  // namespace pc
}  // namespace madrl
