// waterworld.hip -- batched MAWaterWorld for MI355X (gfx950 / CDNA4), float32.
//
// One wavefront owns one env at a time (64-thread workgroups, persistent, striding over
// envs).  The env's particles (pursuers | evaders | poisons: position + velocity), the
// obstacle and the assembled observation rows live in LDS; HBM sees one packed state record
// in / out, the action row in and observation / reward / done / info rows out.
//
// Lane roles change per phase:
//   particle phases   lane j < NP owns particle j (integration, walls, obstacle rebound,
//                     respawn, evader/poison motion);
//   collision phase   lane = (pursuer, evader) / (pursuer, poison) pair;
//   sensing phase     lane = (pursuer, sensor) pair, three passes of 64 pairs held in registers; the objects are
//                     broadcast once each from the owning lane's registers (v_readlane -> SGPR operands) and a
//                     conservative reach mask skips, per pass, the objects none of its pursuers can sense --
//                     the only O(Np*K*N) part (~4k ray tests before the cull).
// No dense contraction -> no MFMA.  ~40 kFLOP and 5.2 KB of HBM traffic per env-step: the
// kernel is VALU-issue bound, not HBM bound.
//
// Reference semantics (file:line under /root/reference/madrl_environments/pursuit/waterworld.py):
//   step phases ........ MAWaterWorld.step :220-436      sensing ...... Archea.sensed :64-72
//   catch rule ......... _caught :180-193                 respawn ...... _respawn :139-142, :355-374
//   reset .............. :144-172 (ends with a zero-action step, W11)
// The device code this kernel has in common with hostage_kernel (hostage.hip) -- the record pipeline, the action and control penalty, the
// generic path's collision bytes, the sensing passes, reach masks, ray test and bit walks, the fused StandardizedEnv epilogue -- is in
// particle_wave.hpp; this file is Waterworld's step in the reference's order and what is its own: the reset draws, the obstacle, the
// ballot form of the collision matrices (BITROWS), the row tail, rewards, respawn and done.
// Envs beyond a wavefront's worth of particles (more than 62, or more than 32 pursuers) run on ww_crowd_kernel (waterworld_crowd.hip) when
// the handle was created with cfg.crowd = 1; the handle, validation, record layout and dispatch of both kernels are in this file.
// Arithmetic is float32 (north_star tolerance 1e-5 against the float64 reference); every
// expression keeps the statement order of the reference's step() so that a float32 CPU restatement agrees bit for bit.
#include "waterworld_dev.hpp"   // WwDev, WwIO, the RNG tags: shared with waterworld_crowd.hip
#include "particle_wave.hpp"    // the device code this kernel shares with hostage_kernel (hostage.hip)

#include <math.h>
#include <string.h>

namespace {

using namespace madrl;

// The launch parameters as read from the kernel-argument segment (kernargs(), common.hpp) at the phase that needs them.
struct WwKArgs {
    WwDev d;
    WwIO io;
};

// Profiling aid (scripts/variants.sh, never the shipped library): 1 no sensing loop, 2 no observation store, 4 no collisions
#ifndef MADRL_WW_ABLATE
#define MADRL_WW_ABLATE 0
#endif

// Resident wavefronts per SIMD the SPECIALISED kernel's registers are allocated for (the generic one is left to the compiler).
// Measured at BASELINE C3, 32 768 envs: 4 waves (104 VGPRs) 77 us, 5 waves (86) 60.4 us, 6 waves (80, no scratch) 57.2 us, 7 waves
// (72 + 32 B of scratch) 57.4 us.
#ifndef MADRL_WW_WAVES
#define MADRL_WW_WAVES 6
#endif
// (the fused-wrapper variant holds float64 statistics: one wave fewer, or it spills)
#define MADRL_WW_OCC_N (TNp > 0 ? (FUSED ? MADRL_WW_WAVES - 1 : MADRL_WW_WAVES) - (TNp > 6 ? 1 : 0) : 0)  // (> 6 pursuers: two words per collision matrix, more live pass state)
#define MADRL_WW_OCC __attribute__((amdgpu_waves_per_eu(MADRL_WW_OCC_N > 0 ? MADRL_WW_OCC_N : 1, MADRL_WW_OCC_N > 0 ? MADRL_WW_OCC_N : 8)))

// MODE 0: reset(mask)   MODE 1: step (+ fused auto-reset)
// TNp..TK > 0: the particle / sensor counts are compile-time constants (loops unroll, the index divisions fold); 0: generic.
// FUSED: the StandardizedEnv epilogue (ParticleStd, common.hpp) is compiled in; a template parameter because its float64 code would otherwise cost the
// plain kernel a wavefront per SIMD (132 instead of 119 VGPRs: 96 instead of 78 us per step)
template <int MODE, int TNp, int TNe, int TNpo, int TK, bool FUSED = false, int TD = 0>
__global__ __launch_bounds__(64) MADRL_WW_OCC void waterworld_kernel(const WwDev d, const WwIO io) {
    // The specialised shape has a compile-time LDS layout in a STATIC array (launched with 0 dynamic bytes): every LDS address is
    // "lane-dependent register + immediate offset".  With the dynamic array the base is a link-time symbol the compiler adds in
    // registers, hoists out of the env loop per access pattern and -- at 5 waves per SIMD -- spills.
    constexpr int SPEC_BYTES = TNp > 0 ? (int)wave_lds_bytes(4 * (TNp + TNe + TNpo) + 4, TNp, TD, TK, TNe, TNpo) : 16;
    static_assert(TNp == 0 || TD > 0, "a specialised shape fixes the observation width too");
    extern __shared__ __attribute__((aligned(16))) float smem_dyn[];
    __shared__ __attribute__((aligned(16))) float smem_static[SPEC_BYTES / 4];
    float *const smem = TNp > 0 ? smem_static : smem_dyn;
    const int lane = threadIdx.x;
    const uint32_t ulane = threadIdx.x;
#define DA (kernargs<WwKArgs>()->d)
#define IOA (kernargs<WwKArgs>()->io)
    static_assert(TNp == 0 || TNp + TNe + TNpo + 1 <= 64, "lane predicates of a specialised shape compare against inline constants");
#define LANE_LT(n) (TNp > 0 ? lane_lt_imm(lane, (n)) : (fresh(lane) < (n)))
#define LANE_EQ(n) (TNp > 0 ? lane_eq_imm(lane, (n)) : (fresh(lane) == (n)))
    const int Np = TNp > 0 ? TNp : d.Np, Ne = TNp > 0 ? TNe : d.Ne, Npo = TNp > 0 ? TNpo : d.Npo, K = TNp > 0 ? TK : d.K;
    const int NP = Np + Ne + Npo, D = TD > 0 ? TD : d.D;  // TD: the observation width of the specialised shape (7 K + 3)
    // ---- LDS carve
    float *S = smem;                                    // packed record: X[NP][2] | V[NP][2] | obst[2] | t | tick
    float *X = S, *V = S + 2 * NP;
    float *OB = S + 4 * NP;
    float *O = S + (((TNp > 0 ? 4 * (TNp + TNe + TNpo) + 4 : d.rec_dw) + 3) & ~3);  // observation staging [Np][D]
    float *const O_SPARE = O + Np * D;                  // one more row: where the sensing lanes without a (pursuer, sensor) pair write
    float *SEN = O + (((Np + 1) * D + 3) & ~3);         // sensor unit vectors [K][2]
    uint64_t *NEAR = reinterpret_cast<uint64_t *>(SEN + ((2 * K + 3) & ~3));  // per pursuer: particles (bit j) / obstacle (bit NP) in sensing reach
    uint8_t *COL = reinterpret_cast<uint8_t *>(NEAR + Np);  // col_ev[Np][Ne] | col_po[Np][Npo]
    uint8_t *COLP = COL + Np * Ne;
    uint8_t *FLG = COLP + Np * Npo;                     // caught_ev[Ne] | enc_ev[Ne] | caught_po[Npo]

    for (int k = lane; k < 2 * K; k += 64) SEN[k] = d.sensors[k];
    const int rec_dw = TNp > 0 ? (4 * (TNp + TNe + TNpo) + 4 + 3) / 4 * 4 : d.rec_dw;  // <= 4 dwords per lane (NP <= 62)

    // ---- software pipeline: next env's record + action row are fetched one env ahead
    WaveRecord cur;
    const int n_envs = (int)d.n_envs;
    if ((int)blockIdx.x < n_envs) cur.fetch<MODE, WwKArgs>(blockIdx.x, rec_dw, Np, lane, ulane);
    cur.hinge();
    wave_sync();

    for (int e32 = blockIdx.x; e32 < n_envs; e32 += (int)gridDim.x) {  // env indices are 32-bit (n_envs < 2^31 - grid), byte offsets 64-bit
        const int64_t env = e32;
        const int n32 = e32 + (int)gridDim.x;
        WaveRecord nxt;
        if (n32 < n_envs) nxt.fetch<MODE, WwKArgs>(n32, rec_dw, Np, lane, ulane);
        bool skip = false;
        if constexpr (MODE == 0) skip = (IOA.mask != nullptr && IOA.mask[env] == 0);
        if (!skip) {
            cur.to_lds(reinterpret_cast<uint32_t *>(S), rec_dw, lane);
            wave_sync();
            int32_t tstep = reinterpret_cast<int32_t *>(S)[4 * NP + 2];
            uint32_t tick = reinterpret_cast<uint32_t *>(S)[4 * NP + 3];
            const uint32_t gid = DA.gid_base + (uint32_t)env;
            float act_lane = cur.act;  // lane 2i / 2i+1 hold pursuer i's action components

            bool do_init = (MODE == 0);
            int npass = 1;
            for (int pass = 0; pass < npass; ++pass) {
                if (do_init) {
                    // ------------------------------------------------ reset (:144-172)
                    tstep = 0;
                    if (fresh(lane) == 0) {
                        float ox = DA.obst_x, oy = DA.obst_y;
                        if (!DA.obstacle_fixed) {  // :147-148
                            const u32x4 r = philox4x32_10(gid, tick, 0u, WW_TAG_OBSTACLE, DA.k0, DA.k1);
                            ox = u24(r.x);
                            oy = u24(r.y);
                        }
                        OB[0] = ox;
                        OB[1] = oy;
                    }
                    wave_sync();
                    if (fresh(lane) < NP) {  // :153-170 each particle: uniform position, redrawn while too close to the obstacle
                        const float pr = fresh(lane) < Np ? DA.r_pu : (fresh(lane) < Np + Ne ? DA.r_ev : DA.r_po);
                        const float thr = pr * 2.0f + DA.obst_r;
                        const float ox = OB[0], oy = OB[1];
                        float x = 0.f, y = 0.f, u0 = 0.f, u1 = 0.f;
                        for (uint32_t att = 0; att < 1024u; ++att) {
                            const u32x4 r = philox4x32_10(gid, tick, (uint32_t)lane, WW_TAG_RESET | (att << 8), DA.k0, DA.k1);
                            x = u24(r.x);
                            y = u24(r.y);
                            if (att == 0) { u0 = u24(r.z); u1 = u24(r.w); }
                            if (!(dist2d(x, y, ox, oy) <= thr)) break;
                        }
                        X[2 * lane] = x;
                        X[2 * lane + 1] = y;
                        V[2 * lane] = LANE_LT(Np) ? 0.0f : (u0 - 0.5f) * DA.ev_speed;      // :164, :170 (W9)
                        V[2 * lane + 1] = LANE_LT(Np) ? 0.0f : (u1 - 0.5f) * DA.ev_speed;
                    }
                    tick += 1;
                    act_lane = 0.0f;  // reset ends with step(zeros) (:172, W11)
                    wave_sync();
                }
                // ---------------------------------------------------- step (:220-436)
                const float ox = OB[0], oy = OB[1];
                // phase A: particles
                float reward = 0.0f;
                {
                    float a0, a1;  // :224; the penalty: :233-237, under the global reward (actions**2).sum() row-major (:234-235, W12)
                    const float pen_local = agent_action<WwKArgs>(act_lane, [&]() { return LANE_LT(Np) ? lane : 0; }, Np, a0, a1);
                    if (LANE_LT(NP)) {
                        float x = X[2 * lane], y = X[2 * lane + 1], vx = V[2 * lane], vy = V[2 * lane + 1];
                        float sq_obst = DA.sq_obst_po, f = -1.0f;
                        if (LANE_LT(Np)) {
                            integrate_agent(a0, a1, x, y, vx, vy);  // :229-231, walls :239-245
                            reward = 0.0f + pen_local;   // :233-237
                            sq_obst = DA.sq_obst_pu; f = -0.5f;
                        } else if (LANE_LT(Np + Ne)) {
                            sq_obst = DA.sq_obst_ev; f = -0.5f;
                        }
                        if (dist2_le(x, y, ox, oy, sq_obst)) {  // dist <= pr + obst_r, :247-270 (W1, W2)
                            vx = f * vx;
                            vy = f * vy;
                        }
                        X[2 * lane] = x; X[2 * lane + 1] = y; V[2 * lane] = vx; V[2 * lane + 1] = vy;
                    }
                }
                wave_sync();
                // phase B: collisions (:272-293)
                // BITROWS (specialised shapes): a collision matrix is a few wave-uniform 64-bit masks (bit r * n + m of word w = pursuer
                // w * G + r touches particle m) made by ballots; columns are counted and rows tested with bit operations.  No byte
                // matrices in LDS, no loop over the other side of the pair.
                // A 64-bit word holds GE = floor(64 / Ne) whole rows; shapes with more pursuers use up to 4 words per matrix.
                constexpr int GE = (TNe > 0 && TNe < 64) ? 64 / TNe : 1, GP = (TNpo > 0 && TNpo < 64) ? 64 / TNpo : 1;  // rows per word
                constexpr int WE = TNp > 0 ? (TNp + GE - 1) / GE : 1, WP = TNp > 0 ? (TNp + GP - 1) / GP : 1;              // words per matrix
                constexpr bool BITROWS = TNp > 0 && TNe < 64 && TNpo < 64 && WE <= 4 && WP <= 4;
                uint64_t col_ev[WE], col_po[WP];
#pragma unroll
                for (int w = 0; w < WE; ++w) col_ev[w] = 0ull;
#pragma unroll
                for (int w = 0; w < WP; ++w) col_po[w] = 0ull;
                bool my_caught = false, my_enc = false;
                if constexpr (BITROWS) {
#pragma unroll
                    for (int w = 0; w < WE; ++w) {
                        const int li = lane / Ne, i0 = w * GE + li;
                        const bool in = LANE_LT(GE * Ne) && i0 < Np;
                        const int i = in ? i0 : 0, m = in ? lane - li * Ne : 0, j = Np + m;
                        col_ev[w] = __ballot(in && dist2_le(X[2 * i], X[2 * i + 1], X[2 * j], X[2 * j + 1], DA.sq_hit_ev));
                    }
#pragma unroll
                    for (int w = 0; w < WP; ++w) {
                        const int li = lane / Npo, i0 = w * GP + li;
                        const bool in = LANE_LT(GP * Npo) && i0 < Np;
                        const int i = in ? i0 : 0, m = in ? lane - li * Npo : 0, j = Np + Ne + m;
                        col_po[w] = __ballot(in && dist2_le(X[2 * i], X[2 * i + 1], X[2 * j], X[2 * j + 1], DA.sq_hit_po));
                    }
#if MADRL_WW_ABLATE & 4
                    for (int w = 0; w < WE; ++w) col_ev[w] = 0ull;
                    for (int w = 0; w < WP; ++w) col_po[w] = 0ull;
#endif
                    // _caught (:180-193): evader lanes / poison lanes count their column
                    uint64_t cm_ev = 0ull, cm_po = 0ull;  // bit r * n of every row of a word
#pragma unroll
                    for (int r = 0; r < GE; ++r) cm_ev |= 1ull << (r * Ne);
#pragma unroll
                    for (int r = 0; r < GP; ++r) cm_po |= 1ull << (r * Npo);
                    if ((!LANE_LT(Np) && LANE_LT(NP))) {
                        const bool is_ev = LANE_LT(Np + Ne);
                        const int m = is_ev ? lane - Np : lane - Np - Ne;
                        int sc = 0;
                        if (is_ev) {
#pragma unroll
                            for (int w = 0; w < WE; ++w) sc += __popcll(col_ev[w] & (cm_ev << m));
                        } else {
#pragma unroll
                            for (int w = 0; w < WP; ++w) sc += __popcll(col_po[w] & (cm_po << m));
                        }
                        my_caught = sc >= (is_ev ? DA.n_coop : 1);
                        my_enc = is_ev && sc >= 1;
                    }
                } else {
#if MADRL_WW_ABLATE & 4
                if (DA.n_envs < 0)
#endif
                contact_bytes(X, COL, Np, Ne, Npo, lane, [&](bool is_ev) { return is_ev ? DA.sq_hit_ev : DA.sq_hit_po; });
                wave_sync();
                // _caught (:180-193): evader lanes / poison lanes count their column
                if ((!LANE_LT(Np) && LANE_LT(NP))) {
                    const bool is_ev = LANE_LT(Np + Ne);
                    const int m = is_ev ? lane - Np : lane - Np - Ne;
                    const int s = column_count(is_ev ? COL : COLP, Np, is_ev ? Ne : Npo, m);
                    my_caught = s >= (is_ev ? DA.n_coop : 1);
                    my_enc = is_ev && s >= 1;
                    column_flags(FLG, is_ev, Ne, m, my_caught, my_enc);
                }
                }
                const uint64_t ev_lanes = low_bits64(Ne) << Np;
                const uint64_t caught_mask = __ballot(my_caught);
                const uint64_t enc_mask = __ballot(my_enc);
                const int n_evc = __popcll(caught_mask & ev_lanes);
                const int n_poc = __popcll(caught_mask & ~ev_lanes);
                const int n_enc = __popcll(enc_mask);
                wave_sync();
                // phase C: sensing (:295-353).  lane = (pursuer i, sensor k)
                const float srange = DA.sensor_range, rad2 = DA.r_pu * DA.r_pu;  // W3
                // The (pursuer, sensor) pairs are spread over the lanes, PCH passes of 64 at a time; the objects they are tested
                // against are wave-uniform, so each object's position is broadcast ONCE from the register of the lane that
                // owns the particle (v_readlane -> SGPR operand) and reused by all passes: the inner loop is pure VALU, no
                // LDS round trip per (pair, object).  Arithmetic and comparison order per pair are those of the reference loop.
                // passes of 64 (pursuer, sensor) pairs held in registers at a time (sense_pass: the lane layout of a pass)
                const int n_pass = sense_n_pass<TK>(Np, K);
                constexpr int N_PASS_T = TNp > 0 ? sense_n_pass<TK>(TNp, TK) : 3;
                const float part_x = LANE_LT(NP) ? X[2 * lane] : 0.f, part_y = LANE_LT(NP) ? X[2 * lane + 1] : 0.f;
                // Conservative cull: NEAR[i] marks the objects within pursuer i's sensing reach (the obstacle: bit NP); everything else
                // would yield INFINITY for every sensor of the pursuer and is skipped per pass.
                {
                    const float thr2 = sensor_reach2(rad2, srange);
                    const float mx = LANE_EQ(NP) ? ox : part_x, my = LANE_EQ(NP) ? oy : part_y;
                    reach_cull(NEAR, Np, part_x, part_y, mx, my, thr2, [&]() { return LANE_LT(NP + 1); }, [&]() { return LANE_EQ(0); });
                    wave_sync();
                }
#if MADRL_WW_ABLATE & 1
                if (DA.n_envs < 0)
#endif
                // ONE PASS AT A TIME (round 6).  A pass walks the set bits of ITS OWN reach mask, class by class -- ascending = the reference's
                // index order: the first minimum wins as in np.argmin.  Round 5 held three passes in registers, walked the union of their
                // masks once and tested per object which of the passes it concerns: 17 scalar instructions per object (loop control +
                // three test-and-skip branches) on the CU's single scalar pipe, the resource this kernel is bound by.  Per (object, pass)
                // visit the walk now costs 6 (32-bit class masks where a class has at most 32 members), nothing is tested and skipped, and
                // one pass's lane constants and ONE running minimum are all that is live in the object loop.
#pragma unroll
                for (int pass_q = 0; pass_q < (TNp > 0 ? N_PASS_T : n_pass); ++pass_q) {
                    const SensePass sp = sense_pass<TK>(pass_q, Np, K, lane);  // the pursuers of this pass, this lane's (pursuer, sensor)
                    const bool okq = sp.okq;
                    const int iq = sp.iq, kq = sp.kq;
                    const float sxq = SEN[2 * kq], syq = SEN[2 * kq + 1];
                    const float pxq = X[2 * iq], pyq = X[2 * iq + 1];
                    const uint64_t reach = pass_reach(NEAR, sp.i_first, sp.i_last);  // wave-uniform: objects in reach of any pursuer of this pass
                    // (a specialised shape fixes the row width, and with it whether the speed features are in the row: 7 K + 2 (+ 1) against 4 K + 2 (+ 1))
                    const bool speed = TNp > 0 ? (TD >= 7 * TK + 2) : (bool)DA.speed_features;
                    // lanes without a (pursuer, sensor) pair -- 4 of 64 in a pass of two pursuers, 34 in the last pass of C3 -- write their features
                    // to a spare row behind the staging rows instead of branching around the stores (an exec-mask round trip per (pass, class))
                    float *const orow_l = okq ? O + iq * D : O_SPARE;
#pragma unroll
                    for (int cls = 0; cls < 4; ++cls) {
                        const int lo = cls == 0 ? NP : (cls == 1 ? Np : (cls == 2 ? Np + Ne : 0));
                        const int cnt = cls == 0 ? 1 : (cls == 1 ? Ne : (cls == 2 ? Npo : Np));
                        float b = INFINITY;
                        int bi = 0;
                        auto visit = [&](int m, float qx, float qy) {
                            // branch-free (bitwise |, selects): no exec-mask round trips in the inner loop; a pursuer does not sense itself
                            float sv;
                            const bool out = ray_misses(sxq, syq, pxq, pyq, qx, qy, srange, rad2, sv) | ((cls == 3) & (m == iq));
                            // (the reference sets an excluded ray to +inf and takes the first minimum: an excluded ray is never "better", a kept one
                            // is when it is smaller -- the same minimum and the same first index without materialising the +inf)
                            const bool better = !out & (sv < b);
                            b = better ? sv : b;
                            bi = better ? m : bi;
                        };
                        if (cls == 0) {
                            if ((reach >> NP) & 1ull) visit(0, ox, oy);
                        } else if (TNp > 0 && cnt <= 32) {
                            walk_bits((uint32_t)(reach >> lo) & low_bits32(cnt), [&](int m) {
                                // the object's position: ONE uniform-address LDS read (a broadcast) instead of two v_readlane + their wait states --
                                // the LDS pipe has room, the VALU port is what this kernel is bound by since the scalar work went
                                const float2 qp = *reinterpret_cast<const float2 *>(&X[2 * (lo + m)]);
                                visit(m, qp.x, qp.y);
                            });
                        } else {
                            walk_bits(reach & (low_bits64(cnt) << lo), [&](int bit) {
                                visit(bit - lo, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(part_x), bit)),
                                      __int_as_float(__builtin_amdgcn_readlane(__float_as_int(part_y), bit)));
                            });
                        }
                        // the features of (pass, class) go to the staging row now: nothing but ONE running minimum is held in registers
                        {
                            float *o = orow_l;
                            const bool fin = b < INFINITY;
                            const float fd = fin ? b : 0.f;  // W4: raw distance or 0
                            if (cls == 0) {
                                o[kq] = fd;
                            } else {
                                const int j = lo + bi;   // (bi = 0 without a hit: a valid particle, its value is not used)
                                const float raw = speed_along(V, sxq, syq, j, iq);   // loaded and computed unconditionally: a select, no branch
                                const float fs = fin ? raw : 0.f;  // W5
                                if (speed) { o[(2 * cls - 1) * K + kq] = fd; o[2 * cls * K + kq] = fs; }
                                else o[cls * K + kq] = fd;
                            }
                        }
                    }
                }
                // pursuer lanes: collision flags, id, who-caught tests for the local rewards
                bool wc = false, wp = false, we = false;
                if (LANE_LT(Np)) {
                    bool tev = false, tpo = false;
                    if constexpr (BITROWS) {
                        uint64_t we_ = col_ev[0], wp_ = col_po[0];  // the word that holds this pursuer's row
#pragma unroll
                        for (int w = 1; w < WE; ++w) we_ = (lane / GE == w) ? col_ev[w] : we_;
#pragma unroll
                        for (int w = 1; w < WP; ++w) wp_ = (lane / GP == w) ? col_po[w] : wp_;
                        const uint64_t row_ev = (we_ >> ((lane % GE) * Ne)) & ((1ull << Ne) - 1ull);
                        const uint64_t row_po = (wp_ >> ((lane % GP) * Npo)) & ((1ull << Npo) - 1ull);
                        tev = row_ev != 0ull;
                        tpo = row_po != 0ull;
                        wc = (row_ev & (caught_mask >> Np)) != 0ull;           // touches a caught evader
                        we = (row_ev & (enc_mask >> Np)) != 0ull;              // touches an encountered evader
                        wp = (row_po & (caught_mask >> (Np + Ne))) != 0ull;    // touches a caught poison
                    } else {
                        agent_contacts(COL, COLP, FLG, lane, Ne, Npo, tev, wc, we, tpo, wp);
                    }
                    float *o = O + lane * D + DA.nfeat * K;  // :411-428
                    o[0] = tev ? 1.f : 0.f;
                    o[1] = tpo ? 1.f : 0.f;
                    if (DA.addid) o[2] = (float)(lane + 1);  // W10
                }
                wave_sync();
                // phase E: respawn caught evaders / poisons (:355-374)
                if ((!LANE_LT(Np) && LANE_LT(NP)) && my_caught) {
                    const bool is_ev = LANE_LT(Np + Ne);
                    float x, y, u0, u1;
                    if (MODE == 1 && IOA.inj_resp != nullptr && !do_init) {
                        const float *r = IOA.inj_resp + (env * NP + lane) * 4;
                        x = r[0]; y = r[1]; u0 = r[2]; u1 = r[3];
                    } else {
                        const float thr = (is_ev ? DA.r_ev : DA.r_po) * 2.0f + DA.obst_r;
                        x = y = u0 = u1 = 0.f;
                        for (uint32_t att = 0; att < 1024u; ++att) {
                            const u32x4 r = philox4x32_10(gid, tick, (uint32_t)lane, WW_TAG_RESPAWN | (att << 8), DA.k0, DA.k1);
                            x = u24(r.x);
                            y = u24(r.y);
                            if (att == 0) { u0 = u24(r.z); u1 = u24(r.w); }
                            if (!(dist2d(x, y, ox, oy) <= thr)) break;
                        }
                    }
                    const float sp = is_ev ? DA.ev_speed : DA.poison_speed;  // W9
                    X[2 * lane] = x; X[2 * lane + 1] = y;
                    V[2 * lane] = (u0 - 0.5f) * sp;
                    V[2 * lane + 1] = (u1 - 0.5f) * sp;
                }
                tick += 1;
                // phase F: rewards (:376-385)
                if (LANE_LT(Np)) {
                    if (DA.reward_global) {
                        reward += ((float)n_evc * DA.food_reward) + ((float)n_poc * DA.poison_reward) +
                                  ((float)n_enc * DA.encounter_reward);
                    } else {  // fancy-index += pays a pursuer once per kind (W7)
                        if (wc) reward += DA.food_reward;
                        if (wp) reward += DA.poison_reward;
                        if (we) reward += DA.encounter_reward;
                    }
                }
                wave_sync();
                // phase G: evaders / poisons move; velocity flips only if BOTH coordinates left [0,1] (W6)
                if ((!LANE_LT(Np) && LANE_LT(NP))) {
                    float x = X[2 * lane], y = X[2 * lane + 1], vx = V[2 * lane], vy = V[2 * lane + 1];
                    free_motion(x, y, vx, vy);
                    X[2 * lane] = x; X[2 * lane + 1] = y; V[2 * lane] = vx; V[2 * lane + 1] = vy;
                }
                tstep += 1;  // :433
                const int limit = DA.max_steps > 0 ? DA.max_steps : 1000;  // timestep_limit :124-126
                const bool is_done = tstep >= limit;                     // :174-178
                wave_sync();

                if (pass == 0) nxt.hinge();  // pipeline hinge
                // ---------------------------------------------------- outputs
                if (MODE == 1 && !do_init) {
                    if (LANE_LT(Np)) uniform_ptr(IOA.rew + env * Np)[ulane] = reward;
                    if (FUSED && IOA.st->rew_out != nullptr && LANE_LT(Np)) std_reward(*IOA.st, env * Np + lane, reward);
                    if (LANE_EQ(0)) {
                        IOA.done[env] = (uint8_t)is_done;
                        IOA.info[2 * env] = n_evc;
                        IOA.info[2 * env + 1] = n_poc;
                    }
                    if (is_done && DA.auto_reset) {  // wave-uniform: run the reset pass next
                        npass = 2;
                        do_init = true;
                    }
                }
                if (pass == npass - 1) {
                    float *const obs_p = IOA.obs;
                    const auto orow = uniform_ptr(obs_p + env * (int64_t)(Np * D));
#if MADRL_WW_ABLATE & 2
                    if (DA.n_envs < 0)
#endif
                    if (obs_p != nullptr) {  // the raw row may be dropped when the fused wrapper output is all the caller reads
                        // 16 bytes per lane (ds_read_b128 + one 16-byte store; an env's rows start on a 4-byte boundary only -- gfx950 under HSA runs
                        // global accesses in unaligned mode -- and the rows of neighbouring envs are contiguous, so whole lines leave the chip anyway)
                        typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
                        typedef float f4a __attribute__((ext_vector_type(4), aligned(16)));
                        const uint32_t n4 = (uint32_t)(Np * D) / 4u;
                        for (uint32_t e = ulane; e < n4; e += 64u)
                            *reinterpret_cast<__attribute__((address_space(1))) f4u *>(orow + 4 * e) = *reinterpret_cast<const f4a *>(O + 4 * e);
                        for (uint32_t e = 4u * n4 + ulane; e < (uint32_t)(Np * D); e += 64u) orow[e] = O[e];
                    }
                    // (hostage.hip hands the helper a copy of *IOA.st and says why; this kernel keeps the reference)
                    if (FUSED) std_obs_row(*IOA.st, O, env * (int64_t)(Np * D), Np * D, lane);
                }
                wave_sync();
            }
            // ---------------------------------------------------------- LDS -> record
            if (fresh(lane) == 0) {
                reinterpret_cast<int32_t *>(S)[4 * NP + 2] = tstep;
                reinterpret_cast<uint32_t *>(S)[4 * NP + 3] = tick;
            }
            wave_sync();
            store_record<WwKArgs>(reinterpret_cast<const uint32_t *>(S), env, rec_dw, ulane);
            wave_sync();
        }
        cur = nxt;
    }
}
#undef DA
#undef IOA
#undef LANE_LT
#undef LANE_EQ

}  // namespace
// =================================================================== host side / C ABI
struct madrl_waterworld : ParticleHandle<madrl_waterworld_config, WwDev> {};

namespace {

int ww_validate(const madrl_waterworld_config *c) {
    if (!c) return fail(MADRL_EINVAL, "config is NULL");
    if (c->struct_size != (int32_t)sizeof(madrl_waterworld_config))
        return fail(MADRL_EINVAL, "madrl_waterworld_config.struct_size=%d, library expects %d", c->struct_size,
                    (int)sizeof(madrl_waterworld_config));
    if (c->crowd != 0 && c->crowd != 1) return fail(MADRL_EINVAL, "madrl_waterworld_config.crowd must be 0 or 1 (got %d)", c->crowd);
    if (c->n_pursuers < 1 || c->n_evaders < 1 || c->n_poison < 1)
        return fail(MADRL_EINVAL, "n_pursuers, n_evaders, n_poison must be >= 1");
    if (c->crowd) {  // ww_crowd_kernel (waterworld_crowd.hip): particles looped over the threads of a multi-wavefront workgroup
        if (c->n_pursuers > 128) return fail(MADRL_EINVAL, "crowd kernel: n_pursuers must be <= 128 (got %d)", c->n_pursuers);
        if ((int64_t)c->n_pursuers + c->n_evaders + c->n_poison > 1023)
            return fail(MADRL_EINVAL, "crowd kernel: at most 1023 particles per env (got %lld)",
                        (long long)c->n_pursuers + c->n_evaders + c->n_poison);
    } else {
        if ((int64_t)c->n_pursuers + c->n_evaders + c->n_poison > 62)
            return fail(MADRL_EINVAL, "at most 62 particles per env (one wavefront per env); crowd=1 runs up to 1023 on the multi-wavefront kernel");
        if (2 * c->n_pursuers > 64) return fail(MADRL_EINVAL, "n_pursuers must be <= 32");
    }
    if (c->n_sensors < 1 || c->n_sensors > 256) return fail(MADRL_EINVAL, "n_sensors must be in 1..256");
    if (c->n_coop < 1) return fail(MADRL_EINVAL, "n_coop must be >= 1");
    return MADRL_OK;
}

int ww_obs_dim_of(const madrl_waterworld_config *c) {
    return c->n_sensors * (c->speed_features ? 7 : 4) + 2 + (c->addid ? 1 : 0);  // Archea.__init__ :18-24
}

void ww_layout(const madrl_waterworld_config *c, WwDev *d) {
    memset(d, 0, sizeof(*d));
    d->Np = c->n_pursuers; d->Ne = c->n_evaders; d->Npo = c->n_poison; d->NP = d->Np + d->Ne + d->Npo;
    d->K = c->n_sensors; d->D = ww_obs_dim_of(c); d->nfeat = c->speed_features ? 7 : 4;
    d->n_coop = c->n_coop; d->addid = c->addid; d->speed_features = c->speed_features;
    d->reward_global = c->reward_global; d->obstacle_fixed = c->obstacle_fixed; d->max_steps = c->max_steps;
    d->auto_reset = c->auto_reset;
    d->rec_dw = (int)align_up((size_t)4 * d->NP + 4, 4);
    d->k0 = (uint32_t)c->seed; d->k1 = (uint32_t)(c->seed >> 32); d->gid_base = (uint32_t)c->env_id_base;
    // radii: pursuer r, evader 2r, poison 3r/4, evaluated in float64 like the reference (:108-118)
    d->r_pu = (float)c->radius; d->r_ev = (float)(c->radius * 2); d->r_po = (float)(c->radius * 3 / 4);
    d->obst_r = (float)c->obstacle_radius; d->ev_speed = (float)c->ev_speed; d->poison_speed = (float)c->poison_speed;
    d->sensor_range = (float)c->sensor_range; d->action_scale = (float)c->action_scale;
    d->poison_reward = (float)c->poison_reward; d->food_reward = (float)c->food_reward;
    d->encounter_reward = (float)c->encounter_reward; d->control_penalty = (float)c->control_penalty;
    d->obst_x = (float)c->obstacle_loc[0]; d->obst_y = (float)c->obstacle_loc[1];
    // the float32 sums are the ones the kernel used to form before comparing (pr + obst_r, r_pu + r_ev, r_pu + r_po)
    d->sq_obst_pu = sq_threshold(d->r_pu + d->obst_r); d->sq_obst_ev = sq_threshold(d->r_ev + d->obst_r);
    d->sq_obst_po = sq_threshold(d->r_po + d->obst_r);
    d->sq_hit_ev = sq_threshold(d->r_pu + d->r_ev); d->sq_hit_po = sq_threshold(d->r_pu + d->r_po);
}

size_t ww_lds_bytes(const WwDev &d) { return wave_lds_bytes(d.rec_dw, d.Np, d.D, d.K, d.Ne, d.Npo); }

size_t ww_lds_bytes_crowd(const WwDev &d) { return ww_crowd_lds_bytes(d.Np, d.Ne, d.Npo, d.K, d.rec_dw); }

struct WwSpec {
    int Np, Ne, Npo, K, D;
    void (*launch)(const WwDev &, const WwIO &, int mode, bool fused, dim3 g, hipStream_t s);
};

template <int TNp, int TNe, int TNpo, int TK, int TD>
void ww_launch_spec(const WwDev &d, const WwIO &io, int mode, bool fused, dim3 g, hipStream_t s) {
    const dim3 b(64);  // static LDS layout: 0 dynamic bytes
    if (mode == 0) {
        if (fused) hipLaunchKernelGGL((waterworld_kernel<0, TNp, TNe, TNpo, TK, true, TD>), g, b, 0, s, d, io);
        else hipLaunchKernelGGL((waterworld_kernel<0, TNp, TNe, TNpo, TK, false, TD>), g, b, 0, s, d, io);
    } else {
        if (fused) hipLaunchKernelGGL((waterworld_kernel<1, TNp, TNe, TNpo, TK, true, TD>), g, b, 0, s, d, io);
        else hipLaunchKernelGGL((waterworld_kernel<1, TNp, TNe, TNpo, TK, false, TD>), g, b, 0, s, d, io);
    }
}

#define X(NP_, NE_, NPO_, K_, D_) {NP_, NE_, NPO_, K_, D_, ww_launch_spec<NP_, NE_, NPO_, K_, D_>},
const WwSpec WW_SPECS[] = {
#include "waterworld_specializations.def"
#if __has_include("waterworld_specializations.local.def")   // shapes added on this machine by `python -m madrl_amd.build --waterworld-shape ...` (git-ignored)
#include "waterworld_specializations.local.def"
#endif
};
#undef X

int ww_launch(const madrl_waterworld *h, const WwIO &io, int mode, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const WwDev &d = h->dev;
    if (h->cfg.crowd) return ww_crowd_launch(&h->dev, &io, mode, h->max_blocks, h->lds_bytes, h->pending, h->live, stream);
    const dim3 g = particle_grid(h->max_blocks, d.n_envs), b(64);
    const bool fused = io.st != nullptr;
    const WwSpec *spec = nullptr;
    for (const WwSpec &w : WW_SPECS)
        if (d.Np == w.Np && d.Ne == w.Ne && d.Npo == w.Npo && d.K == w.K && d.D == w.D) spec = &w;
    if (spec) {
        spec->launch(h->dev, io, mode, fused, g, s);
    } else if (mode == 0) {
        if (fused) hipLaunchKernelGGL((waterworld_kernel<0, 0, 0, 0, 0, true>), g, b, h->lds_bytes, s, h->dev, io);
        else hipLaunchKernelGGL((waterworld_kernel<0, 0, 0, 0, 0, false>), g, b, h->lds_bytes, s, h->dev, io);
    } else {
        if (fused) hipLaunchKernelGGL((waterworld_kernel<1, 0, 0, 0, 0, true>), g, b, h->lds_bytes, s, h->dev, io);
        else hipLaunchKernelGGL((waterworld_kernel<1, 0, 0, 0, 0, false>), g, b, h->lds_bytes, s, h->dev, io);
    }
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}

__global__ void ww_state_copy_kernel(const WwDev d, float *pos, float *vel, float *obst, int32_t *t, uint32_t *tick,
                                     const int to_state) {
    const int64_t env = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (env >= d.n_envs) return;
    float *rec = d.state + env * (int64_t)d.rec_dw;
    const int NP = d.NP;
    for (int k = 0; k < 2 * NP; ++k) {
        if (pos) { if (to_state) rec[k] = pos[env * 2 * NP + k]; else pos[env * 2 * NP + k] = rec[k]; }
        if (vel) { if (to_state) rec[2 * NP + k] = vel[env * 2 * NP + k]; else vel[env * 2 * NP + k] = rec[2 * NP + k]; }
    }
    for (int k = 0; k < 2; ++k)
        if (obst) { if (to_state) rec[4 * NP + k] = obst[env * 2 + k]; else obst[env * 2 + k] = rec[4 * NP + k]; }
    int32_t *ti = reinterpret_cast<int32_t *>(rec) + 4 * NP + 2;
    uint32_t *tk = reinterpret_cast<uint32_t *>(rec) + 4 * NP + 3;
    if (t) { if (to_state) *ti = t[env]; else t[env] = *ti; }
    if (tick) { if (to_state) *tk = tick[env]; else tick[env] = *tk; }
}

}  // namespace

extern "C" {

int madrl_waterworld_obs_dim(const madrl_waterworld_config *cfg, int32_t *out_dim) {
    int rc = ww_validate(cfg);
    if (rc) return rc;
    if (!out_dim) return fail(MADRL_EINVAL, "out_dim is NULL");
    *out_dim = ww_obs_dim_of(cfg);
    return MADRL_OK;
}

int madrl_waterworld_state_bytes(const madrl_waterworld_config *cfg, int64_t n_envs, uint64_t *out_bytes) {
    int rc = ww_validate(cfg);
    if (rc) return rc;
    if (n_envs < 1 || !out_bytes) return fail(MADRL_EINVAL, "n_envs must be >= 1 and out_bytes non-NULL");
    WwDev d;
    ww_layout(cfg, &d);
    *out_bytes = (uint64_t)d.rec_dw * 4u * (uint64_t)n_envs;
    return MADRL_OK;
}

int madrl_waterworld_create(const madrl_waterworld_config *cfg, const double *sensors_host, int64_t n_envs,
                            int32_t device, void *state_dev, madrl_waterworld **out) {
    int rc = ww_validate(cfg);
    if (rc) return rc;
    return particle_create(cfg, sensors_host, n_envs, device, state_dev, out, ww_layout, cfg->crowd ? ww_lds_bytes_crowd : ww_lds_bytes);
}

int madrl_waterworld_kernel_kind(madrl_waterworld *h, int32_t *out) { return particle_kernel_kind(h, out); }

void madrl_waterworld_destroy(madrl_waterworld *h) { particle_destroy(h); }

int madrl_waterworld_set_standardize(madrl_waterworld *h, const madrl_standardize_args *a) { return particle_set_standardize(h, a); }

int madrl_waterworld_set_launch(madrl_waterworld *h, int64_t max_blocks) { return particle_set_launch(h, max_blocks); }

int madrl_waterworld_set_particle_counts(madrl_waterworld *h, const int32_t *pending_dev, int32_t *live_dev) {
    return particle_set_counts(h, pending_dev, live_dev);
}

int madrl_waterworld_reset(madrl_waterworld *h, const uint8_t *mask_dev, float *obs_dev, void *stream) {
    return particle_reset(h, mask_dev, obs_dev, stream, ww_launch);
}

int madrl_waterworld_step(madrl_waterworld *h, const float *actions_dev, const float *inj_respawn_dev, float *obs_dev,
                          float *rew_dev, uint8_t *done_dev, int32_t *info_dev, void *stream) {
    return particle_step(h, actions_dev, inj_respawn_dev, obs_dev, rew_dev, done_dev, info_dev, stream, ww_launch);
}

int madrl_waterworld_get_state(madrl_waterworld *h, float *pos, float *vel, float *obst, int32_t *t, uint32_t *tick,
                               void *stream) {
    return state_copy_launch(h, ww_state_copy_kernel, stream, pos, vel, obst, t, tick, 0);
}

int madrl_waterworld_set_state(madrl_waterworld *h, const float *pos, const float *vel, const float *obst,
                               const int32_t *t, const uint32_t *tick, void *stream) {
    return state_copy_launch(h, ww_state_copy_kernel, stream, (float *)pos, (float *)vel, (float *)obst, (int32_t *)t, (uint32_t *)tick, 1);
}

}  // extern "C"
