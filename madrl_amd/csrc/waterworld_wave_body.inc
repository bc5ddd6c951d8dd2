// waterworld_wave_body.inc -- the body of waterworld_kernel<MODE, TNp, TNe, TNpo, TK, FUSED, TD> and waterworld_kernel_live<MODE>
// (waterworld.hip), included inside both __global__ entries like waterworld_crowd_body.inc: the fixed-shape entry keeps its two arguments,
// its name and its code.  In scope: MODE, TNp .. TD, FUSED, d (WwDev), io (WwIO) and the macro MADRL_WW_BODY_LIVE (0 / 1); the live entry's third
// argument (ParticleCounts) is read through kernargs<WwKArgsLive>().  MADRL_WW_BODY_RANGES (0 / 1): the ranged entry, see RNG below.
// MADRL_WW_BODY_HALF (0 / 1): waterworld_kernel_f16 (waterworld_f16.hip) -- io.obs is a binary16 destination and the staged rows leave through
// store_rows_half (particle_wave.hpp); nothing else differs.  Never with LIVE, RANGES or FUSED.
// LIVE: d.Np / d.Ne / d.Npo are a CAPACITY (Pc, Ec, POc) and every env runs its own counts.  Whatever a caller sees stays at the capacity,
// slotted by class: the record, the rows of inj_resp, the action / reward / observation rows (stride Pc).  The env's counts travel with the
// record prefetch (WaveCounts); the slotted record is packed to the live counts on its way into LDS and scattered back on its way out
// (slot_to_packed, particle_wave.hpp), so the phases between run on the live counts as they stand and the Philox particle index is the one
// of a fixed-shape batch of those counts.  The LDS parts that are carved once (S, O, the spare row, SEN, NEAR, COL) sit at the capacity's
// offsets; X / V / OB / COLP / FLG follow the live counts inside them.  The counts are per env: every branch on them is wave-uniform.
    constexpr bool LIVE = MADRL_WW_BODY_LIVE;
    // The specialised shape has a compile-time LDS layout in a STATIC array (launched with 0 dynamic bytes): every LDS address is
    // "lane-dependent register + immediate offset".  With the dynamic array the base is a link-time symbol the compiler adds in
    // registers, hoists out of the env loop per access pattern and -- at 5 waves per SIMD -- spills.
    constexpr int SPEC_BYTES = TNp > 0 ? (int)wave_lds_bytes(4 * (TNp + TNe + TNpo) + 4, TNp, TD, TK, TNe, TNpo) : 16;
    static_assert(TNp == 0 || TD > 0, "a specialised shape fixes the observation width too");
    static_assert(SPEC_BYTES <= 64 * 1024, "this line of waterworld_specializations.def (or of its .local.def companion) needs more than 64 KiB of static LDS: "
                                           "madrl_waterworld_create refuses such a shape; `python -m madrl_amd.build --waterworld-shape` checks a shape before it lists it");
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
    const int Pc = TNp > 0 ? TNp : d.Np, Ec = TNp > 0 ? TNe : d.Ne, POc = TNp > 0 ? TNpo : d.Npo, K = TNp > 0 ? TK : d.K;
    const int NPc = Pc + Ec + POc, D = TD > 0 ? TD : d.D;  // TD: the observation width of the specialised shape (7 K + 3)
    // the counts the phases run on (LIVE: set per env, WW_SET_COUNTS)
#if MADRL_WW_BODY_LIVE
    int Np = Pc, Ne = Ec, Npo = POc, NP = NPc;
#else
    const int Np = Pc, Ne = Ec, Npo = POc, NP = NPc;
#endif
    // ---- LDS carve
    float *S = smem;                                    // packed record: X[NP][2] | V[NP][2] | obst[2] | t | tick
    float *X = S, *V = S + 2 * NP;
    float *OB = S + 4 * NP;
    float *O = S + (((TNp > 0 ? 4 * (TNp + TNe + TNpo) + 4 : d.rec_dw) + 3) & ~3);  // observation staging [Np][D]
    float *const O_SPARE = O + Pc * D;                  // one more row: where the sensing lanes without a (pursuer, sensor) pair write
    float *SEN = O + (((Pc + 1) * D + 3) & ~3);         // sensor unit vectors [K][2]
    // RANGES (waterworld_kernel_ranges, madrl_waterworld_set_sensor_ranges): every pursuer senses with its own range.  The table [Pc] lies
    // behind the sensor vectors, in global memory (d.sensors + up4(2 K)) as in LDS; a sensing pass reads its lane's pursuer's range from it
    // for the ray test, and d.sensor_range is the table's maximum: the reach cull, which runs on it, is conservative for every pursuer.
#if MADRL_WW_BODY_RANGES
    float *RNG = SEN + ((2 * K + 3) & ~3);
    uint64_t *NEAR = reinterpret_cast<uint64_t *>(RNG + ((Pc + 3) & ~3));
#else
    uint64_t *NEAR = reinterpret_cast<uint64_t *>(SEN + ((2 * K + 3) & ~3));  // per pursuer: particles (bit j) / obstacle (bit NP) in sensing reach
#endif
    uint8_t *COL = reinterpret_cast<uint8_t *>(NEAR + Pc);  // col_ev[Np][Ne] | col_po[Np][Npo]
    uint8_t *COLP = COL + Np * Ne;
    uint8_t *FLG = COLP + Np * Npo;                     // caught_ev[Ne] | enc_ev[Ne] | caught_po[Npo]
    // LIVE: an env's counts (a WaveCounts word) and what follows from them.  p * e + p * po + 2 e + po is monotone in every count: COLP and
    // FLG stay inside the capacity's bytes.
#if MADRL_WW_BODY_LIVE
#define WW_SET_COUNTS(pk) \
    do { \
        Np = WaveCounts::n0(pk); Ne = WaveCounts::n1(pk); Npo = WaveCounts::n2(pk); NP = Np + Ne + Npo; \
        V = S + 2 * NP; OB = S + 4 * NP; COLP = COL + Np * Ne; FLG = COLP + Np * Npo; \
    } while (0)
#else
#define WW_SET_COUNTS(pk) ((void)0)
#endif

    for (int k = lane; k < 2 * K; k += 64) SEN[k] = d.sensors[k];
#if MADRL_WW_BODY_RANGES
    for (int k = lane; k < Pc; k += 64) RNG[k] = d.sensors[up4(2 * K) + k];
#endif
    const int rec_dw = TNp > 0 ? (4 * (TNp + TNe + TNpo) + 4 + 3) / 4 * 4 : d.rec_dw;  // <= 4 dwords per lane (NP <= 62)

    // ---- software pipeline: next env's record + action row (LIVE: and its counts) are fetched one env ahead
    WaveRecord cur;
    [[maybe_unused]] WaveCounts cur_n;
    // LIVE: the record and the action row have the capacity's strides; lanes < 2 p of the env's live p read the action row
#define WW_FETCH(rec, rec_n, e) \
    do { \
        if constexpr (LIVE) { \
            rec_n.fetch<MODE>(kernargs<WwKArgsLive>()->cn.pending, kernargs<WwKArgsLive>()->cn.live, (e), Pc, Ec, POc); \
            rec.fetch_rows<MODE, WwKArgs>((e), rec_dw, Pc, WaveCounts::n0(rec_n.live), lane, ulane); \
        } else { \
            rec.fetch<MODE, WwKArgs>((e), rec_dw, Np, lane, ulane); \
        } \
    } while (0)
    const int n_envs = (int)d.n_envs;
    if ((int)blockIdx.x < n_envs) WW_FETCH(cur, cur_n, blockIdx.x);
    cur.hinge();
    if constexpr (LIVE) cur_n.hinge();
    wave_sync();

    for (int e32 = blockIdx.x; e32 < n_envs; e32 += (int)gridDim.x) {  // env indices are 32-bit (n_envs < 2^31 - grid), byte offsets 64-bit
        const int64_t env = e32;
        const int n32 = e32 + (int)gridDim.x;
        WaveRecord nxt;
        [[maybe_unused]] WaveCounts nxt_n;
        if (n32 < n_envs) WW_FETCH(nxt, nxt_n, n32);
        bool skip = false;
        if constexpr (MODE == 0) skip = (IOA.mask != nullptr && IOA.mask[env] == 0);
        if (!skip) {
            if constexpr (LIVE) {  // a reset runs on the pending counts from the start: of the old record it keeps the tick alone
                WW_SET_COUNTS(MODE == 0 ? cur_n.pend : cur_n.live);
                cur.to_lds(reinterpret_cast<uint32_t *>(S), rec_dw, lane, [&](int k) { return slot_to_packed(k, Pc, Ec, POc, Np, Ne, Npo); });
            } else {
                cur.to_lds(reinterpret_cast<uint32_t *>(S), rec_dw, lane);
            }
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
                    if constexpr (LIVE) {  // a reset takes the env's pending counts, before its draws
                        WW_SET_COUNTS(cur_n.pend);
                        if (fresh(lane) < 3)
                            uniform_ptr(kernargs<WwKArgsLive>()->cn.live + env * 3)[ulane] = (int32_t)((cur_n.pend >> (8u * ulane)) & 255u);
                    }
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
                if constexpr (LIVE) {  // the staged rows of the pursuers that do not exist: +0.0 (no phase writes them; they leave with the others)
                    for (int k = Np * D + lane; k < Pc * D; k += 64) O[k] = 0.f;
                }
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
                constexpr int GE = (TNe > 0 && TNe < 64) ? 64 / (TNe > 0 ? TNe : 1) : 1, GP = (TNpo > 0 && TNpo < 64) ? 64 / (TNpo > 0 ? TNpo : 1) : 1;  // rows per word
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
#if MADRL_WW_BODY_RANGES
                    const float srange_q = RNG[iq];  // the range of this lane's pursuer (iq < Np <= Pc, 0 in a lane without a pair)
#else
                    const float srange_q = srange;
#endif
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
                            const bool out = ray_misses(sxq, syq, pxq, pyq, qx, qy, srange_q, rad2, sv) | ((cls == 3) & (m == iq));
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
                        // (LIVE: the rows are slotted at the capacity)
                        const float *r = IOA.inj_resp + (env * (LIVE ? NPc : NP) + (LIVE ? (is_ev ? Pc + (lane - Np) : Pc + Ec + (lane - Np - Ne)) : lane)) * 4;
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

                if (pass == 0) {  // pipeline hinge
                    nxt.hinge();
                    if constexpr (LIVE) nxt_n.hinge();
                }
                // ---------------------------------------------------- outputs
                if (MODE == 1 && !do_init) {
                    // (LIVE: `reward` is 0.0f in every lane that is no pursuer -- the rows of the pursuers that do not exist)
                    if (LANE_LT(LIVE ? Pc : Np)) uniform_ptr(IOA.rew + env * (LIVE ? Pc : Np))[ulane] = reward;
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
#if MADRL_WW_BODY_HALF
                if (pass == npass - 1) {  // half rows: the binary16 of every staged value (the host refuses a NULL destination and a bound wrapper)
                    const int n_out = Np * D;
                    store_rows_half(O, uniform_ptr(reinterpret_cast<uint16_t *>(IOA.obs) + env * (int64_t)n_out), (uint32_t)n_out, ulane);
                }
#else
                if (pass == npass - 1) {
                    float *const obs_p = IOA.obs;
                    const int n_out = (LIVE ? Pc : Np) * D;  // (LIVE: the capacity's rows, those of absent pursuers zero-filled in O)
                    const auto orow = uniform_ptr(obs_p + env * (int64_t)n_out);
#if MADRL_WW_ABLATE & 2
                    if (DA.n_envs < 0)
#endif
                    if (obs_p != nullptr) {  // the raw row may be dropped when the fused wrapper output is all the caller reads
                        // 16 bytes per lane (ds_read_b128 + one 16-byte store; an env's rows start on a 4-byte boundary only -- gfx950 under HSA runs
                        // global accesses in unaligned mode -- and the rows of neighbouring envs are contiguous, so whole lines leave the chip anyway)
                        typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
                        typedef float f4a __attribute__((ext_vector_type(4), aligned(16)));
                        const uint32_t n4 = (uint32_t)n_out / 4u;
                        for (uint32_t e = ulane; e < n4; e += 64u)
                            *reinterpret_cast<__attribute__((address_space(1))) f4u *>(orow + 4 * e) = *reinterpret_cast<const f4a *>(O + 4 * e);
                        for (uint32_t e = 4u * n4 + ulane; e < (uint32_t)n_out; e += 64u) orow[e] = O[e];
                    }
                    // (hostage.hip hands the helper a copy of *IOA.st and says why; this kernel keeps the reference)
                    if (FUSED) std_obs_row(*IOA.st, O, env * (int64_t)(Np * D), Np * D, lane);
                }
#endif
                wave_sync();
            }
            // ---------------------------------------------------------- LDS -> record
            if (fresh(lane) == 0) {
                reinterpret_cast<int32_t *>(S)[4 * NP + 2] = tstep;
                reinterpret_cast<uint32_t *>(S)[4 * NP + 3] = tick;
            }
            wave_sync();
            if constexpr (LIVE) {  // packed -> slotted: (-1, -1) / 0 into the slots that hold no particle
                store_record<WwKArgs>(reinterpret_cast<const uint32_t *>(S), env, rec_dw, ulane,
                                      [&](int k) { return slot_to_packed(k, Pc, Ec, POc, Np, Ne, Npo); });
            } else {
                store_record<WwKArgs>(reinterpret_cast<const uint32_t *>(S), env, rec_dw, ulane);
            }
            wave_sync();
        }
        cur = nxt;
        if constexpr (LIVE) cur_n = nxt_n;
    }
#undef WW_SET_COUNTS
#undef WW_FETCH
