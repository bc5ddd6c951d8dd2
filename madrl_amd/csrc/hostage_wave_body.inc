// hostage_wave_body.inc -- the body of hostage_kernel<MODE, TNr, TNh, TNc, TK, TD, FUSED> and of hostage_kernel_f16 (hostage.hip), included
// inside both __global__ entries like waterworld_wave_body.inc: the float32 entry keeps its two arguments, its name and its code.
// In scope: MODE, TNr .. TD, FUSED, d (HwDev), io (HwIO), HwKArgs / clipf / bcast and the macro MADRL_HW_BODY_HALF (0 / 1).
// HALF: io.obs is a binary16 destination and the staged rows leave through store_rows_half (particle_wave.hpp); nothing else differs.
// Never with FUSED.
    // specialised shape: compile-time LDS layout in a static array, launched with 0 dynamic bytes (see waterworld.hip)
    constexpr int SPEC_BYTES = TNr > 0 ? (int)wave_lds_bytes(4 * (TNr + TNh + TNc) + 9, TNr, TD, TK, TNh, TNc) : 16;
    static_assert(TNr == 0 || TD > 0, "a specialised shape fixes the observation width too");
    extern __shared__ __attribute__((aligned(16))) float smem_dyn[];
    __shared__ __attribute__((aligned(16))) float smem_static[SPEC_BYTES / 4];
    float *const smem = TNr > 0 ? smem_static : smem_dyn;
    const int lane = threadIdx.x;
    const uint32_t ulane = threadIdx.x;
#define DA (kernargs<HwKArgs>()->d)
#define IOA (kernargs<HwKArgs>()->io)
    const int Nr = TNr > 0 ? TNr : d.Nr, Nh = TNr > 0 ? TNh : d.Nh, Nc = TNr > 0 ? TNc : d.Nc, K = TNr > 0 ? TK : d.K;
    const int NP = Nr + Nh + Nc, D = TD > 0 ? TD : d.D;
    float *S = smem;                                   // packed record
    float *X = S, *V = S + 2 * NP;
    uint32_t *SU = reinterpret_cast<uint32_t *>(S);
    const int OFF_KEY = 4 * NP, OFF_BOMB = 4 * NP + 2, OFF_SAVED = 4 * NP + 4, OFF_FLAGS = 4 * NP + 6, OFF_T = 4 * NP + 7, OFF_TICK = 4 * NP + 8;
    const int rec_dw = TNr > 0 ? (4 * (TNr + TNh + TNc) + 9 + 3) / 4 * 4 : d.rec_dw;
    float *O = S + ((rec_dw + 3) & ~3);                // observation staging [Nr][D]
    float *const O_SPARE = O + Nr * D;                 // one more row: where the sensing lanes without a (rescuer, sensor) pair write
    float *SEN = O + (((Nr + 1) * D + 3) & ~3);        // sensor unit vectors [K][2]
    uint64_t *NEAR = reinterpret_cast<uint64_t *>(SEN + ((2 * K + 3) & ~3));  // per rescuer: particles (bit j), key (bit NP), bomb (bit NP + 1) in sensing reach
    uint8_t *COLH = reinterpret_cast<uint8_t *>(NEAR + Nr);  // [Nr][Nh]
    uint8_t *COLC = COLH + Nr * Nh;                    // [Nr][Nc]
    uint8_t *FLG = COLC + Nr * Nc;                     // ho_caught[Nh] | ho_enc[Nh] | cr_caught[Nc]

    for (int k = lane; k < 2 * K; k += 64) SEN[k] = d.sensors[k];

    WaveRecord cur;  // software pipeline: the next env's record (<= 4 dwords per lane) + action row are fetched one env ahead
    const EnvWalk walk = env_walk(d.n_envs);  // XCD-aware: neighbouring envs share an L2 (common.hpp)
    if (walk.first < walk.lim) cur.fetch<MODE, HwKArgs>(walk.base + walk.first, rec_dw, Nr, lane, ulane);
    cur.hinge();
    wave_sync();

    const int w_base = (int)walk.base, w_stride = (int)walk.stride, w_lim = (int)walk.lim;  // env indices are 32-bit, byte offsets 64-bit
    for (int li = (int)walk.first; li < w_lim; li += w_stride) {
        const int64_t env = w_base + li;
        const int64_t nenv = env + w_stride;
        WaveRecord nxt;
        if (li + w_stride < w_lim) nxt.fetch<MODE, HwKArgs>(nenv, rec_dw, Nr, lane, ulane);
        bool skip = false;
        if constexpr (MODE == 0) skip = (IOA.mask != nullptr && IOA.mask[env] == 0);
        if (!skip) {
            cur.to_lds(SU, rec_dw, lane);
            wave_sync();
            int32_t tstep = (int32_t)SU[OFF_T];
            uint32_t tick = SU[OFF_TICK];
            uint32_t flags = SU[OFF_FLAGS];  // bit0 gate_open, bit1 bombed, bit2 key sampled
            uint64_t saved = (uint64_t)SU[OFF_SAVED] | ((uint64_t)SU[OFF_SAVED + 1] << 32);
            const uint32_t gid = DA.gid_base + (uint32_t)env;
            float act_lane = cur.act;

            bool do_init = (MODE == 0);
            int npass = 1;
            for (int pass = 0; pass < npass; ++pass) {
                if (do_init) {
                    // ------------------------------------------------ reset (:137-177); draw index: key 0, particle j -> 1 + j, bomb 1 + NP
                    tstep = 0;
                    if (fresh(lane) < NP + 2) {
                        const uint32_t di = fresh(lane) < NP ? 1u + (uint32_t)lane : (fresh(lane) == NP ? 0u : 1u + (uint32_t)NP);
                        const u32x4 r = philox4x32_10(gid, tick, di, HW_TAG_RESET, DA.k0, DA.k1);
                        const float u0 = u24(r.x), u1 = u24(r.y), u2 = u24(r.z), u3 = u24(r.w);
                        if (fresh(lane) < Nr) {  // :149-153
                            X[2 * lane] = u0; X[2 * lane + 1] = clipf(u1, 0.55f, 0.95f);
                            V[2 * lane] = 0.f; V[2 * lane + 1] = 0.f;
                        } else if (fresh(lane) < Nr + Nh) {  // :156-160
                            X[2 * lane] = u0; X[2 * lane + 1] = clipf(u1, 0.f, 0.35f + u2 * 0.01f);
                            V[2 * lane] = 0.f; V[2 * lane + 1] = 0.f;
                        } else if (fresh(lane) < NP) {  // :165-168 (velocity not centred here)
                            X[2 * lane] = u0; X[2 * lane + 1] = u1;
                            V[2 * lane] = u2 * DA.bad_speed; V[2 * lane + 1] = u3 * DA.bad_speed;
                        } else if (fresh(lane) == NP) {  // key: the first reset of the env's life only (G2, :143-146)
                            if (!(flags & 4u)) {
                                S[OFF_KEY] = DA.key_fixed ? DA.key_x : 1.f - u0 * 0.1f;
                                S[OFF_KEY + 1] = DA.key_fixed ? DA.key_y : 1.f - u1 * 0.1f;
                            }
                        } else {  // bomb :171
                            S[OFF_BOMB] = clipf(u0, 0.f, 0.25f); S[OFF_BOMB + 1] = clipf(u1, 0.f, 0.25f);
                        }
                    }
                    saved = 0ull;
                    flags = 4u;
                    tick += 1;
                    act_lane = 0.0f;  // reset ends with step(zeros) (:173)
                    wave_sync();
                }
                // ---------------------------------------------------- step (:228-430)
                const float kx = S[OFF_KEY], ky = S[OFF_KEY + 1], bx = S[OFF_BOMB], by = S[OFF_BOMB + 1];
                const bool gate0 = flags & 1u;  // gate state before this step's key processing (G5)
                float reward = 0.0f;
                bool col_bo = false, col_ke = false;
                {   // phase A: rescuers (:231-260)
                    float a0, a1;  // the penalty: under the global reward (actions**2).sum(), row-major (:241-242)
                    const float pen = agent_action<HwKArgs>(act_lane, [&]() { return fresh(lane) < Nr ? lane : 0; }, Nr, a0, a1);
                    if (fresh(lane) < Nr) {
                        float x = X[2 * lane], y = X[2 * lane + 1], vx = V[2 * lane], vy = V[2 * lane + 1];
                        vx = vx + a0; vy = vy + a1;
                        x = x + vx; y = y + vy;
                        reward = 0.0f + pen;
                        float cx = clipf(x, 0.f, 1.f), cy = clipf(y, 0.f, 1.f);  // walls :247-252
                        if (x != cx) vx = 0.f;
                        if (y != cy) vy = 0.f;
                        x = cx; y = cy;
                        if (!gate0) {  // G3: both coordinates, velocity component flipped (:255-260)
                            cx = clipf(x, DA.gate_lo, 1.f); cy = clipf(y, DA.gate_lo, 1.f);
                            if (x != cx) vx *= -1.f;
                            if (y != cy) vy *= -1.f;
                            x = cx; y = cy;
                        }
                        X[2 * lane] = x; X[2 * lane + 1] = y; V[2 * lane] = vx; V[2 * lane + 1] = vy;
                        col_bo = dist2_le(x, y, bx, by, DA.sq_bomb);  // dist <= radius + bomb_radius, :281-291
                        col_ke = dist2_le(x, y, kx, ky, DA.sq_key);   // dist <= radius + key_radius
                    }
                }
                wave_sync();
                // phase B: collisions (:263-279), no saved mask here (G4)
                // BITROWS (specialised shapes with at most 64 rescuer x hostage and rescuer x criminal pairs): a collision matrix is one
                // wave-uniform 64-bit ballot (bit i * n + m), columns counted and rows tested with bit operations (waterworld.hip)
                constexpr bool BITROWS = TNr > 0 && TNr * TNh <= 64 && TNr * TNc <= 64 && TNh < 64 && TNc < 64;
                uint64_t col_ho = 0ull, col_cr = 0ull;
                bool my_caught = false, my_enc = false;  // hostage / criminal lanes count their column (_caught :184-198)
                if constexpr (BITROWS) {
                    {
                        const bool in = fresh(lane) < Nr * Nh;
                        const int i = in ? lane / Nh : 0, m = in ? lane - i * Nh : 0, j = Nr + m;
                        col_ho = __ballot(in && dist2_le(X[2 * i], X[2 * i + 1], X[2 * j], X[2 * j + 1], DA.sq_hit_ho));
                    }
                    {
                        const bool in = fresh(lane) < Nr * Nc;
                        const int i = in ? lane / Nc : 0, m = in ? lane - i * Nc : 0, j = Nr + Nh + m;
                        col_cr = __ballot(in && dist2_le(X[2 * i], X[2 * i + 1], X[2 * j], X[2 * j + 1], DA.sq_hit_cr));
                    }
                    uint64_t cm_ho = 0ull, cm_cr = 0ull;  // bit i * n of every row
#pragma unroll
                    for (int i = 0; i < (TNr > 0 ? TNr : 1); ++i) { cm_ho |= 1ull << (i * Nh); cm_cr |= 1ull << (i * Nc); }
                    if (fresh(lane) >= Nr && fresh(lane) < NP) {
                        const bool is_ho = fresh(lane) < Nr + Nh;
                        const int m = is_ho ? lane - Nr : lane - Nr - Nh;
                        const int sc = __popcll((is_ho ? col_ho : col_cr) & ((is_ho ? cm_ho : cm_cr) << m));
                        my_caught = sc >= (is_ho ? DA.n_coop_save : 1);
                        my_enc = is_ho && sc >= 1;
                    }
                } else {
                contact_bytes(X, COLH, Nr, Nh, Nc, lane, [&](bool is_ho) { return is_ho ? DA.sq_hit_ho : DA.sq_hit_cr; });
                wave_sync();
                if (fresh(lane) >= Nr && fresh(lane) < NP) {
                    const bool is_ho = fresh(lane) < Nr + Nh;
                    const int m = is_ho ? lane - Nr : lane - Nr - Nh;
                    const int s = column_count(is_ho ? COLH : COLC, Nr, is_ho ? Nh : Nc, m);
                    my_caught = s >= (is_ho ? DA.n_coop_save : 1);
                    my_enc = is_ho && s >= 1;
                    column_flags(FLG, is_ho, Nh, m, my_caught, my_enc);
                }
                }
                const uint64_t ho_lanes = low_bits64(Nh) << Nr;
                const uint64_t caught_mask = __ballot(my_caught);
                const int n_ho_caught = __popcll(caught_mask & ho_lanes);
                const int n_cr_caught = __popcll(caught_mask & ~ho_lanes);
                const uint64_t enc_mask = __ballot(my_enc);
                const int n_ho_enc = __popcll(enc_mask);
                const bool bo_caught = __ballot(col_bo) != 0ull, ke_caught = __ballot(col_ke) != 0ull;
                wave_sync();
                // phase C: sensing (:295-362).  Rows: [criminal dist | criminal speed | hostage dist | key dist | bomb dist] (:398-400)
                {
                    // passes of 64 (rescuer, sensor) pairs held in registers at a time (sense_pass: the lane layout of a pass)
                    const int n_pass = sense_n_pass<TK>(Nr, K);
                    constexpr int N_PASS_T = TNr > 0 ? sense_n_pass<TK>(TNr, TK) : 3;
                    const float srange = DA.sensor_range, rad2 = DA.radius * DA.radius;  // G1
                    const float part_x = fresh(lane) < NP ? X[2 * lane] : 0.f, part_y = fresh(lane) < NP ? X[2 * lane + 1] : 0.f;
                    // Conservative cull: NEAR[i] marks the objects within rescuer i's sensing reach (the key: bit NP, the bomb: bit NP + 1); all
                    // others would yield INFINITY for every sensor of the rescuer and are skipped per pass.
                    {
                        const float thr2 = sensor_reach2(rad2, srange);
                        const float mx = fresh(lane) == NP ? kx : (fresh(lane) == NP + 1 ? bx : part_x), my = fresh(lane) == NP ? ky : (fresh(lane) == NP + 1 ? by : part_y);
                        reach_cull(NEAR, Nr, part_x, part_y, mx, my, thr2, [&]() { return fresh(lane) <= NP + 1; }, [&]() { return fresh(lane) == 0; });
                        wave_sync();
                    }
                    // ONE PASS AT A TIME (round 6, as in waterworld.hip): a pass walks the set bits of ITS OWN reach mask (ascending = the
                    // reference's index order: the first minimum wins as in np.argmin) instead of the union of the passes' masks with a
                    // test-and-skip per pass and object -- scalar work on the CU's one scalar pipe; lanes without a (rescuer, sensor) pair write
                    // to a spare row instead of branching around the stores.
#pragma unroll
                    for (int pass_q = 0; pass_q < (TNr > 0 ? N_PASS_T : n_pass); ++pass_q) {
                        const SensePass sp = sense_pass<TK>(pass_q, Nr, K, lane);  // the rescuers of this pass, this lane's (rescuer, sensor)
                        const bool okq = sp.okq;
                        const int iq = sp.iq, kq = sp.kq;
                        const float sxq = SEN[2 * kq], syq = SEN[2 * kq + 1];
                        const float pxq = X[2 * iq], pyq = X[2 * iq + 1];
                        const uint64_t reach = pass_reach(NEAR, sp.i_first, sp.i_last);  // wave-uniform: objects in reach of any rescuer of this pass
                        auto sense = [&](float qx, float qy) -> float {
                            float sv;
                            const bool out = ray_misses(sxq, syq, pxq, pyq, qx, qy, srange, rad2, sv);
                            return out ? INFINITY : sv;
                        };
                        float b_cr = INFINITY, b_ho = INFINITY;
                        int a_cr = 0;
                        if (TNr > 0 && Nc <= 32 && Nh <= 32) {   // 32-bit class masks: half the scalar work of the walk
                            walk_bits((uint32_t)(reach >> (Nr + Nh)) & low_bits32(Nc), [&](int m) {
                                const float sv = sense(bcast(part_x, Nr + Nh + m), bcast(part_y, Nr + Nh + m));
                                const bool better = sv < b_cr;
                                b_cr = better ? sv : b_cr;
                                a_cr = better ? m : a_cr;
                            });
                            // hostages: the saved ones (mask from before this step's processing, G5, :296) are not sensed
                            walk_bits((uint32_t)(reach >> Nr) & low_bits32(Nh) & ~(uint32_t)saved, [&](int m) {
                                const float sv = sense(bcast(part_x, Nr + m), bcast(part_y, Nr + m));
                                b_ho = sv < b_ho ? sv : b_ho;
                            });
                        } else {
                            walk_bits(reach & (low_bits64(Nc) << (Nr + Nh)), [&](int bit) {
                                const float sv = sense(bcast(part_x, bit), bcast(part_y, bit));
                                const bool better = sv < b_cr;
                                b_cr = better ? sv : b_cr;
                                a_cr = better ? bit - (Nr + Nh) : a_cr;
                            });
                            walk_bits(reach & ((low_bits64(Nh) & ~saved) << Nr), [&](int bit) {
                                const float sv = sense(bcast(part_x, bit), bcast(part_y, bit));
                                b_ho = sv < b_ho ? sv : b_ho;
                            });
                        }
                        const float b_ke = ((reach >> NP) & 1ull) ? sense(kx, ky) : INFINITY;
                        const float b_bo = ((reach >> (NP + 1)) & 1ull) ? sense(bx, by) : INFINITY;
                        {
                            float *o = okq ? O + iq * D : O_SPARE;
                            const bool fin = b_cr < INFINITY;
                            const int j = Nr + Nh + a_cr;   // (a_cr = 0 without a hit: a valid particle, its value is not used)
                            const float raw = speed_along(V, sxq, syq, j, iq);   // :204-226; loaded and computed unconditionally: a select, no branch
                            o[kq] = fin ? b_cr : 0.f;
                            o[K + kq] = fin ? raw : 0.f;
                            o[2 * K + kq] = (gate0 && b_ho < INFINITY) ? b_ho : 0.f;   // :320-322
                            o[3 * K + kq] = (!gate0 && b_ke < INFINITY) ? b_ke : 0.f;  // :338-340
                            o[4 * K + kq] = (b_bo < INFINITY) ? b_bo : 0.f;
                        }
                    }
                }
                // rescuer lanes: contact flags and who-caught tests for the local rewards (G9)
                bool w_ho = false, w_enc = false, w_cr = false, t_ho = false, t_cr = false;
                if (fresh(lane) < Nr) {
                    if constexpr (BITROWS) {
                        const uint64_t row_ho = (col_ho >> (lane * Nh)) & ((1ull << Nh) - 1ull);
                        const uint64_t row_cr = (col_cr >> (lane * Nc)) & ((1ull << Nc) - 1ull);
                        t_ho = row_ho != 0ull;
                        t_cr = row_cr != 0ull;
                        w_ho = (row_ho & (caught_mask >> Nr)) != 0ull;          // touches a caught hostage
                        w_enc = (row_ho & (enc_mask >> Nr)) != 0ull;            // touches an encountered hostage
                        w_cr = (row_cr & (caught_mask >> (Nr + Nh))) != 0ull;   // touches a caught criminal
                    } else {
                        agent_contacts(COLH, COLC, FLG, lane, Nh, Nc, t_ho, w_ho, w_enc, t_cr, w_cr);
                    }
                }
                wave_sync();
                // phase D: process collisions (:365-383)
                saved |= (caught_mask & ho_lanes) >> Nr;
                if (fresh(lane) >= Nr + Nh && fresh(lane) < NP && my_caught) {
                    const int m = lane - Nr - Nh;
                    float x, y, u0, u1;
                    if (MODE == 1 && IOA.inj_resp != nullptr && !do_init) {
                        const float *r = IOA.inj_resp + (env * Nc + m) * 4;
                        x = r[0]; y = r[1]; u0 = r[2]; u1 = r[3];
                    } else {
                        const u32x4 r = philox4x32_10(gid, tick, (uint32_t)m, HW_TAG_RESPAWN, DA.k0, DA.k1);
                        x = u24(r.x); y = u24(r.y); u0 = u24(r.z); u1 = u24(r.w);
                    }
                    X[2 * lane] = x; X[2 * lane + 1] = y;
                    V[2 * lane] = (u0 - 0.5f) * DA.bad_speed; V[2 * lane + 1] = (u1 - 0.5f) * DA.bad_speed;
                }
                tick += 1;
                if (bo_caught) flags |= 2u;
                if (ke_caught) flags |= 1u;
                const float gate1 = (flags & 1u) ? 1.f : 0.f, bombed1 = (flags & 2u) ? 1.f : 0.f;  // states after processing (G6)
                // phase E: rewards (:385-396)
                if (fresh(lane) < Nr) {
                    if (DA.reward_global) {
                        reward += ((((float)n_ho_enc * DA.encounter_reward) * gate1 + (float)n_ho_caught * DA.save_reward) +
                                   (float)n_cr_caught * DA.hit_reward) + bombed1 * DA.bomb_reward;
                    } else {
                        if (w_ho) reward += DA.save_reward;
                        if (w_enc) reward += DA.encounter_reward * gate1;
                        if (w_cr) reward += DA.hit_reward;
                        if (col_bo) reward += bombed1 * DA.bomb_reward;
                    }
                }
                wave_sync();
                // phase F: criminals move; velocity flips only if BOTH coordinates left [0,1], no clipping (G7, :402-408)
                if (fresh(lane) >= Nr + Nh && fresh(lane) < NP) {
                    float x = X[2 * lane], y = X[2 * lane + 1], vx = V[2 * lane], vy = V[2 * lane + 1];
                    free_motion(x, y, vx, vy);
                    X[2 * lane] = x; X[2 * lane + 1] = y; V[2 * lane] = vx; V[2 * lane + 1] = vy;
                }
                if (fresh(lane) < Nr) {  // tail of the observation row (:410-425)
                    float *o = O + lane * D + 5 * K;
                    o[0] = t_ho ? 1.f : 0.f; o[1] = t_cr ? 1.f : 0.f; o[2] = col_ke ? 1.f : 0.f; o[3] = col_bo ? 1.f : 0.f;
                    o[4] = gate1;
                    if (DA.addid) o[5] = (float)(lane + 1);
                }
                tstep += 1;  // :427
                const uint64_t all_h = low_bits64(Nh);
                const int limit = DA.max_steps > 0 ? DA.max_steps : 1000;  // timestep_limit :118-120
                const bool is_done = (flags & 2u) || ((saved & all_h) == all_h) || tstep >= limit;  // :179-182
                if (is_done && fresh(lane) < Nr) reward += (float)(Nh - __popcll(saved & all_h)) * DA.not_saved_reward;  // :429-430
                wave_sync();

                if (pass == 0) nxt.hinge();  // pipeline hinge
                // ---------------------------------------------------- outputs
#if MADRL_HW_ABLATE & 8
                if (DA.n_envs < 0)
#endif
                if (MODE == 1 && !do_init) {
                    if (fresh(lane) < Nr) uniform_ptr(IOA.rew + env * Nr)[ulane] = reward;
                    if constexpr (FUSED) {  // StandardizedEnv.step :283-291, the operations of wrappers.hip rewnorm_kernel in its order
                        if (IOA.st->rew_out != nullptr && fresh(lane) < Nr) std_reward(*IOA.st, env * Nr + lane, reward);
                    }
                    if (fresh(lane) == 0) {
                        IOA.done[env] = (uint8_t)is_done;
                        IOA.info[2 * env] = n_ho_caught;
                        IOA.info[2 * env + 1] = n_cr_caught;
                    }
                    if (is_done && DA.auto_reset) {  // wave-uniform: run the reset pass next
                        npass = 2;
                        do_init = true;
                    }
                }
#if MADRL_HW_BODY_HALF
                if (pass == npass - 1)  // half rows: the binary16 of every staged value (the host refuses a NULL destination and a bound wrapper)
                    store_rows_half(O, uniform_ptr(reinterpret_cast<uint16_t *>(IOA.obs) + env * (int64_t)(Nr * D)), (uint32_t)(Nr * D), ulane);
#else
                if constexpr (!FUSED) {
                if (pass == npass - 1) {
                    const auto orow = uniform_ptr(IOA.obs + env * (int64_t)(Nr * D));
#if MADRL_HW_ABLATE & 1
                    if (DA.n_envs < 0)
#endif
#if MADRL_HW_ABLATE & 2
                    for (uint32_t e = ulane; e < (uint32_t)(Nr * D); e += 64u) __builtin_nontemporal_store(O[e], &orow[e]);
#else
                    for (uint32_t e = ulane; e < (uint32_t)(Nr * D); e += 64u) orow[e] = O[e];
#endif
                }
                } else if (pass == npass - 1) {  // StandardizedEnv.standardize_obs :242-263; after a fused auto-reset this is the new episode's first row, standardised once
                    const int n_el = Nr * D;
                    const int64_t base = env * (int64_t)n_el;
                    float *const obs_p = IOA.obs;
                    if (obs_p != nullptr) {  // the raw row may be dropped when the wrapper's output is all the caller reads
                        const auto orow = uniform_ptr(obs_p + base);
                        for (uint32_t e = ulane; e < (uint32_t)n_el; e += 64u) orow[e] = O[e];
                    }
                    // by value: through a reference into global memory every float64 store of the loop could have changed alpha, eps and the
                    // pointers (type-based aliasing), and the compiler would load them again behind each one
                    const ParticleStd st = *IOA.st;
                    std_obs_row(st, O, base, n_el, lane);
                }
#endif
                wave_sync();
            }
            // ---------------------------------------------------------- LDS -> record
            if (fresh(lane) == 0) {
                SU[OFF_SAVED] = (uint32_t)saved; SU[OFF_SAVED + 1] = (uint32_t)(saved >> 32);
                SU[OFF_FLAGS] = flags;
                SU[OFF_T] = (uint32_t)tstep;
                SU[OFF_TICK] = tick;
            }
            wave_sync();
#if MADRL_HW_ABLATE & 4
            if (DA.n_envs < 0)
#endif
            store_record<HwKArgs>(SU, env, rec_dw, ulane);
            wave_sync();
        }
        cur = nxt;
    }
