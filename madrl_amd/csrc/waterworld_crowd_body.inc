// waterworld_crowd_body.inc -- the body of ww_crowd_kernel<MODE, NW> and ww_crowd_kernel_live<MODE, NW> (waterworld_crowd.hip), included
// inside both __global__ entries like pursuit_crowd_body.inc: the fixed-shape entry keeps its two arguments and its code.  In scope: MODE,
// NW, d (WwDev), io (WwIO), `constexpr bool LIVE` and, when LIVE, cn (ParticleCounts); `constexpr bool RANGES` (ww_crowd_kernel_ranges,
// madrl_waterworld_set_sensor_ranges): every pursuer senses with its own range, from the table RNG [Np] behind the sensor vectors (in
// global memory at d.sensors + up4(2 K)); d.sensor_range is then the table's maximum, which keeps the reach walk conservative for every
// pursuer of a pass, and a ray takes the range of its own pursuer.
    static_assert(NW >= 2 && NW <= 16, "a thread owns at most one pursuer (n_pursuers <= 128)");
    constexpr int NT = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float smem_crowd[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Pc = d.Np, Ec = d.Ne, POc = d.Npo, NPc = d.NP;  // the strides and slots of everything host-facing (LIVE: the capacity)
    const int K = d.K, D = d.D, rec_dw = d.rec_dw;
    int Np = Pc, Ne = Ec, Npo = POc, NP = NPc;                // the counts the phases run on (LIVE: set per env)
    int WE = (Ne + 63) >> 6, WP = (Npo + 63) >> 6, W = WE + WP;  // 64-bit words per collision row: evader chunks | poison chunks
    // ---- LDS carve (every part a multiple of 4 dwords)
    float *S = smem_crowd;
    float *X = S, *V = S + 2 * NPc, *OB = S + 4 * NPc;
    float *SEN = S + up4(rec_dw);
    [[maybe_unused]] float *RNG = SEN + up4(2 * K);  // RANGES only
    float *ACT = SEN + up4(2 * K) + (RANGES ? up4(Pc) : 0);
    uint64_t *COL = reinterpret_cast<uint64_t *>(ACT + up4(2 * Np));  // [Np][W]
    uint64_t *CAU = COL + Np * W;                                     // [W]   caught evaders | caught poisons
    uint64_t *ENC = CAU + W;                                          // [WE]  evaders touched by at least one pursuer

    for (int k = tid; k < 2 * K; k += NT) SEN[k] = d.sensors[k];
    if constexpr (RANGES)
        for (int k = tid; k < Pc; k += NT) RNG[k] = d.sensors[up4(2 * K) + k];

    PassShape passes = pass_shape(K, Np, lane);
    // LIVE: an env's counts and what follows from them
#define WW_SET_COUNTS(src) \
    do { \
        const int32_t *c_ = (src) + 3 * env; \
        Np = clampi(c_[0], 1, Pc); Ne = clampi(c_[1], 1, Ec); Npo = clampi(c_[2], 1, POc); NP = Np + Ne + Npo; \
        WE = (Ne + 63) >> 6; WP = (Npo + 63) >> 6; W = WE + WP; \
        passes = pass_shape(K, Np, lane); \
    } while (0)
    const float srange = d.sensor_range, rad2 = d.r_pu * d.r_pu;  // W3: the SENSING pursuer's radius
    const float reach2 = sensor_reach2(rad2, srange);
    const int limit = d.max_steps > 0 ? d.max_steps : 1000;  // timestep_limit :124-126
    const int n_envs = (int)d.n_envs;

    for (int e32 = blockIdx.x; e32 < n_envs; e32 += (int)gridDim.x) {  // env indices are 32-bit (n_envs < 2^31 - grid), byte offsets 64-bit
        const int64_t env = e32;
        if (MODE == 0 && io.mask != nullptr && io.mask[env] == 0) continue;  // workgroup-uniform
        uint32_t *const rec = reinterpret_cast<uint32_t *>(d.state) + env * (int64_t)rec_dw;
        if constexpr (LIVE) {  // the slotted record -> packed arrays of the env's live counts
            WW_SET_COUNTS(cn.live);
            for (int j = tid; j < NP; j += NT) {
                const int s = j < Np ? j : (j < Np + Ne ? Pc + (j - Np) : Pc + Ec + (j - Np - Ne));  // packed index -> slot
                reinterpret_cast<uint2 *>(X)[j] = reinterpret_cast<const uint2 *>(rec)[s];
                reinterpret_cast<uint2 *>(V)[j] = reinterpret_cast<const uint2 *>(rec)[NPc + s];
            }
            if (tid < 4) reinterpret_cast<uint32_t *>(OB)[tid] = rec[4 * NPc + tid];  // obst[2] | t | tick
        } else {
            for (int k = tid; k < rec_dw; k += NT) reinterpret_cast<uint32_t *>(S)[k] = rec[k];
        }
        __syncthreads();
        int32_t tstep = reinterpret_cast<int32_t *>(S)[4 * NPc + 2];  // every thread holds its own copy of the two counters
        uint32_t tick = reinterpret_cast<uint32_t *>(S)[4 * NPc + 3];
        const uint32_t gid = d.gid_base + (uint32_t)env;
        float *const orow_env = io.obs + env * (int64_t)Pc * D;

        bool do_init = (MODE == 0);
        int npass = 1;
        for (int pass = 0; pass < npass; ++pass) {
            if (do_init) {
                // ------------------------------------------------ reset (:144-172)
                tstep = 0;
                if constexpr (LIVE) {  // a reset takes the env's pending counts, before its draws
                    WW_SET_COUNTS(cn.pending);
                    if (tid < 3) cn.live[3 * env + tid] = tid == 0 ? Np : (tid == 1 ? Ne : Npo);
                }
                if (tid == 0) {
                    float ox = d.obst_x, oy = d.obst_y;
                    if (!d.obstacle_fixed) {  // :147-148
                        const u32x4 r = philox4x32_10(gid, tick, 0u, WW_TAG_OBSTACLE, d.k0, d.k1);
                        ox = u24(r.x);
                        oy = u24(r.y);
                    }
                    OB[0] = ox;
                    OB[1] = oy;
                }
                __syncthreads();
                {
                    const float ox = OB[0], oy = OB[1];
                    for (int j = tid; j < NP; j += NT) {  // :153-170 each particle: uniform position, redrawn while too close to the obstacle
                        const float pr = j < Np ? d.r_pu : (j < Np + Ne ? d.r_ev : d.r_po);
                        const float thr = pr * 2.0f + d.obst_r;
                        float x = 0.f, y = 0.f, u0 = 0.f, u1 = 0.f;
                        for (uint32_t att = 0; att < 1024u; ++att) {
                            const u32x4 r = philox4x32_10(gid, tick, (uint32_t)j, WW_TAG_RESET | (att << 8), d.k0, d.k1);
                            x = u24(r.x);
                            y = u24(r.y);
                            if (att == 0) { u0 = u24(r.z); u1 = u24(r.w); }
                            if (!(dist2d(x, y, ox, oy) <= thr)) break;
                        }
                        X[2 * j] = x;
                        X[2 * j + 1] = y;
                        V[2 * j] = j < Np ? 0.0f : (u0 - 0.5f) * d.ev_speed;  // :164, :170 (W9)
                        V[2 * j + 1] = j < Np ? 0.0f : (u1 - 0.5f) * d.ev_speed;
                    }
                }
                tick += 1;
                __syncthreads();
            }
            // ---------------------------------------------------- step (:220-436); a reset ends with step(zeros) (:172, W11)
            const bool live = MODE == 1 && !do_init;  // a step the caller asked for: actions in, rewards / done / info out
            // the time limit is known up front: a step that ends the episode under auto_reset is followed by the reset pass, whose
            // observations replace this one's -- sensing changes no state, so it is left out of such a step
            const bool emit = !(live && d.auto_reset && tstep + 1 >= limit);
            const float ox = OB[0], oy = OB[1];
            // phase A: particles (:221-270)
            for (int j = tid; j < NP; j += NT) {
                float x = X[2 * j], y = X[2 * j + 1], vx = V[2 * j], vy = V[2 * j + 1];
                float sq_obst = d.sq_obst_po, f = -1.0f;
                if (j < Np) {
                    drive_agent(live, io.actions, env * Pc + j, d.action_scale, ACT, j, x, y, vx, vy);  // :224, :229-231, :239-245
                    sq_obst = d.sq_obst_pu; f = -0.5f;
                } else if (j < Np + Ne) {
                    sq_obst = d.sq_obst_ev; f = -0.5f;
                }
                if (dist2_le(x, y, ox, oy, sq_obst)) {  // dist <= pr + obst_r, :247-270 (W1, W2)
                    vx = f * vx;
                    vy = f * vy;
                }
                X[2 * j] = x; X[2 * j + 1] = y; V[2 * j] = vx; V[2 * j + 1] = vy;
            }
            __syncthreads();
            // phase B1: collisions (:272-293)
            contact_ballots<NW>(X, COL, Np, W, WE, {Np, Ne, d.sq_hit_ev}, {Np + Ne, Npo, d.sq_hit_po}, wave, lane);
            __syncthreads();
            // phase B2: _caught (:180-193)
            column_counts<NW>(COL, CAU, ENC, Np, W, WE, d.n_coop, wave, lane);
            __syncthreads();
            int n_evc = 0, n_poc = 0, n_enc = 0;
            for (int c = 0; c < WE; ++c) { n_evc += __popcll(CAU[c]); n_enc += __popcll(ENC[c]); }
            for (int c = WE; c < W; ++c) n_poc += __popcll(CAU[c]);
            // pursuer threads: collision flags and id of the observation row (:411-428), the reward (:233-237, :376-385)
            if (tid < Np) {
                const int i = tid;
                bool tev = false, tpo = false, wc = false, wp = false, we = false;
                for (int c = 0; c < WE; ++c) {
                    const uint64_t row = COL[i * W + c];
                    tev |= row != 0ull;
                    wc |= (row & CAU[c]) != 0ull;   // touches a caught evader
                    we |= (row & ENC[c]) != 0ull;   // touches an encountered evader
                }
                for (int c = WE; c < W; ++c) {
                    const uint64_t row = COL[i * W + c];
                    tpo |= row != 0ull;
                    wp |= (row & CAU[c]) != 0ull;   // touches a caught poison
                }
                if (emit) {
                    float *o = orow_env + (int64_t)i * D + d.nfeat * K;
                    o[0] = tev ? 1.f : 0.f;
                    o[1] = tpo ? 1.f : 0.f;
                    if (d.addid) o[2] = (float)(i + 1);  // W10
                }
                if (live) {
                    float reward;
                    if (d.reward_global) {  // (actions**2).sum(), row-major (:234-235, W12)
                        const float s = control_sum(ACT, Np);
                        reward = 0.0f + d.control_penalty * s;
                        reward += ((float)n_evc * d.food_reward) + ((float)n_poc * d.poison_reward) + ((float)n_enc * d.encounter_reward);
                    } else {  // fancy-index += pays a pursuer once per kind (W7)
                        const float a0 = ACT[2 * i], a1 = ACT[2 * i + 1];
                        reward = 0.0f + d.control_penalty * (a0 * a0 + a1 * a1);
                        if (wc) reward += d.food_reward;
                        if (wp) reward += d.poison_reward;
                        if (we) reward += d.encounter_reward;
                    }
                    io.rew[env * Pc + i] = reward;
                }
            }
            if constexpr (LIVE) {  // the rows of the pursuers that do not exist: +0.0
                if (live && tid >= Np && tid < Pc) io.rew[env * Pc + tid] = 0.f;
                if (emit)
                    for (int k = Np * D + tid; k < Pc * D; k += NT) orow_env[k] = 0.f;
            }
            // phase C: sensing (:295-353, :389-428)
            if (emit) {
                const bool speed = (bool)d.speed_features;
                for (int p = wave; p < passes.n_pass; p += NW) {
                    const PassLanes L = pass_lanes(passes, p, K, Np, lane);  // the pursuers of this pass
                    Ray ray(SEN, X, V, L.iq, L.kq, RANGES ? RNG[L.iq] : srange, rad2);  // (L.iq < Np)
                    float *const o = orow_env + (int64_t)L.iq * D + L.kq;
#pragma unroll
                    for (int cls = 0; cls < 4; ++cls) {  // 0 obstacle, 1 evaders, 2 poison, 3 allies
                        const int lo = cls == 1 ? Np : (cls == 2 ? Np + Ne : 0);
                        const int cnt = cls == 0 ? 1 : (cls == 1 ? Ne : (cls == 2 ? Npo : Np));
                        ray.restart();
                        auto visit = [&](int m, float qx, float qy) { ray.visit(m, qx, qy, (cls == 3) & (m == L.iq)); };  // allies: not itself
                        if (cls == 0) visit(0, ox, oy);
                        else reach_walk(X, lo, cnt, L, reach2, 0ull, lane, visit);
                        const bool fin = ray.b < INFINITY;
                        const float fd = fin ? ray.b : 0.f;  // W4: raw distance or 0
                        if (cls == 0) {
                            if (L.okq) o[0] = fd;
                        } else {
                            const int j = lo + ray.bi;  // (bi = 0 without a hit: a valid particle, its value is not used)
                            const float raw = ray.speed_along(V, j);  // _extract_speed_features :203-218
                            const float fs = fin ? raw : 0.f;  // W5
                            if (L.okq) {  // np.c_[ob, evd, evs, pod, pos, pud, pus] -> blocks of K (:389-395)
                                if (speed) { o[(2 * cls - 1) * K] = fd; o[2 * cls * K] = fs; }
                                else o[cls * K] = fd;
                            }
                        }
                    }
                }
            }
            __syncthreads();  // sensing read the positions of this step: respawn and motion come after it
            // phase E: respawn caught evaders / poisons (:355-374), then evaders / poisons move (:397-409)
            for (int j = Np + tid; j < NP; j += NT) {
                const bool is_ev = j < Np + Ne;
                const int m = is_ev ? j - Np : j - Np - Ne;
                float x = X[2 * j], y = X[2 * j + 1], vx = V[2 * j], vy = V[2 * j + 1];
                if ((CAU[(is_ev ? 0 : WE) + (m >> 6)] >> (m & 63)) & 1ull) {
                    float u0, u1;
                    if (MODE == 1 && io.inj_resp != nullptr && !do_init) {
                        const float *r = io.inj_resp + (env * NPc + (LIVE ? (is_ev ? Pc + m : Pc + Ec + m) : j)) * 4;
                        x = r[0]; y = r[1]; u0 = r[2]; u1 = r[3];
                    } else {  // the same draws per (env, tick, particle, attempt) as the one-wavefront kernel: particles are independent
                        const float thr = (is_ev ? d.r_ev : d.r_po) * 2.0f + d.obst_r;
                        x = y = u0 = u1 = 0.f;
                        for (uint32_t att = 0; att < 1024u; ++att) {
                            const u32x4 r = philox4x32_10(gid, tick, (uint32_t)j, WW_TAG_RESPAWN | (att << 8), d.k0, d.k1);
                            x = u24(r.x);
                            y = u24(r.y);
                            if (att == 0) { u0 = u24(r.z); u1 = u24(r.w); }
                            if (!(dist2d(x, y, ox, oy) <= thr)) break;
                        }
                    }
                    const float sp = is_ev ? d.ev_speed : d.poison_speed;  // W9
                    vx = (u0 - 0.5f) * sp;
                    vy = (u1 - 0.5f) * sp;
                }
                free_motion(x, y, vx, vy);  // W6
                X[2 * j] = x; X[2 * j + 1] = y; V[2 * j] = vx; V[2 * j + 1] = vy;
            }
            tick += 1;
            tstep += 1;  // :433
            const bool is_done = tstep >= limit;  // :174-178
            if (tid == 0) {
                reinterpret_cast<int32_t *>(S)[4 * NPc + 2] = tstep;
                reinterpret_cast<uint32_t *>(S)[4 * NPc + 3] = tick;
                if (live) {
                    io.done[env] = (uint8_t)is_done;
                    io.info[2 * env] = n_evc;
                    io.info[2 * env + 1] = n_poc;
                }
            }
            if (live && is_done && d.auto_reset) {  // workgroup-uniform: run the reset pass next
                npass = 2;
                do_init = true;
            }
            __syncthreads();
        }
        // ---------------------------------------------------------- LDS -> record
        if constexpr (LIVE) {  // packed arrays -> the slotted record
            for (int s = tid; s < NPc; s += NT) {
                const int m = s < Pc ? s : (s < Pc + Ec ? s - Pc : s - Pc - Ec);           // index within the class
                const int lo = s < Pc ? 0 : (s < Pc + Ec ? Np : Np + Ne);                   // where the class starts in the packed arrays
                const bool is = m < (s < Pc ? Np : (s < Pc + Ec ? Ne : Npo));
                const int j = lo + (is ? m : 0);
                const uint2 x = reinterpret_cast<const uint2 *>(X)[j], v = reinterpret_cast<const uint2 *>(V)[j];
                const uint32_t gone = __float_as_uint(-1.0f);
                reinterpret_cast<uint2 *>(rec)[s] = is ? x : make_uint2(gone, gone);
                reinterpret_cast<uint2 *>(rec)[NPc + s] = is ? v : make_uint2(0u, 0u);
            }
            if (tid < 4) rec[4 * NPc + tid] = reinterpret_cast<const uint32_t *>(OB)[tid];
        } else {
            for (int k = tid; k < rec_dw; k += NT) rec[k] = reinterpret_cast<const uint32_t *>(S)[k];
        }
        __syncthreads();  // the next env's record overwrites S
    }
#undef WW_SET_COUNTS
