// hostage_crowd_body.inc -- the body of hw_crowd_kernel<MODE, NW> and hw_crowd_kernel_live<MODE, NW> (hostage_crowd.hip), included inside
// both __global__ entries like waterworld_crowd_body.inc: the fixed-shape entry keeps its two arguments and its code.  In scope: MODE, NW,
// d (HwDev), io (HwIO), `constexpr bool LIVE` and, when LIVE, cn (ParticleCounts).
    static_assert(NW >= 2 && NW <= 16, "a thread owns at most one rescuer (n_good <= 128)");
    constexpr int NT = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float smem_hw_crowd[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Rc = d.Nr, Hc = d.Nh, Cc = d.Nc, NPc = d.NP;  // the strides and slots of everything host-facing (LIVE: the capacity)
    const int K = d.K, D = d.D, rec_dw = d.rec_dw;
    int Nr = Rc, Nh = Hc, Nc = Cc, NP = NPc;                // the counts the phases run on (LIVE: set per env)
    int WC = (Nc + 63) >> 6, W = 1 + WC;  // 64-bit words per collision row: the hostages | criminal chunks
    // ---- LDS carve (every float part a multiple of 4 dwords)
    float *S = smem_hw_crowd;
    float *X = S, *V = S + 2 * NPc;
    uint32_t *SU = reinterpret_cast<uint32_t *>(S);
    const int OFF_KEY = 4 * NPc, OFF_BOMB = 4 * NPc + 2, OFF_SAVED = 4 * NPc + 4, OFF_FLAGS = 4 * NPc + 6, OFF_T = 4 * NPc + 7, OFF_TICK = 4 * NPc + 8;
    float *SEN = S + up4(rec_dw);
    float *ACT = SEN + up4(2 * K);
    uint64_t *COL = reinterpret_cast<uint64_t *>(ACT + up4(2 * Nr));  // [Nr][W]
    uint64_t *CAU = COL + Nr * W;                                     // [W]  caught hostages | caught criminals
    uint64_t *ENC = CAU + W;                                          // [1]  hostages touched by at least one rescuer
    uint64_t *KEB = ENC + 1;                                          // [2]  rescuers in contact with the key (bit = rescuer index)
    uint64_t *BOB = KEB + 2;                                          // [2]  ... with the bomb

    for (int k = tid; k < 2 * K; k += NT) SEN[k] = d.sensors[k];

    PassShape passes = pass_shape(K, Nr, lane);
    const float srange = d.sensor_range, rad2 = d.radius * d.radius;  // G1: the SENSING rescuer's radius
    const float reach2 = sensor_reach2(rad2, srange);
    const int limit = d.max_steps > 0 ? d.max_steps : 1000;  // timestep_limit :118-120
    uint64_t all_h = Nh >= 64 ? ~0ull : ((1ull << Nh) - 1ull);
    // LIVE: an env's counts and what follows from them (a macro: DESIGN.md 4.4b says why)
#define HW_SET_COUNTS(src) \
    do { \
        const int32_t *c_ = (src) + 3 * env; \
        Nr = clampi(c_[0], 1, Rc); Nh = clampi(c_[1], 1, Hc); Nc = clampi(c_[2], 1, Cc); NP = Nr + Nh + Nc; \
        WC = (Nc + 63) >> 6; W = 1 + WC; \
        all_h = Nh >= 64 ? ~0ull : ((1ull << Nh) - 1ull); \
        passes = pass_shape(K, Nr, lane); \
    } while (0)
    const int n_envs = (int)d.n_envs;

    for (int e32 = blockIdx.x; e32 < n_envs; e32 += (int)gridDim.x) {  // env indices are 32-bit (n_envs < 2^31 - grid), byte offsets 64-bit
        const int64_t env = e32;
        if (MODE == 0 && io.mask != nullptr && io.mask[env] == 0) continue;  // workgroup-uniform
        uint32_t *const rec = reinterpret_cast<uint32_t *>(d.state) + env * (int64_t)rec_dw;
        if constexpr (LIVE) {  // the slotted record -> packed arrays of the env's live counts
            HW_SET_COUNTS(cn.live);
            for (int j = tid; j < NP; j += NT) {
                const int s = j < Nr ? j : (j < Nr + Nh ? Rc + (j - Nr) : Rc + Hc + (j - Nr - Nh));  // packed index -> slot
                reinterpret_cast<uint2 *>(X)[j] = reinterpret_cast<const uint2 *>(rec)[s];
                reinterpret_cast<uint2 *>(V)[j] = reinterpret_cast<const uint2 *>(rec)[NPc + s];
            }
            if (tid < 9) SU[OFF_KEY + tid] = rec[OFF_KEY + tid];  // key[2] | bomb[2] | saved_lo saved_hi | flags | t | tick
        } else {
            for (int k = tid; k < rec_dw; k += NT) SU[k] = rec[k];
        }
        __syncthreads();
        // every thread holds its own copy of the env's scalars
        int32_t tstep = (int32_t)SU[OFF_T];
        uint32_t tick = SU[OFF_TICK];
        uint32_t flags = SU[OFF_FLAGS];  // bit0 gate_open, bit1 bombed, bit2 key sampled
        uint64_t saved = (uint64_t)SU[OFF_SAVED] | ((uint64_t)SU[OFF_SAVED + 1] << 32);
        const uint32_t gid = d.gid_base + (uint32_t)env;
        float *const orow_env = io.obs + env * (int64_t)Rc * D;

        bool do_init = (MODE == 0);
        int npass = 1;
        for (int pass = 0; pass < npass; ++pass) {
            if (do_init) {
                // ------------------------------------------------ reset (:137-177); draw index: key 0, particle j -> 1 + j, bomb 1 + NP
                tstep = 0;
                if constexpr (LIVE) {  // a reset takes the env's pending counts, before its draws
                    HW_SET_COUNTS(cn.pending);
                    if (tid < 3) cn.live[3 * env + tid] = tid == 0 ? Nr : (tid == 1 ? Nh : Nc);
                }
                for (int j = tid; j < NP + 2; j += NT) {
                    const uint32_t di = j < NP ? 1u + (uint32_t)j : (j == NP ? 0u : 1u + (uint32_t)NP);
                    const u32x4 r = philox4x32_10(gid, tick, di, HW_TAG_RESET, d.k0, d.k1);
                    const float u0 = u24(r.x), u1 = u24(r.y), u2 = u24(r.z), u3 = u24(r.w);
                    if (j < Nr) {  // :149-153
                        X[2 * j] = u0; X[2 * j + 1] = u1 < 0.55f ? 0.55f : (u1 > 0.95f ? 0.95f : u1);
                        V[2 * j] = 0.f; V[2 * j + 1] = 0.f;
                    } else if (j < Nr + Nh) {  // :156-160
                        const float hi = 0.35f + u2 * 0.01f;
                        X[2 * j] = u0; X[2 * j + 1] = u1 < 0.f ? 0.f : (u1 > hi ? hi : u1);
                        V[2 * j] = 0.f; V[2 * j + 1] = 0.f;
                    } else if (j < NP) {  // :165-168 (velocity not centred here)
                        X[2 * j] = u0; X[2 * j + 1] = u1;
                        V[2 * j] = u2 * d.bad_speed; V[2 * j + 1] = u3 * d.bad_speed;
                    } else if (j == NP) {  // key: the first reset of the env's life only (G2, :143-146)
                        if (!(flags & 4u)) {
                            S[OFF_KEY] = d.key_fixed ? d.key_x : 1.f - u0 * 0.1f;
                            S[OFF_KEY + 1] = d.key_fixed ? d.key_y : 1.f - u1 * 0.1f;
                        }
                    } else {  // bomb :171
                        S[OFF_BOMB] = u0 < 0.f ? 0.f : (u0 > 0.25f ? 0.25f : u0);
                        S[OFF_BOMB + 1] = u1 < 0.f ? 0.f : (u1 > 0.25f ? 0.25f : u1);
                    }
                }
                saved = 0ull;
                flags = 4u;
                tick += 1;
                __syncthreads();
            }
            // ---------------------------------------------------- step (:228-430); a reset ends with step(zeros) (:173)
            const bool live = MODE == 1 && !do_init;  // a step the caller asked for: actions in, rewards / done / info out
            const float kx = S[OFF_KEY], ky = S[OFF_KEY + 1], bx = S[OFF_BOMB], by = S[OFF_BOMB + 1];
            const bool gate0 = flags & 1u;     // gate state and saved mask before this step's processing (G5)
            const uint64_t saved0 = saved;
            // phase A: rescuers (:231-260), key / bomb contact (:281-291)
            {
                bool col_bo = false, col_ke = false;
                if (tid < Nr) {
                    const int i = tid;
                    float x = X[2 * i], y = X[2 * i + 1], vx = V[2 * i], vy = V[2 * i + 1];
                    drive_agent(live, io.actions, env * Rc + i, d.action_scale, ACT, i, x, y, vx, vy);  // :231, :236-238, walls :247-252
                    if (!gate0) {  // G3: both coordinates, velocity component flipped (:255-260)
                        const float cx = x < d.gate_lo ? d.gate_lo : (x > 1.f ? 1.f : x);
                        const float cy = y < d.gate_lo ? d.gate_lo : (y > 1.f ? 1.f : y);
                        if (x != cx) vx *= -1.f;
                        if (y != cy) vy *= -1.f;
                        x = cx; y = cy;
                    }
                    X[2 * i] = x; X[2 * i + 1] = y; V[2 * i] = vx; V[2 * i + 1] = vy;
                    col_bo = dist2_le(x, y, bx, by, d.sq_bomb);  // dist <= radius + bomb_radius
                    col_ke = dist2_le(x, y, kx, ky, d.sq_key);   // dist <= radius + key_radius
                }
                if (wave < 2) {  // the rescuers are the threads of the first two wavefronts
                    const uint64_t kb = __ballot(col_ke), bb = __ballot(col_bo);
                    if (lane == 0) { KEB[wave] = kb; BOB[wave] = bb; }
                }
            }
            __syncthreads();
            // phase B1: collisions (:263-279), saved hostages included (G4)
            contact_ballots<NW>(X, COL, Nr, W, 1, {Nr, Nh, d.sq_hit_ho}, {Nr + Nh, Nc, d.sq_hit_cr}, wave, lane);
            __syncthreads();
            // phase B2: _caught (:184-198)
            column_counts<NW>(COL, CAU, ENC, Nr, W, 1, d.n_coop_save, wave, lane);
            __syncthreads();
            // what the processing of :365-383 will decide
            const uint64_t ho_caught = CAU[0];
            const int n_ho_caught = __popcll(ho_caught), n_ho_enc = __popcll(ENC[0]);
            int n_cr_caught = 0;
            for (int c = 1; c < W; ++c) n_cr_caught += __popcll(CAU[c]);
            saved |= ho_caught;
            if ((BOB[0] | BOB[1]) != 0ull) flags |= 2u;
            if ((KEB[0] | KEB[1]) != 0ull) flags |= 1u;
            const float gate1 = (flags & 1u) ? 1.f : 0.f, bombed1 = (flags & 2u) ? 1.f : 0.f;  // states after processing (G6)
            const bool is_done = (flags & 2u) || ((saved & all_h) == all_h) || tstep + 1 >= limit;  // :179-182, with t after :427
            // a step that ends the episode under auto_reset is followed by the reset pass, whose observations replace this one's -- sensing
            // changes no state, so it is left out of such a step
            const bool emit = !(live && d.auto_reset && is_done);
            // rescuer threads: contact flags, gate state and id of the observation row (:410-425), the reward (:241-244, :385-396, :429-430)
            if (tid < Nr) {
                const int i = tid;
                bool t_ho = false, t_cr = false, w_ho = false, w_enc = false, w_cr = false;
                {
                    const uint64_t row = COL[i * W];
                    t_ho = row != 0ull;
                    w_ho = (row & ho_caught) != 0ull;   // touches a caught hostage
                    w_enc = (row & ENC[0]) != 0ull;     // touches an encountered hostage
                }
                for (int c = 1; c < W; ++c) {
                    const uint64_t row = COL[i * W + c];
                    t_cr |= row != 0ull;
                    w_cr |= (row & CAU[c]) != 0ull;     // touches a caught criminal
                }
                const bool col_ke = (KEB[i >> 6] >> (i & 63)) & 1ull, col_bo = (BOB[i >> 6] >> (i & 63)) & 1ull;
                if (emit) {
                    float *o = orow_env + (int64_t)i * D + 5 * K;
                    o[0] = t_ho ? 1.f : 0.f; o[1] = t_cr ? 1.f : 0.f; o[2] = col_ke ? 1.f : 0.f; o[3] = col_bo ? 1.f : 0.f;
                    o[4] = gate1;
                    if (d.addid) o[5] = (float)(i + 1);
                }
                if (live) {
                    float reward;
                    if (d.reward_global) {  // (actions**2).sum(), row-major (:241-242)
                        const float s = control_sum(ACT, Nr);
                        reward = 0.0f + d.control_penalty * s;
                        reward += ((((float)n_ho_enc * d.encounter_reward) * gate1 + (float)n_ho_caught * d.save_reward) +
                                   (float)n_cr_caught * d.hit_reward) + bombed1 * d.bomb_reward;
                    } else {  // fancy-index += pays a rescuer once per kind (G9)
                        const float a0 = ACT[2 * i], a1 = ACT[2 * i + 1];
                        reward = 0.0f + d.control_penalty * (a0 * a0 + a1 * a1);
                        if (w_ho) reward += d.save_reward;
                        if (w_enc) reward += d.encounter_reward * gate1;
                        if (w_cr) reward += d.hit_reward;
                        if (col_bo) reward += bombed1 * d.bomb_reward;
                    }
                    if (is_done) reward += (float)(Nh - __popcll(saved & all_h)) * d.not_saved_reward;  // :429-430
                    io.rew[env * Rc + i] = reward;
                }
            }
            if constexpr (LIVE) {  // the rows of the rescuers that do not exist: +0.0
                if (live && tid >= Nr && tid < Rc) io.rew[env * Rc + tid] = 0.f;
                if (emit)
                    for (int k = Nr * D + tid; k < Rc * D; k += NT) orow_env[k] = 0.f;
            }
            // phase C: sensing (:295-362).  Rows: [criminal dist | criminal speed | hostage dist | key dist | bomb dist] (:398-400)
            if (emit) {
                for (int p = wave; p < passes.n_pass; p += NW) {
                    const PassLanes L = pass_lanes(passes, p, K, Nr, lane);  // the rescuers of this pass
                    Ray ray(SEN, X, V, L.iq, L.kq, srange, rad2);
                    float *const o = orow_env + (int64_t)L.iq * D + L.kq;
                    auto visit = [&](int m, float qx, float qy) { ray.visit(m, qx, qy); };
                    reach_walk(X, Nr + Nh, Nc, L, reach2, 0ull, lane, visit);  // criminals
                    {
                        const bool fin = ray.b < INFINITY;
                        const int j = Nr + Nh + ray.bi;  // (bi = 0 without a hit: a valid particle, its value is not used)
                        const float raw = ray.speed_along(V, j);  // :204-226
                        if (L.okq) {
                            o[0] = fin ? ray.b : 0.f;
                            o[K] = fin ? raw : 0.f;
                        }
                    }
                    ray.restart();
                    // hostages: the saved ones (mask from before this step, G5, :296) are not sensed.  (gate0 is workgroup-uniform: behind
                    // the closed gate the feature is 0 whatever is sensed, :320-322)
                    if (gate0) reach_walk(X, Nr, Nh, L, reach2, saved0, lane, visit);
                    if (L.okq) o[2 * K] = (gate0 && ray.b < INFINITY) ? ray.b : 0.f;
                    ray.restart();
                    if (!gate0) ray.visit(0, kx, ky);   // :338-340
                    if (L.okq) o[3 * K] = (!gate0 && ray.b < INFINITY) ? ray.b : 0.f;
                    ray.restart();
                    ray.visit(0, bx, by);
                    if (L.okq) o[4 * K] = (ray.b < INFINITY) ? ray.b : 0.f;
                }
            }
            __syncthreads();  // sensing read the positions of this step: respawn and motion come after it
            // phase E: respawn caught criminals (:371-374), then criminals move (G7, :402-408)
            for (int m = tid; m < Nc; m += NT) {
                const int j = Nr + Nh + m;
                float x = X[2 * j], y = X[2 * j + 1], vx = V[2 * j], vy = V[2 * j + 1];
                if ((CAU[1 + (m >> 6)] >> (m & 63)) & 1ull) {
                    float u0, u1;
                    if (MODE == 1 && io.inj_resp != nullptr && !do_init) {
                        const float *r = io.inj_resp + (env * Cc + m) * 4;  // (LIVE: criminal m's row at the capacity's stride)
                        x = r[0]; y = r[1]; u0 = r[2]; u1 = r[3];
                    } else {  // the same draw per (env, tick, criminal) as the one-wavefront kernel
                        const u32x4 r = philox4x32_10(gid, tick, (uint32_t)m, HW_TAG_RESPAWN, d.k0, d.k1);
                        x = u24(r.x); y = u24(r.y); u0 = u24(r.z); u1 = u24(r.w);
                    }
                    vx = (u0 - 0.5f) * d.bad_speed;
                    vy = (u1 - 0.5f) * d.bad_speed;
                }
                free_motion(x, y, vx, vy);
                X[2 * j] = x; X[2 * j + 1] = y; V[2 * j] = vx; V[2 * j + 1] = vy;
            }
            tick += 1;
            tstep += 1;  // :427
            if (tid == 0 && live) {
                io.done[env] = (uint8_t)is_done;
                io.info[2 * env] = n_ho_caught;
                io.info[2 * env + 1] = n_cr_caught;
            }
            if (live && is_done && d.auto_reset) {  // workgroup-uniform: run the reset pass next
                npass = 2;
                do_init = true;
            }
            __syncthreads();
        }
        // ---------------------------------------------------------- LDS -> record
        if (tid == 0) {
            SU[OFF_SAVED] = (uint32_t)saved; SU[OFF_SAVED + 1] = (uint32_t)(saved >> 32);
            SU[OFF_FLAGS] = flags;  // (bit 2 is kept)
            SU[OFF_T] = (uint32_t)tstep;
            SU[OFF_TICK] = tick;
        }
        __syncthreads();
        if constexpr (LIVE) {  // packed arrays -> the slotted record
            for (int s = tid; s < NPc; s += NT) {
                const int m = s < Rc ? s : (s < Rc + Hc ? s - Rc : s - Rc - Hc);           // index within the class
                const int lo = s < Rc ? 0 : (s < Rc + Hc ? Nr : Nr + Nh);                   // where the class starts in the packed arrays
                const bool is = m < (s < Rc ? Nr : (s < Rc + Hc ? Nh : Nc));
                const int j = lo + (is ? m : 0);
                const uint2 x = reinterpret_cast<const uint2 *>(X)[j], v = reinterpret_cast<const uint2 *>(V)[j];
                const uint32_t gone = __float_as_uint(-1.0f);
                reinterpret_cast<uint2 *>(rec)[s] = is ? x : make_uint2(gone, gone);
                reinterpret_cast<uint2 *>(rec)[NPc + s] = is ? v : make_uint2(0u, 0u);
            }
            if (tid < 9) rec[OFF_KEY + tid] = SU[OFF_KEY + tid];
        } else {
            for (int k = tid; k < rec_dw; k += NT) rec[k] = SU[k];
        }
        __syncthreads();  // the next env's record overwrites S
    }
#undef HW_SET_COUNTS
