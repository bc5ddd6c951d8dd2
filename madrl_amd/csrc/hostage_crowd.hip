// hostage_crowd.hip -- ContinuousHostageWorld for envs beyond one wavefront's worth of particles (gfx950 / CDNA4), float32: hw_crowd_kernel,
// one workgroup of NW wavefronts per env.  The scheme (phases, sensing passes, the ordered reach walk) and the code it shares with
// ww_crowd_kernel are in particle_crowd.hpp; this file is the oracle's hw_step_env in its order.  Limits:
//   n_good <= 128            a thread owns at most one rescuer
//   n_hostages <= 64         the saved mask is one 64-bit word in the record, in get_state and in the oracle (64 itself works: "all saved" is ~0)
//   at most 1 023 particles, n_sensors in 1..256, n_coop_save >= 1
// The record is the one hostage_kernel reads and writes (the two kernels are interchangeable on one state buffer).
//
// LDS (dynamic, hw_crowd_lds_bytes; about 35 KB at the limits, 2 KB at 20 / 30 / 40):
//   S     the packed state record  X[NP][2] | V[NP][2] | key[2] | bomb[2] | saved_lo saved_hi | flags | t | tick     (<= 16 KB)
//   SEN   sensor unit vectors [K][2]
//   ACT   the scaled actions [Nr][2]: the global control penalty sums them row-major
//   COL   collision bits, per rescuer one 64-bit word for the hostages and one per chunk of 64 criminals   (<= 14 KB)
//   CAU / ENC   ho_caught | cr_caught bits per chunk / ho_enc bits;  KEB / BOB   key / bomb contact bit per rescuer
// The observation row is NOT staged.  Reference lines (:n) are hostage.py's, as in hostage.hip.  What the processing of :365-383 decides
// (saved mask, gate, bombed, done) is known after B2, before anything reads it.
#include "particle_crowd.hpp"
#include "hostage_dev.hpp"

// wavefronts per workgroup (a profiling variant builds the other value: scripts/hostage_crowd_time.py)
#ifndef MADRL_HWC_NW
#define MADRL_HWC_NW 4
#endif

namespace {

using namespace madrl;

// MODE 0: reset(mask)   MODE 1: step (+ fused auto-reset)
template <int MODE, int NW>
__global__ __launch_bounds__(64 * NW) void hw_crowd_kernel(const HwDev d, const HwIO io) {
    static_assert(NW >= 2 && NW <= 16, "a thread owns at most one rescuer (n_good <= 128)");
    constexpr int NT = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float smem_hw_crowd[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Nr = d.Nr, Nh = d.Nh, Nc = d.Nc, NP = d.NP, K = d.K, D = d.D, rec_dw = d.rec_dw;
    const int WC = (Nc + 63) >> 6, W = 1 + WC;  // 64-bit words per collision row: the hostages | criminal chunks
    // ---- LDS carve (every float part a multiple of 4 dwords)
    float *S = smem_hw_crowd;
    float *X = S, *V = S + 2 * NP;
    uint32_t *SU = reinterpret_cast<uint32_t *>(S);
    const int OFF_KEY = 4 * NP, OFF_BOMB = 4 * NP + 2, OFF_SAVED = 4 * NP + 4, OFF_FLAGS = 4 * NP + 6, OFF_T = 4 * NP + 7, OFF_TICK = 4 * NP + 8;
    float *SEN = S + up4(rec_dw);
    float *ACT = SEN + up4(2 * K);
    uint64_t *COL = reinterpret_cast<uint64_t *>(ACT + up4(2 * Nr));  // [Nr][W]
    uint64_t *CAU = COL + Nr * W;                                     // [W]  caught hostages | caught criminals
    uint64_t *ENC = CAU + W;                                          // [1]  hostages touched by at least one rescuer
    uint64_t *KEB = ENC + 1;                                          // [2]  rescuers in contact with the key (bit = rescuer index)
    uint64_t *BOB = KEB + 2;                                          // [2]  ... with the bomb

    for (int k = tid; k < 2 * K; k += NT) SEN[k] = d.sensors[k];

    const PassShape passes = pass_shape(K, Nr, lane);
    const float srange = d.sensor_range, rad2 = d.radius * d.radius;  // G1: the SENSING rescuer's radius
    const float reach2 = sensor_reach2(rad2, srange);
    const int limit = d.max_steps > 0 ? d.max_steps : 1000;  // timestep_limit :118-120
    const uint64_t all_h = Nh >= 64 ? ~0ull : ((1ull << Nh) - 1ull);
    const int n_envs = (int)d.n_envs;

    for (int e32 = blockIdx.x; e32 < n_envs; e32 += (int)gridDim.x) {  // env indices are 32-bit (n_envs < 2^31 - grid), byte offsets 64-bit
        const int64_t env = e32;
        if (MODE == 0 && io.mask != nullptr && io.mask[env] == 0) continue;  // workgroup-uniform
        uint32_t *const rec = reinterpret_cast<uint32_t *>(d.state) + env * (int64_t)rec_dw;
        for (int k = tid; k < rec_dw; k += NT) SU[k] = rec[k];
        __syncthreads();
        // every thread holds its own copy of the env's scalars
        int32_t tstep = (int32_t)SU[OFF_T];
        uint32_t tick = SU[OFF_TICK];
        uint32_t flags = SU[OFF_FLAGS];  // bit0 gate_open, bit1 bombed, bit2 key sampled
        uint64_t saved = (uint64_t)SU[OFF_SAVED] | ((uint64_t)SU[OFF_SAVED + 1] << 32);
        const uint32_t gid = d.gid_base + (uint32_t)env;
        float *const orow_env = io.obs + env * (int64_t)Nr * D;

        bool do_init = (MODE == 0);
        int npass = 1;
        for (int pass = 0; pass < npass; ++pass) {
            if (do_init) {
                // ------------------------------------------------ reset (:137-177); draw index: key 0, particle j -> 1 + j, bomb 1 + NP
                tstep = 0;
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
                    drive_agent(live, io.actions, env * Nr + i, d.action_scale, ACT, i, x, y, vx, vy);  // :231, :236-238, walls :247-252
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
                    io.rew[env * Nr + i] = reward;
                }
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
                        const float *r = io.inj_resp + (env * Nc + m) * 4;
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
        for (int k = tid; k < rec_dw; k += NT) rec[k] = SU[k];
        __syncthreads();  // the next env's record overwrites S
    }
}

}  // namespace

namespace madrl {

size_t hw_crowd_lds_bytes(int Nr, int Nh, int Nc, int K, int rec_dw) {
    (void)Nh;  // at most 64: one word per rescuer
    const size_t W = 1 + ((size_t)Nc + 63) / 64;
    return ((size_t)up4(rec_dw) + up4(2 * K) + up4(2 * Nr)) * 4 + ((size_t)Nr * W + W + 1 + 2 + 2) * 8;
}

int hw_crowd_launch(const void *dev, const void *io, int mode, int64_t max_blocks, size_t lds_bytes, void *stream) {
    return crowd_launch<HwDev, HwIO>(mode == 0 ? hw_crowd_kernel<0, MADRL_HWC_NW> : hw_crowd_kernel<1, MADRL_HWC_NW>, MADRL_HWC_NW, dev, io,
                                     max_blocks, lds_bytes, stream);
}

}  // namespace madrl
