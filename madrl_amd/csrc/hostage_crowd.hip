// hostage_crowd.hip -- ContinuousHostageWorld for envs beyond one wavefront's worth of particles (gfx950 / CDNA4), float32.
//
// hostage_kernel (hostage.hip) gives every particle a lane of ONE wavefront: at most 61 particles, 32 rescuers.  Here one WORKGROUP of NW
// wavefronts owns an env at a time (persistent, striding over the envs) and its threads loop over the particles, the scheme of
// ww_crowd_kernel (waterworld_crowd.hip).  Reached on request only (madrl_hostage_config.crowd = 1).  Limits:
//   n_good <= 128            a thread owns at most one rescuer
//   n_hostages <= 64         the saved mask is one 64-bit word in the record, in get_state and in the oracle (64 itself works: "all saved" is ~0)
//   at most 1 023 particles, n_sensors in 1..256, n_coop_save >= 1
// The record is the one hostage_kernel reads and writes (the two kernels are interchangeable on one state buffer), and the results are
// those of that kernel and of the float32 C restatement of the reference the tests use ("the oracle") bit for bit: every float expression
// keeps the oracle's statement order, and whatever the oracle does in a loop whose order matters is done in that order here.
//
// LDS (dynamic, hw_crowd_lds_bytes; about 35 KB at the limits, 2 KB at 20 / 30 / 40):
//   S     the packed state record  X[NP][2] | V[NP][2] | key[2] | bomb[2] | saved_lo saved_hi | flags | t | tick     (<= 16 KB)
//   SEN   sensor unit vectors [K][2]
//   ACT   the scaled actions [Nr][2]: the global control penalty sums them row-major
//   COL   collision bits, per rescuer one 64-bit word for the hostages and one per chunk of 64 criminals   (<= 14 KB)
//   CAU / ENC   ho_caught | cr_caught bits per chunk / ho_enc bits;  KEB / BOB   key / bomb contact bit per rescuer
// The observation row is NOT staged: a (rescuer, sensor) lane stores its five features straight to global memory; for a fixed rescuer and
// feature the K sensor values are contiguous, so the lanes of a rescuer write whole runs.
//
// Phases of a step, a workgroup barrier between them, in the order of the oracle's hw_step_env (reference lines: hostage.py, as in hostage.hip):
//   A   thread = rescuer: actions, integration, walls, closed gate (G3), key / bomb contact                :231-260, :281-291
//   B1  wavefront = (rescuer, chunk of 64 objects), lane = object: contact test, ballot -> COL             :263-279 (G4: no saved mask)
//   B2  wavefront = chunk, lane = object: column count over the rescuers -> CAU / ENC                     _caught :184-198
//       thread = rescuer: contact flags, gate state and id of the observation row, the reward (G6, G9)    :385-396, :410-430
//   C   wavefront = pass of (rescuer, sensor) lanes: ray tests, features to global (G1, G5)               :295-362, :398-400
//   E   thread = criminal: respawn if caught, then motion (G7)                                            :365-383, :402-408
// What the processing of :365-383 decides (saved mask, gate, bombed, done) is known after B2, before anything reads it.  Sensing is the
// bulk.  A pass holds floor(64 / K) whole rescuers (K > 64: 64 sensors of one rescuer).  Per class and chunk of 64 objects the lanes test
// which objects are within reach of a rescuer of the pass (the conservative predicate of hostage.hip), one ballot makes that a
// wave-uniform mask, and its set bits are walked in ascending order -- the oracle's index order, so the running minimum with a strict `<`
// is the oracle's first minimum.  The objects out of reach would yield +inf and are skipped.  Key and bomb are single objects.
//
// Known costs, as in ww_crowd_kernel: the next env's record is not fetched ahead, and the launch parameters are held in registers across
// the env loop instead of being read through kernargs<>() where a phase needs them.
#include "hostage_dev.hpp"

#include <math.h>

// wavefronts per workgroup (a profiling variant builds the other value: scripts/hostage_crowd_time.py)
#ifndef MADRL_HWC_NW
#define MADRL_HWC_NW 4
#endif

namespace {

using namespace madrl;

__host__ __device__ inline int up4(int v) { return (v + 3) & ~3; }

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

    // the lanes of a sensing pass: PPP whole rescuers of K sensors (K <= 64), or one chunk of 64 sensors of one rescuer
    const int PPP = K <= 64 ? 64 / K : 1, KC = K <= 64 ? 1 : (K + 63) >> 6;
    const int li = K <= 64 ? lane / K : 0;
    const int n_pass = ((Nr + PPP - 1) / PPP) * KC;
    const float srange = d.sensor_range, rad2 = d.radius * d.radius;  // G1: the SENSING rescuer's radius
    // a sensor of rescuer i can only return a finite value for an object with d2 <= rad2 + sv^2 <= rad2 + range^2 (plus a relative margin
    // far above the rounding of the test itself): everything else yields +inf in the oracle and never becomes a minimum
    const float reach2 = (rad2 + srange * srange) * 1.0001f + 1e-9f;
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
                    float r0 = 0.0f, r1 = 0.0f;
                    if (live) {
                        const float *a = io.actions + (env * Nr + i) * 2;
                        r0 = a[0];
                        r1 = a[1];
                    }
                    const float a0 = r0 * d.action_scale, a1 = r1 * d.action_scale;  // :231
                    ACT[2 * i] = a0;
                    ACT[2 * i + 1] = a1;
                    float x = X[2 * i], y = X[2 * i + 1], vx = V[2 * i], vy = V[2 * i + 1];
                    vx = vx + a0; vy = vy + a1;  // :236-238
                    x = x + vx; y = y + vy;
                    float cx = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);  // walls :247-252
                    float cy = y < 0.f ? 0.f : (y > 1.f ? 1.f : y);
                    if (x != cx) vx = 0.f;
                    if (y != cy) vy = 0.f;
                    x = cx; y = cy;
                    if (!gate0) {  // G3: both coordinates, velocity component flipped (:255-260)
                        cx = x < d.gate_lo ? d.gate_lo : (x > 1.f ? 1.f : x);
                        cy = y < d.gate_lo ? d.gate_lo : (y > 1.f ? 1.f : y);
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
            // phase B1: collisions (:263-279), saved hostages included (G4).  Bits past the end of a class stay 0.
            for (int i = wave; i < Nr; i += NW) {
                const float pix = X[2 * i], piy = X[2 * i + 1];
                for (int c = 0; c < W; ++c) {
                    const bool is_ho = c == 0;
                    const int m = (is_ho ? 0 : c - 1) * 64 + lane;
                    const bool in = m < (is_ho ? Nh : Nc);
                    const int j = (is_ho ? Nr : Nr + Nh) + (in ? m : 0);
                    const uint64_t hit = __ballot(in && dist2_le(pix, piy, X[2 * j], X[2 * j + 1], is_ho ? d.sq_hit_ho : d.sq_hit_cr));
                    if (lane == 0) COL[i * W + c] = hit;
                }
            }
            __syncthreads();
            // phase B2: _caught (:184-198): an object counts its column
            for (int c = wave; c < W; c += NW) {
                int s = 0;
                for (int i = 0; i < Nr; ++i) s += (int)((COL[i * W + c] >> lane) & 1ull);
                const uint64_t cm = __ballot(s >= (c == 0 ? d.n_coop_save : 1));
                const uint64_t em = __ballot(s >= 1);
                if (lane == 0) {
                    CAU[c] = cm;
                    if (c == 0) ENC[0] = em;
                }
            }
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
                    if (d.reward_global) {  // (actions**2).sum(), row-major (:241-242): summed in that order, not as a tree
                        float s = 0.0f;
                        for (int q = 0; q < Nr; ++q) {
                            const float b0 = ACT[2 * q], b1 = ACT[2 * q + 1];
                            s += b0 * b0;
                            s += b1 * b1;
                        }
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
                for (int p = wave; p < n_pass; p += NW) {
                    const int ig = KC == 1 ? p : p / KC, kc = p - ig * KC;
                    const int i_first = ig * PPP, i_cnt = min(PPP, Nr - i_first);  // the rescuers of this pass
                    const int k0 = K <= 64 ? lane - li * K : kc * 64 + lane;
                    const bool okq = li < i_cnt && k0 < K;   // lanes without a (rescuer, sensor) pair compute along and store nothing
                    const int iq = i_first + (okq ? li : 0), kq = okq ? k0 : 0;
                    const float sxq = SEN[2 * kq], syq = SEN[2 * kq + 1];
                    const float pxq = X[2 * iq], pyq = X[2 * iq + 1], pvx = V[2 * iq], pvy = V[2 * iq + 1];
                    float *const o = orow_env + (int64_t)iq * D + kq;
                    float b = INFINITY;
                    int bi = 0;  // the first minimum of an all-inf row is 0
                    auto visit = [&](int m, float qx, float qy) {
                        const float rx = qx - pxq, ry = qy - pyq;
                        const float sv = sxq * rx + syq * ry;  // sensors.dot(relpos.T) :67
                        const float d2 = rx * rx + ry * ry;
                        // sv < 0 || sv > srange as ONE compare: the median of (sv, 0, srange) is sv exactly when 0 <= sv <= srange (hostage.hip)
                        const bool out = (__builtin_amdgcn_fmed3f(sv, 0.f, srange) != sv) | (d2 - sv * sv > rad2);
                        // an excluded ray is +inf in the reference and never "better"; a kept one is when it is smaller: first minimum
                        const bool better = !out & (sv < b);
                        b = better ? sv : b;
                        bi = better ? m : bi;
                    };
                    // cls 0: criminals; cls 1: hostages, the saved ones (mask from before this step, G5, :296) not sensed
                    auto walk = [&](int lo, int cnt, bool hostages) {
                        for (int base = 0; base < cnt; base += 64) {
                            const int m = base + lane;
                            const bool in = m < cnt;
                            const float2 mp = *reinterpret_cast<const float2 *>(&X[2 * (lo + (in ? m : 0))]);
                            bool near = false;
                            for (int q = 0; q < i_cnt; ++q) {
                                const float2 pp = *reinterpret_cast<const float2 *>(&X[2 * (i_first + q)]);
                                const float rx = mp.x - pp.x, ry = mp.y - pp.y;
                                near |= rx * rx + ry * ry <= reach2;
                            }
                            uint64_t todo = __ballot(in && near);  // wave-uniform: the objects of this chunk within reach of the pass
                            if (hostages) todo &= ~saved0;
#pragma nounroll
                            while (todo != 0ull) {
                                const int m2 = base + __builtin_ctzll(todo);
                                todo &= todo - 1ull;
                                const float2 qp = *reinterpret_cast<const float2 *>(&X[2 * (lo + m2)]);  // uniform address: a broadcast
                                visit(m2, qp.x, qp.y);
                            }
                        }
                    };
                    walk(Nr + Nh, Nc, false);
                    {
                        const bool fin = b < INFINITY;
                        const int j = Nr + Nh + bi;  // (bi = 0 without a hit: a valid particle, its value is not used)
                        const float raw = sxq * (V[2 * j] - pvx) + syq * (V[2 * j + 1] - pvy);  // :204-226
                        if (okq) {
                            o[0] = fin ? b : 0.f;
                            o[K] = fin ? raw : 0.f;
                        }
                    }
                    b = INFINITY;
                    if (gate0) walk(Nr, Nh, true);  // (workgroup-uniform: behind the closed gate the feature is 0 whatever is sensed, :320-322)
                    if (okq) o[2 * K] = (gate0 && b < INFINITY) ? b : 0.f;
                    b = INFINITY;
                    if (!gate0) visit(0, kx, ky);   // :338-340
                    if (okq) o[3 * K] = (!gate0 && b < INFINITY) ? b : 0.f;
                    b = INFINITY;
                    visit(0, bx, by);
                    if (okq) o[4 * K] = (b < INFINITY) ? b : 0.f;
                }
            }
            __syncthreads();  // sensing read the positions of this step: respawn and motion come after it
            // phase E: respawn caught criminals (:371-374), then criminals move; the velocity flips only if BOTH coordinates left [0,1], no
            // clipping (G7, :402-408)
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
                x = x + vx; y = y + vy;
                const bool outx = !(x >= 0.f && x <= 1.f), outy = !(y >= 0.f && y <= 1.f);
                if (outx && outy) { vx = -1.0f * vx; vy = -1.0f * vy; }
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

int hw_crowd_launch(const void *dev, const void *io_, int mode, int64_t max_blocks, size_t lds_bytes, void *stream) {
    const HwDev &d = *static_cast<const HwDev *>(dev);
    const HwIO &io = *static_cast<const HwIO *>(io_);
    const dim3 g = particle_grid(max_blocks, d.n_envs), b(64 * MADRL_HWC_NW);
    if (mode == 0) hipLaunchKernelGGL((hw_crowd_kernel<0, MADRL_HWC_NW>), g, b, lds_bytes, (hipStream_t)stream, d, io);
    else hipLaunchKernelGGL((hw_crowd_kernel<1, MADRL_HWC_NW>), g, b, lds_bytes, (hipStream_t)stream, d, io);
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}

}  // namespace madrl
