// waterworld_crowd.hip -- MAWaterWorld for envs beyond one wavefront's worth of particles (gfx950 / CDNA4), float32.
//
// waterworld_kernel (waterworld.hip) gives every particle a lane of ONE wavefront: at most 62 particles, 32 pursuers.  Here one WORKGROUP
// of NW wavefronts owns an env at a time (persistent, striding over the envs) and its threads loop over the particles: up to 1 023
// particles, 128 pursuers, any sensor count.  Reached on request only (madrl_waterworld_config.crowd = 1); the results are those of the
// one-wavefront kernel and of the float32 C restatement of the reference the tests use ("the oracle") bit for bit: every float expression keeps the oracle's
// statement order, and whatever the oracle does in a loop whose order matters is done in that order here.
//
// LDS (dynamic, ww_crowd_lds_bytes; about 35 KB at the limits, 3 KB at 20 / 60 / 40):
//   S     the packed state record  X[NP][2] | V[NP][2] | obst[2] | t | tick     (<= 16 KB)
//   SEN   sensor unit vectors [K][2]
//   ACT   the scaled actions [Np][2]: the global control penalty sums them row-major
//   COL   collision bits, one 64-bit word per (pursuer, chunk of 64 evaders | chunk of 64 poisons)   (<= 15 KB)
//   CAU / ENC   caught / encountered bits per chunk
// The observation row is NOT staged (40 pursuers x 200 sensors would be 224 KB): a (pursuer, sensor) lane stores its features straight to
// global memory; for a fixed pursuer and feature the K sensor values are contiguous, so the lanes of a pursuer write whole runs.
//
// Phases of a step, a workgroup barrier between them (reference lines: waterworld.py, as in waterworld.hip):
//   A   thread = particle: actions, integration, walls, obstacle rebound                          :221-270
//   B1  wavefront = (pursuer, chunk of 64 objects), lane = object: contact test, ballot -> COL    :272-293
//   B2  wavefront = chunk, lane = object: column count over the pursuers -> CAU / ENC            _caught :180-193
//   C   wavefront = pass of (pursuer, sensor) lanes: ray tests, features to global                :295-353, :389-428
//       thread = pursuer: collision flags, id, reward                                              :376-385, :411-428
//   E   thread = evader / poison: respawn if caught, then motion                                  :355-374, :397-409
// Sensing is the bulk (Np * K * NP ray tests).  A pass holds floor(64 / K) whole pursuers (K > 64: 64 sensors of one pursuer).  Per class
// and chunk of 64 objects the lanes test which objects are within reach of a pursuer of the pass (the conservative predicate of
// waterworld.hip), one ballot makes that a wave-uniform mask, and its set bits are walked in ascending order -- the oracle's index order,
// so the running minimum with a strict `<` is np.argmin's first minimum.  The objects out of reach would yield +inf and are skipped.
#include "waterworld_dev.hpp"

#include <math.h>

// wavefronts per workgroup (a profiling variant builds the other value: scripts/ww_crowd_time.py)
#ifndef MADRL_WWC_NW
#define MADRL_WWC_NW 4
#endif

namespace {

using namespace madrl;

__host__ __device__ inline int up4(int v) { return (v + 3) & ~3; }

// MODE 0: reset(mask)   MODE 1: step (+ fused auto-reset)
template <int MODE, int NW>
__global__ __launch_bounds__(64 * NW) void ww_crowd_kernel(const WwDev d, const WwIO io) {
    static_assert(NW >= 2 && NW <= 16, "a thread owns at most one pursuer (n_pursuers <= 128)");
    constexpr int NT = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float smem_crowd[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Np = d.Np, Ne = d.Ne, Npo = d.Npo, NP = d.NP, K = d.K, D = d.D, rec_dw = d.rec_dw;
    const int WE = (Ne + 63) >> 6, WP = (Npo + 63) >> 6, W = WE + WP;  // 64-bit words per collision row: evader chunks | poison chunks
    // ---- LDS carve (every part a multiple of 4 dwords)
    float *S = smem_crowd;
    float *X = S, *V = S + 2 * NP, *OB = S + 4 * NP;
    float *SEN = S + up4(rec_dw);
    float *ACT = SEN + up4(2 * K);
    uint64_t *COL = reinterpret_cast<uint64_t *>(ACT + up4(2 * Np));  // [Np][W]
    uint64_t *CAU = COL + Np * W;                                     // [W]   caught evaders | caught poisons
    uint64_t *ENC = CAU + W;                                          // [WE]  evaders touched by at least one pursuer

    for (int k = tid; k < 2 * K; k += NT) SEN[k] = d.sensors[k];

    // the lanes of a sensing pass: PPP whole pursuers of K sensors (K <= 64), or one chunk of 64 sensors of one pursuer
    const int PPP = K <= 64 ? 64 / K : 1, KC = K <= 64 ? 1 : (K + 63) >> 6;
    const int li = K <= 64 ? lane / K : 0;
    const int n_pass = ((Np + PPP - 1) / PPP) * KC;
    const float srange = d.sensor_range, rad2 = d.r_pu * d.r_pu;  // W3: the SENSING pursuer's radius
    // a sensor of pursuer i can only return a finite value for an object with d2 <= rad2 + sv^2 <= rad2 + range^2 (plus a relative margin
    // far above the rounding of the test itself): everything else yields +inf in the oracle and never becomes a minimum
    const float reach2 = (rad2 + srange * srange) * 1.0001f + 1e-9f;
    const int limit = d.max_steps > 0 ? d.max_steps : 1000;  // timestep_limit :124-126
    const int n_envs = (int)d.n_envs;

    for (int e32 = blockIdx.x; e32 < n_envs; e32 += (int)gridDim.x) {  // env indices are 32-bit (n_envs < 2^31 - grid), byte offsets 64-bit
        const int64_t env = e32;
        if (MODE == 0 && io.mask != nullptr && io.mask[env] == 0) continue;  // workgroup-uniform
        uint32_t *const rec = reinterpret_cast<uint32_t *>(d.state) + env * (int64_t)rec_dw;
        for (int k = tid; k < rec_dw; k += NT) reinterpret_cast<uint32_t *>(S)[k] = rec[k];
        __syncthreads();
        int32_t tstep = reinterpret_cast<int32_t *>(S)[4 * NP + 2];  // every thread holds its own copy of the two counters
        uint32_t tick = reinterpret_cast<uint32_t *>(S)[4 * NP + 3];
        const uint32_t gid = d.gid_base + (uint32_t)env;
        float *const orow_env = io.obs + env * (int64_t)Np * D;

        bool do_init = (MODE == 0);
        int npass = 1;
        for (int pass = 0; pass < npass; ++pass) {
            if (do_init) {
                // ------------------------------------------------ reset (:144-172)
                tstep = 0;
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
            // phase A: particles
            for (int j = tid; j < NP; j += NT) {
                float x = X[2 * j], y = X[2 * j + 1], vx = V[2 * j], vy = V[2 * j + 1];
                float sq_obst = d.sq_obst_po, f = -1.0f;
                if (j < Np) {
                    float r0 = 0.0f, r1 = 0.0f;
                    if (live) {
                        const float *a = io.actions + (env * Np + j) * 2;
                        r0 = a[0];
                        r1 = a[1];
                    }
                    const float a0 = r0 * d.action_scale, a1 = r1 * d.action_scale;  // :224
                    ACT[2 * j] = a0;
                    ACT[2 * j + 1] = a1;
                    vx = vx + a0; vy = vy + a1;  // :229-231
                    x = x + vx; y = y + vy;
                    const float cx = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);  // :239-245
                    const float cy = y < 0.f ? 0.f : (y > 1.f ? 1.f : y);
                    if (x != cx) vx = 0.f;
                    if (y != cy) vy = 0.f;
                    x = cx; y = cy;
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
            // phase B1: collisions (:272-293).  Bits past the end of a class stay 0.
            for (int i = wave; i < Np; i += NW) {
                const float pix = X[2 * i], piy = X[2 * i + 1];
                for (int c = 0; c < W; ++c) {
                    const bool is_ev = c < WE;
                    const int m = (is_ev ? c : c - WE) * 64 + lane;
                    const bool in = m < (is_ev ? Ne : Npo);
                    const int j = (is_ev ? Np : Np + Ne) + (in ? m : 0);
                    const uint64_t hit = __ballot(in && dist2_le(pix, piy, X[2 * j], X[2 * j + 1], is_ev ? d.sq_hit_ev : d.sq_hit_po));
                    if (lane == 0) COL[i * W + c] = hit;
                }
            }
            __syncthreads();
            // phase B2: _caught (:180-193): an object counts its column
            for (int c = wave; c < W; c += NW) {
                const bool is_ev = c < WE;
                int s = 0;
                for (int i = 0; i < Np; ++i) s += (int)((COL[i * W + c] >> lane) & 1ull);
                const uint64_t cm = __ballot(s >= (is_ev ? d.n_coop : 1));
                const uint64_t em = __ballot(s >= 1);
                if (lane == 0) {
                    CAU[c] = cm;
                    if (is_ev) ENC[c] = em;
                }
            }
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
                    if (d.reward_global) {  // (actions**2).sum(), row-major (:234-235, W12): summed in that order, not as a tree
                        float s = 0.0f;
                        for (int q = 0; q < Np; ++q) {
                            const float b0 = ACT[2 * q], b1 = ACT[2 * q + 1];
                            s += b0 * b0;
                            s += b1 * b1;
                        }
                        reward = 0.0f + d.control_penalty * s;
                        reward += ((float)n_evc * d.food_reward) + ((float)n_poc * d.poison_reward) + ((float)n_enc * d.encounter_reward);
                    } else {  // fancy-index += pays a pursuer once per kind (W7)
                        const float a0 = ACT[2 * i], a1 = ACT[2 * i + 1];
                        reward = 0.0f + d.control_penalty * (a0 * a0 + a1 * a1);
                        if (wc) reward += d.food_reward;
                        if (wp) reward += d.poison_reward;
                        if (we) reward += d.encounter_reward;
                    }
                    io.rew[env * Np + i] = reward;
                }
            }
            // phase C: sensing (:295-353)
            if (emit) {
                const bool speed = (bool)d.speed_features;
                for (int p = wave; p < n_pass; p += NW) {
                    const int ig = KC == 1 ? p : p / KC, kc = p - ig * KC;
                    const int i_first = ig * PPP, i_cnt = min(PPP, Np - i_first);  // the pursuers of this pass
                    const int k0 = K <= 64 ? lane - li * K : kc * 64 + lane;
                    const bool okq = li < i_cnt && k0 < K;   // lanes without a (pursuer, sensor) pair compute along and store nothing
                    const int iq = i_first + (okq ? li : 0), kq = okq ? k0 : 0;
                    const float sxq = SEN[2 * kq], syq = SEN[2 * kq + 1];
                    const float pxq = X[2 * iq], pyq = X[2 * iq + 1], pvx = V[2 * iq], pvy = V[2 * iq + 1];
                    float *const o = orow_env + (int64_t)iq * D + kq;
#pragma unroll
                    for (int cls = 0; cls < 4; ++cls) {  // 0 obstacle, 1 evaders, 2 poison, 3 allies
                        const int lo = cls == 1 ? Np : (cls == 2 ? Np + Ne : 0);
                        const int cnt = cls == 0 ? 1 : (cls == 1 ? Ne : (cls == 2 ? Npo : Np));
                        float b = INFINITY;
                        int bi = 0;  // np.argmin of an all-inf row is 0
                        auto visit = [&](int m, float qx, float qy) {
                            const float rx = qx - pxq, ry = qy - pyq;
                            const float sv = sxq * rx + syq * ry;  // sensors.dot(relpos.T) :67
                            const float d2 = rx * rx + ry * ry;
                            // sv < 0 || sv > srange as ONE compare: the median of (sv, 0, srange) is sv exactly when 0 <= sv <= srange (waterworld.hip)
                            const bool out = (__builtin_amdgcn_fmed3f(sv, 0.f, srange) != sv) | (d2 - sv * sv > rad2) | ((cls == 3) & (m == iq));
                            // an excluded ray is +inf in the reference and never "better"; a kept one is when it is smaller: first minimum
                            const bool better = !out & (sv < b);
                            b = better ? sv : b;
                            bi = better ? m : bi;
                        };
                        if (cls == 0) {
                            visit(0, ox, oy);
                        } else {
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
#pragma nounroll
                                while (todo != 0ull) {
                                    const int m2 = base + __builtin_ctzll(todo);
                                    todo &= todo - 1ull;
                                    const float2 qp = *reinterpret_cast<const float2 *>(&X[2 * (lo + m2)]);  // uniform address: a broadcast
                                    visit(m2, qp.x, qp.y);
                                }
                            }
                        }
                        const bool fin = b < INFINITY;
                        const float fd = fin ? b : 0.f;  // W4: raw distance or 0
                        if (cls == 0) {
                            if (okq) o[0] = fd;
                        } else {
                            const int j = lo + bi;  // (bi = 0 without a hit: a valid particle, its value is not used)
                            const float raw = sxq * (V[2 * j] - pvx) + syq * (V[2 * j + 1] - pvy);  // _extract_speed_features :203-218
                            const float fs = fin ? raw : 0.f;  // W5
                            if (okq) {  // np.c_[ob, evd, evs, pod, pos, pud, pus] -> blocks of K (:389-395)
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
                        const float *r = io.inj_resp + (env * NP + j) * 4;
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
                x = x + vx; y = y + vy;
                const bool outx = !(x >= 0.f && x <= 1.f), outy = !(y >= 0.f && y <= 1.f);
                if (outx && outy) { vx = -1.0f * vx; vy = -1.0f * vy; }  // only if BOTH coordinates left [0,1] (W6)
                X[2 * j] = x; X[2 * j + 1] = y; V[2 * j] = vx; V[2 * j + 1] = vy;
            }
            tick += 1;
            tstep += 1;  // :433
            const bool is_done = tstep >= limit;  // :174-178
            if (tid == 0) {
                reinterpret_cast<int32_t *>(S)[4 * NP + 2] = tstep;
                reinterpret_cast<uint32_t *>(S)[4 * NP + 3] = tick;
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
        for (int k = tid; k < rec_dw; k += NT) rec[k] = reinterpret_cast<const uint32_t *>(S)[k];
        __syncthreads();  // the next env's record overwrites S
    }
}

}  // namespace

namespace madrl {

size_t ww_crowd_lds_bytes(int Np, int Ne, int Npo, int K, int rec_dw) {
    const size_t WE = ((size_t)Ne + 63) / 64, WP = ((size_t)Npo + 63) / 64;
    return ((size_t)up4(rec_dw) + up4(2 * K) + up4(2 * Np)) * 4 + ((size_t)Np * (WE + WP) + (WE + WP) + WE) * 8;
}

int ww_crowd_launch(const void *dev, const void *io_, int mode, int64_t max_blocks, size_t lds_bytes, void *stream) {
    const WwDev &d = *static_cast<const WwDev *>(dev);
    const WwIO &io = *static_cast<const WwIO *>(io_);
    const dim3 g = particle_grid(max_blocks, d.n_envs), b(64 * MADRL_WWC_NW);
    if (mode == 0) hipLaunchKernelGGL((ww_crowd_kernel<0, MADRL_WWC_NW>), g, b, lds_bytes, (hipStream_t)stream, d, io);
    else hipLaunchKernelGGL((ww_crowd_kernel<1, MADRL_WWC_NW>), g, b, lds_bytes, (hipStream_t)stream, d, io);
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}

}  // namespace madrl
