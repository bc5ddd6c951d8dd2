// particle_crowd.hpp -- what the multi-wavefront kernels of the two particle worlds share: ww_crowd_kernel (waterworld_crowd.hip) and
// hw_crowd_kernel (hostage_crowd.hip), gfx950 / CDNA4, float32.
//
// The one-wavefront kernels (waterworld.hip, hostage.hip) give every particle a lane of ONE wavefront.  In a crowd kernel one WORKGROUP of
// NW wavefronts owns an env at a time (persistent, striding over the envs) and its threads loop over the particles: up to 1 023 particles,
// 128 agents (pursuers / rescuers: a thread owns at most one), any sensor count.  Reached on request only (config.crowd = 1); the results
// are those of the one-wavefront kernel and of the float32 C restatement of the reference the tests use ("the oracle") bit for bit: every
// float expression keeps the oracle's statement order, and whatever the oracle does in a loop whose order matters is done in that order.
// integrate_agent, free_motion and sensor_reach2, the float text the one-wavefront kernels use too, are in common.hpp.
// The helpers below take the LDS arrays and the counts as arguments and know nothing of a world's structs; each .hip is its world's step
// in the oracle's order and keeps what is its own (reset, obstacle / gate / key / bomb, flags and row tail, rewards, respawn draws, done).
//
// Phases of a step, a workgroup barrier between them:
//   A   thread = agent: drive_agent (action, integration, walls), then the world's obstacle rebound / closed gate
//   B1  contact_ballots: wavefront = (agent, chunk of 64 objects), lane = object: contact test, ballot -> COL
//   B2  column_counts (_caught): wavefront = chunk, lane = object: column count over the agents -> CAU / ENC
//       thread = agent: contact flags and id of the observation row, the reward (control_sum under the global reward)
//   C   wavefront = pass of (agent, sensor) lanes: ray tests, features straight to global memory (the row is not staged in LDS: for a
//       fixed agent and feature the K sensor values are contiguous, so the lanes of an agent write whole runs)
//   E   thread = moving non-agent: respawn if caught, then free_motion
// Sensing is the bulk (agents * K * objects ray tests).  A pass holds floor(64 / K) whole agents (K > 64: 64 sensors of one agent).  Per
// class and chunk of 64 objects the lanes test which objects are within reach of an agent of the pass (the conservative predicate of the
// one-wavefront kernels), one ballot makes that a wave-uniform mask, and its set bits are walked in ascending order -- the oracle's index
// order, so the running minimum with a strict `<` is np.argmin's first minimum.  The objects out of reach would yield +inf and are
// skipped.  Single objects (obstacle, key, bomb) are one Ray::visit.
//
// Known costs: the next env's record is not fetched ahead, a ray test waits for its object's LDS broadcast, and the launch parameters are
// held in registers across the env loop instead of being read through kernargs<>() where a phase needs them.
#pragma once

#include "common.hpp"

#include <math.h>

namespace madrl {

// (ParticleCounts, the third argument of the live-count entries, and clampi are in common.hpp: waterworld_kernel_live takes them too)
// ---- phase A.  An agent's action row (zeros unless live) is scaled and kept in ACT[i]; the agent integrates and is clipped to the
// walls, the velocity component zeroed where it was.
__device__ __forceinline__ void drive_agent(bool live, const float *actions, int64_t row, float action_scale, float *ACT, int i, float &x,
                                            float &y, float &vx, float &vy) {
    float r0 = 0.0f, r1 = 0.0f;
    if (live) {
        const float *a = actions + row * 2;
        r0 = a[0];
        r1 = a[1];
    }
    const float a0 = r0 * action_scale, a1 = r1 * action_scale;
    ACT[2 * i] = a0;
    ACT[2 * i + 1] = a1;
    integrate_agent(a0, a1, x, y, vx, vy);
}

// ---- phases B1 / B2.  A collision row is W 64-bit words per agent: `first_words` chunks of the first class, then the chunks of the second.
struct ObjClass { int lo, cnt; float sq; };  // particles lo .. lo + cnt - 1; contact with an agent is dist2_le(..., sq)

// B1: COL[i][c] = the objects of chunk c in contact with agent i.  Bits past the end of a class stay 0.
template <int NW>
__device__ __forceinline__ void contact_ballots(const float *X, uint64_t *COL, int n_agents, int W, int first_words, const ObjClass &c0,
                                                const ObjClass &c1, int wave, int lane) {
    for (int i = wave; i < n_agents; i += NW) {
        const float pix = X[2 * i], piy = X[2 * i + 1];
        for (int c = 0; c < W; ++c) {
            const bool first = c < first_words;
            const int m = (first ? c : c - first_words) * 64 + lane;
            const bool in = m < (first ? c0.cnt : c1.cnt);
            const int j = (first ? c0.lo : c1.lo) + (in ? m : 0);
            const uint64_t hit = __ballot(in && dist2_le(pix, piy, X[2 * j], X[2 * j + 1], first ? c0.sq : c1.sq));
            if (lane == 0) COL[i * W + c] = hit;
        }
    }
}

// B2, _caught: an object counts its column.  CAU[c]: caught (first class: by n_coop agents; second: by one); ENC[c], first class only:
// touched by at least one agent.
template <int NW>
__device__ __forceinline__ void column_counts(const uint64_t *COL, uint64_t *CAU, uint64_t *ENC, int n_agents, int W, int first_words,
                                              int n_coop, int wave, int lane) {
    for (int c = wave; c < W; c += NW) {
        const bool first = c < first_words;
        int s = 0;
        for (int i = 0; i < n_agents; ++i) s += (int)((COL[i * W + c] >> lane) & 1ull);
        const uint64_t cm = __ballot(s >= (first ? n_coop : 1));
        const uint64_t em = __ballot(s >= 1);
        if (lane == 0) {
            CAU[c] = cm;
            if (first) ENC[c] = em;
        }
    }
}

// (actions**2).sum() of the global control penalty, row-major over ACT: summed in that order, not as a tree
__device__ __forceinline__ float control_sum(const float *ACT, int n_agents) {
    float s = 0.0f;
    for (int q = 0; q < n_agents; ++q) {
        const float b0 = ACT[2 * q], b1 = ACT[2 * q + 1];
        s += b0 * b0;
        s += b1 * b1;
    }
    return s;
}

// ---- phase C.  The lanes of a sensing pass: PPP whole agents of K sensors (K <= 64), or one of the KC chunks of 64 sensors of one agent.
struct PassShape { int PPP, KC, li, n_pass; };
__device__ __forceinline__ PassShape pass_shape(int K, int n_agents, int lane) {
    const int PPP = K <= 64 ? 64 / K : 1, KC = K <= 64 ? 1 : (K + 63) >> 6;
    const int li = K <= 64 ? lane / K : 0;
    return {PPP, KC, li, ((n_agents + PPP - 1) / PPP) * KC};
}

// Pass p: its agents i_first .. i_first + i_cnt - 1 and this lane's (agent iq, sensor kq).  Lanes without a pair (okq false) compute
// along and store nothing.
struct PassLanes { int i_first, i_cnt, iq, kq; bool okq; };
__device__ __forceinline__ PassLanes pass_lanes(const PassShape &s, int p, int K, int n_agents, int lane) {
    const int ig = s.KC == 1 ? p : p / s.KC, kc = p - ig * s.KC;
    const int i_first = ig * s.PPP, i_cnt = min(s.PPP, n_agents - i_first);
    const int k0 = K <= 64 ? lane - s.li * K : kc * 64 + lane;
    const bool okq = s.li < i_cnt && k0 < K;
    return {i_first, i_cnt, i_first + (okq ? s.li : 0), okq ? k0 : 0, okq};
}

// One (agent, sensor) lane's ray and its running first minimum (b, bi) over the objects visited in index order.
struct Ray {
    float sxq, syq, pxq, pyq, pvx, pvy;  // the sensor's unit vector, the sensing agent's position and velocity
    float srange, rad2;                  // the sensor range, the SENSING agent's squared radius
    float b;
    int bi;  // np.argmin of an all-inf row is 0

    __device__ __forceinline__ Ray(const float *SEN, const float *X, const float *V, int iq, int kq, float srange_, float rad2_)
        : sxq(SEN[2 * kq]), syq(SEN[2 * kq + 1]), pxq(X[2 * iq]), pyq(X[2 * iq + 1]), pvx(V[2 * iq]), pvy(V[2 * iq + 1]), srange(srange_),
          rad2(rad2_) {
        restart();
    }
    __device__ __forceinline__ void restart() { b = INFINITY; bi = 0; }
    // object m at (qx, qy); `excluded`: the oracle sets this ray to +inf whatever it hits (an agent does not sense itself)
    __device__ __forceinline__ void visit(int m, float qx, float qy, bool excluded = false) {
        const float rx = qx - pxq, ry = qy - pyq;
        const float sv = sxq * rx + syq * ry;  // sensors.dot(relpos.T) :67
        const float d2 = rx * rx + ry * ry;
        // sv < 0 || sv > srange as ONE compare: the median of (sv, 0, srange) is sv exactly when 0 <= sv <= srange
        const bool out = (__builtin_amdgcn_fmed3f(sv, 0.f, srange) != sv) | (d2 - sv * sv > rad2) | excluded;
        // an excluded ray is +inf in the reference and never "better"; a kept one is when it is smaller: first minimum
        const bool better = !out & (sv < b);
        b = better ? sv : b;
        bi = better ? m : bi;
    }
    // _extract_speed_features: particle j's velocity relative to the sensing agent's, along the sensor
    __device__ __forceinline__ float speed_along(const float *V, int j) const { return sxq * (V[2 * j] - pvx) + syq * (V[2 * j + 1] - pvy); }
};

// visit(m, x, y) for every object m of the class lo .. lo + cnt - 1 within reach of an agent of the pass and not in `skip` (bit m: a
// class of at most 64 objects; otherwise 0), in ascending m.
template <class Visit>
__device__ __forceinline__ void reach_walk(const float *X, int lo, int cnt, const PassLanes &L, float reach2, uint64_t skip, int lane,
                                           Visit visit) {
    for (int base = 0; base < cnt; base += 64) {
        const int m = base + lane;
        const bool in = m < cnt;
        const float2 mp = *reinterpret_cast<const float2 *>(&X[2 * (lo + (in ? m : 0))]);
        bool near = false;
        for (int q = 0; q < L.i_cnt; ++q) {
            const float2 pp = *reinterpret_cast<const float2 *>(&X[2 * (L.i_first + q)]);
            const float rx = mp.x - pp.x, ry = mp.y - pp.y;
            near |= rx * rx + ry * ry <= reach2;
        }
        uint64_t todo = __ballot(in && near) & ~skip;  // wave-uniform: the objects of this chunk within reach of the pass
#pragma nounroll
        while (todo != 0ull) {
            const int m2 = base + __builtin_ctzll(todo);
            const float2 qp = *reinterpret_cast<const float2 *>(&X[2 * (lo + m2)]);  // uniform address: a broadcast
            todo &= todo - 1ull;  // after the read is issued: the ray test waits for it, the mask does not
            visit(m2, qp.x, qp.y);
        }
    }
}

// ---- host.  `kernel`: the reset or the step instantiation; dev / io: the world's Dev and IO structs behind the untyped pointers of *_dev.hpp
template <class Dev, class IO>
int crowd_launch(void (*kernel)(Dev, IO), int nw, const void *dev, const void *io, int64_t max_blocks, size_t lds_bytes, void *stream) {
    const Dev &d = *static_cast<const Dev *>(dev);
    hipLaunchKernelGGL(kernel, particle_grid(max_blocks, d.n_envs), dim3(64 * nw), lds_bytes, (hipStream_t)stream, d, *static_cast<const IO *>(io));
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}


// ... of a live-count entry, with the count arrays as its third argument
template <class Dev, class IO>
int crowd_launch(void (*kernel)(Dev, IO, ParticleCounts), int nw, const void *dev, const void *io, const ParticleCounts &cn,
                 int64_t max_blocks, size_t lds_bytes, void *stream) {
    const Dev &d = *static_cast<const Dev *>(dev);
    hipLaunchKernelGGL(kernel, particle_grid(max_blocks, d.n_envs), dim3(64 * nw), lds_bytes, (hipStream_t)stream, d, *static_cast<const IO *>(io),
                       cn);
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}

}  // namespace madrl
