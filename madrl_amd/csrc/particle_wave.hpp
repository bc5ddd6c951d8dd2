// particle_wave.hpp -- what the one-wavefront kernels of the two particle worlds share: waterworld_kernel (waterworld.hip) and
// hostage_kernel (hostage.hip), gfx950 / CDNA4, float32.  These are the kernels bench.py runs.
//
// One wavefront owns one env at a time (64-thread persistent workgroups walking the envs).  The env's packed state record (particle
// positions and velocities, then the world's own words), the staged observation rows [agents + 1][D] (the last: a spare row), the sensor
// unit vectors, the per-agent reach masks NEAR and the generic path's collision bytes live in LDS (wave_lds_bytes); HBM sees the record in
// and out, the action row in and observation / reward / done / info rows out.  Lane roles change per phase:
//   record      the next env's record (4 dwords per lane) and action row are fetched one env ahead into registers (WaveRecord)
//   A           lane = particle; an agent (pursuer / rescuer: the first n_agents particles) takes its action (agent_action), integrates
//               and is clipped to the walls (integrate_agent, common.hpp; hostage.hip keeps its own lines: the helper cost it 1 %)
//   B           lane = (agent, object) pair: contact tests; then lane = object: it counts its column (_caught) -- bytes in LDS here
//               (contact_bytes, column_count, agent_contacts); the ballot form of the specialised shapes (BITROWS) stays in each .hip
//   C           lane = (agent, sensor) pair, a pass of 64 at a time (sense_pass).  reach_cull marks per agent the objects within sensing
//               reach, pass_reach is their union over the agents of a pass, and the pass walks its set bits class by class in ascending
//               order (walk_bits) -- the reference's index order, so a running minimum with a strict `<` is np.argmin's first minimum.
//               One ray test: ray_misses
//   epilogue    the fused StandardizedEnv (std_reward, std_obs_row), then the record goes back (store_record)
//   live counts a live-count entry (waterworld_kernel_live) fetches the env's counts with its record (WaveCounts) and moves the record between the
//               capacity's slotted layout and the packed layout of the env's counts (slot_to_packed; the mapped to_lds / store_record)
//   ranges      a ranged entry (waterworld_kernel_ranges) keeps phase C's helpers as they are: ray_misses takes srange per lane -- there the
//               range of the lane's own agent, from a table next to the sensor vectors in LDS -- and reach_cull / pass_reach run on the
//               table's maximum, which keeps the cull conservative for every agent (it only skips what the ray test would reject)
// The helpers take the LDS arrays, the counts and the lane as arguments and know nothing of a world's structs.  Two kinds of argument
// keep the kernels' code as it was measured: a launch parameter that a kernel reads inside a branch or a loop is read there, through
// kernargs<KA>() (common.hpp; KA is the kernel's view struct {Dev d; IO io;}, and only fields both worlds have under one name are
// named: d.state, d.action_scale, d.control_penalty, d.reward_global, io.actions); and a lane predicate evaluated inside a loop is passed
// as a callable, since Waterworld and hostage spell theirs differently (lane_lt_imm / fresh, common.hpp).  Each .hip is its world's step in
// the reference's order and keeps what is its own: reset draws, obstacle / gate / key / bomb, flags and row tail, rewards, respawn, done.
#pragma once

#include "common.hpp"

#include <math.h>

namespace madrl {

// The dynamic (generic kernels) or static (specialised shapes) LDS of a workgroup: record | rows [agents + 1][D] | sensors [K][2], each a
// multiple of 4 dwords, then NEAR [agents] (8 bytes each), the collision bytes [agents][n1] | [agents][n2] and the flags
// caught[n1] | encountered[n1] | caught[n2].  n1, n2: the objects of the two classes an agent can touch.
constexpr __host__ __device__ inline size_t wave_lds_bytes(int rec_dw, int agents, int D, int K, int n1, int n2) {
    return ((size_t)(up4(rec_dw) + up4((agents + 1) * D) + up4(2 * K)) * 4 + 8 * (size_t)agents + (size_t)agents * (n1 + n2) + 2 * (size_t)n1 + n2 + 15) / 16 * 16;
}

__device__ __forceinline__ uint64_t low_bits64(int n) { return (n >= 64) ? ~0ull : ((1ull << n) - 1ull); }
__device__ __forceinline__ uint32_t low_bits32(int n) { return n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u); }

// ---- record pipeline.  An env's record (rec_dw <= 256 dwords) and this lane's word of its action row, held in registers.
struct WaveRecord {
    uint32_t r[4] = {0, 0, 0, 0};
    float act = 0.0f;  // lane 2i / 2i+1: agent i's action components (MODE 1)

    template <int MODE, class KA>
    __device__ __forceinline__ void fetch(int64_t env, int rec_dw, int n_agents, int lane, uint32_t ulane) {
        fetch_rows<MODE, KA>(env, rec_dw, n_agents, n_agents, lane, ulane);
    }
    // row_agents: the agents the action tensor has a row for (the stride); the first n_agents rows are read
    template <int MODE, class KA>
    __device__ __forceinline__ void fetch_rows(int64_t env, int rec_dw, int row_agents, int n_agents, int lane, uint32_t ulane) {
        const int nreg = (rec_dw + 63) >> 6;
        const auto src = uniform_ptr(reinterpret_cast<const uint32_t *>(kernargs<KA>()->d.state) + env * (int64_t)rec_dw);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t k = ulane + 64u * q;
            r[q] = (q < nreg && (int)k < rec_dw) ? src[k] : 0u;
        }
        if constexpr (MODE == 1) act = (lane < 2 * n_agents) ? uniform_ptr(kernargs<KA>()->io.actions + env * 2 * row_agents)[ulane] : 0.0f;
        else act = 0.0f;
    }
    // The hinge of the software pipeline: the compiler may not move the loads of a fetch past this point, nor what follows ahead of them.
    __device__ __forceinline__ void hinge() { asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(act)); }
    // record -> LDS
    __device__ __forceinline__ void to_lds(uint32_t *SU, int rec_dw, int lane) const {
        const int nreg = (rec_dw + 63) >> 6;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = lane + 64 * q;
            if (q < nreg && k < rec_dw) SU[k] = r[q];
        }
    }
    // slotted record -> the packed record of an env's live counts: dword k goes to packed(k), those of absent slots (packed(k) < 0) are dropped
    template <class Packed>
    __device__ __forceinline__ void to_lds(uint32_t *SU, int rec_dw, int lane, Packed packed) const {
        const int nreg = (rec_dw + 63) >> 6;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = lane + 64 * q;
            if (q < nreg && k < rec_dw) {
                const int j = packed(k);
                if (j >= 0) SU[j] = r[q];
            }
        }
    }
};

// ---- per-env particle counts of a live-count entry (ParticleCounts, common.hpp).  An env's pending and live triples, each clamped to
// 1 .. the capacity (c0, c1, c2 <= 62) as it is read -- nothing in the arrays leads outside the capacity's LDS or rows -- and packed into
// one word (n0 | n1 << 8 | n2 << 16).  They are fetched with the env's record, one env ahead: the env index is wave-uniform, so these are
// scalar loads, and the first record access of an env waits for none of them.
struct WaveCounts {
    uint32_t pend = 0u, live = 0u;

    static __device__ __forceinline__ int n0(uint32_t pk) { return (int)(pk & 255u); }
    static __device__ __forceinline__ int n1(uint32_t pk) { return (int)((pk >> 8) & 255u); }
    static __device__ __forceinline__ int n2(uint32_t pk) { return (int)(pk >> 16); }
    static __device__ __forceinline__ uint32_t pack(const int32_t *c, int c0, int c1, int c2) {
        return (uint32_t)clampi(c[0], 1, c0) | ((uint32_t)clampi(c[1], 1, c1) << 8) | ((uint32_t)clampi(c[2], 1, c2) << 16);
    }
    // MODE 0 (reset) runs on the pending triple alone; a step on the live one, and on the pending one in the reset pass of an auto-reset
    template <int MODE, class P, class L>
    __device__ __forceinline__ void fetch(P pending, L live_arr, int64_t env, int c0, int c1, int c2) {
        pend = pack(pending + 3 * env, c0, c1, c2);
        live = MODE == 1 ? pack(live_arr + 3 * env, c0, c1, c2) : pend;
    }
    __device__ __forceinline__ void hinge() { asm volatile("" : "+s"(pend), "+s"(live)); }
};

// Dword k of a record slotted at the capacity (c0 | c1 | c2 particles by class: X[NPc][2] | V[NPc][2] | the world's own words) -> its dword
// in the packed record of the live counts (n0, n1, n2), X[NP][2] | V[NP][2] | the same words; -1 for a dword of a slot that holds no
// particle.  Class member m of a slot keeps its index: packed particles are in the live class order, which is the lane order of the phases.
__device__ __forceinline__ int slot_to_packed(int k, int c0, int c1, int c2, int n0, int n1, int n2) {
    const int NPc = c0 + c1 + c2, NP = n0 + n1 + n2;
    if (k >= 4 * NPc) return 4 * NP + (k - 4 * NPc);
    const bool vel = k >= 2 * NPc;
    const int kk = vel ? k - 2 * NPc : k;
    const int s = kk >> 1;
    const int m = s < c0 ? s : (s < c0 + c1 ? s - c0 : s - c0 - c1);           // index within the class
    const int lo = s < c0 ? 0 : (s < c0 + c1 ? n0 : n0 + n1);                   // where the class starts in the packed arrays
    const bool is = m < (s < c0 ? n0 : (s < c0 + c1 ? n1 : n2));
    return is ? (vel ? 2 * NP : 0) + 2 * (lo + m) + (kk & 1) : -1;
}

// LDS -> record
template <class KA>
__device__ __forceinline__ void store_record(const uint32_t *SU, int64_t env, int rec_dw, uint32_t ulane) {
    const auto dst = uniform_ptr(reinterpret_cast<uint32_t *>(kernargs<KA>()->d.state) + env * (int64_t)rec_dw);
    for (uint32_t k = ulane; k < (uint32_t)rec_dw; k += 64u) dst[k] = SU[k];
}
// the packed record of an env's live counts -> the slotted record: every dword of the capacity's record is written, from packed(k) or,
// for a slot that holds no particle, -1.0f (positions: the first half of the particle words) / 0 (velocities)
template <class KA, class Packed>
__device__ __forceinline__ void store_record(const uint32_t *SU, int64_t env, int rec_dw, uint32_t ulane, Packed packed) {
    const auto dst = uniform_ptr(reinterpret_cast<uint32_t *>(kernargs<KA>()->d.state) + env * (int64_t)rec_dw);
    const uint32_t half = ((uint32_t)rec_dw - 4u) >> 1;  // rec_dw = 4 NPc + 4 here: positions below 2 NPc
    for (uint32_t k = ulane; k < (uint32_t)rec_dw; k += 64u) {
        const int j = packed((int)k);
        dst[k] = j >= 0 ? SU[j] : (k < half ? __float_as_uint(-1.0f) : 0u);
    }
}

// ---- half-precision rows (waterworld_kernel_f16, hostage_kernel_f16).  The env's staged float32 rows O[n_out] (16-byte aligned in LDS) leave
// as binary16: element e of the destination holds half_bits(O[e]) (common.hpp: round to nearest even, subnormals kept -- never the packed
// round-toward-zero conversion).  Eight values per lane: two 16-byte LDS reads, eight conversions, ONE 16-byte store; the n_out % 8 values
// behind them leave in 2-byte stores.  The destination is 2-byte aligned and no more (slot t of a [T + 1, N, A, D] half tensor with odd
// N * A * D starts on an odd element): the 16-byte store is declared so, and gfx950 under HSA runs global accesses in unaligned mode -- what
// the float32 rows' 16-byte stores rely on for their 4-byte-aligned base.  Nothing is written outside orow[0 .. n_out - 1]: a chunk ends at
// 8 * (n_out / 8) at the latest, the tail below n_out.
__device__ __forceinline__ void store_rows_half(const float *O, __attribute__((address_space(1))) uint16_t *orow, uint32_t n_out, uint32_t ulane) {
    typedef float f4a __attribute__((ext_vector_type(4), aligned(16)));
    typedef uint32_t u4h __attribute__((ext_vector_type(4), aligned(2)));
    const uint32_t n8 = n_out / 8u;
    for (uint32_t e = ulane; e < n8; e += 64u) {
        const f4a a = *reinterpret_cast<const f4a *>(O + 8 * e), b = *reinterpret_cast<const f4a *>(O + 8 * e + 4);
        u4h w;
        w.x = (uint32_t)half_bits(a.x) | ((uint32_t)half_bits(a.y) << 16);
        w.y = (uint32_t)half_bits(a.z) | ((uint32_t)half_bits(a.w) << 16);
        w.z = (uint32_t)half_bits(b.x) | ((uint32_t)half_bits(b.y) << 16);
        w.w = (uint32_t)half_bits(b.z) | ((uint32_t)half_bits(b.w) << 16);
        *reinterpret_cast<__attribute__((address_space(1))) u4h *>(orow + 8 * e) = w;
    }
    for (uint32_t e = 8u * n8 + ulane; e < n_out; e += 64u) orow[e] = half_bits(O[e]);
}

// ---- phase A.  act_lane: the action row spread over the lanes (WaveRecord::act); agent(): the lane's agent index, 0 for a lane that is
// no agent (a callable: the kernels evaluate the lane predicate in it once per use).  -> the lane's scaled action (a0, a1) and its control penalty: its own under the local reward, and under the global one
// (actions**2).sum() over the agents, summed row-major in that order, not as a tree.
template <class KA, class Agent>
__device__ __forceinline__ float agent_action(float act_lane, Agent agent, int n_agents, float &a0, float &a1) {
    const float a_raw0 = __shfl(act_lane, 2 * agent());
    const float a_raw1 = __shfl(act_lane, 2 * agent() + 1);
    a0 = a_raw0 * kernargs<KA>()->d.action_scale;
    a1 = a_raw1 * kernargs<KA>()->d.action_scale;
    float pen = kernargs<KA>()->d.control_penalty * (a0 * a0 + a1 * a1);
    if (kernargs<KA>()->d.reward_global) {
        float s = 0.0f;
        for (int i = 0; i < n_agents; ++i) {
            const float b0 = __shfl(a0, i), b1 = __shfl(a1, i);
            s += b0 * b0;
            s += b1 * b1;
        }
        pen = kernargs<KA>()->d.control_penalty * s;
    }
    return pen;
}

// ---- phase B, generic path.  COL: [n_agents][n1] bytes of the first class (particles n_agents .. n_agents + n1 - 1), then
// [n_agents][n2] of the second (the particles behind them); a byte is 1 where the agent touches the object.  sq(first): the squared
// contact threshold of a class, read where it is used.
template <class Sq>
__device__ __forceinline__ void contact_bytes(const float *X, uint8_t *COL, int n_agents, int n1, int n2, int lane, Sq sq) {
    for (int idx = lane; idx < n_agents * (n1 + n2); idx += 64) {
        const bool first = idx < n_agents * n1;
        const int r = first ? idx : idx - n_agents * n1;
        const int nn = first ? n1 : n2;
        const int i = r / nn, m = r % nn;
        const int j = (first ? n_agents : n_agents + n1) + m;
        COL[idx] = dist2_le(X[2 * i], X[2 * i + 1], X[2 * j], X[2 * j + 1], sq(first));
    }
}

// _caught: object m of a class counts its column over the agents
__device__ __forceinline__ int column_count(const uint8_t *col, int n_agents, int nn, int m) {
    int s = 0;
    for (int i = 0; i < n_agents; ++i) s += col[i * nn + m];
    return s;
}

// ... and leaves its flags for the agents: FLG = caught[n1] | encountered[n1] | caught[n2]
__device__ __forceinline__ void column_flags(uint8_t *FLG, bool first, int n1, int m, bool caught, bool enc) {
    if (first) { FLG[m] = caught; FLG[n1 + m] = enc; }
    else FLG[2 * n1 + m] = caught;
}

// Agent i's rows: t1 / t2 it touches an object of the class, w1 / w2 one that was caught, e1 one of the first class that was encountered
// (the local rewards pay an agent once per kind)
__device__ __forceinline__ void agent_contacts(const uint8_t *COL1, const uint8_t *COL2, const uint8_t *FLG, int i, int n1, int n2, bool &t1,
                                               bool &w1, bool &e1, bool &t2, bool &w2) {
    for (int m = 0; m < n1; ++m) {
        const bool c = COL1[i * n1 + m];
        t1 |= c;
        w1 |= c && FLG[m];
        e1 |= c && FLG[n1 + m];
    }
    for (int m = 0; m < n2; ++m) {
        const bool c = COL2[i * n2 + m];
        t2 |= c;
        w2 |= c && FLG[2 * n1 + m];
    }
}

// ---- phase C.  The lanes of a sensing pass.  ALIGNED (a compile-time K <= 64): a pass holds floor(64 / K) WHOLE agents (the last lanes
// idle), so the objects a pass must visit are those in reach of its own agents -- 2 at BASELINE C3 instead of the 2.1 - 3 that 64
// consecutive (agent, sensor) pairs straddle: about a quarter fewer (object, pass) visits.  Otherwise: consecutive pairs.
template <int TK>
constexpr __host__ __device__ inline int sense_n_pass(int n_agents, int K) {
    return (TK > 0 && TK <= 64) ? (n_agents + 64 / (TK > 0 ? TK : 1) - 1) / (64 / (TK > 0 ? TK : 1)) : (n_agents * K + 63) / 64;
}

// Pass q: its agents i_first .. i_last and this lane's (agent iq, sensor kq).  Lanes without a pair (okq false) compute along on pair
// (0, 0); the kernels let them write to the spare row instead of branching around the stores.
struct SensePass { int i_first, i_last, iq, kq; bool okq; };
template <int TK>
__device__ __forceinline__ SensePass sense_pass(int pass_q, int n_agents, int K, int lane) {
    constexpr bool ALIGNED = TK > 0 && TK <= 64;
    constexpr int PPP = ALIGNED ? 64 / (TK > 0 ? TK : 1) : 1;  // agents per pass
    SensePass p;
    if constexpr (ALIGNED) {
        const int li = lane / K;
        p.i_first = pass_q * PPP; p.i_last = min(p.i_first + PPP, n_agents) - 1;
        p.okq = li < PPP && p.i_first + li <= p.i_last;
        p.iq = p.okq ? p.i_first + li : 0;
        p.kq = p.okq ? lane - li * K : 0;
    } else {
        const int idx = 64 * pass_q + lane;
        p.okq = idx < n_agents * K;
        p.iq = p.okq ? idx / K : 0;
        p.kq = p.okq ? idx - p.iq * K : 0;
        p.i_first = 64 * pass_q / K; p.i_last = min(64 * pass_q + 63, n_agents * K - 1) / K;
    }
    return p;
}

// Conservative cull: NEAR[i] = the lanes whose object (mx, my) -- a particle's own position, or a single object of the world in a lane
// behind the particles -- is within sensor_reach2 of agent i.  d2 is computed exactly as in the ray test.  in(): the lane holds an object;
// first(): it is lane 0.  part_x / part_y: the lane's particle, agent i's being read from lane i.
template <class In, class First>
__device__ __forceinline__ void reach_cull(uint64_t *NEAR, int n_agents, float part_x, float part_y, float mx, float my, float thr2, In in,
                                           First first) {
    for (int i = 0; i < n_agents; ++i) {
        const float rx = mx - __int_as_float(__builtin_amdgcn_readlane(__float_as_int(part_x), i));
        const float ry = my - __int_as_float(__builtin_amdgcn_readlane(__float_as_int(part_y), i));
        const uint64_t mk = __ballot(in() && (rx * rx + ry * ry <= thr2));
        if (first()) NEAR[i] = mk;
    }
}

// wave-uniform: the objects in reach of any agent of the pass
__device__ __forceinline__ uint64_t pass_reach(const uint64_t *NEAR, int i_first, int i_last) {
    uint64_t u = 0ull;
    for (int i = i_first; i <= i_last; ++i) u |= NEAR[i];
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u)) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32)) << 32);
}

// The ray of the sensor with unit vector (sx, sy) of an agent at (px, py) against the object at (qx, qy): -> sv, the distance along the
// sensor (sensors.dot(relpos.T)); true when the object is not sensed: behind the agent, beyond srange, or off the ray by more than the
// SENSING agent's radius (rad2: its square).  sv < 0 || sv > srange as ONE compare: the median of (sv, 0, srange) is sv exactly when
// 0 <= sv <= srange (sv is finite; -0.0 compares equal to the +0.0 the median may return, as it passes `sv < 0`).
__device__ __forceinline__ bool ray_misses(float sx, float sy, float px, float py, float qx, float qy, float srange, float rad2, float &sv) {
    const float rx = qx - px, ry = qy - py;
    sv = sx * rx + sy * ry;
    const float d2 = rx * rx + ry * ry;
    return (__builtin_amdgcn_fmed3f(sv, 0.f, srange) != sv) | (d2 - sv * sv > rad2);
}

// _extract_speed_features: particle j's velocity relative to agent iq's, along the sensor (sx, sy)
__device__ __forceinline__ float speed_along(const float *V, float sx, float sy, int j, int iq) {
    return sx * (V[2 * j] - V[2 * iq]) + sy * (V[2 * j + 1] - V[2 * iq + 1]);
}

// visit(bit) for every set bit of a wave-uniform mask, ascending.  The 32-bit walk is half the scalar work of the 64-bit one.
template <class Visit>
__device__ __forceinline__ void walk_bits(uint32_t todo, Visit visit) {
#pragma nounroll
    while (todo != 0u) {
        const int m = __builtin_ctz(todo);
        todo &= todo - 1u;
        visit(m);
    }
}
template <class Visit>
__device__ __forceinline__ void walk_bits(uint64_t todo, Visit visit) {
#pragma nounroll
    while (todo != 0ull) {
        const int bit = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        visit(bit);
    }
}

// ---- the fused StandardizedEnv epilogue (ParticleStd, common.hpp): the operations of wrappers.hip rewnorm_kernel / obsnorm_kernel in
// their order.  st: a reference into global memory, or the kernel's own copy of the struct (hostage.hip says why it makes one).
// StandardizedEnv.step :283-291, agent row i = env * n_agents + agent
__device__ __forceinline__ void std_reward(const ParticleStd &st, int64_t i, float reward) {
    double r = (double)reward;
    if (st.enable_rewnorm) {
        double m = st.rew_mean[i], v = st.rew_var[i];
        ema_update(m, v, r, st.rew_alpha);  // :253-257
        st.rew_mean[i] = m;
        st.rew_var[i] = v;
        r = r / (sqrt(v) + st.eps);         // :268-271
    }
    st.rew_out[i] = (float)(st.scale * r);  // :290
}

// StandardizedEnv.standardize_obs :242-263 of the env's staged rows O[n_el], base = env * n_el.  Batches of 4 elements per lane: all 8
// statistics loads of a batch are in flight before the first dependent float64 operation (element by element the loop pays one HBM
// round trip each: 421 instead of 357 us per wrapped Waterworld step; 16-byte pair accesses on top measured no further gain).  Every
// statistics byte is touched once per step: non-temporal.
__device__ __forceinline__ void std_obs_row(const ParticleStd &st, const float *O, int64_t base, int n_el, int lane) {
    if (st.enable_obsnorm) {
        const double *__restrict__ gm = st.obs_mean + base;
        const double *__restrict__ gv = st.obs_var + base;
        for (int e0 = lane; e0 < n_el; e0 += 256) {
            double m[4], v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + 64 * u;
                m[u] = e < n_el ? __builtin_nontemporal_load(&gm[e]) : 0.0;
                v[u] = e < n_el ? __builtin_nontemporal_load(&gv[e]) : 1.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + 64 * u;
                if (e < n_el) {
                    const double x = (double)O[e];
                    double mm = m[u], vv = v[u];
                    ema_update(mm, vv, x, st.obs_alpha);  // :245-249
                    __builtin_nontemporal_store(mm, &st.obs_mean[base + e]);
                    __builtin_nontemporal_store(vv, &st.obs_var[base + e]);
                    __builtin_nontemporal_store((float)((x - mm) / (sqrt(vv) + st.eps)), &st.obs_out[base + e]);  // :262-263
                }
            }
        }
    } else {
        for (int e = lane; e < n_el; e += 64) st.obs_out[base + e] = O[e];
    }
}

// ---- host.  get_state / set_state: `kernel` copies one env per thread between the record and the caller's arrays (args)
template <class H, class Dev, class... A>
int state_copy_launch(H *h, void (*kernel)(Dev, A...), void *stream, A... args) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    const unsigned blocks = (unsigned)((h->dev.n_envs + 127) / 128);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(128), 0, (hipStream_t)stream, h->dev, args...);
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}

}  // namespace madrl
