// common.hpp -- shared host/device helpers for libmadrl_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdarg.h>
#include <new>
#include <vector>

#include "../../include/madrl_hip.h"
#include "philox.hpp"   // u32x4, philox4x32_10, the TAG_* enum, u53

namespace madrl {

// ---------------------------------------------------------------- error reporting
char *last_error_buf();  // thread-local, defined in abi.hip

inline int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

#define MADRL_HIP_TRY(expr)                                                                  \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return ::madrl::fail(MADRL_EHIP, "%s failed: %s (%s:%d)", #expr,                 \
                                 hipGetErrorString(_e), __FILE__, __LINE__);                 \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
constexpr __host__ __device__ inline int up4(int v) { return (v + 3) & ~3; }

// The flag plane of a step launch (include/madrl_hip.h, madrl_pursuit_flags_offset): the done byte split into one 0 / 1 byte per
// meaning, so that the host side hands out bool views of it instead of launching kernels that mask bits.
//   byte 0 = bit 0 (episode over)   byte 1 = bit 1 (max_steps reached)   byte 2 = bit 7 (a capacity overflowed)   byte 3 = the done byte
__host__ __device__ inline uint32_t done_flag_word(uint32_t done_byte) {
    return (done_byte & 1u) | ((done_byte & 2u) << 7) | ((done_byte & 0x80u) << 9) | (done_byte << 24);
}

// XCD-aware walk of the env range by a grid of persistent one-wavefront workgroups.  Workgroups are dealt round-robin to
// the 8 XCDs (block b runs on XCD b % 8, each with its own L2), so the plain walk env = b + k * gridDim hands NEIGHBOURING
// envs to DIFFERENT L2s: every cache line shared by two envs' rows / records / reward words is then written back partially
// by two or more L2s.  Here XCD x owns the contiguous eighth [x * per, (x + 1) * per) of the envs and its workgroups stride
// through that chunk, so lines shared by neighbours merge in one L2.  (Measured on the hostage world: 4 107 -> 2 3xx bytes
// written per env-step; speed-only -- env results do not depend on the order in which they are processed.)
struct EnvWalk {
    int64_t base, first, stride, lim;  // env = base + li for li = first, first + stride, ... < lim
};
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
__device__ __forceinline__ EnvWalk env_walk(int64_t n_envs) {
    EnvWalk w;
    const int64_t G = gridDim.x, b = blockIdx.x;
    if ((G & 7) == 0 && n_envs >= 8 * 8) {
        const int64_t per = (n_envs + 7) / 8;
        w.base = (b & 7) * per;
        w.first = b >> 3;
        w.stride = G >> 3;
        w.lim = (w.base + per <= n_envs ? per : n_envs - w.base);
        if (w.lim < 0) w.lim = 0;
    } else {
        w.base = 0; w.first = b; w.stride = G; w.lim = n_envs;
    }
    return w;
}

// ---------------------------------------------------------------- wavefront helpers of the env kernels
// Launch parameters that a phase only reads now and then are not held in SGPRs across the env loop: the loop's scalar live set
// (broadcast masks, reach sets, counters) is already at the SGPR limit, and what does not fit is parked in VGPR lanes -- one
// v_readlane_b32 (a VALU issue slot) per value and use.  The kernel reads them from its kernel-argument segment (scalar loads) where
// they are needed, through a view A = struct {Dev d; IO io;} of its two by-value arguments.
template <class A>
__device__ __forceinline__ const __attribute__((address_space(4))) A *kernargs() {
    auto p = (const __attribute__((address_space(4))) A *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));  // a fresh pointer at every call: the loads cannot be merged with the ones at kernel entry or hoisted
    return p;
}

// A wave-uniform pointer pinned to an SGPR pair at this point of the program.  Per-lane accesses written as
// uniform_ptr(base + env * stride)[lane] then select the "SGPR base + 32-bit VGPR offset" addressing form; without the pin the
// compiler reassociates to (base + lane * 4) + env * stride, keeps one 64-bit VGPR pair per array live across the env loop and,
// at 96 VGPRs, spills them -- and a scratch reload in the loop waits (in-order vmcnt) for the previous env's observation stores.
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T *uniform_ptr(T *p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (__attribute__((address_space(1))) T *)(((uint64_t)hi << 32) | lo);  // global address space: global_*, not flat_*, instructions
}

// The IEEE binary16 of a float32 value, round to nearest even with gradual underflow and overflow to infinity (v_cvt_f16_f32 under the
// default rounding mode: what torch.Tensor.to(torch.float16) gives) -- the half-precision observation slots of madrl_pursuit_step_to_f16.
// (Not the packed conversion v_cvt_pkrtz_f16_f32: that one rounds toward zero, 0.3f -> 0x34CC instead of 0x34CD.)
__device__ __forceinline__ uint16_t half_bits(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }

// Register-pressure control.  The compiler hoists every loop-invariant lane compare (lane < P, lane == k, ...)
// out of the env loop as an SGPR-pair mask and, with ~100 uniform values already live there, spills them to
// VGPR lanes: each use then costs two v_readlane_b32 (VALU issue slots, the resource these kernels are bound by).
// fresh(lane) hides the invariance, so a predicate is one v_cmp at its use site and dies there.
__device__ __forceinline__ int fresh(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ uint32_t fresh_s(uint32_t v) {
    asm volatile("" : "+s"(v));
    return v;
}

// The same for the SPECIALISED shapes, one instruction cheaper: fresh() costs a v_mov before its v_cmp; here the compare is written
// out (volatile: it stays where it is used and its mask dies there), its right-hand side an inline constant of the shape (<= 64), and the
// wave-uniform mask becomes the lane predicate without an instruction (inverse ballot).
__device__ __forceinline__ bool lane_lt_imm(int lane, int n) {   // lane < n; n must fold to a constant in -16 .. 64
    unsigned long long m;
    asm volatile("v_cmp_gt_i32_e64 %0, %1, %2" : "=s"(m) : "i"(n), "v"(lane));
    return __builtin_amdgcn_inverse_ballot_w64(m);
}
__device__ __forceinline__ bool lane_eq_imm(int lane, int n) {
    unsigned long long m;
    asm volatile("v_cmp_eq_i32_e64 %0, %1, %2" : "=s"(m) : "i"(n), "v"(lane));
    return __builtin_amdgcn_inverse_ballot_w64(m);
}

// Wave-local synchronisation.  A workgroup (or an env's group of lanes) is one wavefront, its DS (LDS) instructions are
// executed in issue order, so cross-lane LDS hand-offs only need the COMPILER to keep the order; unlike __syncthreads()
// this emits no s_waitcnt vmcnt(0), i.e. the wave never waits for its observation stores to reach HBM.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// uniform float in [0,1) from the top 24 bits
__device__ __forceinline__ float u24(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }

__device__ __forceinline__ float dist2d(float ax, float ay, float bx, float by) {
    const float dx = ax - bx, dy = ay - by;
    return sqrtf(dx * dx + dy * dy);  // scipy cdist 'euclidean'
}

// dist2d(a, b) <= thr, with sq = sq_threshold(thr) (host side): same truth value, no square root
__device__ __forceinline__ bool dist2_le(float ax, float ay, float bx, float by, float sq) {
    const float dx = ax - bx, dy = ay - by;
    return dx * dx + dy * dy <= sq;
}

// StandardizedEnv.update_obs_estimate / update_rew_estimate (madrl_environments/__init__.py:245-249, :253-257): one element's exponential
// running mean m and variance v take the value x, in float64 and in the reference's order of operations.
__device__ __forceinline__ void ema_update(double &m, double &v, double x, double alpha) {
    m = (1.0 - alpha) * m + alpha * x;
    const double d = x - m;
    v = (1.0 - alpha) * v + alpha * (d * d);
}

// ---------------------------------------------------------------- float text the particle worlds' kernels share
// (particle_wave.hpp: one wavefront per env; particle_crowd.hpp: a multi-wavefront workgroup per env)
// An agent takes its scaled action (a0, a1), integrates and is clipped to the walls, the velocity component zeroed where it was.
__device__ __forceinline__ void integrate_agent(float a0, float a1, float &x, float &y, float &vx, float &vy) {
    vx = vx + a0; vy = vy + a1;
    x = x + vx; y = y + vy;
    const float cx = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
    const float cy = y < 0.f ? 0.f : (y > 1.f ? 1.f : y);
    if (x != cx) vx = 0.f;
    if (y != cy) vy = 0.f;
    x = cx; y = cy;
}

// A non-agent moves; its velocity flips only if BOTH coordinates left [0, 1], and nothing is clipped.
__device__ __forceinline__ void free_motion(float &x, float &y, float &vx, float &vy) {
    x = x + vx; y = y + vy;
    const bool outx = !(x >= 0.f && x <= 1.f), outy = !(y >= 0.f && y <= 1.f);
    if (outx && outy) { vx = -1.0f * vx; vy = -1.0f * vy; }
}

// A sensor of agent i can only return a finite value for an object with d2 <= rad2 + sv^2 <= rad2 + range^2 (plus a relative margin far
// above the rounding of the test itself): everything else yields +inf in the oracle and never becomes a minimum.
__device__ __forceinline__ float sensor_reach2(float rad2, float srange) { return (rad2 + srange * srange) * 1.0001f + 1e-9f; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
#endif

// ---------------------------------------------------------------- host side of the env handles
// The global env index (env_id_base + env) is a 32-bit word of the RNG counter.
inline int check_env_ids(int64_t n_envs, int64_t env_id_base) {
    if (n_envs + env_id_base > 0xFFFFFFFFll) return fail(MADRL_EINVAL, "global env index must fit 32 bits");
    return MADRL_OK;
}

// The largest float32 x with sqrtf(x) <= thr (thr >= 0 finite), so that "distance <= thr" is the single compare
// "dx*dx + dy*dy <= x" with the same truth value for every input (sqrtf is monotonic and correctly rounded); the correctly
// rounded sqrtf itself is a 20-instruction sequence.
inline float sq_threshold(float thr) {
    float x = thr * thr;
    while (x > 0.0f && sqrtf(x) > thr) x = nextafterf(x, 0.0f);
    for (;;) {
        const float up = nextafterf(x, INFINITY);
        if (!(sqrtf(up) <= thr)) break;
        x = up;
    }
    return x;
}

// The launch grid of the particle worlds (waterworld.hip, hostage.hip): persistent one-wavefront workgroups, max_blocks of them
// (madrl_*_set_launch; 0 = 256 * 64), never more than one per env.
inline dim3 particle_grid(int64_t max_blocks, int64_t n_envs) {
    int64_t blocks = max_blocks > 0 ? max_blocks : 256 * 64;
    if (blocks > n_envs) blocks = n_envs;
    return dim3((unsigned)blocks);
}

// Fused StandardizedEnv (madrl_environments/__init__.py:204-311) of the particle worlds, the device copy of madrl_standardize_args:
// the kernels' FUSED instantiations normalise the observation row as it leaves LDS and scale / normalise the rewards as they are
// produced -- per env, per agent, per element exponential running mean / variance in float64, the arithmetic of the stand-alone
// epilogue kernels (wrappers.hip obsnorm_kernel / rewnorm_kernel) in their order -- instead of storing the row raw for a second
// launch to read back: 36 instead of 44 bytes of HBM traffic per observation element.
struct ParticleStd {
    double *obs_mean, *obs_var;   // [N][agents][D]
    float *obs_out;               // [N][agents][D] standardised observations (a copy of the row without enable_obsnorm)
    double *rew_mean, *rew_var;   // [N][agents]
    float *rew_out;               // [N][agents] scale * (reward / (sqrt(var) + eps)); NULL = rewards are not touched
    double obs_alpha, rew_alpha, eps, scale;
    int32_t enable_obsnorm, enable_rewnorm;
};

// Per-env particle counts (madrl_waterworld_set_particle_counts, madrl_hostage_set_particle_counts): the two caller-owned int32
// [n_envs][3] arrays of the live-count entries (*_crowd_kernel_live, waterworld_kernel_live), in the world's class order, the agents first
struct ParticleCounts {
    const int32_t *pending;  // the counts an env takes at its next reset, clamped to 1 .. capacity
    int32_t *live;           // the counts of its running episode: read per env, written by the reset pass
};

// What a particle world's handle holds: struct madrl_waterworld / madrl_hostage derive from it with their configuration and Dev types.
template <class C, class Dev>
struct ParticleHandle {
    C cfg;
    Dev dev;
    int device;
    int64_t max_blocks;
    size_t lds_bytes;
    void *tables;
    ParticleStd *std_dev;   // device copy of the bound StandardizedEnv arguments (particle_set_standardize)
    bool std_bound;
    const int32_t *pending;  // particle_set_counts: caller-owned [n_envs][3], both NULL = one shape for all envs
    int32_t *live;
    void *range_tables;      // madrl_waterworld_set_sensor_ranges: the handle's copy of `tables` with the per-agent sensor ranges behind it
    bool ranged;             // ... is bound: dev.sensors points to it, dev.sensor_range is its maximum, lds_bytes holds the ranges too
};

// madrl_waterworld_create / madrl_hostage_create after the world's own validation of cfg: H is the handle, layout() and lds_bytes()
// the world's functions of its configuration.
template <class H, class C, class Dev>
int particle_create(const C *cfg, const double *sensors_host, int64_t n_envs, int32_t device, void *state_dev, H **out,
                    void (*layout)(const C *, Dev *), size_t (*lds_bytes)(const Dev &)) {
    if (!sensors_host || !state_dev || !out || n_envs < 1) return fail(MADRL_EINVAL, "create: NULL argument or n_envs < 1");
    if (n_envs >= 0x7FF00000ll)  // the kernels index envs with 32-bit integers (index + workgroup count must stay below 2^31)
        return fail(MADRL_EINVAL, "n_envs=%lld is too large for one handle (limit 2146435071); shard the batch", (long long)n_envs);
    const int rc = check_env_ids(n_envs, cfg->env_id_base);
    if (rc) return rc;
    MADRL_HIP_TRY(hipSetDevice(device));
    H *h = new (std::nothrow) H();
    if (!h) return fail(MADRL_ENOMEM, "out of host memory");
    h->cfg = *cfg;
    h->device = device;
    layout(cfg, &h->dev);
    h->dev.n_envs = n_envs;
    h->dev.state = (float *)state_dev;
    h->lds_bytes = lds_bytes(h->dev);
    h->max_blocks = 0;
    if (h->lds_bytes > 64 * 1024) {
        const size_t need = h->lds_bytes;
        delete h;
        return fail(MADRL_EINVAL, "configuration needs %zu B of LDS (> 64 KiB)", need);
    }
    std::vector<float> sens(2 * (size_t)cfg->n_sensors);
    for (size_t k = 0; k < sens.size(); ++k) sens[k] = (float)sensors_host[k];  // float64 cos/sin rounded once
    hipError_t e = hipMalloc(&h->tables, sens.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->tables, sens.data(), sens.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (h->tables) (void)hipFree(h->tables);
        delete h;
        return fail(MADRL_EHIP, "sensor table upload failed: %s", hipGetErrorString(e));
    }
    h->dev.sensors = (const float *)h->tables;
    *out = h;
    return MADRL_OK;
}

// The rest of the two worlds' C ABI (madrl_waterworld_* / madrl_hostage_*) over a handle H.
template <class H>
int particle_kernel_kind(H *h, int32_t *out) {
    if (!h || !out) return fail(MADRL_EINVAL, "kernel_kind: NULL argument");
    *out = h->cfg.crowd ? 1 : 0;
    return MADRL_OK;
}

template <class H>
void particle_destroy(H *h) {
    if (!h) return;
    if (h->tables) (void)hipFree(h->tables);
    if (h->range_tables) (void)hipFree(h->range_tables);
    if (h->std_dev) (void)hipFree(h->std_dev);
    delete h;
}

template <class H>
int particle_set_launch(H *h, int64_t max_blocks) {
    if (!h || max_blocks < 0) return fail(MADRL_EINVAL, "set_launch: bad argument");
    h->max_blocks = max_blocks;
    return MADRL_OK;
}

// madrl_waterworld_set_particle_counts / madrl_hostage_set_particle_counts
// wave_live: the world's one-wavefront kernel has a live-count entry too (cfg.crowd = 0); it has no fused StandardizedEnv, so a bound one
// and the counts refuse each other (particle_set_standardize)
template <class H>
int particle_set_counts(H *h, const int32_t *pending_dev, int32_t *live_dev, bool wave_live = false) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    if (!h->cfg.crowd && !wave_live) return fail(MADRL_EINVAL, "set_particle_counts: per-env particle counts run on the crowd kernel (cfg.crowd = 1)");
    if ((pending_dev == nullptr) != (live_dev == nullptr))
        return fail(MADRL_EINVAL, "set_particle_counts: pending_dev and live_dev are both arrays or both NULL");
    if (live_dev != nullptr && h->ranged)
        return fail(MADRL_EINVAL, "set_particle_counts: per-pursuer sensor ranges are bound (set_sensor_ranges), and the live-count kernels take one range; unbind them first (set_sensor_ranges(NULL))");
    if (live_dev != nullptr && h->std_bound)
        return fail(MADRL_EINVAL, "set_particle_counts: a fused StandardizedEnv is bound, and the live-count kernel has none; unbind it first (set_standardize(NULL))");
    h->pending = pending_dev;
    h->live = live_dev;
    return MADRL_OK;
}

template <class H>
int particle_set_standardize(H *h, const madrl_standardize_args *a) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    if (!a) { h->std_bound = false; return MADRL_OK; }
    if (h->ranged)
        return fail(MADRL_EINVAL, "set_standardize: the ranged kernel (set_sensor_ranges) has no fused StandardizedEnv; use the epilogue kernels (madrl_wrap_obsnorm / madrl_wrap_rewnorm)");
    if (h->cfg.crowd)
        return fail(MADRL_EINVAL, "set_standardize: the crowd kernel has no fused StandardizedEnv; use the epilogue kernels (madrl_wrap_obsnorm / madrl_wrap_rewnorm)");
    if (h->live != nullptr)
        return fail(MADRL_EINVAL, "set_standardize: the live-count kernel (set_particle_counts) has no fused StandardizedEnv; use the epilogue kernels (madrl_wrap_obsnorm / madrl_wrap_rewnorm)");
    if (a->struct_size != (int32_t)sizeof(madrl_standardize_args))
        return fail(MADRL_EINVAL, "madrl_standardize_args.struct_size=%d, library expects %d", a->struct_size, (int)sizeof(madrl_standardize_args));
    if (!a->obs_out || (a->enable_obsnorm && (!a->obs_mean || !a->obs_var)) || (a->rew_out && a->enable_rewnorm && (!a->rew_mean || !a->rew_var)))
        return fail(MADRL_EINVAL, "set_standardize: obs_out and the running statistics of every enabled normalisation are required");
    ParticleStd st;
    st.obs_mean = a->obs_mean; st.obs_var = a->obs_var; st.obs_out = a->obs_out;
    st.rew_mean = a->rew_mean; st.rew_var = a->rew_var; st.rew_out = a->rew_out;
    st.obs_alpha = a->obs_alpha; st.rew_alpha = a->rew_alpha; st.eps = a->eps; st.scale = a->scale_reward;
    st.enable_obsnorm = a->enable_obsnorm; st.enable_rewnorm = a->enable_rewnorm;
    MADRL_HIP_TRY(hipSetDevice(h->device));
    if (!h->std_dev) MADRL_HIP_TRY(hipMalloc((void **)&h->std_dev, sizeof(ParticleStd)));
    MADRL_HIP_TRY(hipMemcpy(h->std_dev, &st, sizeof(ParticleStd), hipMemcpyHostToDevice));
    h->std_bound = true;
    return MADRL_OK;
}

// reset / step: the world's IO struct filled (both have these fields under these names) and handed to its launch(h, io, mode, stream),
// mode 0 = reset, 1 = step
template <class H, class IO>
int particle_reset(H *h, const uint8_t *mask_dev, float *obs_dev, void *stream, int (*launch)(const H *, const IO &, int, void *)) {
    if (!h || (!obs_dev && !h->std_bound)) return fail(MADRL_EINVAL, "reset: handle/obs is NULL");
    IO io;
    memset(&io, 0, sizeof(io));
    io.mask = mask_dev;
    io.obs = obs_dev;
    io.st = h->std_bound ? h->std_dev : nullptr;
    return launch(h, io, 0, stream);
}

template <class H, class IO>
int particle_step(H *h, const float *actions_dev, const float *inj_respawn_dev, float *obs_dev, float *rew_dev, uint8_t *done_dev,
                  int32_t *info_dev, void *stream, int (*launch)(const H *, const IO &, int, void *)) {
    if (!h || !actions_dev || (!obs_dev && !h->std_bound) || !rew_dev || !done_dev || !info_dev) return fail(MADRL_EINVAL, "step: NULL argument");
    IO io;
    memset(&io, 0, sizeof(io));
    io.actions = actions_dev;
    io.inj_resp = inj_respawn_dev;
    io.obs = obs_dev;
    io.st = h->std_bound ? h->std_dev : nullptr;
    io.rew = rew_dev;
    io.done = done_dev;
    io.info = info_dev;
    return launch(h, io, 1, stream);
}

// The half-precision entries (madrl_*_reset_f16 / madrl_*_step_f16) run the fixed-shape one-wavefront kernel alone and have no other
// output for the rows than `obs`: checked at every call, since the set_* calls of a handle know nothing of the entry that comes next.
template <class H>
int particle_half_ok(const H *h, const void *obs_dev, const char *what) {
    if (!h) return fail(MADRL_EINVAL, "%s: handle is NULL", what);
    if (!obs_dev) return fail(MADRL_EINVAL, "%s: obs is NULL (the half rows have no other destination)", what);
    if (h->cfg.crowd) return fail(MADRL_EINVAL, "%s: the crowd kernel (cfg.crowd = 1) has no half-precision rows; they run on the one-wavefront kernel", what);
    if (h->live != nullptr)
        return fail(MADRL_EINVAL, "%s: per-env particle counts are bound (set_particle_counts), and the live-count kernel has no half-precision rows; unbind them first (set_particle_counts(NULL, NULL))", what);
    if (h->ranged)
        return fail(MADRL_EINVAL, "%s: per-pursuer sensor ranges are bound (set_sensor_ranges), and the ranged kernel has no half-precision rows; unbind them first (set_sensor_ranges(NULL))", what);
    if (h->std_bound)
        return fail(MADRL_EINVAL, "%s: a fused StandardizedEnv is bound (set_standardize), and it has no half-precision rows; unbind it first (set_standardize(NULL))", what);
    return MADRL_OK;
}

}  // namespace madrl
