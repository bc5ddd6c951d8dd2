// hostage.hip -- batched ContinuousHostageWorld for MI355X (gfx950 / CDNA4), float32.
//
// Same execution model as waterworld.hip: one wavefront owns one env at a time (64-thread persistent workgroups striding
// over envs); the particles (rescuers | hostages | criminals: position + velocity), key, bomb, flags and the assembled
// observation rows live in LDS; HBM sees one packed state record in / out, the action row in and observation / reward /
// done / info rows out.  Lane roles per phase: particle lanes (integration, walls, gate, respawn, motion), (rescuer,
// object) collision pairs, (rescuer, sensor) sensing pairs -- the objects a sensor is tested against are broadcast once
// from the owning lane's registers (v_readlane -> SGPR operands) and reused by three passes of pairs held in registers.
//
// The device code shared with waterworld_kernel is in particle_wave.hpp (its opening comment has the scheme); this file is the hostage
// world's step in the reference's order and what is its own: the reset draws, gate, key and bomb, the saved mask and flags, the ballot
// form of the collision matrices (BITROWS), the row tail, rewards, respawn and done.
//
// The kernel's text is hostage_wave_body.inc, included inside two __global__ entries: hostage_kernel<...> (the instantiations as they were)
// and hostage_kernel_f16<...> (the same step with half-precision observation rows: madrl_hostage_reset_f16 / madrl_hostage_step_f16).
//
// Reference semantics (file:line under /root/reference/madrl_environments/hostage.py):
//   sensing ...... CircAgent.sensed :62-71     reset ...... ContinuousHostageWorld.reset :137-177 (ends with a zero-action step)
//   catch rule ... _caught :184-198             step ....... :228-430
// Quirks kept (G1..G9) are listed where they occur.  Arithmetic is float32, every expression keeps the statement order of the
// reference's step() so that a float32 CPU restatement agrees bit for bit.
#include "hostage_dev.hpp"
#include "particle_wave.hpp"   // the device code this kernel shares with waterworld_kernel (waterworld.hip)

#include <math.h>
#include <stddef.h>
#include <string.h>

// Profiling aid (scripts/variants.sh builds one library per value, never the shipped one):
//   1 no observation store   2 non-temporal observation store   4 no record store   8 no reward / done / info stores
#ifndef MADRL_HW_ABLATE
#define MADRL_HW_ABLATE 0
#endif
#ifndef MADRL_HW_WAVES
#define MADRL_HW_WAVES 7   // resident wavefronts per SIMD the SPECIALISED kernel's register allocation aims at (generic: compiler's choice).  Round 1 kernel: 117 VGPRs, 4 waves (at 5 it spilled
                           // 60 B per lane and the spill stores reached HBM).  With the launch parameters out of the SGPR file
                           // and the static LDS layout: 72 VGPRs, no scratch at 7 waves.  32 768 envs: 4 waves 55.2 us, 5 50.7, 6 48.0, 7 46.9.
#endif
// The fused-wrapper variants of the specialised kernel hold a batch of float64 statistics: fewer resident wavefronts, the most at which
// they have no scratch.  Step: 5 (at 6 it spills 4 VGPRs, 20 B of scratch per lane).  Reset: 6.
#ifndef MADRL_HW_FUSED_STEP_WAVES
#define MADRL_HW_FUSED_STEP_WAVES 5
#endif
#ifndef MADRL_HW_FUSED_RESET_WAVES
#define MADRL_HW_FUSED_RESET_WAVES 6
#endif

namespace {

using namespace madrl;

// Same register discipline as waterworld.hip (helpers in common.hpp): launch parameters are read from the kernel-argument segment
// where a phase needs them (kernargs), per-lane global accesses go through an SGPR base + 32-bit VGPR offset (uniform_ptr), a lane
// predicate is recomputed at its use (fresh) instead of being hoisted out of the env loop as an SGPR pair.
struct HwKArgs {
    HwDev d;
    HwIO io;
};
__device__ __forceinline__ float clipf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float bcast(float v, int src_lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane)); }

// MODE 0: reset(mask)   MODE 1: step (+ fused auto-reset)
// TNr..TK > 0: the particle / sensor counts are compile-time constants (small loops unroll, the index divisions fold); 0: generic.
// FUSED: the StandardizedEnv epilogue (ParticleStd, common.hpp) is compiled in; a template parameter and not a run-time branch because its float64 code
// would otherwise cost the plain kernel registers, i.e. resident wavefronts (measured on Waterworld: 96 instead of 78 us per step)
#define MADRL_HW_OCC_N (TNr > 0 ? (FUSED ? (MODE == 1 ? MADRL_HW_FUSED_STEP_WAVES : MADRL_HW_FUSED_RESET_WAVES) : MADRL_HW_WAVES) : 0)
template <int MODE, int TNr, int TNh, int TNc, int TK, int TD = 0, bool FUSED = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(MADRL_HW_OCC_N > 0 ? MADRL_HW_OCC_N : 1, MADRL_HW_OCC_N > 0 ? MADRL_HW_OCC_N : 8))) void hostage_kernel(const HwDev d, const HwIO io) {
#define MADRL_HW_BODY_HALF 0
#include "hostage_wave_body.inc"
#undef MADRL_HW_BODY_HALF
}

// The half-precision entry (BatchedContinuousHostageWorld(obs_dtype=torch.float16)): the same body with MADRL_HW_BODY_HALF set.  The step is
// hostage_kernel's, float32 from the record to the staged rows in LDS; the one thing that differs is how the rows leave -- as the
// round-to-nearest-even binary16 of each staged value (half_bits, common.hpp; store_rows_half, particle_wave.hpp), to a destination that is
// 2-byte aligned.  The half pointer travels in io.obs, cast.  The template parameters are hostage_kernel's, FUSED among them (the occupancy
// rule reads it): the specialised shape keeps the float32 kernel's MADRL_HW_WAVES.  No fused StandardizedEnv.
template <int MODE, int TNr, int TNh, int TNc, int TK, int TD = 0, bool FUSED = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(MADRL_HW_OCC_N > 0 ? MADRL_HW_OCC_N : 1, MADRL_HW_OCC_N > 0 ? MADRL_HW_OCC_N : 8))) void hostage_kernel_f16(const HwDev d, const HwIO io) {
    static_assert(!FUSED, "the half entries have no fused StandardizedEnv");
#define MADRL_HW_BODY_HALF 1
#include "hostage_wave_body.inc"
#undef MADRL_HW_BODY_HALF
}
#undef DA
#undef IOA
#undef MADRL_HW_OCC_N

}  // namespace

// =================================================================== host side / C ABI
struct madrl_hostage : ParticleHandle<madrl_hostage_config, HwDev> {};

namespace {

// The configuration grew by `crowd` (and a reserved word) at its end: a caller compiled against the struct without them passes the old
// struct_size and means crowd = 0.  -> *full: the whole struct, zero-extended, which everything after this function reads.
constexpr int32_t HW_CONFIG_SIZE_V1 = (int32_t)offsetof(madrl_hostage_config, crowd);

int hw_validate(const madrl_hostage_config *c, madrl_hostage_config *full) {
    if (!c) return fail(MADRL_EINVAL, "config is NULL");
    if (c->struct_size != (int32_t)sizeof(madrl_hostage_config) && c->struct_size != HW_CONFIG_SIZE_V1)
        return fail(MADRL_EINVAL, "madrl_hostage_config.struct_size=%d, library expects %d (or %d: the struct without crowd)", c->struct_size,
                    (int)sizeof(madrl_hostage_config), (int)HW_CONFIG_SIZE_V1);
    memset(full, 0, sizeof(*full));
    memcpy(full, c, (size_t)c->struct_size);
    full->struct_size = (int32_t)sizeof(madrl_hostage_config);
    c = full;
    if (c->crowd != 0 && c->crowd != 1) return fail(MADRL_EINVAL, "madrl_hostage_config.crowd must be 0 or 1 (got %d)", c->crowd);
    if (c->n_good < 1 || c->n_hostages < 1 || c->n_bad < 1) return fail(MADRL_EINVAL, "n_good, n_hostages, n_bad must be >= 1");
    if (c->crowd) {  // hw_crowd_kernel (hostage_crowd.hip): particles looped over the threads of a multi-wavefront workgroup
        if (c->n_good > 128) return fail(MADRL_EINVAL, "crowd kernel: n_good must be <= 128 (got %d)", c->n_good);
        if (c->n_hostages > 64) return fail(MADRL_EINVAL, "crowd kernel: n_hostages must be <= 64, the bits of the saved mask (got %d)", c->n_hostages);
        if ((int64_t)c->n_good + c->n_hostages + c->n_bad > 1023)
            return fail(MADRL_EINVAL, "crowd kernel: at most 1023 particles per env (got %lld)", (long long)c->n_good + c->n_hostages + c->n_bad);
    } else {
        // one wavefront per env; the packed record (4 * NP + 9 dwords) is prefetched as 4 dwords per lane
        if ((int64_t)c->n_good + c->n_hostages + c->n_bad > 61)
            return fail(MADRL_EINVAL, "at most 61 particles per env (one wavefront per env); crowd=1 runs up to 1023 on the multi-wavefront kernel");
        if (2 * c->n_good > 64) return fail(MADRL_EINVAL, "n_good must be <= 32");
    }
    if (c->n_sensors < 1 || c->n_sensors > 256) return fail(MADRL_EINVAL, "n_sensors must be in 1..256");
    if (c->n_coop_save < 1) return fail(MADRL_EINVAL, "n_coop_save must be >= 1");
    return MADRL_OK;
}

int hw_obs_dim_of(const madrl_hostage_config *c) { return c->n_sensors * 5 + 5 + (c->addid ? 1 : 0); }  // CircAgent.__init__ :19-23

void hw_layout(const madrl_hostage_config *c, HwDev *d) {
    memset(d, 0, sizeof(*d));
    d->Nr = c->n_good; d->Nh = c->n_hostages; d->Nc = c->n_bad; d->NP = d->Nr + d->Nh + d->Nc;
    d->K = c->n_sensors; d->D = hw_obs_dim_of(c);
    d->n_coop_save = c->n_coop_save; d->addid = c->addid; d->reward_global = c->reward_global; d->key_fixed = c->key_fixed;
    d->max_steps = c->max_steps; d->auto_reset = c->auto_reset;
    d->rec_dw = (int)align_up((size_t)4 * d->NP + 9, 4);
    d->k0 = (uint32_t)c->seed; d->k1 = (uint32_t)(c->seed >> 32); d->gid_base = (uint32_t)c->env_id_base;
    d->radius = (float)c->radius; d->r_ho = (float)(c->radius * 2); d->gate_lo = (float)(0.5 + c->radius);  // evaluated in float64 like the reference
    d->bad_speed = (float)c->bad_speed; d->sensor_range = (float)c->sensor_range; d->action_scale = (float)c->action_scale;
    d->save_reward = (float)c->save_reward; d->hit_reward = (float)c->hit_reward; d->encounter_reward = (float)c->encounter_reward;
    d->not_saved_reward = (float)c->not_saved_reward; d->bomb_reward = (float)c->bomb_reward; d->bomb_radius = (float)c->bomb_radius;
    d->key_radius = (float)c->key_radius; d->control_penalty = (float)c->control_penalty;
    d->key_x = (float)c->key_loc[0]; d->key_y = (float)c->key_loc[1];
    // the float32 sums the kernel used to form before comparing
    d->sq_hit_ho = sq_threshold(d->radius + d->r_ho); d->sq_hit_cr = sq_threshold(d->radius + d->radius);
    d->sq_bomb = sq_threshold(d->radius + d->bomb_radius); d->sq_key = sq_threshold(d->radius + d->key_radius);
}

size_t hw_lds_bytes(const HwDev &d) { return wave_lds_bytes(d.rec_dw, d.Nr, d.D, d.K, d.Nh, d.Nc); }

size_t hw_lds_bytes_crowd(const HwDev &d) { return hw_crowd_lds_bytes(d.Nr, d.Nh, d.Nc, d.K, d.rec_dw); }

int hw_launch(const madrl_hostage *h, const HwIO &io, int mode, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const HwDev &d = h->dev;
    if (h->cfg.crowd) return hw_crowd_launch(&h->dev, &io, mode, h->max_blocks, h->lds_bytes, h->pending, h->live, stream);
    const dim3 g = particle_grid(h->max_blocks, d.n_envs);
    const bool ex = d.Nr == 3 && d.Nh == 10 && d.Nc == 5 && d.K == 30 && d.D == 156;  // the module's own configuration (hostage.py:483), 30 sensors, agent id
    if (io.st != nullptr) {  // a bound StandardizedEnv: the instantiations with its epilogue
        if (mode == 0) {
            if (ex) hipLaunchKernelGGL((hostage_kernel<0, 3, 10, 5, 30, 156, true>), g, dim3(64), 0, s, h->dev, io);
            else hipLaunchKernelGGL((hostage_kernel<0, 0, 0, 0, 0, 0, true>), g, dim3(64), h->lds_bytes, s, h->dev, io);
        } else {
            if (ex) hipLaunchKernelGGL((hostage_kernel<1, 3, 10, 5, 30, 156, true>), g, dim3(64), 0, s, h->dev, io);
            else hipLaunchKernelGGL((hostage_kernel<1, 0, 0, 0, 0, 0, true>), g, dim3(64), h->lds_bytes, s, h->dev, io);
        }
    } else if (mode == 0) {
        if (ex) hipLaunchKernelGGL((hostage_kernel<0, 3, 10, 5, 30, 156>), g, dim3(64), 0, s, h->dev, io);
        else hipLaunchKernelGGL((hostage_kernel<0, 0, 0, 0, 0>), g, dim3(64), h->lds_bytes, s, h->dev, io);
    } else {
        if (ex) hipLaunchKernelGGL((hostage_kernel<1, 3, 10, 5, 30, 156>), g, dim3(64), 0, s, h->dev, io);
        else hipLaunchKernelGGL((hostage_kernel<1, 0, 0, 0, 0>), g, dim3(64), h->lds_bytes, s, h->dev, io);
    }
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}

// the half-precision entries: hostage_kernel_f16 on the handle's shape, the half pointer in io.obs (the caller has checked the handle:
// particle_half_ok)
int hw_launch_f16(const madrl_hostage *h, const HwIO &io, int mode, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const HwDev &d = h->dev;
    const dim3 g = particle_grid(h->max_blocks, d.n_envs);
    const bool ex = d.Nr == 3 && d.Nh == 10 && d.Nc == 5 && d.K == 30 && d.D == 156;  // the module's own configuration, as in hw_launch
    if (mode == 0) {
        if (ex) hipLaunchKernelGGL((hostage_kernel_f16<0, 3, 10, 5, 30, 156>), g, dim3(64), 0, s, h->dev, io);
        else hipLaunchKernelGGL((hostage_kernel_f16<0, 0, 0, 0, 0>), g, dim3(64), h->lds_bytes, s, h->dev, io);
    } else {
        if (ex) hipLaunchKernelGGL((hostage_kernel_f16<1, 3, 10, 5, 30, 156>), g, dim3(64), 0, s, h->dev, io);
        else hipLaunchKernelGGL((hostage_kernel_f16<1, 0, 0, 0, 0>), g, dim3(64), h->lds_bytes, s, h->dev, io);
    }
    MADRL_HIP_TRY(hipGetLastError());
    return MADRL_OK;
}

__global__ void hw_state_copy_kernel(const HwDev d, float *pos, float *vel, float *key, float *bomb, uint64_t *saved, uint8_t *flags, int32_t *t,
                                     uint32_t *tick, const int to_state) {
    const int64_t env = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (env >= d.n_envs) return;
    float *rec = d.state + env * (int64_t)d.rec_dw;
    uint32_t *ru = reinterpret_cast<uint32_t *>(rec);
    const int NP = d.NP;
    for (int k = 0; k < 2 * NP; ++k) {
        if (pos) { if (to_state) rec[k] = pos[env * 2 * NP + k]; else pos[env * 2 * NP + k] = rec[k]; }
        if (vel) { if (to_state) rec[2 * NP + k] = vel[env * 2 * NP + k]; else vel[env * 2 * NP + k] = rec[2 * NP + k]; }
    }
    for (int k = 0; k < 2; ++k) {
        if (key) { if (to_state) rec[4 * NP + k] = key[env * 2 + k]; else key[env * 2 + k] = rec[4 * NP + k]; }
        if (bomb) { if (to_state) rec[4 * NP + 2 + k] = bomb[env * 2 + k]; else bomb[env * 2 + k] = rec[4 * NP + 2 + k]; }
    }
    if (saved) {
        if (to_state) { ru[4 * NP + 4] = (uint32_t)saved[env]; ru[4 * NP + 5] = (uint32_t)(saved[env] >> 32); }
        else saved[env] = (uint64_t)ru[4 * NP + 4] | ((uint64_t)ru[4 * NP + 5] << 32);
    }
    if (flags) { if (to_state) ru[4 * NP + 6] = flags[env]; else flags[env] = (uint8_t)ru[4 * NP + 6]; }
    if (t) { if (to_state) ru[4 * NP + 7] = (uint32_t)t[env]; else t[env] = (int32_t)ru[4 * NP + 7]; }
    if (tick) { if (to_state) ru[4 * NP + 8] = tick[env]; else tick[env] = ru[4 * NP + 8]; }
}

}  // namespace

extern "C" {

int madrl_hostage_obs_dim(const madrl_hostage_config *cfg, int32_t *out_dim) {
    madrl_hostage_config full;
    int rc = hw_validate(cfg, &full);
    if (rc) return rc;
    if (!out_dim) return fail(MADRL_EINVAL, "out_dim is NULL");
    *out_dim = hw_obs_dim_of(&full);
    return MADRL_OK;
}

int madrl_hostage_state_bytes(const madrl_hostage_config *cfg, int64_t n_envs, uint64_t *out_bytes) {
    madrl_hostage_config full;
    int rc = hw_validate(cfg, &full);
    if (rc) return rc;
    if (n_envs < 1 || !out_bytes) return fail(MADRL_EINVAL, "n_envs must be >= 1 and out_bytes non-NULL");
    HwDev d;
    hw_layout(&full, &d);  // (the record does not depend on the kernel)
    *out_bytes = (uint64_t)d.rec_dw * 4u * (uint64_t)n_envs;
    return MADRL_OK;
}

int madrl_hostage_create(const madrl_hostage_config *cfg, const double *sensors_host, int64_t n_envs, int32_t device, void *state_dev,
                         madrl_hostage **out) {
    madrl_hostage_config full;
    int rc = hw_validate(cfg, &full);
    if (rc) return rc;
    return particle_create(&full, sensors_host, n_envs, device, state_dev, out, hw_layout, full.crowd ? hw_lds_bytes_crowd : hw_lds_bytes);
}

int madrl_hostage_kernel_kind(madrl_hostage *h, int32_t *out) { return particle_kernel_kind(h, out); }

void madrl_hostage_destroy(madrl_hostage *h) { particle_destroy(h); }

int madrl_hostage_set_standardize(madrl_hostage *h, const madrl_standardize_args *a) { return particle_set_standardize(h, a); }

int madrl_hostage_set_launch(madrl_hostage *h, int64_t max_blocks) { return particle_set_launch(h, max_blocks); }

int madrl_hostage_set_particle_counts(madrl_hostage *h, const int32_t *pending_dev, int32_t *live_dev) {
    return particle_set_counts(h, pending_dev, live_dev);
}

int madrl_hostage_reset(madrl_hostage *h, const uint8_t *mask_dev, float *obs_dev, void *stream) {
    return particle_reset(h, mask_dev, obs_dev, stream, hw_launch);
}

int madrl_hostage_step(madrl_hostage *h, const float *actions_dev, const float *inj_respawn_dev, float *obs_dev, float *rew_dev,
                       uint8_t *done_dev, int32_t *info_dev, void *stream) {
    return particle_step(h, actions_dev, inj_respawn_dev, obs_dev, rew_dev, done_dev, info_dev, stream, hw_launch);
}

int madrl_hostage_reset_f16(madrl_hostage *h, const uint8_t *mask_dev, uint16_t *obs_dev, void *stream) {
    const int rc = particle_half_ok(h, obs_dev, "madrl_hostage_reset_f16");
    if (rc) return rc;
    return particle_reset(h, mask_dev, reinterpret_cast<float *>(obs_dev), stream, hw_launch_f16);
}

int madrl_hostage_step_f16(madrl_hostage *h, const float *actions_dev, const float *inj_respawn_dev, uint16_t *obs_dev, float *rew_dev,
                           uint8_t *done_dev, int32_t *info_dev, void *stream) {
    const int rc = particle_half_ok(h, obs_dev, "madrl_hostage_step_f16");
    if (rc) return rc;
    return particle_step(h, actions_dev, inj_respawn_dev, reinterpret_cast<float *>(obs_dev), rew_dev, done_dev, info_dev, stream, hw_launch_f16);
}

int madrl_hostage_get_state(madrl_hostage *h, float *pos, float *vel, float *key, float *bomb, uint64_t *saved, uint8_t *flags, int32_t *t,
                            uint32_t *tick, void *stream) {
    return state_copy_launch(h, hw_state_copy_kernel, stream, pos, vel, key, bomb, saved, flags, t, tick, 0);
}

int madrl_hostage_set_state(madrl_hostage *h, const float *pos, const float *vel, const float *key, const float *bomb, const uint64_t *saved,
                            const uint8_t *flags, const int32_t *t, const uint32_t *tick, void *stream) {
    return state_copy_launch(h, hw_state_copy_kernel, stream, (float *)pos, (float *)vel, (float *)key, (float *)bomb, (uint64_t *)saved,
                             (uint8_t *)flags, (int32_t *)t, (uint32_t *)tick, 1);
}

}  // extern "C"
