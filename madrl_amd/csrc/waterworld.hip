// waterworld.hip -- batched MAWaterWorld for MI355X (gfx950 / CDNA4), float32.
//
// One wavefront owns one env at a time (64-thread workgroups, persistent, striding over
// envs).  The env's particles (pursuers | evaders | poisons: position + velocity), the
// obstacle and the assembled observation rows live in LDS; HBM sees one packed state record
// in / out, the action row in and observation / reward / done / info rows out.
//
// Lane roles change per phase:
//   particle phases   lane j < NP owns particle j (integration, walls, obstacle rebound,
//                     respawn, evader/poison motion);
//   collision phase   lane = (pursuer, evader) / (pursuer, poison) pair;
//   sensing phase     lane = (pursuer, sensor) pair, three passes of 64 pairs held in registers; the objects are
//                     broadcast once each from the owning lane's registers (v_readlane -> SGPR operands) and a
//                     conservative reach mask skips, per pass, the objects none of its pursuers can sense --
//                     the only O(Np*K*N) part (~4k ray tests before the cull).
// No dense contraction -> no MFMA.  ~40 kFLOP and 5.2 KB of HBM traffic per env-step: the
// kernel is VALU-issue bound, not HBM bound.
//
// Reference semantics (file:line under /root/reference/madrl_environments/pursuit/waterworld.py):
//   step phases ........ MAWaterWorld.step :220-436      sensing ...... Archea.sensed :64-72
//   catch rule ......... _caught :180-193                 respawn ...... _respawn :139-142, :355-374
//   reset .............. :144-172 (ends with a zero-action step, W11)
// The device code this kernel has in common with hostage_kernel (hostage.hip) -- the record pipeline, the action and control penalty, the
// generic path's collision bytes, the sensing passes, reach masks, ray test and bit walks, the fused StandardizedEnv epilogue -- is in
// particle_wave.hpp; this file is Waterworld's step in the reference's order and what is its own: the reset draws, the obstacle, the
// ballot form of the collision matrices (BITROWS), the row tail, rewards, respawn and done.
// Envs beyond a wavefront's worth of particles (more than 62, or more than 32 pursuers) run on ww_crowd_kernel (waterworld_crowd.hip) when
// the handle was created with cfg.crowd = 1; the handle, validation, record layout and dispatch of both kernels are in this file.
// The kernel's text is waterworld_wave_body.inc, included inside two __global__ entries: waterworld_kernel<...> (one shape for all envs, the
// instantiations as they were) and waterworld_kernel_live<MODE> (per-env particle counts within the handle's capacity,
// madrl_waterworld_set_particle_counts on a handle with cfg.crowd = 0: the generic body, the count arrays as a third argument) and
// waterworld_kernel_ranges<MODE> (a sensor range per pursuer, madrl_waterworld_set_sensor_ranges: the generic body, the ranges behind
// the sensor table).  waterworld_kernel_f16 (waterworld_f16.hip) is the fourth: the fixed-shape entry with half-precision observation rows.
// Arithmetic is float32 (north_star tolerance 1e-5 against the float64 reference); every
// expression keeps the statement order of the reference's step() so that a float32 CPU restatement agrees bit for bit.
#include "waterworld_wave.hpp"   // WwDev, WwIO, the views of the kernel-argument segment, the occupancy rule: shared with waterworld_f16.hip

#include <math.h>
#include <string.h>

namespace {

using namespace madrl;

// MODE 0: reset(mask)   MODE 1: step (+ fused auto-reset)
// TNp..TK > 0: the particle / sensor counts are compile-time constants (loops unroll, the index divisions fold); 0: generic.
// FUSED: the StandardizedEnv epilogue (ParticleStd, common.hpp) is compiled in; a template parameter because its float64 code would otherwise cost the
// plain kernel a wavefront per SIMD (132 instead of 119 VGPRs: 96 instead of 78 us per step)
template <int MODE, int TNp, int TNe, int TNpo, int TK, bool FUSED = false, int TD = 0>
__global__ __launch_bounds__(64) MADRL_WW_OCC void waterworld_kernel(const WwDev d, const WwIO io) {
#define MADRL_WW_BODY_LIVE 0
#define MADRL_WW_BODY_RANGES 0
#define MADRL_WW_BODY_HALF 0
#include "waterworld_wave_body.inc"
#undef MADRL_WW_BODY_HALF
#undef MADRL_WW_BODY_RANGES
#undef MADRL_WW_BODY_LIVE
}

// The live-count entry: the generic body (run-time counts, dynamic LDS, registers left to the compiler) on per-env counts within the capacity
// d.Np / d.Ne / d.Npo (madrl_waterworld_set_particle_counts on a handle with cfg.crowd = 0).  No fused StandardizedEnv.
template <int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void waterworld_kernel_live(const WwDev d, const WwIO io, const ParticleCounts cn) {
    constexpr int TNp = 0, TNe = 0, TNpo = 0, TK = 0, TD = 0;
    constexpr bool FUSED = false;
#define MADRL_WW_BODY_LIVE 1
#define MADRL_WW_BODY_RANGES 0
#define MADRL_WW_BODY_HALF 0
#include "waterworld_wave_body.inc"
#undef MADRL_WW_BODY_HALF
#undef MADRL_WW_BODY_RANGES
#undef MADRL_WW_BODY_LIVE
}

// The ranged entry: the generic body (run-time counts, dynamic LDS, registers left to the compiler) with a sensor range per pursuer
// (madrl_waterworld_set_sensor_ranges on a handle with cfg.crowd = 0).  d.sensors holds the ranges [Np] behind the sensor vectors, the
// workgroup's LDS up4(Np) floats more, and d.sensor_range their maximum.  Whatever the shape: no specialised form, no fused StandardizedEnv.
template <int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void waterworld_kernel_ranges(const WwDev d, const WwIO io) {
    constexpr int TNp = 0, TNe = 0, TNpo = 0, TK = 0, TD = 0;
    constexpr bool FUSED = false;
#define MADRL_WW_BODY_LIVE 0
#define MADRL_WW_BODY_RANGES 1
#define MADRL_WW_BODY_HALF 0
#include "waterworld_wave_body.inc"
#undef MADRL_WW_BODY_HALF
#undef MADRL_WW_BODY_RANGES
#undef MADRL_WW_BODY_LIVE
}
#undef DA
#undef IOA
#undef LANE_LT
#undef LANE_EQ

}  // namespace
// =================================================================== host side / C ABI
struct madrl_waterworld : ParticleHandle<madrl_waterworld_config, WwDev> {
    mutable int32_t last_launch = MADRL_WW_LAUNCH_NONE;  // the kernel family of the last reset / step launch (madrl_waterworld_last_launch_kernel)
};

namespace {

int ww_validate(const madrl_waterworld_config *c) {
    if (!c) return fail(MADRL_EINVAL, "config is NULL");
    if (c->struct_size != (int32_t)sizeof(madrl_waterworld_config))
        return fail(MADRL_EINVAL, "madrl_waterworld_config.struct_size=%d, library expects %d", c->struct_size,
                    (int)sizeof(madrl_waterworld_config));
    if (c->crowd != 0 && c->crowd != 1) return fail(MADRL_EINVAL, "madrl_waterworld_config.crowd must be 0 or 1 (got %d)", c->crowd);
    if (c->n_pursuers < 1 || c->n_evaders < 1 || c->n_poison < 1)
        return fail(MADRL_EINVAL, "n_pursuers, n_evaders, n_poison must be >= 1");
    if (c->crowd) {  // ww_crowd_kernel (waterworld_crowd.hip): particles looped over the threads of a multi-wavefront workgroup
        if (c->n_pursuers > 128) return fail(MADRL_EINVAL, "crowd kernel: n_pursuers must be <= 128 (got %d)", c->n_pursuers);
        if ((int64_t)c->n_pursuers + c->n_evaders + c->n_poison > 1023)
            return fail(MADRL_EINVAL, "crowd kernel: at most 1023 particles per env (got %lld)",
                        (long long)c->n_pursuers + c->n_evaders + c->n_poison);
    } else {
        if ((int64_t)c->n_pursuers + c->n_evaders + c->n_poison > 62)
            return fail(MADRL_EINVAL, "at most 62 particles per env (one wavefront per env); crowd=1 runs up to 1023 on the multi-wavefront kernel");
        if (2 * c->n_pursuers > 64) return fail(MADRL_EINVAL, "n_pursuers must be <= 32");
    }
    if (c->n_sensors < 1 || c->n_sensors > 256) return fail(MADRL_EINVAL, "n_sensors must be in 1..256");
    if (c->n_coop < 1) return fail(MADRL_EINVAL, "n_coop must be >= 1");
    return MADRL_OK;
}

int ww_obs_dim_of(const madrl_waterworld_config *c) {
    return c->n_sensors * (c->speed_features ? 7 : 4) + 2 + (c->addid ? 1 : 0);  // Archea.__init__ :18-24
}

void ww_layout(const madrl_waterworld_config *c, WwDev *d) {
    memset(d, 0, sizeof(*d));
    d->Np = c->n_pursuers; d->Ne = c->n_evaders; d->Npo = c->n_poison; d->NP = d->Np + d->Ne + d->Npo;
    d->K = c->n_sensors; d->D = ww_obs_dim_of(c); d->nfeat = c->speed_features ? 7 : 4;
    d->n_coop = c->n_coop; d->addid = c->addid; d->speed_features = c->speed_features;
    d->reward_global = c->reward_global; d->obstacle_fixed = c->obstacle_fixed; d->max_steps = c->max_steps;
    d->auto_reset = c->auto_reset;
    d->rec_dw = (int)align_up((size_t)4 * d->NP + 4, 4);
    d->k0 = (uint32_t)c->seed; d->k1 = (uint32_t)(c->seed >> 32); d->gid_base = (uint32_t)c->env_id_base;
    // radii: pursuer r, evader 2r, poison 3r/4, evaluated in float64 like the reference (:108-118)
    d->r_pu = (float)c->radius; d->r_ev = (float)(c->radius * 2); d->r_po = (float)(c->radius * 3 / 4);
    d->obst_r = (float)c->obstacle_radius; d->ev_speed = (float)c->ev_speed; d->poison_speed = (float)c->poison_speed;
    d->sensor_range = (float)c->sensor_range; d->action_scale = (float)c->action_scale;
    d->poison_reward = (float)c->poison_reward; d->food_reward = (float)c->food_reward;
    d->encounter_reward = (float)c->encounter_reward; d->control_penalty = (float)c->control_penalty;
    d->obst_x = (float)c->obstacle_loc[0]; d->obst_y = (float)c->obstacle_loc[1];
    // the float32 sums are the ones the kernel used to form before comparing (pr + obst_r, r_pu + r_ev, r_pu + r_po)
    d->sq_obst_pu = sq_threshold(d->r_pu + d->obst_r); d->sq_obst_ev = sq_threshold(d->r_ev + d->obst_r);
    d->sq_obst_po = sq_threshold(d->r_po + d->obst_r);
    d->sq_hit_ev = sq_threshold(d->r_pu + d->r_ev); d->sq_hit_po = sq_threshold(d->r_pu + d->r_po);
}

size_t ww_lds_bytes(const WwDev &d) { return wave_lds_bytes(d.rec_dw, d.Np, d.D, d.K, d.Ne, d.Npo); }

size_t ww_lds_bytes_crowd(const WwDev &d) { return ww_crowd_lds_bytes(d.Np, d.Ne, d.Npo, d.K, d.rec_dw); }

struct WwSpec {
    int Np, Ne, Npo, K, D;
    void (*launch)(const WwDev &, const WwIO &, int mode, bool fused, dim3 g, hipStream_t s);
};

template <int TNp, int TNe, int TNpo, int TK, int TD>
void ww_launch_spec(const WwDev &d, const WwIO &io, int mode, bool fused, dim3 g, hipStream_t s) {
    const dim3 b(64);  // static LDS layout: 0 dynamic bytes
    if (mode == 0) {
        if (fused) hipLaunchKernelGGL((waterworld_kernel<0, TNp, TNe, TNpo, TK, true, TD>), g, b, 0, s, d, io);
        else hipLaunchKernelGGL((waterworld_kernel<0, TNp, TNe, TNpo, TK, false, TD>), g, b, 0, s, d, io);
    } else {
        if (fused) hipLaunchKernelGGL((waterworld_kernel<1, TNp, TNe, TNpo, TK, true, TD>), g, b, 0, s, d, io);
        else hipLaunchKernelGGL((waterworld_kernel<1, TNp, TNe, TNpo, TK, false, TD>), g, b, 0, s, d, io);
    }
}

#define X(NP_, NE_, NPO_, K_, D_) {NP_, NE_, NPO_, K_, D_, ww_launch_spec<NP_, NE_, NPO_, K_, D_>},
const WwSpec WW_SPECS[] = {
#include "waterworld_specializations.def"
#if __has_include("waterworld_specializations.local.def")   // shapes added on this machine by `python -m madrl_amd.build --waterworld-shape ...` (git-ignored)
#include "waterworld_specializations.local.def"
#endif
};
#undef X

int ww_launch(const madrl_waterworld *h, const WwIO &io, int mode, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const WwDev &d = h->dev;
    if (h->cfg.crowd) {
        const int rc = ww_crowd_launch(&h->dev, &io, mode, h->max_blocks, h->lds_bytes, h->pending, h->live, h->ranged, stream);
        if (rc == MADRL_OK) h->last_launch = MADRL_WW_LAUNCH_CROWD;
        return rc;
    }
    const dim3 g = particle_grid(h->max_blocks, d.n_envs), b(64);
    const bool fused = io.st != nullptr;
    if (h->live != nullptr) {  // per-env particle counts: the generic body at the capacity's LDS bytes, whatever the shape
        if (fused) return fail(MADRL_EINVAL, "the live-count kernel has no fused StandardizedEnv");
        const ParticleCounts cn{h->pending, h->live};
        if (mode == 0) hipLaunchKernelGGL(waterworld_kernel_live<0>, g, b, h->lds_bytes, s, h->dev, io, cn);
        else hipLaunchKernelGGL(waterworld_kernel_live<1>, g, b, h->lds_bytes, s, h->dev, io, cn);
        MADRL_HIP_TRY(hipGetLastError());
        h->last_launch = MADRL_WW_LAUNCH_LIVE;
        return MADRL_OK;
    }
    if (h->ranged) {  // per-pursuer sensor ranges: the generic body with the ranges in LDS, whatever the shape
        if (fused) return fail(MADRL_EINVAL, "the ranged kernel has no fused StandardizedEnv");
        if (mode == 0) hipLaunchKernelGGL(waterworld_kernel_ranges<0>, g, b, h->lds_bytes, s, h->dev, io);
        else hipLaunchKernelGGL(waterworld_kernel_ranges<1>, g, b, h->lds_bytes, s, h->dev, io);
        MADRL_HIP_TRY(hipGetLastError());
        h->last_launch = MADRL_WW_LAUNCH_RANGED;
        return MADRL_OK;
    }
    const WwSpec *spec = nullptr;
    for (const WwSpec &w : WW_SPECS)
        if (d.Np == w.Np && d.Ne == w.Ne && d.Npo == w.Npo && d.K == w.K && d.D == w.D) spec = &w;
    if (spec) {
        spec->launch(h->dev, io, mode, fused, g, s);
    } else if (mode == 0) {
        if (fused) hipLaunchKernelGGL((waterworld_kernel<0, 0, 0, 0, 0, true>), g, b, h->lds_bytes, s, h->dev, io);
        else hipLaunchKernelGGL((waterworld_kernel<0, 0, 0, 0, 0, false>), g, b, h->lds_bytes, s, h->dev, io);
    } else {
        if (fused) hipLaunchKernelGGL((waterworld_kernel<1, 0, 0, 0, 0, true>), g, b, h->lds_bytes, s, h->dev, io);
        else hipLaunchKernelGGL((waterworld_kernel<1, 0, 0, 0, 0, false>), g, b, h->lds_bytes, s, h->dev, io);
    }
    MADRL_HIP_TRY(hipGetLastError());
    h->last_launch = spec ? MADRL_WW_LAUNCH_SPECIALISED : MADRL_WW_LAUNCH_GENERIC;
    return MADRL_OK;
}

// the half-precision entries: waterworld_kernel_f16 (waterworld_f16.hip) on the handle's shape, the half pointer in io.obs
int ww_launch_f16(const madrl_waterworld *h, const WwIO &io, int mode, void *stream) {
    int specialised = 0;
    const int rc = ww_f16_launch(&h->dev, &io, mode, h->max_blocks, h->lds_bytes, stream, &specialised);
    if (rc == MADRL_OK) h->last_launch = specialised ? MADRL_WW_LAUNCH_SPECIALISED : MADRL_WW_LAUNCH_GENERIC;
    return rc;
}

__global__ void ww_state_copy_kernel(const WwDev d, float *pos, float *vel, float *obst, int32_t *t, uint32_t *tick,
                                     const int to_state) {
    const int64_t env = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (env >= d.n_envs) return;
    float *rec = d.state + env * (int64_t)d.rec_dw;
    const int NP = d.NP;
    for (int k = 0; k < 2 * NP; ++k) {
        if (pos) { if (to_state) rec[k] = pos[env * 2 * NP + k]; else pos[env * 2 * NP + k] = rec[k]; }
        if (vel) { if (to_state) rec[2 * NP + k] = vel[env * 2 * NP + k]; else vel[env * 2 * NP + k] = rec[2 * NP + k]; }
    }
    for (int k = 0; k < 2; ++k)
        if (obst) { if (to_state) rec[4 * NP + k] = obst[env * 2 + k]; else obst[env * 2 + k] = rec[4 * NP + k]; }
    int32_t *ti = reinterpret_cast<int32_t *>(rec) + 4 * NP + 2;
    uint32_t *tk = reinterpret_cast<uint32_t *>(rec) + 4 * NP + 3;
    if (t) { if (to_state) *ti = t[env]; else t[env] = *ti; }
    if (tick) { if (to_state) *tk = tick[env]; else tick[env] = *tk; }
}

}  // namespace

extern "C" {

int madrl_waterworld_obs_dim(const madrl_waterworld_config *cfg, int32_t *out_dim) {
    int rc = ww_validate(cfg);
    if (rc) return rc;
    if (!out_dim) return fail(MADRL_EINVAL, "out_dim is NULL");
    *out_dim = ww_obs_dim_of(cfg);
    return MADRL_OK;
}

int madrl_waterworld_state_bytes(const madrl_waterworld_config *cfg, int64_t n_envs, uint64_t *out_bytes) {
    int rc = ww_validate(cfg);
    if (rc) return rc;
    if (n_envs < 1 || !out_bytes) return fail(MADRL_EINVAL, "n_envs must be >= 1 and out_bytes non-NULL");
    WwDev d;
    ww_layout(cfg, &d);
    *out_bytes = (uint64_t)d.rec_dw * 4u * (uint64_t)n_envs;
    return MADRL_OK;
}

int madrl_waterworld_create(const madrl_waterworld_config *cfg, const double *sensors_host, int64_t n_envs,
                            int32_t device, void *state_dev, madrl_waterworld **out) {
    int rc = ww_validate(cfg);
    if (rc) return rc;
    return particle_create(cfg, sensors_host, n_envs, device, state_dev, out, ww_layout, cfg->crowd ? ww_lds_bytes_crowd : ww_lds_bytes);
}

int madrl_waterworld_kernel_kind(madrl_waterworld *h, int32_t *out) { return particle_kernel_kind(h, out); }

int madrl_waterworld_last_launch_kernel(const madrl_waterworld *h, int32_t *out) {
    if (!h || !out) return fail(MADRL_EINVAL, "last_launch_kernel: NULL argument");
    *out = h->last_launch;
    return MADRL_OK;
}

void madrl_waterworld_destroy(madrl_waterworld *h) { particle_destroy(h); }

int madrl_waterworld_set_standardize(madrl_waterworld *h, const madrl_standardize_args *a) { return particle_set_standardize(h, a); }

int madrl_waterworld_set_launch(madrl_waterworld *h, int64_t max_blocks) { return particle_set_launch(h, max_blocks); }

int madrl_waterworld_set_particle_counts(madrl_waterworld *h, const int32_t *pending_dev, int32_t *live_dev) {
    return particle_set_counts(h, pending_dev, live_dev, /*wave_live=*/true);
}

int madrl_waterworld_set_sensor_ranges(madrl_waterworld *h, const double *ranges_host) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    const size_t base_lds = h->cfg.crowd ? ww_lds_bytes_crowd(h->dev) : ww_lds_bytes(h->dev);
    if (!ranges_host) {  // back to cfg.sensor_range and the dispatch the handle had
        h->ranged = false;
        h->dev.sensors = (const float *)h->tables;
        h->dev.sensor_range = (float)h->cfg.sensor_range;
        h->lds_bytes = base_lds;
        return MADRL_OK;
    }
    if (h->live != nullptr)
        return fail(MADRL_EINVAL, "set_sensor_ranges: per-env particle counts are bound (set_particle_counts), and the live-count kernels take one range; unbind them first (set_particle_counts(NULL, NULL))");
    if (h->std_bound)
        return fail(MADRL_EINVAL, "set_sensor_ranges: a fused StandardizedEnv is bound (set_standardize), and the ranged kernel has none; unbind it first (set_standardize(NULL))");
    const int Np = h->dev.Np, sen = up4(2 * h->dev.K);  // the ranges lie behind the sensor vectors [K][2], on a 16-byte boundary
    std::vector<float> tab((size_t)sen + up4(Np), 0.0f);
    float top = 0.0f;
    for (int i = 0; i < Np; ++i) {
        if (!(ranges_host[i] > 0.0) || !isfinite(ranges_host[i]))
            return fail(MADRL_EINVAL, "set_sensor_ranges: ranges[%d]=%g must be finite and > 0", i, ranges_host[i]);
        const float r = (float)ranges_host[i];  // rounded once, like cfg.sensor_range (ww_layout)
        if (!(r > 0.0f) || !isfinite(r)) return fail(MADRL_EINVAL, "set_sensor_ranges: ranges[%d]=%g is no positive finite float32", i, ranges_host[i]);
        tab[sen + i] = r;
        top = r > top ? r : top;
    }
    const size_t lds = base_lds + (size_t)up4(Np) * 4;
    if (lds > 64 * 1024) return fail(MADRL_EINVAL, "set_sensor_ranges: configuration needs %zu B of LDS (> 64 KiB)", lds);
    MADRL_HIP_TRY(hipSetDevice(h->device));
    MADRL_HIP_TRY(hipMemcpy(tab.data(), h->tables, (size_t)2 * h->dev.K * sizeof(float), hipMemcpyDeviceToHost));
    if (!h->range_tables) MADRL_HIP_TRY(hipMalloc(&h->range_tables, tab.size() * sizeof(float)));
    MADRL_HIP_TRY(hipMemcpy(h->range_tables, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    h->dev.sensors = (const float *)h->range_tables;
    h->dev.sensor_range = top;  // the reach cull runs on it: conservative for every pursuer; the ray test takes the pursuer's own
    h->lds_bytes = lds;
    h->ranged = true;
    return MADRL_OK;
}

int madrl_waterworld_reset(madrl_waterworld *h, const uint8_t *mask_dev, float *obs_dev, void *stream) {
    return particle_reset(h, mask_dev, obs_dev, stream, ww_launch);
}

int madrl_waterworld_step(madrl_waterworld *h, const float *actions_dev, const float *inj_respawn_dev, float *obs_dev,
                          float *rew_dev, uint8_t *done_dev, int32_t *info_dev, void *stream) {
    return particle_step(h, actions_dev, inj_respawn_dev, obs_dev, rew_dev, done_dev, info_dev, stream, ww_launch);
}

int madrl_waterworld_reset_f16(madrl_waterworld *h, const uint8_t *mask_dev, uint16_t *obs_dev, void *stream) {
    const int rc = particle_half_ok(h, obs_dev, "madrl_waterworld_reset_f16");
    if (rc) return rc;
    return particle_reset(h, mask_dev, reinterpret_cast<float *>(obs_dev), stream, ww_launch_f16);
}

int madrl_waterworld_step_f16(madrl_waterworld *h, const float *actions_dev, const float *inj_respawn_dev, uint16_t *obs_dev,
                              float *rew_dev, uint8_t *done_dev, int32_t *info_dev, void *stream) {
    const int rc = particle_half_ok(h, obs_dev, "madrl_waterworld_step_f16");
    if (rc) return rc;
    return particle_step(h, actions_dev, inj_respawn_dev, reinterpret_cast<float *>(obs_dev), rew_dev, done_dev, info_dev, stream, ww_launch_f16);
}

int madrl_waterworld_get_state(madrl_waterworld *h, float *pos, float *vel, float *obst, int32_t *t, uint32_t *tick,
                               void *stream) {
    return state_copy_launch(h, ww_state_copy_kernel, stream, pos, vel, obst, t, tick, 0);
}

int madrl_waterworld_set_state(madrl_waterworld *h, const float *pos, const float *vel, const float *obst,
                               const int32_t *t, const uint32_t *tick, void *stream) {
    return state_copy_launch(h, ww_state_copy_kernel, stream, (float *)pos, (float *)vel, (float *)obst, (int32_t *)t, (uint32_t *)tick, 1);
}

}  // extern "C"
