// waterworld_dev.hpp -- the launch arguments of the Waterworld kernels, shared by waterworld.hip (handle, validation, layout, dispatch,
// the one-wavefront kernel), waterworld_f16.hip (its half-precision entry) and waterworld_crowd.hip (the multi-wavefront kernel).
//
// The structs stay in the unnamed namespace: they are part of the mangled names of waterworld_kernel<...>, which must not change.
// Each translation unit therefore has its own (identical) copy of the types, and the functions that cross the files,
// ww_crowd_launch and ww_f16_launch below, take them as untyped pointers.
#pragma once

#include "common.hpp"

namespace {

using namespace madrl;

enum : uint32_t { WW_TAG_RESPAWN = 16, WW_TAG_RESET = 17, WW_TAG_OBSTACLE = 18 };

struct WwDev {
    int32_t Np, Ne, Npo, NP, K, D, nfeat;
    int32_t n_coop, addid, speed_features, reward_global, obstacle_fixed, max_steps, auto_reset;
    int32_t rec_dw;  // dwords per packed state record: pos[NP][2] vel[NP][2] obst[2] t tick
    uint32_t k0, k1, gid_base;
    float r_pu, r_ev, r_po, obst_r, ev_speed, poison_speed, sensor_range, action_scale;
    float poison_reward, food_reward, encounter_reward, control_penalty;
    float obst_x, obst_y;
    // sq_*: sq_threshold() (common.hpp) of the distance thresholds: obstacle rebound per particle kind (:247-270), pursuer-evader /
    // pursuer-poison contact (:272-293)
    float sq_obst_pu, sq_obst_ev, sq_obst_po, sq_hit_ev, sq_hit_po;
    int64_t n_envs;
    const float *sensors;  // [K][2]
    float *state;
};

struct WwIO {
    const uint8_t *mask;    // reset mode
    const float *actions;   // [N][Np][2]
    const float *inj_resp;  // [N][NP][4] or NULL
    float *obs;             // [N][Np][D]
    float *rew;             // [N][Np]
    uint8_t *done;          // [N]
    int32_t *info;          // [N][2]  evcatches, pocatches
    const ParticleStd *st;  // device copy of the fused-wrapper arguments (common.hpp), or NULL
};

}  // namespace

namespace madrl {

// waterworld_crowd.hip.  dev / io: a WwDev and a WwIO (see the note at the top); mode 0 = reset, 1 = step.  live != NULL: the per-env
// particle counts of madrl_waterworld_set_particle_counts (the kernels' live-count instantiations), the shape of dev being the capacity.
// ranged: the per-pursuer sensor ranges of madrl_waterworld_set_sensor_ranges lie behind dev's sensor table and lds_bytes has room for them.
int ww_crowd_launch(const void *dev, const void *io, int mode, int64_t max_blocks, size_t lds_bytes, const int32_t *pending, int32_t *live,
                    bool ranged, void *stream);
// waterworld_f16.hip: waterworld_kernel_f16 on dev's shape (a line of waterworld_specializations.def: its specialised instantiation), io.obs
// holding the binary16 destination.  The caller has checked the handle: no crowd, counts, ranges or StandardizedEnv (particle_half_ok).
// *specialised: 1 / 0, whether the launch took a line's instantiation (madrl_waterworld_last_launch_kernel), written once it is enqueued.
int ww_f16_launch(const void *dev, const void *io, int mode, int64_t max_blocks, size_t lds_bytes, void *stream, int *specialised);
// the dynamic LDS of one ww_crowd_kernel workgroup
size_t ww_crowd_lds_bytes(int n_pursuers, int n_evaders, int n_poison, int n_sensors, int rec_dw);

}  // namespace madrl
