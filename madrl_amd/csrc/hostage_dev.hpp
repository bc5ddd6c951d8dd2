// hostage_dev.hpp -- the launch arguments of the hostage-world kernels, shared by hostage.hip (handle, validation, layout, dispatch, the
// one-wavefront kernel) and hostage_crowd.hip (the multi-wavefront kernel).
//
// The structs stay in the unnamed namespace: they are part of the mangled names of hostage_kernel<...>, which must not change.  Each
// translation unit therefore has its own (identical) copy of the types, and the one function that crosses the two files,
// hw_crowd_launch below, takes them as untyped pointers (as waterworld_dev.hpp does).
#pragma once

#include "common.hpp"

namespace {

using namespace madrl;

enum : uint32_t { HW_TAG_RESPAWN = 48, HW_TAG_RESET = 49 };

struct HwDev {
    int32_t Nr, Nh, Nc, NP, K, D;
    int32_t n_coop_save, addid, reward_global, key_fixed, max_steps, auto_reset;
    int32_t rec_dw;  // dwords per packed state record: pos[NP][2] vel[NP][2] key[2] bomb[2] saved_lo saved_hi flags t tick
    uint32_t k0, k1, gid_base;
    float radius, r_ho, bad_speed, sensor_range, action_scale, gate_lo;
    float save_reward, hit_reward, encounter_reward, not_saved_reward, bomb_reward, bomb_radius, key_radius, control_penalty;
    float key_x, key_y;
    // sq_*: sq_threshold() (common.hpp) of the distance thresholds: rescuer-hostage / rescuer-criminal contact, bomb and key radii
    float sq_hit_ho, sq_hit_cr, sq_bomb, sq_key;
    int64_t n_envs;
    const float *sensors;  // [K][2]
    float *state;
};

struct HwIO {
    const uint8_t *mask;    // reset mode
    const float *actions;   // [N][Nr][2]
    const float *inj_resp;  // [N][Nc][4] or NULL
    float *obs;             // [N][Nr][D]
    float *rew;             // [N][Nr]
    uint8_t *done;          // [N]
    int32_t *info;          // [N][2]  ho_saved, cr_encs
    const ParticleStd *st;  // device copy of the fused-wrapper arguments (common.hpp), or NULL (last: the offsets of the fields above stay)
};

}  // namespace

namespace madrl {

// hostage_crowd.hip.  dev / io: a HwDev and a HwIO (see the note at the top); mode 0 = reset, 1 = step.  live != NULL: the per-env
// particle counts of madrl_hostage_set_particle_counts (the kernels' live-count instantiations), the shape of dev being the capacity.
int hw_crowd_launch(const void *dev, const void *io, int mode, int64_t max_blocks, size_t lds_bytes, const int32_t *pending, int32_t *live,
                    void *stream);
// the dynamic LDS of one hw_crowd_kernel workgroup
size_t hw_crowd_lds_bytes(int n_good, int n_hostages, int n_bad, int n_sensors, int rec_dw);

}  // namespace madrl
