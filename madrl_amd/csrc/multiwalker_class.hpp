// multiwalker_class.hpp -- what multiwalker.hip (the C ABI) and one capacity class of the MultiWalker kernels (multiwalker_impl.hpp compiled
// with MW_CAPW / MW_NLANES) share: the handle's base, from which the class's own handle derives, and the class's three functions that
// run before a handle exists.  multiwalker.hip has validated every argument by the time it calls either.
#pragma once
#include <stdint.h>

#include "../../include/madrl_hip.h"

struct madrl_multiwalker {
    int32_t cap_walkers = 0, lanes = 0;   // of the class: n_walkers it has room for, lanes of a wavefront one env is spread over
    int32_t n_bodies = 0, n_terrain = 0, stride_bytes = 0, world_bytes = 0;   // set by create(): madrl_multiwalker_dims / _record_bytes
    int32_t fused = 0, use_spares = 1;    // madrl_multiwalker_set_mode
    madrl_multiwalker() = default;
    madrl_multiwalker(const madrl_multiwalker &) = delete;
    madrl_multiwalker &operator=(const madrl_multiwalker &) = delete;
    virtual ~madrl_multiwalker() {}   // madrl_multiwalker_destroy is `delete h`
    virtual int reset(const uint8_t *mask, const double *terrain, const double *push, float *obs, void *stream) = 0;
    virtual int step(const float *actions, float *obs, float *rew, uint8_t *done, void *stream) = 0;
    // flags rows [1 + 3W], or [2 + 3W] with_overflow (get_bodies / get_state)
    virtual int get_state(float *bodies, float *joints, float *aux, uint8_t *flags, int with_overflow, float *terrain, void *stream) = 0;
    virtual int set_state(const float *bodies, const float *joints, void *stream) = 0;
};

namespace madrl {

struct MwClass {
    int cap_walkers;   // n_walkers this class has room for
    int lanes;         // lanes of a wavefront one env is spread over
    int (*obs_dim)(int one_hot);
    uint64_t (*state_bytes)(const madrl_multiwalker_config *, int64_t n_envs);
    int (*create)(const madrl_multiwalker_config *, int64_t n_envs, int32_t device, void *state_dev, madrl_multiwalker **out);
};

}  // namespace madrl

extern const madrl::MwClass madrl_mw_class_c4, madrl_mw_class_c8, madrl_mw_class_c10;
