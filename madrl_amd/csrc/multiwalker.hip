// multiwalker.hip -- the MultiWalkerEnv entry points of include/madrl_hip.h: every argument is checked HERE, once, and the call goes on to
// the handle (a madrl_multiwalker, multiwalker_class.hpp: one derived type per capacity class) or, before a handle exists, to its class.
//
// The kernels exist in three capacity classes (multiwalker_c4.hip, _c8.hip, _c10.hip: the same source, multiwalker_impl.hpp, with room for
// 4 / 8 / 10 walkers on 4 / 8 / 16 lanes of a wavefront per env): per-env records, LDS blocks and register budgets are sized by the class,
// so three walkers do not pay for ten.  The reference's curriculum runs n_walkers = 2 .. 10 (lessons/multiwalker/env.yaml:1-27,
// runners/curriculum.py:56-91; multi_walker.py:286-301 scales the package and the terrain with n_walkers).  A handle belongs to the
// smallest class that holds its n_walkers; a change of n_walkers is a new handle (and a new state buffer) like in the reference, where
// `update_curriculum` builds a new env.
#include "common.hpp"
#include "multiwalker_class.hpp"

#include <stdlib.h>

namespace {

using namespace madrl;

// the one validation of a config: its size, and a class that holds its n_walkers
const MwClass *mw_class_of(const madrl_multiwalker_config *c) {
    if (!c) { (void)fail(MADRL_EINVAL, "config is NULL"); return nullptr; }
    if (c->struct_size != (int32_t)sizeof(madrl_multiwalker_config)) {
        (void)fail(MADRL_EINVAL, "madrl_multiwalker_config.struct_size=%d, library expects %d", c->struct_size, (int)sizeof(madrl_multiwalker_config));
        return nullptr;
    }
    const MwClass *classes[3] = {&madrl_mw_class_c4, &madrl_mw_class_c8, &madrl_mw_class_c10};
#ifdef MADRL_EXPERIMENTS   // measurement builds only (scripts/mw_occupancy.sh): run a walker count on a LARGER class than it needs (fewer envs per wavefront)
    if (const char *e = getenv("MADRL_MW_MIN_CLASS")) {
        const int want = atoi(e);
        for (const MwClass *k : classes) if (c->n_walkers >= 1 && c->n_walkers <= k->cap_walkers && k->cap_walkers >= want) return k;
    }
#endif
    if (c->n_walkers >= 1)
        for (const MwClass *k : classes) if (c->n_walkers <= k->cap_walkers) return k;
    (void)fail(MADRL_EINVAL, "n_walkers=%d unsupported (1..%d)", c->n_walkers, madrl_mw_class_c10.cap_walkers);
    return nullptr;
}

}  // namespace

extern "C" {

int madrl_multiwalker_obs_dim(const madrl_multiwalker_config *cfg, int32_t *out_dim) {
    const MwClass *k = mw_class_of(cfg);
    if (!k) return MADRL_EINVAL;
    if (!out_dim) return fail(MADRL_EINVAL, "out_dim is NULL");
    *out_dim = k->obs_dim(cfg->one_hot);
    return MADRL_OK;
}

int madrl_multiwalker_state_bytes(const madrl_multiwalker_config *cfg, int64_t n_envs, uint64_t *out_bytes) {
    const MwClass *k = mw_class_of(cfg);
    if (!k) return MADRL_EINVAL;
    if (n_envs < 1 || !out_bytes) return fail(MADRL_EINVAL, "n_envs must be >= 1 and out_bytes non-NULL");
    *out_bytes = k->state_bytes(cfg, n_envs);
    return MADRL_OK;
}

int madrl_multiwalker_create(const madrl_multiwalker_config *cfg, int64_t n_envs, int32_t device, void *state_dev, madrl_multiwalker **out) {
    const MwClass *k = mw_class_of(cfg);
    if (!k) return MADRL_EINVAL;
    if (!state_dev || !out || n_envs < 1) return fail(MADRL_EINVAL, "create: NULL argument or n_envs < 1");
    const int rc = check_env_ids(n_envs, cfg->env_id_base);
    return rc ? rc : k->create(cfg, n_envs, device, state_dev, out);
}

void madrl_multiwalker_destroy(madrl_multiwalker *h) { delete h; }   // (the class's destructor frees what its create() allocated)

int madrl_multiwalker_set_mode(madrl_multiwalker *h, int32_t fused, int32_t use_spares) {
    if (!h || (fused & ~1) || (use_spares & ~1)) return fail(MADRL_EINVAL, "set_mode: handle is NULL or a flag is not 0 / 1");
    h->fused = fused;
    h->use_spares = use_spares;
    return MADRL_OK;
}

int madrl_multiwalker_dims(const madrl_multiwalker *h, int32_t *n_bodies, int32_t *n_terrain) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    if (n_bodies) *n_bodies = h->n_bodies;
    if (n_terrain) *n_terrain = h->n_terrain;
    return MADRL_OK;
}

int madrl_multiwalker_record_bytes(const madrl_multiwalker *h, int32_t *stride_bytes, int32_t *world_bytes) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    if (stride_bytes) *stride_bytes = h->stride_bytes;
    if (world_bytes) *world_bytes = h->world_bytes;
    return MADRL_OK;
}

int madrl_multiwalker_lanes(const madrl_multiwalker *h, int32_t *cap_walkers, int32_t *lanes_per_env) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    if (cap_walkers) *cap_walkers = h->cap_walkers;
    if (lanes_per_env) *lanes_per_env = h->lanes;
    return MADRL_OK;
}

int madrl_multiwalker_reset(madrl_multiwalker *h, const uint8_t *mask_dev, float *obs_dev, void *stream) {
    return madrl_multiwalker_reset_with(h, mask_dev, nullptr, nullptr, obs_dev, stream);
}

int madrl_multiwalker_reset_with(madrl_multiwalker *h, const uint8_t *mask_dev, const double *terrain_dev, const double *push_dev,
                                 float *obs_dev, void *stream) {
    if (!h || !obs_dev) return fail(MADRL_EINVAL, "reset: handle/obs is NULL");
    return h->reset(mask_dev, terrain_dev, push_dev, obs_dev, stream);
}

int madrl_multiwalker_get_state(madrl_multiwalker *h, float *bodies_dev, float *joints_dev, float *aux_dev, uint8_t *flags_dev,
                                float *terrain_dev, void *stream) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    return h->get_state(bodies_dev, joints_dev, aux_dev, flags_dev, 1, terrain_dev, stream);
}

int madrl_multiwalker_set_state(madrl_multiwalker *h, const float *bodies_dev, const float *joints_dev, void *stream) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    return h->set_state(bodies_dev, joints_dev, stream);
}

int madrl_multiwalker_step(madrl_multiwalker *h, const float *actions_dev, float *obs_dev, float *rew_dev, uint8_t *done_dev, void *stream) {
    if (!h || !actions_dev || !obs_dev || !rew_dev || !done_dev) return fail(MADRL_EINVAL, "step: NULL argument");
    return h->step(actions_dev, obs_dev, rew_dev, done_dev, stream);
}

int madrl_multiwalker_get_bodies(madrl_multiwalker *h, float *bodies_dev, uint8_t *flags_dev, float *terrain_dev, void *stream) {
    if (!h) return fail(MADRL_EINVAL, "handle is NULL");
    return h->get_state(bodies_dev, nullptr, nullptr, flags_dev, 0, terrain_dev, stream);
}

}  // extern "C"
