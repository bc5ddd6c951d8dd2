// multiwalker_layout.hpp -- where everything lives in the state buffer of a MultiWalker handle, written down ONCE: madrl_multiwalker_state_bytes
// returns mw_layout(..).total and create() points MwDev at its offsets (multiwalker_impl.hpp), so the size a caller allocates and the
// addresses the kernels write cannot drift apart.  Nothing of HIP in here: tests/host/multiwalker_layout_check.cpp builds it with the host
// compiler, once per capacity class (MW_CAPW / MW_NLANES as in multiwalker_c4 / _c8 / _c10.hip).
//
//   records      [n_envs] blocks of world_dw dwords: mw::World, then (scratch_off_dw) the schedule handed from launch to launch and the
//                step's manifold pool (scratch_bytes) -- what state_buffer / record_stride show the caller
//   pending      [n_envs] bytes: this env runs the reset + trailing step in the second pass
//   spare_state  [n_envs] records like the first region: the NEXT episode of every env, prepared ahead of time
//   spare_obs    [n_envs][W][obs_dim] float32: the observation reset returns for that episode
//   ready_step   [n_envs] dwords, dirty_list [2][n_envs] dwords, then four dwords: n_dirty[2], step_count, one unused
#pragma once
#include <stddef.h>

#include "multiwalker_core.hpp"

namespace MW_NS {

struct MwLayout {
    uint64_t records, pending, spare_state, spare_obs, ready_step, dirty_list, n_dirty, step_count, total;   // byte offsets; total: the buffer's size
    int32_t world_dw, scratch_off_dw, scratch_bytes;   // of one record
    int32_t cold_q;   // 16-byte words of mw::Cold in use (up to the last contact slot of this walker count)
};

constexpr uint64_t layout_up16(uint64_t v) { return (v + 15) / 16 * 16; }
constexpr int SOLVE_HDR_BYTES = (int)layout_up16(offsetof(Scratch, m_bA));   // the part of Scratch the solver and the continuous pass work on

// the static model of a walker count, as state_bytes and create() start from it
inline void host_model(Model &M, int n_walkers) {
    memset(&M, 0, sizeof(M));
    build_model(M, n_walkers);
}
// obs_dim_of (what the kernels index the observation rows with) for a configuration of which only one_hot is known yet
inline int host_obs_dim(int one_hot) {
    EnvCfg c;
    memset(&c, 0, sizeof(c));
    c.one_hot = one_hot ? 1 : 0;
    return obs_dim_of(c);
}

inline MwLayout mw_layout(const Model &M, int one_hot, int64_t n_envs) {
    const uint64_t n = (uint64_t)n_envs;
    MwLayout L;
    L.scratch_bytes = SOLVE_HDR_BYTES + (int32_t)layout_up16((uint64_t)M.max_manifolds * sizeof(Manifold));
    L.scratch_off_dw = (int32_t)(layout_up16(sizeof(World)) / 4);
    L.world_dw = L.scratch_off_dw + L.scratch_bytes / 4;
    L.cold_q = (int32_t)(layout_up16(offsetof(Cold, slot) + (uint64_t)M.n_slots * sizeof(Slot)) / 16);
    const uint64_t rec = (uint64_t)L.world_dw * 4;
    L.records = 0;
    L.pending = L.records + rec * n;
    L.spare_state = L.pending + layout_up16(n);
    L.spare_obs = L.spare_state + rec * n;
    L.ready_step = L.spare_obs + layout_up16((uint64_t)M.W * (uint64_t)host_obs_dim(one_hot) * 4 * n);
    L.dirty_list = L.ready_step + 4 * n;
    L.n_dirty = L.dirty_list + 8 * n;
    L.step_count = L.n_dirty + 8;   // (the third of the four dwords behind the lists)
    L.total = L.n_dirty + 16;
    return L;
}

}  // namespace MW_NS
