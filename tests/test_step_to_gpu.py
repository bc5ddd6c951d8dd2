"""The two-buffer step: BatchedPursuitEvade.step_to / madrl_pursuit_step_to, and `obs_out=` of the other envs' step().

The yardstick is the in-place step, which the rest of the suite pins to the reference's goldens and the C oracle.  Every comparison is a
twin comparison, bit for bit (InPlaceTwins of tests/step_to_twins.py): two envs with the same seed and configuration, one stepping in
place, the other through a ring of three buffers with step_to.  Before the first reset the in-place buffer and the ring's first slot are
filled with 7.0, the ring's other slots with 101.0 and 102.0 (none of them an observation value), and the envs are told so
(invalidate_obs): every cell a step never stores is then visible, and so is a read from the wrong slot or a mask that claims "zero" for a
cell that holds 7.0."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import same_bits
from step_to_twins import DEV, Case, InPlaceTwins, agents, make_env

pytestmark = pytest.mark.gpu

N_ENVS, STEPS = 7, 12

# every case: seed 21, max_steps 3, two workgroups (make_env's defaults); `kind`: the kernel a step_to launches
CASES = {
    "X_10x10_2v2": Case("rect16", (10, 10), agents(2, 2, 3, 1), None, {}, kind="wave"),
    "X_16x16_8v30": Case("rect16", (16, 16), agents(8, 30, 7, 1, surround=True, n_catch=2), None, {}, kind="wave"),
    "X_16x16_8v30_hwc": Case("rect16", (16, 16), agents(8, 30, 7, 0), None, {}, kind="wave"),
    "X_window_gt_map": Case("rect16", (6, 6), agents(3, 5, 11, 0), None, {}, kind="wave"),   # window wider than the map: every row has kept cells
    "XC_20v300": Case("rect16", (24, 24), agents(20, 300, 9, 1, surround=True, n_catch=2), None, {}, kind="wave"),
    "XC_cnn48": Case("rect16", (48, 48), agents(100, 300, 21, 0, surround=True, n_catch=2), None, {}, kind="wave"),
    "XL_16x16_8v30": Case("rect16", (16, 16), agents(8, 30, 7, 1, per_env_counts=True),
                          [(8, 30), (7, 29), (4, 26), (1, 1), (8, 1), (1, 30), (5, 0)], {}, kind="wave"),
    "XLC_20v300": Case("rect16", (24, 24), agents(20, 300, 9, 1, per_env_counts=True),
                       [(20, 300), (19, 299), (4, 284), (1, 1), (20, 1), (1, 300), (12, 0)], {}, kind="wave"),
    "generic_unlisted_7v30": Case("rect16", (16, 16), agents(7, 30, 7, 1), None, {}, kind="generic"),
    "generic_no_id_dword_path": Case("rect16", (16, 16), agents(8, 30, 7, 1, include_id=False), None, {}, kind="generic"),
    "generic_XG_20v50": Case("rect16", (16, 16), agents(20, 50, 5, 1), None, {}, kind="generic"),
    "generic_evader_control": Case("rect16", (16, 16), agents(8, 12, 7, 1, train_pursuit=False), None, {}, kind="generic"),
    "kernel_generic_8v30": Case("rect16", (16, 16), agents(8, 30, 7, 1, kernel="generic"), None, {}, kind="generic"),
}


def _twins(name):
    return InPlaceTwins(CASES[name], n=N_ENVS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_to_equals_the_in_place_step(name):
    tw = _twins(name)
    assert tw.env.step_to_kernel_kind == tw.kind
    dones = 0
    for k in range(STEPS):
        if k == 4:
            tw.recount()
        tw.hop(k)
        dones += int((tw.ref._done != 0).sum())
    assert dones >= 3 * N_ENVS   # max_steps=3: fused resets, and their second observation pass, occurred
    if name in ("X_window_gt_map", "X_16x16_8v30_hwc", "XC_cnn48"):   # cells no step ever stores still hold the fill value, in the slot too
        assert bool((tw.ring[tw.at] == 7.0).any()) and not bool((tw.ring[tw.at] > 100.0).any())
    tw.check_state()
    assert tw.env.step_to_kernel_kind == tw.kind


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_to_kernel_kind(name):
    """'wave' exactly for the handles on a line of csrc/pursuit_to_specializations.def"""
    assert make_env(CASES[name], n=N_ENVS).step_to_kernel_kind == CASES[name].kind


@pytest.mark.parametrize("name", ["X_16x16_8v30", "X_16x16_8v30_hwc", "X_window_gt_map", "XC_cnn48", "XL_16x16_8v30", "XLC_20v300",
                                  "generic_unlisted_7v30"])
def test_knowledge_travels_with_the_buffer(name):
    """six hops, four in-place steps on the last slot without any invalidate, four more hops: what the fast path knows about the buffer
    (stale-zero masks, the channel-3 word) must describe the slot the env is on"""
    tw = _twins(name)
    for k in range(6):
        tw.hop(("hop", k))
    for k in range(4):
        tw.in_place(("in place", k))
    tw.recount()
    for k in range(4):
        tw.hop(("hop again", k))
    tw.check_state()


def test_argument_checks():
    from madrl_amd import _lib
    tw = _twins("X_16x16_8v30")
    env, act = tw.env, tw.actions()[0]
    cur = env.obs_buffer
    n = cur.numel()
    with pytest.raises(ValueError):
        env.step_to(act, torch.zeros(n, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        env.step_to(act, torch.zeros(n - 4, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        env.step_to(act, torch.zeros(n, dtype=torch.float32))   # another device
    with pytest.raises(ValueError):
        env.step_to(act, torch.zeros(2 * n, dtype=torch.float32, device=DEV)[::2])
    with pytest.raises(TypeError):
        env.step_to(act, np.zeros(n, np.float32))
    # overlapping, not identical: the tail of one allocation over its head
    big = torch.full((n + 64,), 7.0, dtype=torch.float32, device=DEV)
    big[:n].copy_(cur.reshape(-1))
    env2 = _twins("X_16x16_8v30").env
    env2.step_to(act, big[:n])   # (disjoint from the env's own buffer: fine)
    with pytest.raises(_lib.MadrlError):
        env2.step_to(act, big[64:])
    # NULL pointers through the C ABI
    L = _lib.lib()
    rew, dn, rm = env._rew, env._done, env._removed
    other = torch.zeros_like(cur)
    p = _lib.ptr
    stream = _lib.current_stream(env.device)
    assert L.madrl_pursuit_step_to(env._handle, p(act), None, None, p(other), p(rew), p(dn), p(rm), stream) != 0
    assert L.madrl_pursuit_step_to(env._handle, p(act), None, p(cur), None, p(rew), p(dn), p(rm), stream) != 0
    assert L.madrl_pursuit_step_to(env._handle, None, None, p(cur), p(other), p(rew), p(dn), p(rm), stream) != 0
    assert L.madrl_pursuit_step_to(None, p(act), None, p(cur), p(other), p(rew), p(dn), p(rm), stream) != 0
    assert L.madrl_pursuit_step_to_kernel_kind(env._handle, None) != 0
    out = C.c_int32(-1)
    assert L.madrl_pursuit_step_to_kernel_kind(env._handle, C.byref(out)) == 0 and out.value == _lib.KERNEL_WAVE
    # obs_out that IS the current buffer behaves as step()
    ra, rb = tw.ref.step(act), env.step_to(act, env.obs_buffer)
    tw.check_results(ra, rb, "same buffer")
    assert env.obs_buffer.data_ptr() == cur.data_ptr() and same_bits(cur, tw.ref.obs_buffer)
    # ... and step_into(obs_out=) is step_to()
    act = tw.actions()[0]
    ra = tw.ref.step(act)
    rew_slot, dn_slot = torch.zeros_like(rew), torch.zeros_like(dn)
    o = env.step_into(act, rew_slot, dn_slot, obs_out=other)
    assert o.data_ptr() == other.data_ptr() and same_bits(other, tw.ref.obs_buffer) and same_bits(rew_slot, ra[1]) and torch.equal(dn_slot, ra[3]["done_bits"])


def _other_envs():
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    from madrl_amd.multiwalker import BatchedMultiWalkerEnv
    from madrl_amd.waterworld import BatchedMAWaterWorld
    N = 33
    return {
        "waterworld": (lambda: BatchedMAWaterWorld(3, 10, n_poison=5, n_envs=N, device=DEV, seed=2, max_steps=8, auto_reset=True), 2),
        "hostage": (lambda: BatchedContinuousHostageWorld(3, 10, 5, 2, 2, n_envs=N, device=DEV, seed=2, max_steps=8, auto_reset=True), 2),
        "multiwalker": (lambda: BatchedMultiWalkerEnv(n_walkers=3, n_envs=N, device=DEV, seed=2, max_steps=8, auto_reset=True), 4),
    }


@pytest.mark.parametrize("world", ["waterworld", "hostage", "multiwalker"])
def test_obs_out_on_the_other_envs(world):
    mk, adim = _other_envs()[world]
    ref, env = mk(), mk()
    a, b = ref.reset(), env.reset()
    assert same_bits(a, b)
    ring = [torch.full_like(a, 101.0), torch.full_like(a, 102.0)]
    gen = torch.Generator(device="cpu").manual_seed(9)
    for k in range(20):
        act = (torch.rand(a.shape[:2] + (adim,), generator=gen) * 2 - 1).to(DEV)
        slot = ring[k % 2]
        ra, rb = ref.step(act), env.step(act, obs_out=slot.view(-1))   # (any contiguous tensor of the right size)
        assert rb[0].data_ptr() == slot.data_ptr() and rb[0].shape == ra[0].shape
        assert same_bits(slot, ra[0]) and same_bits(ra[1], rb[1]) and torch.equal(ra[2], rb[2]), k
    with pytest.raises(ValueError):
        env.step(act, obs_out=torch.zeros(a.numel() + 1, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        env.step(act, obs_out=torch.zeros(a.numel(), dtype=torch.float64, device=DEV))


def test_fused_standardisation_refuses_obs_out():
    from madrl_amd.waterworld import BatchedMAWaterWorld
    from madrl_amd.wrappers import StandardizedEnv
    raw = BatchedMAWaterWorld(3, 10, n_poison=5, n_envs=8, device=DEV, seed=2)
    w = StandardizedEnv(raw, enable_obsnorm=True)
    assert w._fused
    obs = w.reset()
    act = torch.zeros((8, 3, 2), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        raw.step(act, obs_out=torch.zeros_like(obs))
