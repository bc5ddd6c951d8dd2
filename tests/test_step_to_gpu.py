"""The two-buffer step: BatchedPursuitEvade.step_to / madrl_pursuit_step_to, and `obs_out=` of the other envs' step().

The yardstick is the in-place step, which the rest of the suite pins to the reference's goldens and the C oracle.  Every comparison is a
twin comparison, bit for bit: two envs with the same seed and configuration, one stepping in place, the other through a ring of three
buffers with step_to.  Before the first reset the in-place buffer and the ring's first slot are filled with 7.0, the ring's other slots with
101.0 and 102.0 (none of them an observation value), and the envs are told so (invalidate_obs): every cell a step never stores is then
visible, and so is a read from the wrong slot or a mask that claims "zero" for a cell that holds 7.0."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ENVS, STEPS = 7, 12


def _maps(xs, ys):
    from madrl_amd.maps import rectangle_map
    return [rectangle_map(xs, ys)] if min(xs, ys) >= 16 else [np.zeros((xs, ys), np.int32)]


def _shape(xs, ys, p, e, r, fl, **kw):
    return dict(map=(xs, ys), n_pursuers=p, n_evaders=e, obs_range=r, flatten=bool(fl), **kw)


# name: (configuration, env kwargs, per-env counts or None, the kernel a step_to launches)
CASES = {
    "X_10x10_2v2": (_shape(10, 10, 2, 2, 3, 1), {}, None, "wave"),
    "X_16x16_8v30": (_shape(16, 16, 8, 30, 7, 1, surround=True, n_catch=2), {}, None, "wave"),
    "X_16x16_8v30_hwc": (_shape(16, 16, 8, 30, 7, 0), {}, None, "wave"),
    "X_window_gt_map": (_shape(6, 6, 3, 5, 11, 0), {}, None, "wave"),   # window wider than the map: every row has kept cells
    "XC_20v300": (_shape(24, 24, 20, 300, 9, 1, surround=True, n_catch=2), {}, None, "wave"),
    "XC_cnn48": (_shape(48, 48, 100, 300, 21, 0, surround=True, n_catch=2), {}, None, "wave"),
    "XL_16x16_8v30": (_shape(16, 16, 8, 30, 7, 1), dict(per_env_counts=True),
                      [(8, 30), (7, 29), (4, 26), (1, 1), (8, 1), (1, 30), (5, 0)], "wave"),
    "XLC_20v300": (_shape(24, 24, 20, 300, 9, 1), dict(per_env_counts=True),
                   [(20, 300), (19, 299), (4, 284), (1, 1), (20, 1), (1, 300), (12, 0)], "wave"),
    "generic_unlisted_7v30": (_shape(16, 16, 7, 30, 7, 1), {}, None, "generic"),
    "generic_no_id_dword_path": (_shape(16, 16, 8, 30, 7, 1, include_id=False), {}, None, "generic"),
    "generic_XG_20v50": (_shape(16, 16, 20, 50, 5, 1), {}, None, "generic"),
    "generic_evader_control": (_shape(16, 16, 8, 12, 7, 1, train_pursuit=False), {}, None, "generic"),
    "kernel_generic_8v30": (_shape(16, 16, 8, 30, 7, 1), dict(kernel="generic"), None, "generic"),
}


def _mk(cfg, n=N_ENVS, **kw):
    from madrl_amd.pursuit import BatchedPursuitEvade
    cfg = dict(cfg)
    xs, ys = cfg.pop("map")
    env = BatchedPursuitEvade(_maps(xs, ys), n_envs=n, device=DEV, seed=21, max_steps=3, auto_reset=True, **dict(cfg, **kw))
    env.set_launch(max_blocks=2)   # a workgroup walks several envs: the loop-carried state is exercised
    return env


class Twins(object):
    """`ref` steps in place; `env` steps through `ring`, whose first slot is its own buffer"""

    def __init__(self, name):
        cfg, kw, counts, self.kind = CASES[name]
        self.ref, self.env = _mk(cfg, **kw), _mk(cfg, **kw)
        self.P = int(self.ref.n_pursuers)
        self.n_act = self.P
        self.counts = counts
        for e in (self.ref, self.env):
            e.obs_buffer.fill_(7.0)
        first = self.env.obs_buffer
        self.ring = [first, torch.full_like(first, 101.0), torch.full_like(first, 102.0)]
        self.at = 0
        self.gen = torch.Generator(device="cpu").manual_seed(5)
        for e in (self.ref, self.env):
            e.invalidate_obs()
            if counts is not None:
                c = torch.tensor(counts, dtype=torch.int32, device=DEV)
                e.set_agent_counts(c[:, 0], c[:, 1])
        a, b = self.ref.reset(), self.env.reset()
        assert same_bits(a, b)

    def actions(self):
        return torch.randint(0, 5, (N_ENVS, self.n_act), generator=self.gen).to(torch.int32).to(DEV)

    def check_results(self, ra, rb, what):
        (oa, rwa, da, ia), (ob, rwb, db, ib) = ra, rb
        assert same_bits(oa, ob), (what, "observations")
        assert same_bits(rwa, rwb), (what, "rewards")
        assert torch.equal(da, db), (what, "done")
        for k in ("done_bits", "removed", "truncated", "count_overflow"):
            assert torch.equal(ia[k], ib[k]), (what, k)

    def hop(self, what):
        act = self.actions()
        nxt = (self.at + 1) % 3
        prev_before = self.ring[self.at].clone()
        ra = self.ref.step(act)
        rb = self.env.step_to(act, self.ring[nxt])
        self.check_results(ra, rb, what)
        assert rb[0].data_ptr() == self.ring[nxt].data_ptr() and self.env.obs_buffer.data_ptr() == self.ring[nxt].data_ptr()
        assert same_bits(self.ring[nxt], self.ref.obs_buffer), (what, "slot")
        assert same_bits(self.ring[self.at], prev_before), (what, "the previous slot was written")
        self.at = nxt

    def in_place(self, what):
        act = self.actions()
        self.check_results(self.ref.step(act), self.env.step(act), what)
        assert same_bits(self.ring[self.at], self.ref.obs_buffer), (what, "slot")

    def check_state(self):
        a, b = self.ref.get_state(), self.env.get_state()
        for k in a:
            assert torch.equal(a[k], b[k]), k

    def recount(self):
        """per-env counts: other pending counts, taken at each env's next fused reset (the row count of an env changes between the passes)"""
        if self.counts is None:
            return
        c = torch.tensor(self.counts[::-1], dtype=torch.int32, device=DEV)
        for e in (self.ref, self.env):
            e.set_agent_counts(c[:, 0], c[:, 1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_to_equals_the_in_place_step(name):
    tw = Twins(name)
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
    cfg, kw, counts, kind = CASES[name]
    assert _mk(cfg, **kw).step_to_kernel_kind == kind


@pytest.mark.parametrize("name", ["X_16x16_8v30", "X_16x16_8v30_hwc", "X_window_gt_map", "XC_cnn48", "XL_16x16_8v30", "XLC_20v300",
                                  "generic_unlisted_7v30"])
def test_knowledge_travels_with_the_buffer(name):
    """six hops, four in-place steps on the last slot without any invalidate, four more hops: what the fast path knows about the buffer
    (stale-zero masks, the channel-3 word) must describe the slot the env is on"""
    tw = Twins(name)
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
    tw = Twins("X_16x16_8v30")
    env, act = tw.env, tw.actions()
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
    env2 = Twins("X_16x16_8v30").env
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
    act = tw.actions()
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
