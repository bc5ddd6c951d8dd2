"""GPU tests (-m gpu) of the half-precision observation rows of the particle worlds: BatchedMAWaterWorld / BatchedContinuousHostageWorld with
obs_dtype=torch.float16 (waterworld_kernel_f16, hostage_kernel_f16) and WaterworldHeuristicPolicy(obs_dtype=torch.float16).

The float32 kernels are pinned to the reference by the other suites; here the half rows are pinned to the float32 kernels BIT FOR BIT, with
no tolerance anywhere.  Twins: a float32 env F and a half env H run the same case (seed, env_id_base, actions, max_blocks); after every
reset and every step H's rows are the round-to-nearest-even halves of F's (torch's .to(float16): subnormals kept, so a truncating or
flushing conversion fails), and rewards, done, info and every key of the state are equal.  Shapes: the smallest at which the row store can
go wrong -- rows shorter than one 16-byte chunk, one chunk and a tail, odd element counts (every env's rows then start on another 2-byte
boundary), the generic and the specialised instantiations -- with few workgroups, so that a wavefront walks several envs, and a short
max_steps with auto_reset, so that the fused auto-reset pass stores rows too."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from step_to_twins import as_half_bits, b16, same16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32 = torch.float16, torch.float32
NAN16 = 0x7E5A   # a quiet NaN no row holds: what a slot and its guards are filled with

WW_KW = dict(radius=0.03, ev_speed=0.03, action_scale=0.03)   # large and fast particles: catches and respawns within a few steps
# name -> (world, constructor arguments, n envs, elements per env)
CASES = {
    "ww_tail_only": ("ww", dict(n_pursuers=1, n_evaders=1, n_poison=1, n_coop=1, n_sensors=1, speed_features=False, addid=False), 7, 6),
    "ww_chunk_and_tail": ("ww", dict(n_pursuers=1, n_evaders=1, n_poison=1, n_coop=1, n_sensors=1), 7, 10),
    "ww_generic_odd": ("ww", dict(n_pursuers=3, n_evaders=4, n_poison=4, n_sensors=4), 7, 93),
    "ww_configs2": ("ww", dict(n_pursuers=5, n_evaders=10, n_poison=10, n_sensors=30), 13, 1065),
    "hw_generic_11": ("hw", dict(n_good=1, n_hostages=1, n_bad=1, n_coop_save=1, n_coop_avoid=1, n_sensors=1), 7, 11),
    "hw_generic_105": ("hw", dict(n_good=5, n_hostages=3, n_bad=4, n_coop_save=2, n_coop_avoid=2, n_sensors=3), 7, 105),
    "hw_default": ("hw", dict(n_good=3, n_hostages=10, n_bad=5, n_coop_save=2, n_coop_avoid=2, n_sensors=30), 13, 468),
}


def make(case, dtype, n=None, seed=11, env_id_base=5, max_steps=3, max_blocks=2, **kw):
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    from madrl_amd.waterworld import BatchedMAWaterWorld
    world, args, n_case, n_el = CASES[case]
    extra = {} if dtype is F32 else dict(obs_dtype=dtype)   # (F is built as every float32 env was before the flag existed)
    cls, base = (BatchedMAWaterWorld, WW_KW) if world == "ww" else (BatchedContinuousHostageWorld, {})
    env = cls(n_envs=n or n_case, device=DEV, seed=seed, env_id_base=env_id_base, max_steps=max_steps, auto_reset=True, max_blocks=max_blocks,
              **dict(base, **args), **extra, **kw)
    assert env._obs[0].numel() == n_el and env._obs.dtype is dtype
    return env


class Twins(object):
    def __init__(self, case, **kw):
        self.F, self.H = make(case, F32, **kw), make(case, F16, **kw)
        self.g = torch.Generator(device="cpu").manual_seed(3)
        self.agents = self.F._obs.shape[1]
        assert self.H.obs_dtype is F16 and self.F.obs_dtype is F32 and self.H.kernel_kind == "wave"
        self.H._obs.view(torch.int16).fill_(NAN16)   # whatever the first launch leaves unwritten stays a NaN: most values of a small row are 0.0

    def actions(self):
        return (torch.rand((self.F.n_envs, self.agents, 2), generator=self.g) * 2 - 1).to(DEV)

    def check_rows(self, h, f, what):
        assert h.dtype is F16 and f.dtype is F32 and h.shape == f.shape, what
        diff = int((b16(h).reshape(-1) != as_half_bits(f).reshape(-1)).sum())
        assert same16(h, f), "%s: %d of %d elements differ from the float32 twin's halves" % (what, diff, f.numel())

    def check_state(self, what):
        sf, sh = self.F.get_state(), self.H.get_state()
        assert sf.keys() == sh.keys()
        for k in sf:
            assert torch.equal(sf[k].contiguous().view(torch.uint8), sh[k].contiguous().view(torch.uint8)), (what, k)

    def reset(self, **kw):
        of, oh = self.F.reset(**kw), self.H.reset(**kw)
        self.check_rows(oh, of, "reset")
        self.check_state("reset")
        return of, oh

    def step(self, t, **kw):
        a = self.actions()
        (of, rf, df, inf), (oh, rh, dh, inh) = self.F.step(a, **kw), self.H.step(a, **kw)
        self.check_outputs(t, (of, rf, df, inf), (oh, rh, dh, inh))
        return (of, rf, df, inf), (oh, rh, dh, inh)

    def check_outputs(self, t, f, h):
        (of, rf, df, inf), (oh, rh, dh, inh) = f, h
        self.check_rows(oh, of, "step %d" % t)
        assert rh.dtype is F32 and torch.equal(rh.view(torch.int32), rf.view(torch.int32)), t
        assert torch.equal(dh.view(torch.uint8), df.view(torch.uint8)), t
        assert inf.keys() == inh.keys()
        for k in inf:
            assert torch.equal(inf[k], inh[k]), (t, k)
        self.check_state("step %d" % t)


@pytest.mark.parametrize("case", sorted(CASES))
def test_half_rows_are_the_float32_rows_rounded(case):
    tw = Twins(case)
    of, oh = tw.reset()
    assert oh.data_ptr() == tw.H._obs.data_ptr()
    ends, events, inexact = 0, 0, 0
    for t in range(8):
        (of, rf, df, inf), _h = tw.step(t)
        ends += int(df.sum())
        events += int(sum(v.sum() for k, v in inf.items() if k != "done_bits"))
        inexact += int((of.to(F16).float() != of).sum())
    assert ends >= 2 * tw.F.n_envs, ends          # max_steps = 3: every env ran its fused auto-reset pass at least twice
    if case in ("ww_configs2", "hw_default"):     # (one sensor of one agent rarely sees anything: the small shapes are about the store's paths)
        assert inexact > 0                        # values with more than 11 significant bits were stored: rounding took place
    if case == "ww_configs2":
        assert events > 0, "no catch in the run: the respawn path was not exercised"


@pytest.mark.parametrize("case", ["ww_configs2", "hw_generic_11"])
def test_obs_out_slots_at_odd_elements_leave_their_guards_alone(case):
    """step(obs_out=) into slots carved at odd element offsets of ONE int16 tensor filled with a NaN pattern, guard bands before, between
    and after them: after every step the whole tensor is what it was, but for the slot, which holds the halves of the float32 twin's rows"""
    tw = Twins(case)
    n = tw.F._obs.numel()
    assert n % 2 == 1 and tw.F.n_envs % 2 == 1 and tw.F._obs[0].numel() % 2 == 1
    guard, offs, at = 63, [], 0
    for _ in range(3):
        at += guard
        at += 1 - at % 2        # every slot starts on an odd element: 2-byte aligned and no more
        offs.append(at)
        at += n
    ring = torch.full((at + guard,), NAN16, dtype=torch.int16, device=DEV)
    want = ring.clone()
    slots = [ring[o:o + n].view(F16) for o in offs]
    assert all(s.data_ptr() % 4 == 2 and s.is_contiguous() for s in slots)
    tw.reset()
    for t in range(7):
        k = t % 3
        a = tw.actions()
        f = tw.F.step(a)
        h = tw.H.step(a, obs_out=slots[k])
        assert h[0].data_ptr() == slots[k].data_ptr() and h[0].shape == tw.F._obs.shape
        tw.check_outputs(t, f, h)
        want[offs[k]:offs[k] + n] = as_half_bits(f[0]).reshape(-1)
        bad = (ring != want).nonzero().reshape(-1)
        assert bad.numel() == 0, "step %d, slot %d at element %d: %d elements of the ring are wrong, the first at %d" % (
            t, k, offs[k], bad.numel(), int(bad[0]))
    # the env's own buffer was not written by those steps: it still holds the reset's rows
    with pytest.raises(ValueError, match="float16"):
        tw.H.step(tw.actions(), obs_out=torch.zeros(n, dtype=F32, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        tw.F.step(tw.actions(), obs_out=torch.zeros(n, dtype=F16, device=DEV))


@pytest.mark.parametrize("case", ["ww_generic_odd", "ww_configs2", "hw_generic_105", "hw_default"])
def test_reset_mask_keeps_the_other_rows_16_bits(case):
    tw = Twins(case, max_steps=50)
    tw.reset()
    for t in range(2):
        tw.step(t)
    before = b16(tw.H._obs).clone()
    mask = torch.arange(tw.F.n_envs, device=DEV) % 3 != 1
    of, oh = tw.reset(mask=mask)
    now = b16(oh)
    assert torch.equal(now[~mask], before[~mask])                      # outside the mask: the 16 bits they held
    assert torch.equal(now[mask], as_half_bits(of)[mask])              # inside: the float32 twin's new rows
    assert not torch.equal(now[mask], before[mask])
    tw.step(2)


def test_teacher_forced_waterworld_step_with_injected_respawns():
    """one teacher-forced step of the recorded catches through both twins, the protocol of test_waterworld_gpu.py: the rows of the half env
    are the halves of the float32 env's, among them values that round away from zero and subnormal halves"""
    from madrl_amd.waterworld import BatchedMAWaterWorld
    from oracle import waterworld as ww
    g = np.load(os.path.join(GOLDEN, "waterworld_c3_catches.npz"))
    T = len(g["pre_t"])
    out = []
    for extra in ({}, dict(obs_dtype=F16)):
        env = BatchedMAWaterWorld(n_envs=T, device=DEV, max_blocks=3, **ww.kwargs_from_golden(g), **extra)
        env.set_state(pos=g["pre_pos"], vel=g["pre_vel"], obst=g["obst"], t=g["pre_t"])
        out.append(env.step(g["act"], respawn=g["resp"]) + (env.get_state(),))
    (of, rf, df, inf, sf), (oh, rh, dh, inh, sh) = out
    assert oh.dtype is F16 and same16(oh, of)
    assert torch.equal(rf.view(torch.int32), rh.view(torch.int32)) and torch.equal(df, dh)
    assert all(torch.equal(inf[k], inh[k]) for k in inf) and int(inf["evcatches"].sum() + inf["pocatches"].sum()) > 0
    assert all(torch.equal(sf[k], sh[k]) for k in sf)
    wide = oh.float()
    away = (wide.abs() > of.abs()).sum()
    sub = ((of != 0) & (of.abs() < 2.0 ** -14)).sum()
    assert int(away) > 1000 and int(sub) > 0, (int(away), int(sub))   # what a truncating or flushing conversion gets wrong is in the rows
    assert int(((wide != 0) & (wide.abs() < 2.0 ** -14)).sum()) > 0       # ... and subnormal halves were stored as such


def test_teacher_forced_hostage_step_with_injected_respawns():
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    from oracle import hostage as ho
    g = np.load(os.path.join(GOLDEN, "hostage_default_global.npz"))
    T = len(g["pre_t"])
    saved = np.array([sum(int(b) << j for j, b in enumerate(g["pre_saved"][t])) for t in range(T)], np.int64)
    flags = (g["pre_gate"].astype(np.uint8) | (g["pre_bombed"].astype(np.uint8) << 1) | 4).astype(np.uint8)
    resp = np.where(g["resp"] >= 0, g["resp"], 0.0)
    out = []
    for extra in ({}, dict(obs_dtype=F16)):
        env = BatchedContinuousHostageWorld(n_envs=T, device=DEV, max_blocks=3, **ho.kwargs_from_golden(g), **extra)
        env.set_state(pos=g["pre_pos"], vel=g["pre_vel"], key=g["key"], bomb=g["bomb"], saved=saved, flags=flags, t=g["pre_t"].astype(np.int32),
                      tick=np.arange(T, dtype=np.int32))
        out.append(env.step(g["act"], respawn=resp) + (env.get_state(),))
    (of, rf, df, inf, sf), (oh, rh, dh, inh, sh) = out
    assert oh.dtype is F16 and same16(oh, of)
    assert torch.equal(rf.view(torch.int32), rh.view(torch.int32)) and torch.equal(df, dh)
    assert all(torch.equal(inf[k], inh[k]) for k in inf) and all(torch.equal(sf[k], sh[k]) for k in sf)
    assert int((oh.float().abs() > of.abs()).sum()) > 500   # values that round away from zero


@pytest.mark.parametrize("case,n", [("ww_configs2", 13), ("ww_chunk_and_tail", 65)], ids=["K30", "K1"])
def test_half_policy_gives_the_float32_policys_actions_on_the_widened_rows(case, n):
    from madrl_amd.heuristics import WaterworldHeuristicPolicy
    H = make(case, F16, n=n)
    ph, pf = WaterworldHeuristicPolicy(obs_dtype=F16), WaterworldHeuristicPolicy()
    obs = H.reset()
    assert obs.shape[0] * obs.shape[1] == 65   # no multiple of the 32 rows a block of the policy kernel takes
    g = torch.Generator(device="cpu").manual_seed(8)
    for t in range(4):
        ah, af = ph(obs), pf(obs.float())
        assert ah.dtype is F32 and ah.shape == obs.shape[:2] + (2,)
        assert torch.equal(ah.view(torch.int32), af.view(torch.int32)), t
        assert torch.isfinite(ah).all()
        obs = H.step(ah if t % 2 else (torch.rand(ah.shape, generator=g) * 2 - 1).to(DEV))[0]
    with pytest.raises(TypeError, match="float32"):
        pf(obs)
    with pytest.raises(TypeError, match="float16"):
        ph(obs.float())


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_rollout_collector_keeps_half_slots(graph):
    """the half step kernel writes the trajectory's float16 observation slots itself, and the half policy reads them: a rollout equals
    stepping a second half env by hand with a second half policy (not a float32 rollout: the policy sees rounded rows)"""
    from madrl_amd.heuristics import WaterworldHeuristicPolicy
    from madrl_amd.rollout import RolloutCollector
    T = 5
    mk = lambda: make("ww_configs2", F16, max_steps=4)
    col = RolloutCollector(mk(), WaterworldHeuristicPolicy(obs_dtype=F16), horizon=T, store_observations=True, graph=graph)
    assert col._slots
    env, pol = mk(), WaterworldHeuristicPolicy(obs_dtype=F16)
    obs = env.reset()
    for it in range(3):   # (graph: call 1 eager, call 2 captures and replays, call 3 replays)
        traj = col.collect()
        torch.cuda.synchronize()
        assert traj.observations.dtype is F16 and traj.last_observation.dtype is F16 and col._obs_slots.dtype is F16
        assert col._obs_slots.shape == (T + 1,) + tuple(obs.shape)
        for t in range(T):
            assert torch.equal(b16(traj.observations[t]), b16(obs)), (it, t)
            act = pol(obs)
            assert torch.equal(traj.actions[t].view(torch.int32), act.view(torch.int32)), (it, t)
            obs, rew, done, _info = env.step(act)
            assert torch.equal(traj.rewards[t].view(torch.int32), rew.view(torch.int32)) and torch.equal(traj.dones[t] != 0, done), (it, t)
        assert torch.equal(b16(traj.last_observation), b16(obs)), it
    assert int((traj.dones != 0).sum()) >= env.n_envs


@pytest.mark.parametrize("case", ["ww_generic_odd", "hw_default"])
def test_stream_sharded_half_sub_batches_equal_one_half_batch(case):
    from madrl_amd.sharded import StreamSharded
    n = 14
    whole = make(case, F16, n=n, env_id_base=3)
    sh = StreamSharded(lambda n_envs, env_id_base, device: make(case, F16, n=n_envs, env_id_base=env_id_base), n, n_streams=2, env_id_base=3)
    assert all(e.obs_dtype is F16 for e in sh.envs)
    ow = whole.reset()
    assert torch.equal(b16(torch.cat(sh.reset())), b16(ow))
    g = torch.Generator(device="cpu").manual_seed(5)
    for t in range(6):
        a = (torch.rand((n,) + tuple(ow.shape[1:2]) + (2,), generator=g) * 2 - 1).to(DEV)
        ow, rw, dw, _ = whole.step(a)
        parts = sh.step(a)   # (conforming actions: step_on_stream of every sub-batch)
        assert all(p[0].dtype is F16 for p in parts)
        assert torch.equal(b16(torch.cat([p[0] for p in parts])), b16(ow)), t
        assert torch.equal(torch.cat([p[1] for p in parts]).view(torch.int32), rw.view(torch.int32)), t
        assert torch.equal(torch.cat([p[2] for p in parts]), dw), t


def test_wrappers_over_a_half_env():
    from madrl_amd import _lib
    from madrl_amd.wrappers import ObservationBuffer, StandardizedEnv
    H = make("hw_generic_105", F16)
    assert H.fused_standardize is False
    with pytest.raises(_lib.MadrlError, match="half-precision"):
        H.bind_standardize()
    plain = StandardizedEnv(H, scale_reward=0.5)   # no obsnorm: the half rows pass through, the rewards are scaled
    assert not plain._fused
    o = plain.reset()
    assert o.dtype is F16 and o.data_ptr() == H._obs.data_ptr()
    o, r, d, _ = plain.step(torch.zeros((H.n_envs, 5, 2), device=DEV))
    assert o.dtype is F16 and torch.equal(r, H._rew * 0.5)
    with pytest.raises(ValueError, match="fused=True"):
        StandardizedEnv(make("hw_generic_105", F16), fused=True)
    with pytest.raises(TypeError, match="float32"):
        StandardizedEnv(make("hw_generic_105", F16), enable_obsnorm=True).reset()
    with pytest.raises(TypeError, match="float32"):
        ObservationBuffer(make("hw_generic_105", F16), 2).reset()


def _last_error():
    from madrl_amd import _lib
    return _lib.lib().madrl_last_error().decode()


def _half_calls(env, prefix):
    """-> [(name, call)]: the two half entries on env's handle with valid buffers of the env's own sizes"""
    from madrl_amd import _lib
    L = _lib.lib()
    rows = torch.zeros(env._obs.shape, dtype=F16, device=DEV)
    act = torch.zeros(tuple(env._obs.shape[:2]) + (2,), dtype=F32, device=DEV)
    s = _lib.current_stream(env.device)
    env._keep = (rows, act)
    return [("reset_f16", lambda obs=rows: getattr(L, prefix + "_reset_f16")(env._handle, None, _lib.ptr(obs), s)),
            ("step_f16", lambda obs=rows: getattr(L, prefix + "_step_f16")(env._handle, _lib.ptr(act), None, _lib.ptr(obs), _lib.ptr(env._rew),
                                                                            _lib.ptr(env._done), _lib.ptr(env._info), s))]


def test_c_entries_refuse_what_has_no_half_rows():
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    from madrl_amd.waterworld import BatchedMAWaterWorld
    ww = lambda **kw: BatchedMAWaterWorld(3, 4, n_poison=4, n_sensors=4, n_envs=5, device=DEV, **kw)
    hw = lambda **kw: BatchedContinuousHostageWorld(3, 10, 5, 2, 2, n_envs=5, device=DEV, **kw)
    std = ww()
    std.bind_standardize(enable_obsnorm=True)
    hstd = hw()
    hstd.bind_standardize(enable_obsnorm=True)
    for env, prefix, word in ((ww(crowd=True), "madrl_waterworld", "crowd"),
                              (ww(per_env_counts="wave"), "madrl_waterworld", "set_particle_counts"),
                              (ww(sensor_range=[0.2, 0.3, 0.2]), "madrl_waterworld", "set_sensor_ranges"),
                              (std, "madrl_waterworld", "set_standardize"),
                              (hw(crowd=True), "madrl_hostage", "crowd"),
                              (hw(crowd=True, per_env_counts=True), "madrl_hostage", "crowd"),
                              (hstd, "madrl_hostage", "set_standardize")):
        for name, call in _half_calls(env, prefix):
            assert call() != 0, (prefix, name, word)
            msg = _last_error()
            assert prefix + "_" + name in msg and word in msg, msg
    # a NULL destination, on a handle that would otherwise run
    for env, prefix in ((ww(), "madrl_waterworld"), (hw(), "madrl_hostage")):
        for name, call in _half_calls(env, prefix):
            assert call(obs=None) != 0 and "obs is NULL" in _last_error(), (prefix, name)
    # unbound again, the same handle runs the half entries: they check at each call
    std.unbind_standardize()
    rows = torch.full(std._obs.shape, float("nan"), dtype=F16, device=DEV)
    for name, call in _half_calls(std, "madrl_waterworld"):
        assert call(obs=rows) == 0, _last_error()
    twin = ww()
    twin.reset()
    of = twin.step(torch.zeros((5, 3, 2), device=DEV))[0]
    assert same16(rows, of)
