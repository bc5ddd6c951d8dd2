"""AbstractMAEnv.step_into on the device: every env family, one wrapper and the collector's copies.

Twins with the same seed, one driven by step_into into caller tensors, one by step(): observations, rewards, done bytes and get_state()
are compared as bits after each of 8 steps, with max_steps=3 and auto_reset so that episodes end and restart inside; each case once
with obs_out=None and once with a fresh destination per step.  The last test counts the torch copies of a collector step."""
import pytest
import torch

from helpers import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, STEPS = 64, 8
EPISODE = dict(max_steps=3, auto_reset=True)
F32, F16 = torch.float32, torch.float16


# ---------------------------------------------------------------- envs
def _pursuit(shape, n_envs=N, **kw):
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    xs, ys, P, E, R = shape
    return BatchedPursuitEvade([rectangle_map(xs, ys)], n_envs=n_envs, device=DEV, seed=4, n_pursuers=P, n_evaders=E, obs_range=R, **EPISODE, **kw)


def _waterworld(n_envs=N):
    from madrl_amd.waterworld import BatchedMAWaterWorld
    return BatchedMAWaterWorld(3, 10, n_poison=5, n_envs=n_envs, device=DEV, seed=4, **EPISODE)


def _hostage(n_envs=N):
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    return BatchedContinuousHostageWorld(3, 10, 5, 2, 2, n_envs=n_envs, device=DEV, seed=4, **EPISODE)


def _multiwalker(n_envs=16):
    from madrl_amd.multiwalker import BatchedMultiWalkerEnv
    return BatchedMultiWalkerEnv(n_walkers=3, n_envs=n_envs, device=DEV, seed=4, **EPISODE)


def _fused(mk):
    def make():
        from madrl_amd.wrappers import StandardizedEnv
        env = mk()
        env._wrapper = StandardizedEnv(env, enable_obsnorm=True, enable_rewnorm=True, fused=True)   # (binds its statistics to the env)
        return env
    return make


def _buffered():
    from madrl_amd.wrappers import ObservationBuffer
    return ObservationBuffer(_waterworld(), 3)


def _int_actions(n_agents, dtype, n_envs=N):
    g = torch.Generator().manual_seed(11)
    acts = [torch.randint(0, 5, (n_envs, n_agents), generator=g).to(dtype).to(DEV) for _ in range(STEPS)]
    return lambda t: acts[t]


def _float_actions(n_agents, adim, n_envs=N):
    g = torch.Generator().manual_seed(11)
    acts = [(torch.rand((n_envs, n_agents, adim), generator=g) * 2 - 1).to(DEV) for _ in range(STEPS)]
    return lambda t: acts[t]


# ---------------------------------------------------------------- the twin run
class CopySpy(object):
    """counts every torch.Tensor.copy_ while it is active (the spy of tests/test_rollout_obs_slots_gpu.py without its size filter)"""

    def __init__(self, monkeypatch):
        self.n, self._mp, self._orig = 0, monkeypatch, torch.Tensor.copy_

    def __enter__(self):
        orig = self._orig

        def spy(tensor, src, *args, **kw):
            self.n += 1
            return orig(tensor, src, *args, **kw)

        self._mp.setattr(torch.Tensor, "copy_", spy)
        return self

    def __exit__(self, *exc):
        self._mp.setattr(torch.Tensor, "copy_", self._orig)


def _state(env):
    env = getattr(env, "unwrapped", env)
    st = dict(env.get_state())
    for k, v in (getattr(env, "_std", None) or {}).items():   # a fused StandardizedEnv: its running statistics and outputs
        st["std_" + k] = v
    return st


def _twins(make, actions, with_dest, monkeypatch, copies=None):
    """copies: how many copy_ calls one step_into may make (None: not counted)"""
    from madrl_amd.base import done_bytes
    a, b = make(), make()
    oa, ob = a.reset(), b.reset()
    assert same_bits(oa, ob)
    ends = 0
    for t in range(STEPS):
        act = actions(t)
        ob, rb, db, info = b.step(act)
        want_done = done_bytes(db, info)
        rew, done = torch.full_like(rb, float("nan")), torch.full_like(want_done, 0x55)
        dest = torch.full_like(ob, float("nan")) if with_dest else None
        with CopySpy(monkeypatch) as spy:
            oa = a.step_into(act, rew, done, obs_out=dest)
        if copies is not None:
            assert spy.n == copies, (t, spy.n)
        if with_dest:
            assert oa.data_ptr() == dest.data_ptr() and oa.shape == ob.shape
        assert oa.dtype is ob.dtype and same_bits(oa, ob), t
        assert same_bits(rew, rb), t
        assert done.dtype is torch.uint8 and same_bits(done, want_done), t
        sa, sb = _state(a), _state(b)
        assert sorted(sa) == sorted(sb)
        for k in sa:
            assert same_bits(sa[k], sb[k]), (t, k)
        ends += int(((done & 3) != 0).sum())
    assert ends >= 2 * done.numel()   # max_steps=3: every env ended twice, and went on from its reset
    return a


DEST = pytest.mark.parametrize("with_dest", [False, True], ids=["in_place", "obs_out"])

# X(10, 10, 2, 2, 3, 1) of csrc/pursuit_specializations.def, in both observation dtypes, and a shape in no list (the generic kernel)
PURSUIT = {"listed_f32": ((10, 10, 2, 2, 3), {}, "wave"), "listed_f16": ((10, 10, 2, 2, 3), dict(obs_dtype=F16), None),
           "generic_f32": ((9, 9, 3, 4, 3), {}, "generic")}


@DEST
@pytest.mark.parametrize("act_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("case", sorted(PURSUIT))
def test_pursuit(case, act_dtype, with_dest, monkeypatch):
    shape, kw, kind = PURSUIT[case]
    env = _twins(lambda: _pursuit(shape, **kw), _int_actions(shape[2], act_dtype), with_dest, monkeypatch)
    assert env.takes_obs_out is True
    if kind is not None:
        assert env.kernel_kind == kind


PARTICLE = {"waterworld": (_waterworld, 3), "hostage": (_hostage, 3)}


@DEST
@pytest.mark.parametrize("world", sorted(PARTICLE))
def test_particle_world_writes_the_callers_tensors(world, with_dest, monkeypatch):
    mk, n_agents = PARTICLE[world]
    env = _twins(mk, _float_actions(n_agents, 2), with_dest, monkeypatch, copies=0)
    assert env.takes_obs_out is True


@pytest.mark.parametrize("world", sorted(PARTICLE))
def test_particle_world_under_a_fused_standardized_env_takes_the_default(world, monkeypatch):
    mk, n_agents = PARTICLE[world]
    env = _twins(_fused(mk), _float_actions(n_agents, 2), False, monkeypatch, copies=2)
    assert env._wrapper._fused and env.takes_obs_out is False
    obs = env.reset()
    rew, done = torch.empty((N, n_agents), device=DEV), torch.empty(N, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        env.step_into(_float_actions(n_agents, 2)(0), rew, done, obs_out=torch.empty_like(obs))
    env.unbind_standardize()
    assert env.takes_obs_out is True


@DEST
def test_multiwalker(with_dest, monkeypatch):
    env = _twins(_multiwalker, _float_actions(3, 4, n_envs=16), with_dest, monkeypatch, copies=0)
    assert env.takes_obs_out is True


def test_a_wrapper_is_step_plus_the_two_copies(monkeypatch):
    env = _twins(_buffered, _float_actions(3, 2), False, monkeypatch, copies=2)
    assert env.takes_obs_out is False
    rew, done = torch.empty((N, 3), device=DEV), torch.empty(N, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        env.step_into(_float_actions(3, 2)(0), rew, done, obs_out=torch.empty_like(env._buf))


# ---------------------------------------------------------------- copies per collector step
def _collector_world(family):
    from madrl_amd import heuristics as h
    if family == "pursuit":
        return _pursuit((10, 10, 2, 2, 3)), h.PursuitHeuristicPolicy(3, seed=3)
    if family == "multiwalker":
        return _multiwalker(), h.MultiWalkerHeuristicPolicy()
    if family == "buffered":
        return _buffered(), lambda obs: torch.tanh(obs[..., :2, -1] * 20.0)
    return PARTICLE[family][0](), h.WaterworldHeuristicPolicy() if family == "waterworld" else (lambda obs: torch.tanh(obs[..., :2] * 20.0))


def copy_counts(family, store, monkeypatch, T=4):
    """copy_ calls in each _step(t) of a collector's second horizon (the first one allocates)"""
    from madrl_amd.rollout import RolloutCollector
    env, policy = _collector_world(family)
    col = RolloutCollector(env, policy, T, store_observations=store)
    col.collect()
    col._begin()
    counts = []
    for t in range(T):
        with CopySpy(monkeypatch) as spy:
            col._step(t)
        counts.append(spy.n)
    col._finish()
    torch.cuda.synchronize()
    return counts


# What the collector did before its envs shared step_into, counted with copy_counts() on that commit: {(family, store): per step}.
# With store_observations the first step of a horizon also brings the previous horizon's last observation to slot 0.
BEFORE = {("pursuit", False): [0, 0, 0, 0], ("pursuit", True): [1, 0, 0, 0],
          ("waterworld", False): [3, 3, 3, 3], ("waterworld", True): [4, 3, 3, 3],
          ("hostage", False): [3, 3, 3, 3], ("hostage", True): [4, 3, 3, 3],
          ("multiwalker", False): [1, 1, 1, 1], ("multiwalker", True): [2, 1, 1, 1],
          ("buffered", False): [3, 3, 3, 3], ("buffered", True): [4, 4, 4, 4]}
LOWER = {"waterworld": 2, "hostage": 2}   # rewards and done bytes: the particle worlds' kernel writes them into the trajectory now


@pytest.mark.parametrize("store", [False, True], ids=["plain", "store_observations"])
@pytest.mark.parametrize("family", ["pursuit", "waterworld", "hostage", "multiwalker", "buffered"])
def test_copies_per_collector_step(family, store, monkeypatch):
    counts = copy_counts(family, store, monkeypatch)
    before = BEFORE[family, store]
    print("copy_ per step:", family, store, counts, "before:", before)
    assert all(c <= b for c, b in zip(counts, before)), (counts, before)
    if family == "pursuit":
        assert counts == before
    assert counts == [b - LOWER.get(family, 0) for b in before], (counts, before)
