"""RolloutCollector(store_observations=True) over an env whose step kernel can write its observations into a trajectory slot: the same
trajectory as the collector that copies the observations after every step, and no per-step pass over the observations."""
import pytest
import torch

from helpers import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, T = 256, 12
KEYS = ("observations", "actions", "rewards", "dones", "returns")


def _pursuit(n_envs=N, env_id_base=0, device=DEV):
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    return BatchedPursuitEvade([rectangle_map(16, 16)], n_envs=n_envs, device=device, seed=4, env_id_base=env_id_base, max_steps=5, auto_reset=True,
                               n_pursuers=8, n_evaders=30, obs_range=7, n_catch=2, surround=True)


def _pursuit_policy(row_id_base=0):
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    return PursuitHeuristicPolicy(7, seed=3, row_id_base=row_id_base)


def _waterworld(n_envs=N, env_id_base=0, device=DEV):
    from madrl_amd.waterworld import BatchedMAWaterWorld
    return BatchedMAWaterWorld(3, 10, n_poison=5, n_envs=n_envs, device=device, seed=4, env_id_base=env_id_base, max_steps=5, auto_reset=True)


def _waterworld_policy(row_id_base=0):
    from madrl_amd.heuristics import WaterworldHeuristicPolicy
    return WaterworldHeuristicPolicy()


WORLDS = {"pursuit": (_pursuit, _pursuit_policy), "waterworld": (_waterworld, _waterworld_policy)}


def _check(a, b, what):
    for k in KEYS:
        assert same_bits(getattr(a, k), getattr(b, k)), (what, k)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("world", sorted(WORLDS))
def test_same_trajectory_as_the_copying_collector(world, graph):
    from madrl_amd.rollout import RolloutCollector
    mk, pol = WORLDS[world]
    slots = RolloutCollector(mk(), pol(), T, store_observations=True, graph=graph)
    copying = RolloutCollector(mk(), pol(), T, store_observations=True, obs_slots=False)
    assert slots._slots and not copying._slots
    last = None
    for it in range(3):   # (graph: call 1 eager, call 2 captures and replays, call 3 replays)
        a, b = slots.collect(), copying.collect()
        _check(a, b, (world, it))
        assert a.observations.shape[0] == T and a.last_observation.shape == a.observations.shape[1:]
        assert same_bits(a.last_observation, b.last_observation), (world, it)
        if last is not None:   # the first observation of this horizon is the last one of the previous horizon
            assert same_bits(last, a.observations[0]), (world, it)
        last = a.last_observation.clone()
    assert int((a.dones != 0).sum()) >= N   # max_steps=5: episodes ended and restarted inside the horizon
    if graph:
        assert slots._graph is not None


def test_sharded_collector_equals_the_one_batch_collector():
    from madrl_amd.rollout import RolloutCollector, ShardedRolloutCollector
    from madrl_amd.sharded import StreamSharded
    per = N // 2
    one = RolloutCollector(_pursuit(), _pursuit_policy(), T, store_observations=True, obs_slots=False)
    cols = [ShardedRolloutCollector(StreamSharded(_pursuit, N, n_streams=2, device=DEV), [_pursuit_policy(j * per * 8) for j in range(2)], T,
                                    store_observations=True, graph=g) for g in (False, True)]
    for it in range(3):
        a = one.collect()
        for col in cols:
            assert all(c._slots for c in col.collectors)
            parts = col.collect()
            torch.cuda.synchronize()
            for k in KEYS:
                assert same_bits(getattr(a, k), torch.cat([getattr(p, k) for p in parts], dim=1)), (it, k)
            assert same_bits(a.last_observation, torch.cat([p.last_observation for p in parts], dim=0)), it


def test_a_plain_step_follows_the_collector():
    """after a collect() the env's current buffer is the trajectory's last slot: a plain step() goes on from there"""
    from madrl_amd.rollout import RolloutCollector
    env, twin = _pursuit(), _pursuit()
    a = RolloutCollector(env, _pursuit_policy(), T, store_observations=True).collect()
    b = RolloutCollector(twin, _pursuit_policy(), T, store_observations=True, obs_slots=False).collect()
    assert env.obs_buffer.data_ptr() == a.last_observation.data_ptr()
    act = torch.full((N, 8), 2, dtype=torch.int32, device=DEV)
    ra, rb = env.step(act), twin.step(act)
    assert same_bits(ra[0], rb[0]) and same_bits(ra[1], rb[1])


@pytest.mark.parametrize("world", sorted(WORLDS))
def test_no_per_step_copy(world, monkeypatch):
    """at most one observation-sized copy_ in a whole horizon"""
    from madrl_amd.rollout import RolloutCollector
    mk, pol = WORLDS[world]
    col = RolloutCollector(mk(), pol(), T, store_observations=True)
    col.collect()   # (allocations)
    n_obs = col._obs.numel()
    count = {"slots": 0}
    orig = torch.Tensor.copy_

    def spy(self, src, *args, **kw):
        if self.numel() == n_obs or (torch.is_tensor(src) and src.numel() == n_obs):
            count["slots"] += 1
        return orig(self, src, *args, **kw)

    monkeypatch.setattr(torch.Tensor, "copy_", spy)
    col.collect()
    monkeypatch.undo()
    assert count["slots"] <= 1, count
    # the spy sees the copying collector's copies
    ref = RolloutCollector(mk(), pol(), T, store_observations=True, obs_slots=False)
    ref.collect()
    count["slots"] = 0
    monkeypatch.setattr(torch.Tensor, "copy_", spy)
    ref.collect()
    monkeypatch.undo()
    assert count["slots"] >= T


def test_wrapped_envs_keep_the_copy_path():
    from madrl_amd.rollout import RolloutCollector
    from madrl_amd.wrappers import StandardizedEnv
    w = StandardizedEnv(_waterworld(), enable_obsnorm=True)
    col = RolloutCollector(w, _waterworld_policy(), T, store_observations=True)
    assert not col._slots
    tr = col.collect()
    assert tr.observations.shape[0] == T and tr.last_observation is not None
    with pytest.raises(ValueError):
        RolloutCollector(w, _waterworld_policy(), T, store_observations=True, obs_slots=True)
