"""AbstractMAEnv.step_into, the one call RolloutCollector steps an env through, on fake envs over CPU tensors: the default implementation
(step() plus the two copies, the done-byte rule of madrl_amd.base.done_bytes) and an env that overrides it.  The collectors are driven
through _begin() / _step(t) alone: _finish() launches the return scan."""
import pytest
import torch

from madrl_amd.base import AbstractMAEnv, done_bytes
from madrl_amd.rollout import RolloutCollector

N, A, D, T = 5, 2, 3, 6
BITS = torch.tensor([0, 1, 2, 3, 0x80, 0x81], dtype=torch.uint8)   # (bit 7: the overflow mark, no episode boundary)


def _tables(seed=0):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((T + 1, N, A, D), generator=g)
    rew = torch.randn((T, N, A), generator=g)
    bits = BITS[torch.randint(0, len(BITS), (T, N), generator=g)]
    assert bool((bits & 0x80).any()) and bool((bits & 3).any())
    return obs, rew, bits


class StepOnly(AbstractMAEnv):
    """step() alone, a bool `done` and an empty info: the collector reaches it through the inherited step_into"""
    with_bits = False

    def __init__(self):
        self.obs, self.rew, self.bits = _tables()
        self.t, self.seen = 0, []

    def reset(self):
        self.t = 0
        return self.obs[0]

    def step(self, actions):
        t = self.t
        self.t += 1
        self.seen.append(actions.clone())
        return self.obs[t + 1], self.rew[t], (self.bits[t] & 3) != 0, {"done_bits": self.bits[t]} if self.with_bits else {}


class StepWithBits(StepOnly):
    with_bits = True


class Into(StepOnly):
    """overrides step_into and takes an observation destination"""
    takes_obs_out = True

    def __init__(self):
        super().__init__()
        self.calls = []

    def step(self, actions):
        raise AssertionError("the collector must call step_into alone")

    def step_into(self, actions, rew_out, done_out, obs_out=None):
        t = self.t
        self.t += 1
        self.calls.append(None if obs_out is None else obs_out.data_ptr())
        rew_out.copy_(self.rew[t])
        done_out.copy_(self.bits[t])
        if obs_out is None:
            return self.obs[t + 1]
        obs_out.copy_(self.obs[t + 1])
        return obs_out


def _policy(obs):   # a function of the observation: a wrong observation shows in the action
    return (obs.sum(dim=-1) * 7).to(torch.int32)


def _drive(col):
    col._begin()
    for t in range(T):
        col._step(t)
    return col._buf


@pytest.mark.parametrize("cls", [StepOnly, StepWithBits])
@pytest.mark.parametrize("store", [False, True])
def test_default_step_into_equals_a_loop_over_step(cls, store):
    env, twin = cls(), cls()
    col = RolloutCollector(env, _policy, T, store_observations=store)
    assert col._slots is False
    b = _drive(col)
    obs = twin.reset()
    for t in range(T):
        act = _policy(obs)
        if store:
            assert torch.equal(b["observations"][t], obs), t
        obs, rew, done, info = twin.step(act)
        assert torch.equal(b["actions"][t], act), t
        assert torch.equal(b["rewards"][t], rew), t
        want = info["done_bits"] if cls.with_bits else done.to(torch.uint8)
        assert b["dones"].dtype is torch.uint8 and torch.equal(b["dones"][t], want), t
    assert torch.equal(col._obs, obs)
    if not store:
        assert b["observations"] is None
    if cls.with_bits:
        assert bool((b["dones"] & 0x80).any())
    else:
        assert int(b["dones"].max()) == 1


def test_done_bytes_rule():
    done = torch.tensor([True, False, True])
    bits = torch.tensor([0x81, 0, 2], dtype=torch.uint8)
    assert done_bytes(done, {"done_bits": bits}) is bits
    for info in ({}, None, {"other": 1}):
        got = done_bytes(done, info)
        assert got.dtype is torch.uint8 and got.tolist() == [1, 0, 1]


@pytest.mark.parametrize("store,obs_slots,slots", [(True, None, True), (True, True, True), (True, False, False), (False, None, False)])
def test_an_overriding_env_is_called_once_per_step_with_slot_t_plus_1(store, obs_slots, slots):
    env = Into()
    col = RolloutCollector(env, _policy, T, store_observations=store, obs_slots=obs_slots)
    assert col._slots is slots
    col._begin()
    for t in range(T):
        col._step(t)
        assert len(env.calls) == t + 1
        assert env.calls[t] == (col._env_slots[t + 1].data_ptr() if slots else None)
    b = col._buf
    assert torch.equal(b["rewards"], env.rew) and torch.equal(b["dones"], env.bits)
    if store:
        assert torch.equal(b["observations"], env.obs[:T])
    if slots:
        assert torch.equal(b["last_observation"], env.obs[T]) and col._obs.data_ptr() == col._obs_slots[T].data_ptr()


def test_obs_slots_true_needs_a_destination():
    with pytest.raises(ValueError):
        RolloutCollector(StepOnly(), _policy, T, store_observations=True, obs_slots=True)


def test_default_step_into_refuses_obs_out():
    env = StepOnly()
    env.reset()
    assert StepOnly.takes_obs_out is False
    rew, done = torch.empty((N, A)), torch.empty(N, dtype=torch.uint8)
    with pytest.raises(ValueError):
        env.step_into(_policy(env.obs[0]), rew, done, obs_out=torch.empty((N, A, D)))
    assert env.t == 0 and env.seen == []   # refused before the env stepped
    assert env.step_into(_policy(env.obs[0]), rew, done) is not None and env.t == 1
