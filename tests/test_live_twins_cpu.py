"""CPU test (-m "not gpu") of the comparisons of live_twins.py, which otherwise only ever run on a GPU: "env outputs" that are right by
construction -- each oracle twin's own outputs and state, scattered into the slotted capacity layout -- pass, and one changed bit or
value in any compared field raises."""
import copy
import functools

import numpy as np
import pytest

import live_twins
from helpers import raw, slots

CAP, TRIPLES, N = (3, 4, 4), [(3, 4, 4), (2, 1, 3)], 4
CUR, PEND = np.array([0, 1, 0, 1]), np.array([1, 1, 0, 0])
ENV = 1   # the env the changes are made in: it runs (2, 1, 3), so row 2 and slots 2, 4 .. 6 and 10 are absent
WORLDS = {
    "waterworld": lambda: live_twins.waterworld(dict(n_pursuers=3, n_evaders=4, n_poison=4, n_coop=1, n_sensors=5, radius=0.03), 7, 50),
    "hostage": lambda: live_twins.hostage(CAP, 2, dict(n_sensors=5, action_scale=0.03, bad_speed=0.03), 7, 50),
}


def _case(world):
    """three steps of the twins, then what a right env would hold: -1 / +0.0 in absent slots, zero rows and rewards for absent agents"""
    twins = [world.make_twin(tri, N, 6) for tri in TRIPLES]
    rng = np.random.RandomState(1)
    for o in twins:
        o.reset()
    for t in range(3):
        act = rng.uniform(-1, 1, size=(N, CAP[0], 2)).astype(np.float32)
        for o, tri in zip(twins, TRIPLES):
            o.step(act[:, :tri[0]])
    NP, D = sum(CAP), twins[0].obs.shape[-1]
    c = dict(obs=np.zeros((N, CAP[0], D), np.float32), rew=np.zeros((N, CAP[0]), np.float32), done=np.zeros(N, bool),
             count0=np.zeros(N, np.int32), count1=np.zeros(N, np.int32), live=np.asarray(TRIPLES)[CUR], pending=np.asarray(TRIPLES)[PEND])
    st = dict(pos=np.full((N, NP, 2), -1, np.float32), vel=np.zeros((N, NP, 2), np.float32), counts=c["live"].copy())
    for q, (o, tri) in enumerate(zip(twins, TRIPLES)):
        idx, s, ost = np.nonzero(CUR == q)[0], slots(CAP, tri), o.get_state()
        c["obs"][idx, :tri[0]], c["rew"][idx, :tri[0]], c["done"][idx] = o.obs[idx], o.rew[idx], o.done[idx] != 0
        c["count0"][idx], c["count1"][idx] = o.info[idx, 0], o.info[idx, 1]
        st["pos"][np.ix_(idx, s)], st["vel"][np.ix_(idx, s)] = ost["pos"][idx], ost["vel"][idx]
        for k in world.state_keys:
            st.setdefault(k, np.zeros_like(ost[k]))[idx] = ost[k][idx]
    return twins, dict(c, st=st)


@functools.lru_cache(None)
def _world_and_case(name):
    """computed once per world and left unchanged: a test changes a copy"""
    world = WORLDS[name]()
    return (world,) + _case(world)


def _compare(world, twins, c):
    live_twins.compare_step(twins, TRIPLES, CUR, c["rew"], c["done"], c["count0"], c["count1"], "step")
    live_twins.compare_state(twins, CAP, TRIPLES, CUR, PEND, c["st"], c["live"], c["pending"], world.state_keys, "step", obs=c["obs"])


def _flip(a, *index):
    """the lowest bit of one element, whatever its type"""
    assert a.flags.c_contiguous
    raw(a)[index] ^= 1


def _set(a, index, value):
    a[index] = value


CHANGES = {
    "obs_present_row": lambda c: _flip(c["obs"], ENV, 1, 0),
    "obs_absent_row": lambda c: _set(c["obs"], (ENV, 2, 3), -0.0),
    "reward": lambda c: _flip(c["rew"], ENV, 0),
    "reward_absent_agent": lambda c: _set(c["rew"], (ENV, 2), -0.0),
    "done": lambda c: _flip(c["done"], ENV),
    "counter_0": lambda c: _flip(c["count0"], ENV),
    "counter_1": lambda c: _flip(c["count1"], ENV),
    "pos": lambda c: _flip(c["st"]["pos"], ENV, 3, 1),
    "vel": lambda c: _flip(c["st"]["vel"], ENV, 7, 0),
    "pos_absent_slot": lambda c: _set(c["st"]["pos"], (ENV, 4, 0), 0.5),
    "vel_absent_slot": lambda c: _set(c["st"]["vel"], (ENV, 10, 1), -0.0),
    "live_count": lambda c: _set(c["live"], (ENV, 1), 2),
    "pending_count": lambda c: _set(c["pending"], (ENV, 2), 4),
}
STATE_KEYS = {"waterworld": ("obst", "t", "tick"), "hostage": ("key", "bomb", "saved", "flags", "t", "tick")}


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_right_outputs_pass(name):
    world, twins, c = _world_and_case(name)
    assert world.state_keys == STATE_KEYS[name] and (c["rew"] != 0).any() and (c["st"]["pos"][ENV] == -1).any()
    _compare(world, twins, c)


@pytest.mark.parametrize("name,what", [(n, w) for n in sorted(WORLDS) for w in sorted(CHANGES) + ["state_" + k for k in STATE_KEYS[n]]])
def test_one_changed_bit_or_value_raises(name, what):
    world, twins, c = _world_and_case(name)
    c = copy.deepcopy(c)
    if what in CHANGES:
        CHANGES[what](c)
    else:
        _flip(c["st"][what[6:]], ENV)   # (obst, key and bomb have two elements per env: both)
    with pytest.raises(AssertionError):
        _compare(world, twins, c)
