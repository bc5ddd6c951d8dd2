"""GPU tests (-m gpu) of per-env particle counts on the hostage-world crowd kernel (`crowd=True, per_env_counts=True`:
hw_crowd_kernel_live, csrc/hostage_crowd.hip).  The definition of right: an env at live counts (r, h, c) computes what env n of a
fixed-shape (r, h, c) batch with the same seed and env_id_base + n computes.  So every test runs free against float32 oracle twins, one
twin of N envs per distinct triple, env n against env n of its triple's twin; nothing is copied across after the staging, and every
output and the whole state, slotted, are compared in every bit at every step.  Host-facing layouts stay at the capacity, slotted by class.
What depends on the count in this world -- "all saved", the not_saved_reward term, the reset's draw indices -- is what the event
conditions are there for: an all-saved termination at h < the capacity, and the rewards of that step, go wrong with the capacity's mask."""
import os
import pickle

import numpy as np
import pytest
import torch

from helpers import bits, i32, raw, same_bits, slots
from live_twins import (HOSTAGE_EVENTS as EVENTS, LiveTwins, all_h, assert_collector_equals_stepping_by_hand, assert_obs_out_leaves_no_nan,
                        hostage, lockstep)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, BASE = 77, 500
STATE_KEYS = ("key", "bomb", "saved", "flags", "t", "tick")

# test_hostage_crowd_gpu.py::BEYOND["62_particles"] as a capacity
CAP_62 = ((12, 20, 30), 2, dict(n_sensors=16, action_scale=0.03, bad_speed=0.03))
TRI_62 = [(12, 20, 30), (11, 19, 29), (5, 3, 20), (2, 1, 1)]
# ... ["33_rescuers_local"]
CAP_33 = ((33, 5, 7), 2, dict(n_sensors=7, reward_mech="local", key_loc=(0.93, 0.96), addid=False, action_scale=0.03, bad_speed=0.03))
TRI_33 = [(33, 5, 7), (32, 1, 7), (5, 5, 1)]


def _mk(*args, n_envs, crowd=True, **kw):
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    return BatchedContinuousHostageWorld(*args, n_envs=n_envs, device=DEV, crowd=crowd, **kw)


def _np(t):
    return t.cpu().numpy()


def _run(cap, coop, kw, triples, N, H, **more):
    return LiveTwins(hostage(cap, coop, kw, SEED, BASE, "crowd", _mk), triples, N, H, **more)


def _stage(run, coop):
    """Random actions never open the gate: every twin is staged with stage() of test_hostage_crowd_gpu.py on its own triple, and the
    live batch through set_state(counts=, pos=, vel=, saved=, flags=), each env's rows from its twin, scattered into slots; the slots
    that hold no particle are given values that would matter if they were kept"""
    from test_hostage_crowd_gpu import stage
    N, NPc = run.N, sum(run.cap)
    rng = np.random.RandomState(9)
    pos, vel = rng.uniform(0, 1, (N, NPc, 2)).astype(np.float32), rng.uniform(-.03, .03, (N, NPc, 2)).astype(np.float32)
    saved, flags = np.zeros(N, np.uint64), np.zeros(N, np.uint8)
    for q, (o, tri) in enumerate(zip(run.twins, run.triples)):
        st = o.get_state()
        sg = stage(st, tri + (coop,))
        o.set_state(**sg)
        idx, s = np.nonzero(run.cur == q)[0], slots(run.cap, tri)
        pos[np.ix_(idx, s)], vel[np.ix_(idx, s)] = sg["pos"][idx], st["vel"][idx]
        saved[idx], flags[idx] = sg["saved"][idx], sg["flags"][idx]
    full = np.uint64(2 ** 64 - 1)   # bits at or above an env's hostage count: set_state(counts=) clears them
    hh = np.asarray(run.triples)[run.cur][:, 1]
    junk = np.array([full & ~all_h(h) for h in hh], np.uint64)
    run.env.set_state(counts=np.asarray(run.triples)[run.cur], pos=pos, vel=vel, saved=saved | junk, flags=flags)
    run.check("staged", obs=False)


def _free_run(cap, coop, kw, triples, N, T, H):
    run = _run(cap, coop, kw, triples, N, H)
    run.reset()
    _stage(run, coop)
    rng = np.random.RandomState(1)
    for t in range(T):
        run.step(rng.uniform(-1, 1, size=(N, cap[0], 2)).astype(np.float32), "step %d" % t)
    for tri, ev in zip(run.triples, run.ev):
        print(tri, ev)
    return run


def _every_event_per_triple(run):
    for tri, ev in zip(run.triples, run.ev):
        assert all(v > 0 for v in ev.values()), (tri, ev)


def _every_event_somewhere(run):
    total = {k: run.total(k) for k in EVENTS}
    assert all(v > 0 for v in total.values()), total


def test_first_shape_past_a_wavefront_events_per_triple():
    """for every one of the four triples a save, a criminal hit, a gate opening, a bombing, an all-saved termination and a time-limit reset
    occur among the envs dealt to it"""
    cap, coop, kw = CAP_62
    _every_event_per_triple(_free_run(cap, coop, kw, TRI_62, N=65, T=40, H=13))


def test_chunk_boundaries_that_differ_per_env():
    """W (64-bit words per collision row) and the rescuers' second ballot word change from env to env inside one launch, and h = 64
    ("all saved" is ~0) sits beside h = 63"""
    kw = dict(action_scale=0.03, bad_speed=0.04)
    _every_event_somewhere(_free_run((65, 64, 129), 2, kw, [(65, 64, 129), (64, 63, 128), (33, 1, 65), (2, 64, 1)], N=20, T=30, H=10))


def test_variant_local_reward_fixed_key_no_id():
    cap, coop, kw = CAP_33
    _every_event_per_triple(_free_run(cap, coop, kw, TRI_33, N=33, T=40, H=13))


def test_variant_rows_longer_than_a_wavefront():
    """K = 200: a sensing pass is 64 sensors of one rescuer, and the number of passes is per env"""
    kw = dict(n_sensors=200, sensor_range=0.5, action_scale=0.03)
    _every_event_per_triple(_free_run((40, 10, 20), 2, kw, [(40, 10, 20), (39, 1, 20), (3, 10, 1)], N=15, T=30, H=10))


def test_the_limits():
    _free_run((128, 64, 831), 3, dict(bad_speed=0.03), [(128, 64, 831), (127, 33, 700)], N=3, T=8, H=4)


def test_counts_change_at_a_reset_not_before():
    """staggered ages and a staging, so that an env's episode ends by its own bomb, all-saved termination or time limit; one shrinking and
    one growing change set mid-episode: the set of changed envs is the set of envs whose own episode has ended, step by step"""
    (cap, coop, kw), N, H = CAP_62, 20, 9
    tri = TRI_62[:3] + [(1, 1, 1)]
    run = _run(cap, coop, kw, tri, N, H, deal=np.arange(N) % 2)   # (12, 20, 30) and (11, 19, 29)
    run.reset()
    rng = np.random.RandomState(2)
    act = lambda: rng.uniform(-1, 1, size=(N, cap[0], 2)).astype(np.float32)
    for t in range(3):
        run.step(act(), "warm-up %d" % t)
    young = np.arange(N) % 3 == 0
    run.reset(mask=young)                       # staggered ages: t = 1 for a third of the envs, 4 for the others; nothing is pending
    run.step(act(), "after the stagger")
    ages = _np(run.env.get_state()["t"])
    assert set(ages[young]) == {2} and set(ages[~young]) == {5}
    _stage(run, coop)                                 # by env index modulo 5: an all-saved termination, a gate opening, a bombing, a save, nothing
    # one shrinking change and one growing change, on all envs in the middle of their episodes
    old = run.cur.copy()
    run.set_pending(np.where(old == 0, 2, 0))   # (12, 20, 30) -> (5, 3, 20), (11, 19, 29) -> (12, 20, 30)
    pending, live = run.env.particle_counts()
    assert np.array_equal(_np(live), np.asarray(tri)[old]) and not (_np(pending) == _np(live)).all(1).any()
    switched = np.zeros(N, bool)
    for t in range(H):
        done = run.step(act(), "changing %d" % t)   # (check(): live == the twin each env is compared with, pending as set)
        assert np.array_equal(run.cur != old, switched | done), "an env changes when its own episode ends, not before"
        shrunk = done & (old == 0)
        assert not i32(run.obs[shrunk, 5:]).any()  # the reset pass zeroes the rows between the new and the old rescuer count
        if t == 0:   # only a staged env can end this early (ages 3 and 6 of 9), and not one whose gate stays closed
            assert done.any() and not done[np.isin(np.arange(N) % 5, (1, 4))].any()
        switched |= done
    assert switched.all() and np.array_equal(run.cur, run.pend)
    ended = {k: run.total(k) for k in EVENTS}
    assert ended["bombings"] > 0 and ended["all_saved"] > 0 and ended["time_limit"] > 0, ended
    # reset(mask=) applies the pending counts to the masked envs only
    before = run.cur.copy()
    run.set_pending(3)                          # (1, 1, 1): fewer rescuers than n_coop_save
    m = np.arange(N) % 4 == 1
    run.reset(mask=m)
    assert (run.cur[m] == 3).all() and np.array_equal(run.cur[~m], before[~m])
    for t in range(3):
        run.step(act(), "after the masked reset %d" % t)
    assert run.resets >= N


RECORDINGS = {"hwcrowd_20_30_40": (24, 32, 48), "hwcrowd_33_10_20_local": (40, 12, 24), "hwcrowd_8_64_100": (10, 64, 128)}


@pytest.mark.parametrize("name", sorted(RECORDINGS))
def test_teacher_forcing_through_the_slotted_layout(name):
    """a recording replayed on a batch of a capacity one notch above its shape: set_state(counts=, ...) and step(respawn=) take their rows
    in slot order, with random values in the absent slots and rows.  Protocol of
    test_hostage_crowd_gpu.py::test_crowd_matches_reference_golden_teacher_forced."""
    from oracle import hostage as ho
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    T, cap = len(g["pre_t"]), RECORDINGS[name]
    kw = ho.kwargs_from_golden(g)
    tri = (kw["n_good"], kw["n_hostages"], kw["n_bad"])
    r, h, c = tri
    ckw = dict(kw, n_good=cap[0], n_hostages=cap[1], n_bad=cap[2])
    env = _mk(n_envs=T, per_env_counts=True, **ckw)
    orc = ho.HostageOracle(n_envs=T, sensors=g["sensors"], dtype=np.float32, **kw)
    s, NPc = slots(cap, tri), sum(cap)
    gone = np.setdiff1d(np.arange(NPc), s)
    rng = np.random.RandomState(5)

    def slotted(a, where, n, fill):
        out = fill((T, n) + a.shape[2:]).astype(np.float32)
        out[:, where] = a
        return out
    pos = slotted(g["pre_pos"], s, NPc, lambda sh: rng.uniform(0, 1, sh))
    vel = slotted(g["pre_vel"], s, NPc, lambda sh: rng.uniform(-.01, .01, sh))
    resp0 = np.where(g["resp"] >= 0, g["resp"], 0.0)
    resp = slotted(resp0, np.arange(c), cap[2], lambda sh: rng.uniform(0, 1, sh))       # criminal m at row m
    act = slotted(g["act"], np.arange(r), cap[0], lambda sh: rng.uniform(-1, 1, sh))    # rows >= r are not read
    saved = np.array([sum(int(b) << j for j, b in enumerate(g["pre_saved"][t])) for t in range(T)], np.uint64)
    flags = (g["pre_gate"].astype(np.uint8) | (g["pre_bombed"].astype(np.uint8) << 1) | 4).astype(np.uint8)
    counts, tick = np.tile(tri, (T, 1)), np.arange(T, dtype=np.int32)
    with pytest.raises(ValueError, match="pos and vel"):
        env.set_state(counts=counts, pos=pos)
    env.set_state(counts=counts, pos=pos, vel=vel, key=g["key"], bomb=g["bomb"], saved=saved, flags=flags, t=g["pre_t"].astype(np.int32), tick=tick)
    orc.set_state(pos=g["pre_pos"], vel=g["pre_vel"], key=g["key"], bomb=g["bomb"], saved=saved, flags=flags, t=g["pre_t"].astype(np.int32),
                  tick=tick.view(np.uint32))
    st0 = {k: _np(v) for k, v in env.get_state().items()}
    assert (st0["pos"][:, gone] == -1).all() and (st0["vel"][:, gone] == 0).all() and (st0["counts"] == tri).all()
    obs, rew, done, info = env.step(act, respawn=resp)
    oobs, orew, odone, oinfo = orc.step(g["act"], resp=resp0)
    st1, ost = env.get_state(), orc.get_state()
    st = {k: _np(v) for k, v in st1.items()}
    obs, rew = _np(obs), _np(rew)
    live = g["is_reset_step"] == 0
    # the kernel IS the float32 oracle of the live shape
    assert np.array_equal(i32(obs[:, :r]), i32(oobs)) and not i32(obs[:, r:]).any()
    assert np.array_equal(i32(rew[live, :r]), i32(orew[live])) and not i32(rew[:, r:]).any()
    assert np.array_equal(i32(st["pos"][:, s]), i32(ost["pos"])) and np.array_equal(i32(st["vel"][:, s]), i32(ost["vel"]))
    assert (st["pos"][:, gone] == -1).all() and not i32(st["vel"][:, gone]).any()
    for k in STATE_KEYS:
        assert np.array_equal(raw(st[k]), raw(ost[k])), k
    # ... and within 1e-5 of the recording, in the reference's float64, wherever that oracle is: every step of these files
    err = np.abs(obs[:, :r] - g["obs"]).reshape(T, -1).max(1)
    oerr = np.abs(oobs - g["obs"]).reshape(T, -1).max(1)
    print("%s: worst error kernel %.3g, float32 oracle %.3g" % (name, err.max(), oerr.max()))
    assert oerr.max() <= TOL and err.max() <= TOL
    assert np.abs(st["pos"][:, s] - g["post_pos"]).max() < 1e-6 and np.abs(st["vel"][:, s] - g["post_vel"]).max() < 1e-6
    post_saved = np.array([sum(int(b) << j for j, b in enumerate(g["post_saved"][t])) for t in range(T)], np.uint64)
    assert np.array_equal(st["saved"].view(np.uint64), post_saved)
    assert np.array_equal(st["flags"] & 3, g["post_gate"] | (g["post_bombed"] << 1)) and np.array_equal(st["t"], g["post_t"])
    assert np.abs(rew[live, :r] - g["rew"][live]).max() < TOL
    assert np.array_equal(_np(done)[live], g["done"][live] == 1)
    assert np.array_equal(_np(torch.stack([info["ho_saved"], info["cr_encs"]], 1))[live], g["info"][live])
    # get_state -> set_state on a second env object, which continues identically (free-running: the same seed and env ids)
    first, second = env, _mk(n_envs=T, per_env_counts=True, **ckw)
    second.set_state(**st1)
    a = torch.as_tensor(act, device=DEV)
    for t in range(5):
        o1, r1, d1, i1 = first.step(a)
        o2, r2, d2, i2 = second.step(a)
        assert same_bits(o1, o2) and same_bits(r1, r2) and torch.equal(i1["cr_encs"], i2["cr_encs"])
        s1, s2 = first.get_state(), second.get_state()
        for k in s1:
            assert same_bits(s1[k], s2[k]), (k, t)
    assert (_np(s1["counts"]) == tri).all() and (s1["t"] == st1["t"] + 5).all()


def test_live_kernel_at_the_capacity_equals_the_fixed_shape_kernel():
    args, N = (12, 24, 25, 2, 1), 65
    kw = dict(n_sensors=16, seed=5, env_id_base=9, max_steps=15, auto_reset=True, action_scale=0.03, bad_speed=0.03)
    a, b = _mk(*args, n_envs=N, per_env_counts=True, **kw), _mk(*args, n_envs=N, **kw)
    assert len(list(lockstep(a, b, (N, 12, 2), 40, ("ho_saved", "cr_encs")))) == 40


def _mixed(N=9, **kw):
    (cap, coop, ckw) = CAP_33
    env = _mk(*cap, coop, 1, n_envs=N, per_env_counts=True, seed=4, **dict(dict(ckw, addid=True, max_steps=5, auto_reset=True), **kw))
    tri = np.asarray(TRI_33)[np.arange(N) % 3]
    env.set_particle_counts(tri[:, 0], tri[:, 1], tri[:, 2])
    return env


def test_interface_errors_and_counts_across_a_new_handle():
    from madrl_amd.hostage import BatchedContinuousHostageWorld, ContinuousHostageWorld
    (cap, coop, ckw), N = CAP_33, 9
    with pytest.raises(ValueError, match="crowd=True"):
        BatchedContinuousHostageWorld(3, 4, 2, 1, 1, n_envs=2, device=DEV, per_env_counts=True)
    fixed = _mk(*cap, coop, 1, n_envs=2, **ckw)
    with pytest.raises(RuntimeError, match="per_env_counts=True"):
        fixed.set_particle_counts(n_good=3)
    with pytest.raises(RuntimeError, match="per_env_counts=True"):
        fixed.particle_counts()
    assert "counts" not in fixed.get_state() and "per_env_counts" not in fixed._ctor
    plain = _mk(3, 4, 2, 1, 1, n_envs=2, crowd=False)
    assert set(plain._ctor) == set(pickle.loads(pickle.dumps(plain))._ctor) and not {"crowd", "per_env_counts"} & set(plain._ctor)
    env = _mixed()
    for bad in (dict(n_good=0), dict(n_good=34), dict(n_hostages=6), dict(n_bad=[1, 2, 3, 4, 5, 6, 7, 7, 0])):
        with pytest.raises(ValueError, match="capacity"):
            env.set_particle_counts(**bad)
    env.set_particle_counts(n_good=34, mask=np.zeros(N, bool))         # out of range where the mask does not reach: nothing is set
    env.reset()
    env.set_particle_counts(n_hostages=2, mask=np.arange(N) < 4)
    pending, live = env.particle_counts()
    assert np.array_equal(_np(live), np.asarray(TRI_33)[np.arange(N) % 3])
    assert pending[:4, 1].tolist() == [2] * 4 and torch.equal(pending[4:], live[4:])
    assert torch.equal(env.live_agents(), torch.arange(33, device=DEV)[None, :] < live[:, :1])
    env.seed(11)                                                       # a new handle, the same count tensors
    p2, l2 = env.particle_counts()
    assert torch.equal(p2, pending) and torch.equal(l2, live)
    env.reset()
    assert torch.equal(env.particle_counts()[1], pending)
    again = pickle.loads(pickle.dumps(env))                            # a pickle keeps the constructor arguments: back at the capacity
    assert again._ctor["per_env_counts"] is True and again.kernel_kind == "crowd"
    assert (_np(again.particle_counts()[1]) == cap).all()
    one = ContinuousHostageWorld(*cap, coop, 1, device=DEV, crowd=True, per_env_counts=True, **dict(ckw, addid=True))   # the N == 1 drop-in passes the flag through
    one._env.set_particle_counts(n_good=5)
    rows = one.reset()
    assert len(rows) == 33 and np.abs(rows[4]).max() > 0 and not np.abs(rows[5]).any()
    # set_state(counts=, saved=) clears the bits at or above an env's hostage count
    st = env.get_state()
    env.set_state(counts=st["counts"], pos=st["pos"], vel=st["vel"], saved=np.full(N, 2 ** 64 - 1, np.uint64))
    want = [2 ** int(h) - 1 for h in st["counts"][:, 1]]
    assert _np(env.get_state()["saved"]).view(np.uint64).tolist() == want


def test_is_terminal_uses_each_envs_live_hostage_count():
    """a mixed batch without auto_reset, staged: the envs of kind 0 end by "all saved" at their own hostage count"""
    (cap, coop, kw), N = CAP_62, 20
    run = _run(cap, coop, kw, TRI_62, N, H=50, auto_reset=False)
    run.reset()
    _stage(run, coop)
    assert not _np(run.env.is_terminal).any()
    act = np.random.RandomState(3).uniform(-1, 1, size=(N, cap[0], 2)).astype(np.float32)
    _obs, _rew, done, _info = run.env.step(act)
    want, by_all_saved = np.zeros(N, bool), np.zeros(N, bool)
    for q, (o, (r, h, _c)) in enumerate(zip(run.twins, run.triples)):
        o.step(act[:, :r])
        st, idx = o.get_state(), run.cur == q
        all_saved = (st["saved"] & all_h(h)) == all_h(h)
        want[idx] = (((st["flags"] & 2) != 0) | all_saved | (st["t"] >= 50))[idx]
        by_all_saved[idx] = all_saved[idx]
    assert np.array_equal(_np(run.env.is_terminal), want) and np.array_equal(_np(done), want)
    hh = np.asarray(run.triples)[run.cur][:, 1]
    assert (by_all_saved & (hh < cap[1])).any() and (by_all_saved & (hh == cap[1])).any() and not want.all()
    run.check("after the step", obs=False)


def test_obs_out_leaves_no_nan_in_an_uninitialised_destination():
    assert_obs_out_leaves_no_nan(_mixed(), steps=6)   # (max_steps=5: the last step goes through the reset pass)


def test_rollout_collector_and_standardized_env_over_a_mixed_batch():
    from madrl_amd.wrappers import StandardizedEnv
    # the policy of test_hostage_crowd_gpu.py::test_rollout_collector_over_a_crowd_env: a fixed function of the observation
    policy = lambda obs: torch.tanh(torch.stack([obs[..., :7].sum(-1) * 20.0 - 0.3, obs[..., 21:28].sum(-1) * 20.0 + 0.2], -1))
    assert_collector_equals_stepping_by_hand(_mixed, lambda: policy, H=8, min_dones=9)
    # StandardizedEnv takes its epilogue kernels over the capacity-shaped rows: scaling alone is the raw step times the scale, and the
    # rows of absent rescuers standardise to exactly 0 (mean 0, value 0)
    raw, scaled, normed = _mixed(), StandardizedEnv(_mixed(), scale_reward=2.0), StandardizedEnv(_mixed(), enable_obsnorm=True, enable_rewnorm=True)
    assert not scaled._fused and not normed._fused
    o0 = raw.reset()
    assert same_bits(scaled.reset(), o0)
    on = normed.reset()
    g = torch.Generator(device="cpu").manual_seed(2)
    for t in range(7):
        a = (torch.rand((9, 33, 2), generator=g) * 2 - 1).to(DEV)
        o0, r0, d0, _ = raw.step(a)
        o1, r1, d1, _ = scaled.step(a)
        on, rn, dn, _ = normed.step(a)
        assert same_bits(o1, o0) and same_bits(r1, r0 * 2) and torch.equal(d1, d0) and torch.equal(dn, d0), t
        absent = ~raw.live_agents()
        assert torch.isfinite(on).all() and torch.isfinite(rn).all() and not bits(on[absent]).any() and not bits(rn[absent]).any(), t
