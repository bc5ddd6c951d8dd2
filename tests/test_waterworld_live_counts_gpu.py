"""GPU tests (-m gpu) of per-env particle counts on the Waterworld crowd kernel (`crowd=True, per_env_counts=True`:
ww_crowd_kernel_live, csrc/waterworld_crowd.hip).  The definition of right: an env at live counts (p, e, po) computes what env n of a
fixed-shape (p, e, po) batch with the same seed and env_id_base + n computes.  So every test runs free against float32 oracle twins, one
twin of N envs per distinct triple, env n against env n of its triple's twin; nothing is copied across, and every output and the state
are compared in every bit at every step.  Host-facing layouts stay at the capacity, slotted by class."""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from helpers import bits, i32, same_bits, slots
from live_twins import LiveTwins, assert_collector_equals_stepping_by_hand, assert_obs_out_leaves_no_nan, lockstep, waterworld

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, BASE = 77, 500

# the parameters of test_waterworld_crowd_gpu.py::BEYOND at the capacities of this file
CAP_63 = dict(n_pursuers=13, n_evaders=25, n_poison=25, n_coop=3, n_sensors=16, radius=0.03, ev_speed=0.03, action_scale=0.03)
TRI_63 = [(13, 25, 25), (12, 24, 24), (7, 3, 20), (1, 1, 1)]


def _mk(n_envs, crowd=True, **kw):
    from madrl_amd.waterworld import BatchedMAWaterWorld
    return BatchedMAWaterWorld(n_envs=n_envs, device=DEV, crowd=crowd, **kw)


def _run(kw, triples, N, H, **more):
    return LiveTwins(waterworld(kw, SEED, BASE, "crowd", functools.partial(_mk, per_env_counts=True)), triples, N, H, **more)


def _free_run(kw, triples, N, T, H, **env_kw):
    run = _run(kw, triples, N, H, **env_kw)
    run.reset()
    rng = np.random.RandomState(1)
    for t in range(T):
        run.step(rng.uniform(-1, 1, size=(N, kw["n_pursuers"], 2)).astype(np.float32), "step %d" % t)
    print("%d evader catches, %d poison catches, %d time-limit resets" % (run.total("evc"), run.total("poc"), run.resets))
    return run


def test_first_shape_past_a_wavefront():
    run = _free_run(CAP_63, TRI_63, N=65, T=40, H=13)
    assert run.total("evc") > 0 and run.total("poc") > 0 and run.resets > 0


def test_chunk_boundaries_that_differ_per_env():
    """WE and WP (64-bit words per collision row) change from env to env inside one launch"""
    kw = dict(n_pursuers=65, n_evaders=65, n_poison=129, n_coop=2, n_sensors=30, ev_speed=0.04, action_scale=0.03)
    run = _free_run(kw, [(65, 65, 129), (64, 64, 128), (33, 1, 65), (1, 64, 1)], N=16, T=30, H=10)
    assert run.total("evc") + run.total("poc") > 0 and run.resets > 0


def test_rows_longer_than_a_wavefront():
    """K = 200: a sensing pass is 64 sensors of one pursuer, and the number of passes is per env"""
    kw = dict(n_pursuers=40, n_evaders=30, n_poison=20, n_coop=2, n_sensors=200, sensor_range=0.5)
    _free_run(kw, [(40, 30, 20), (39, 1, 20), (3, 30, 1)], N=6, T=20, H=7)


@pytest.mark.parametrize("kw,triples", [
    (dict(n_pursuers=33, n_evaders=20, n_poison=12, n_coop=2, n_sensors=7, radius=0.03, ev_speed=0.03, action_scale=0.03, obstacle_loc=None,
          reward_mech="global"), [(33, 20, 12), (32, 1, 12), (5, 20, 1)]),
    (dict(n_pursuers=8, n_evaders=8, n_poison=8, n_coop=1, n_sensors=12, speed_features=False, addid=False, sensor_range=0.3, radius=0.02),
     [(8, 8, 8), (3, 8, 2)])], ids=["random_obstacle_global_reward", "no_speed_features_no_id"])
def test_variants(kw, triples):
    run = _free_run(kw, triples, N=9, T=24, H=8)
    assert run.resets > 0


def test_counts_change_at_a_reset_not_before():
    N, H = 12, 9
    run = _run(CAP_63, TRI_63, N, H, deal=np.arange(N) % 2)   # (13, 25, 25) and (12, 24, 24)
    run.reset()
    rng = np.random.RandomState(2)
    act = lambda: rng.uniform(-1, 1, size=(N, 13, 2)).astype(np.float32)
    for t in range(3):
        run.step(act(), "warm-up %d" % t)
    young = np.arange(N) % 3 == 0
    run.reset(mask=young)                       # staggered ages: t = 1 for a third of the envs, 4 for the others; nothing is pending
    run.step(act(), "after the stagger")
    ages = run.env.get_state()["t"].cpu().numpy()
    assert set(ages[young]) == {2} and set(ages[~young]) == {5}
    # one shrinking change and one growing change, on all envs in the middle of their episodes
    old = run.cur.copy()
    run.set_pending(np.where(old == 0, 2, 0))   # (13, 25, 25) -> (7, 3, 20), (12, 24, 24) -> (13, 25, 25)
    pending, live = run.env.particle_counts()
    assert np.array_equal(live.cpu().numpy(), np.asarray(TRI_63)[old]) and not np.array_equal(pending.cpu().numpy(), live.cpu().numpy())
    switched = np.zeros(N, bool)
    for t in range(H):
        done = run.step(act(), "changing %d" % t)   # (check(): live == the twin each env is compared with, pending as set)
        assert np.array_equal(run.cur != old, switched | done), "an env changes at its own time limit, not before"
        switched |= done
        if t == 3:
            assert switched[~young].all() and not switched[young].any()   # the old envs are through, the young ones still on their old triple
    assert switched.all() and np.array_equal(run.cur, run.pend)
    # reset(mask=) applies the pending counts to the masked envs only
    before = run.cur.copy()
    run.set_pending(3)                          # (1, 1, 1)
    m = np.arange(N) % 4 == 1
    run.reset(mask=m)
    assert (run.cur[m] == 3).all() and np.array_equal(run.cur[~m], before[~m])
    run.step(act(), "after the masked reset")
    assert run.resets >= N


def test_teacher_forcing_through_the_slotted_layout():
    """the recording at 20 / 60 / 40 replayed on a capacity 24 / 64 / 48 batch at live (20, 60, 40): set_state(counts=, pos=, vel=) and
    step(respawn=) take their rows in slot order.  Protocol of test_waterworld_crowd_gpu.py::test_crowd_matches_reference_golden_teacher_forced."""
    from oracle import waterworld as ww
    g = np.load(os.path.join(ROOT, "tests", "golden", "wwcrowd_20_60_40.npz"))
    T, tri, cap = len(g["pre_t"]), (20, 60, 40), (24, 64, 48)
    kw = ww.kwargs_from_golden(g)
    assert (kw["n_pursuers"], kw["n_evaders"], kw["n_poison"]) == tri
    ckw = dict(kw, n_pursuers=cap[0], n_evaders=cap[1], n_poison=cap[2])
    env = _mk(T, per_env_counts=True, **ckw)
    orc = ww.WaterworldOracle(n_envs=T, dtype=np.float32, sensors=g["sensors"], **kw)
    s, NPc = slots(cap, tri), sum(cap)
    rng = np.random.RandomState(5)

    def slotted(a, fill):   # absent slots hold values that would matter if they were read
        out = fill((T, NPc) + a.shape[2:]).astype(np.float32)
        out[:, s] = a
        return out
    pos, vel = slotted(g["pre_pos"], lambda sh: rng.uniform(0, 1, sh)), slotted(g["pre_vel"], lambda sh: rng.uniform(-.01, .01, sh))
    resp = slotted(g["resp"], lambda sh: rng.uniform(0, 1, sh))
    act = np.zeros((T, cap[0], 2), np.float32); act[:, tri[0]:] = 1.0; act[:, :tri[0]] = g["act"]
    with pytest.raises(ValueError, match="pos and vel"):
        env.set_state(counts=np.tile(tri, (T, 1)), pos=pos)
    env.set_state(counts=np.tile(tri, (T, 1)), pos=pos, vel=vel, obst=g["obst"], t=g["pre_t"])
    orc.set_state(pos=g["pre_pos"], vel=g["pre_vel"], obst=g["obst"], t=g["pre_t"])
    st0 = env.get_state()
    gone = np.setdiff1d(np.arange(NPc), s)
    assert (st0["pos"][:, gone] == -1).all() and (st0["vel"][:, gone] == 0).all() and (st0["counts"].cpu().numpy() == tri).all()
    obs, rew, done, info = env.step(act, respawn=resp)
    oobs, orew, odone, oinfo = orc.step(g["act"], resp=g["resp"])
    st, ost = env.get_state(), orc.get_state()
    obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
    pos1, vel1 = st["pos"].cpu().numpy(), st["vel"].cpu().numpy()
    live = ~g["is_reset_step"].astype(bool)
    worst = oworst = 0.0
    for t in range(T):
        errs = [np.abs(pos1[t, s] - g["post_pos"][t]).max(), np.abs(vel1[t, s] - g["post_vel"][t]).max(), np.abs(obs[t, :20] - g["obs"][t]).max()]
        oerrs = [np.abs(ost["pos"][t] - g["post_pos"][t]).max(), np.abs(ost["vel"][t] - g["post_vel"][t]).max(), np.abs(oobs[t] - g["obs"][t]).max()]
        if live[t]:
            errs.append(np.abs(rew[t, :20] - g["rew"][t]).max())
            oerrs.append(np.abs(orew[t] - g["rew"][t]).max())
            assert bool(done[t]) == bool(g["done"][t])
            assert int(info["evcatches"][t]) == int(g["evc"][t]) and int(info["pocatches"][t]) == int(g["poc"][t]), "catches, step %d" % t
        assert int(st["t"][t]) == int(g["post_t"][t])
        worst, oworst = max(worst, max(errs)), max(oworst, max(oerrs))
    print("worst error kernel %.3g, float32 oracle %.3g" % (worst, oworst))
    assert oworst <= TOL and worst <= TOL
    assert np.array_equal(i32(obs[:, :20]), i32(oobs)) and not i32(obs[:, 20:]).any()
    assert np.array_equal(i32(rew[live, :20]), i32(orew[live])) and not i32(rew[:, 20:]).any()
    assert np.array_equal(i32(pos1[:, s]), i32(ost["pos"])) and np.array_equal(i32(vel1[:, s]), i32(ost["vel"]))
    assert (pos1[:, gone] == -1).all() and not i32(vel1[:, gone]).any()
    # get_state -> set_state on a second env object, which continues identically (free-running: the same seed and env ids)
    first, second = env, _mk(T, per_env_counts=True, **ckw)
    second.set_state(**st)
    a = torch.as_tensor(act, device=DEV)
    for t in range(5):
        o1, r1, d1, i1 = first.step(a)
        o2, r2, d2, i2 = second.step(a)
        assert same_bits(o1, o2) and same_bits(r1, r2) and torch.equal(i1["evcatches"], i2["evcatches"])
        s1, s2 = first.get_state(), second.get_state()
        for k in s1:
            assert same_bits(s1[k], s2[k]), (k, t)
    assert (s1["counts"].cpu().numpy() == tri).all() and (s1["t"] == st["t"] + 5).all()


def test_live_kernel_at_the_capacity_equals_the_fixed_shape_kernel():
    kw, N = dict(n_pursuers=12, n_evaders=25, n_poison=25, n_coop=3, n_sensors=16, radius=0.03), 65
    a = _mk(N, per_env_counts=True, seed=5, env_id_base=9, max_steps=15, auto_reset=True, **kw)
    b = _mk(N, seed=5, env_id_base=9, max_steps=15, auto_reset=True, **kw)
    assert len(list(lockstep(a, b, (N, 12, 2), 40, ("evcatches", "pocatches")))) == 40


def _mixed(N=8, **kw):
    env = _mk(N, per_env_counts=True, seed=4, max_steps=5, auto_reset=True, **dict(CAP_63, **kw))
    tri = np.asarray(TRI_63)[np.arange(N) % 4]
    env.set_particle_counts(tri[:, 0], tri[:, 1], tri[:, 2])
    return env


def test_interface_errors_and_counts_across_a_new_handle():
    from madrl_amd.waterworld import BatchedMAWaterWorld, MAWaterWorld
    with pytest.raises(ValueError, match="crowd=True"):
        BatchedMAWaterWorld(3, 4, n_envs=2, device=DEV, per_env_counts=True)
    fixed = _mk(2, **CAP_63)
    with pytest.raises(RuntimeError, match="per_env_counts=True"):
        fixed.set_particle_counts(n_pursuers=3)
    assert "counts" not in fixed.get_state() and "per_env_counts" not in fixed._ctor
    plain = _mk(2, crowd=False, n_pursuers=3, n_evaders=4)
    assert set(plain._ctor) == set(pickle.loads(pickle.dumps(plain))._ctor) and not {"crowd", "per_env_counts"} & set(plain._ctor)
    env = _mixed()
    for bad in (dict(n_pursuers=0), dict(n_pursuers=14), dict(n_evaders=26), dict(n_poison=[1, 2, 3, 4, 5, 6, 7, 0])):
        with pytest.raises(ValueError, match="capacity"):
            env.set_particle_counts(**bad)
    env.set_particle_counts(n_pursuers=14, mask=np.zeros(8, bool))     # out of range where the mask does not reach: nothing is set
    env.reset()
    env.set_particle_counts(n_evaders=2, mask=np.arange(8) < 4)
    pending, live = env.particle_counts()
    assert np.array_equal(live.cpu().numpy(), np.asarray(TRI_63)[np.arange(8) % 4])
    assert pending[:4, 1].tolist() == [2] * 4 and torch.equal(pending[4:], live[4:])
    assert torch.equal(env.live_agents(), torch.arange(13, device=DEV)[None, :] < live[:, :1])
    env.seed(11)                                                       # a new handle, the same count tensors
    p2, l2 = env.particle_counts()
    assert torch.equal(p2, pending) and torch.equal(l2, live)
    env.reset()
    assert torch.equal(env.particle_counts()[1], pending)
    again = pickle.loads(pickle.dumps(env))                            # a pickle keeps the constructor arguments: back at the capacity
    assert again._ctor["per_env_counts"] is True and again.kernel_kind == "crowd"
    assert (again.particle_counts()[1].cpu().numpy() == (13, 25, 25)).all()
    one = MAWaterWorld(device=DEV, crowd=True, per_env_counts=True, **CAP_63)   # the N == 1 drop-in passes the flag through
    one._env.set_particle_counts(n_pursuers=5)
    rows = one.reset()
    assert len(rows) == 13 and np.abs(rows[4]).max() > 0 and not np.abs(rows[5]).any()


def test_obs_out_leaves_no_nan_in_an_uninitialised_destination():
    assert_obs_out_leaves_no_nan(_mixed())


def test_rollout_collector_and_standardized_env_over_a_mixed_batch():
    from madrl_amd.heuristics import WaterworldHeuristicPolicy
    from madrl_amd.wrappers import StandardizedEnv
    assert_collector_equals_stepping_by_hand(_mixed, WaterworldHeuristicPolicy, H=8, min_dones=8)
    # StandardizedEnv takes its epilogue kernels over the capacity-shaped rows: scaling alone is the raw step times the scale, and the
    # rows of absent pursuers standardise to exactly 0 (mean 0, value 0)
    raw, scaled, normed = _mixed(), StandardizedEnv(_mixed(), scale_reward=2.0), StandardizedEnv(_mixed(), enable_obsnorm=True, enable_rewnorm=True)
    assert not scaled._fused and not normed._fused
    o0 = raw.reset()
    assert same_bits(scaled.reset(), o0)
    on = normed.reset()
    absent = ~raw.live_agents()
    g = torch.Generator(device="cpu").manual_seed(2)
    for t in range(7):
        a = (torch.rand((8, 13, 2), generator=g) * 2 - 1).to(DEV)
        o0, r0, d0, _ = raw.step(a)
        o1, r1, d1, _ = scaled.step(a)
        on, rn, dn, _ = normed.step(a)
        assert same_bits(o1, o0) and same_bits(r1, r0 * 2) and torch.equal(d1, d0) and torch.equal(dn, d0), t
        absent = ~raw.live_agents()
        assert torch.isfinite(on).all() and torch.isfinite(rn).all() and not bits(on[absent]).any() and not bits(rn[absent]).any(), t
