"""GPU tests (-m gpu) of per-env particle counts on the one-wavefront Waterworld kernel (`per_env_counts="wave"`: waterworld_kernel_live,
csrc/waterworld.hip).  The definition of right is the crowd form's (test_waterworld_live_counts_gpu.py): an env at live counts (p, e, po)
computes what env n of a fixed-shape (p, e, po) batch with the same seed and env_id_base + n computes.  Every free run has one float32
oracle twin of N envs per distinct triple, env n is compared with env n of its triple's twin, nothing is copied across, and every output
and the whole state are compared in every bit at every step.  Host-facing layouts stay at the capacity, slotted by class."""
import os
import pickle

import numpy as np
import pytest
import torch

from helpers import i32, same_bits, slots
from live_twins import LiveTwins, assert_collector_equals_stepping_by_hand, assert_obs_out_leaves_no_nan, lockstep, waterworld

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, BASE = 31, 900

# BASELINE configs[2] (the reference's Waterworld) as the capacity, moving fast enough for catches inside short episodes
CAP_C3 = dict(n_pursuers=5, n_evaders=10, n_poison=10, n_coop=2, n_sensors=30, radius=0.03, ev_speed=0.03, action_scale=0.03)
TRI_C3 = [(5, 10, 10), (4, 9, 9), (2, 3, 7), (1, 1, 1)]


def _mk(n_envs, per_env_counts="wave", **kw):
    from madrl_amd.waterworld import BatchedMAWaterWorld
    env = BatchedMAWaterWorld(n_envs=n_envs, device=DEV, per_env_counts=per_env_counts, **kw)
    if not kw.get("crowd"):
        assert env.kernel_kind == "wave"
    return env


def _run(kw, triples, N, H, **more):
    return LiveTwins(waterworld(kw, SEED, BASE, "wave", _mk), triples, N, H, **more)


def _free_run(kw, triples, N, T, H, max_blocks=0):
    run = _run(kw, triples, N, H, max_blocks=max_blocks)
    run.reset()
    rng = np.random.RandomState(1)
    for t in range(T):
        run.step(rng.uniform(-1, 1, size=(N, kw["n_pursuers"], 2)).astype(np.float32), "step %d" % t)
    print("%d evader catches, %d poison catches, %d time-limit resets" % (run.total("evc"), run.total("poc"), run.resets))
    return run


def test_reference_shape_as_capacity_one_wavefront_walks_mixed_envs():
    """13 envs on 3 wavefronts: a wavefront's consecutive envs have different triples -- the prefetch with capacity strides, per-env LDS contents"""
    run = _free_run(CAP_C3, TRI_C3, N=13, T=40, H=12, max_blocks=3)
    assert run.total("evc") > 0 and run.total("poc") > 0 and run.resets >= 3 * 13


def test_both_limits_of_a_wavefront_at_once():
    """62 particles and 32 pursuers: a record of 252 dwords (4 in every lane), the action row on all 64 lanes"""
    kw = dict(n_pursuers=32, n_evaders=15, n_poison=15, n_coop=2, n_sensors=4, radius=0.03, ev_speed=0.03, action_scale=0.03)
    run = _free_run(kw, [(32, 15, 15), (32, 1, 1), (1, 15, 15), (17, 8, 9)], N=9, T=30, H=8, max_blocks=2)
    assert run.total("evc") + run.total("poc") > 0 and run.resets > 0


def test_number_of_sensing_passes_differs_per_env():
    """K = 200: 10, 4 or 7 passes of 64 (pursuer, sensor) pairs"""
    kw = dict(n_pursuers=3, n_evaders=4, n_poison=4, n_coop=1, n_sensors=200, sensor_range=0.5)
    _free_run(kw, [(3, 4, 4), (1, 4, 1), (2, 1, 3)], N=7, T=20, H=7, max_blocks=2)


@pytest.mark.parametrize("kw,triples", [
    (dict(n_pursuers=6, n_evaders=7, n_poison=5, n_coop=2, n_sensors=7, radius=0.03, ev_speed=0.03, action_scale=0.03, obstacle_loc=None,
          reward_mech="global"), [(6, 7, 5), (5, 1, 5), (2, 7, 1)]),
    (dict(n_pursuers=8, n_evaders=8, n_poison=8, n_coop=1, n_sensors=12, speed_features=False, addid=False, sensor_range=0.3, radius=0.02),
     [(8, 8, 8), (3, 8, 2)])], ids=["random_obstacle_global_reward", "no_speed_features_no_id"])
def test_variants(kw, triples):
    run = _free_run(kw, triples, N=9, T=24, H=8, max_blocks=4)
    assert run.resets > 0


def test_counts_change_at_a_reset_not_before():
    N, H = 12, 9
    run = _run(CAP_C3, TRI_C3, N, H, deal=np.arange(N) % 2, max_blocks=5)   # (5, 10, 10) and (4, 9, 9)
    run.reset()
    rng = np.random.RandomState(2)
    act = lambda: rng.uniform(-1, 1, size=(N, 5, 2)).astype(np.float32)
    for t in range(3):
        run.step(act(), "warm-up %d" % t)
    young = np.arange(N) % 3 == 0
    run.reset(mask=young)                       # staggered ages: t = 1 for a third of the envs, 4 for the others; nothing is pending
    run.step(act(), "after the stagger")
    ages = run.env.get_state()["t"].cpu().numpy()
    assert set(ages[young]) == {2} and set(ages[~young]) == {5}
    # one shrinking change and one growing change, on all envs in the middle of their episodes
    old = run.cur.copy()
    run.set_pending(np.where(old == 0, 2, 0))   # (5, 10, 10) -> (2, 3, 7), (4, 9, 9) -> (5, 10, 10)
    pending, live = run.env.particle_counts()
    assert np.array_equal(live.cpu().numpy(), np.asarray(TRI_C3)[old]) and not np.array_equal(pending.cpu().numpy(), live.cpu().numpy())
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
    """the reference's recording at 5 / 10 / 10 replayed on a capacity 6 / 12 / 12 batch at live (5, 10, 10): set_state(counts=, pos=, vel=)
    and step(respawn=) take their rows in slot order.  Protocol of test_waterworld_gpu.py::test_hip_matches_reference_golden_teacher_forced."""
    from oracle import waterworld as ww
    g = np.load(os.path.join(ROOT, "tests", "golden", "waterworld_c3_catches.npz"))
    T, tri, cap = len(g["pre_t"]), (5, 10, 10), (6, 12, 12)
    kw = ww.kwargs_from_golden(g)
    assert (kw["n_pursuers"], kw["n_evaders"], kw["n_poison"]) == tri
    env = _mk(T, **dict(kw, n_pursuers=cap[0], n_evaders=cap[1], n_poison=cap[2]))
    orc = ww.WaterworldOracle(n_envs=T, dtype=np.float32, sensors=g["sensors"], **kw)
    s, NPc, p = slots(cap, tri), sum(cap), tri[0]
    gone = np.setdiff1d(np.arange(NPc), s)
    rng = np.random.RandomState(5)

    def slotted(a, fill):   # absent slots hold values that would matter if they were read
        out = fill((T, NPc) + a.shape[2:]).astype(np.float32)
        out[:, s] = a
        return out
    pos, vel = slotted(g["pre_pos"], lambda sh: rng.uniform(0, 1, sh)), slotted(g["pre_vel"], lambda sh: rng.uniform(-.01, .01, sh))
    resp = slotted(g["resp"], lambda sh: rng.uniform(0, 1, sh))
    act = np.ones((T, cap[0], 2), np.float32); act[:, :p] = g["act"]
    env.set_state(counts=np.tile(tri, (T, 1)), pos=pos, vel=vel, obst=g["obst"], t=g["pre_t"])
    orc.set_state(pos=g["pre_pos"], vel=g["pre_vel"], obst=g["obst"], t=g["pre_t"])
    st0 = env.get_state()
    assert (st0["pos"][:, gone] == -1).all() and (st0["vel"][:, gone] == 0).all() and (st0["counts"].cpu().numpy() == tri).all()
    obs, rew, done, info = env.step(act, respawn=resp)
    oobs, orew, _odone, _oinfo = orc.step(g["act"], resp=g["resp"])
    st, ost = env.get_state(), orc.get_state()
    obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
    pos1, vel1 = st["pos"].cpu().numpy(), st["vel"].cpu().numpy()
    live = ~g["is_reset_step"].astype(bool)
    worst = oworst = 0.0
    for t in range(T):
        errs = [np.abs(pos1[t, s] - g["post_pos"][t]).max(), np.abs(vel1[t, s] - g["post_vel"][t]).max(), np.abs(obs[t, :p] - g["obs"][t]).max()]
        oerrs = [np.abs(ost["pos"][t] - g["post_pos"][t]).max(), np.abs(ost["vel"][t] - g["post_vel"][t]).max(), np.abs(oobs[t] - g["obs"][t]).max()]
        if live[t]:
            errs.append(np.abs(rew[t, :p] - g["rew"][t]).max())
            oerrs.append(np.abs(orew[t] - g["rew"][t]).max())
            assert bool(done[t]) == bool(g["done"][t])
            assert int(info["evcatches"][t]) == int(g["evc"][t]) and int(info["pocatches"][t]) == int(g["poc"][t]), "catches, step %d" % t
        assert int(st["t"][t]) == int(g["post_t"][t])
        worst, oworst = max(worst, max(errs)), max(oworst, max(oerrs))
    print("worst error kernel %.3g, float32 oracle %.3g; %d catches" % (worst, oworst, int(np.nansum(g["evc"][live]) + np.nansum(g["poc"][live]))))
    assert oworst <= TOL and worst <= TOL
    assert np.array_equal(i32(obs[:, :p]), i32(oobs)) and not i32(obs[:, p:]).any()
    assert np.array_equal(i32(rew[live, :p]), i32(orew[live])) and not i32(rew[:, p:]).any()
    assert np.array_equal(i32(pos1[:, s]), i32(ost["pos"])) and np.array_equal(i32(vel1[:, s]), i32(ost["vel"]))
    assert (pos1[:, gone] == -1).all() and not i32(vel1[:, gone]).any()


CATCHES = ("evcatches", "pocatches")


@pytest.mark.parametrize("kw", [dict(CAP_C3), dict(n_pursuers=12, n_evaders=25, n_poison=25, n_coop=3, n_sensors=16, radius=0.03)],
                         ids=["specialised_5_10_10_30", "generic_12_25_25_16"])
def test_live_kernel_at_the_capacity_equals_the_fixed_shape_kernel(kw):
    N = 65
    a = _mk(N, seed=5, env_id_base=9, max_steps=15, auto_reset=True, **kw)
    b = _mk(N, per_env_counts=False, seed=5, env_id_base=9, max_steps=15, auto_reset=True, **kw)
    assert b.kernel_kind == "wave" and not b.per_env_counts
    assert len(list(lockstep(a, b, (N, kw["n_pursuers"], 2), 40, CATCHES))) == 40


def test_live_kernel_equals_the_crowd_live_kernel_on_mixed_triples():
    kw, N = dict(n_pursuers=12, n_evaders=25, n_poison=25, n_coop=3, n_sensors=16, radius=0.03, ev_speed=0.03, action_scale=0.03), 21
    tri = np.asarray([(12, 25, 25), (11, 24, 2), (3, 1, 25), (1, 1, 1), (7, 13, 12)])
    a = _mk(N, seed=5, env_id_base=9, max_steps=9, auto_reset=True, **kw)
    b = _mk(N, per_env_counts=True, crowd=True, seed=5, env_id_base=9, max_steps=9, auto_reset=True, **kw)
    assert a.kernel_kind == "wave" and b.kernel_kind == "crowd"
    a.set_launch(4)
    deal = tri[np.arange(N) % 5]
    for e in (a, b):
        e.set_particle_counts(deal[:, 0], deal[:, 1], deal[:, 2])
    for t in lockstep(a, b, (N, 12, 2), 30, CATCHES, counts=True):
        if t == 12:   # a count change in the middle of the episodes: taken at each env's next time limit
            deal = tri[(np.arange(N) + 2) % 5]
            for e in (a, b):
                e.set_particle_counts(deal[:, 0], deal[:, 1], deal[:, 2])
    assert np.array_equal(a.particle_counts()[1].cpu().numpy(), deal)


def _mixed(N=8, **kw):
    env = _mk(N, seed=4, max_steps=5, auto_reset=True, **dict(CAP_C3, **kw))
    tri = np.asarray(TRI_C3)[np.arange(N) % 4]
    env.set_particle_counts(tri[:, 0], tri[:, 1], tri[:, 2])
    return env


def test_interface():
    from madrl_amd import _lib
    from madrl_amd.waterworld import MAWaterWorld
    env = _mixed()
    for bad in (dict(n_pursuers=0), dict(n_pursuers=6), dict(n_evaders=11), dict(n_poison=[1, 2, 3, 4, 5, 6, 7, 0])):
        with pytest.raises(ValueError, match="capacity"):
            env.set_particle_counts(**bad)
    env.reset()
    env.set_particle_counts(n_evaders=2, mask=np.arange(8) < 4)
    pending, live = env.particle_counts()
    assert np.array_equal(live.cpu().numpy(), np.asarray(TRI_C3)[np.arange(8) % 4])
    assert pending[:4, 1].tolist() == [2] * 4 and torch.equal(pending[4:], live[4:])
    assert torch.equal(env.live_agents(), torch.arange(5, device=DEV)[None, :] < live[:, :1])
    env.seed(11)                                                       # a new handle, the same count tensors
    p2, l2 = env.particle_counts()
    assert torch.equal(p2, pending) and torch.equal(l2, live) and env.kernel_kind == "wave"
    env.reset()
    assert torch.equal(env.particle_counts()[1], pending)
    again = pickle.loads(pickle.dumps(env))                            # a pickle keeps the constructor arguments: back at the capacity
    assert again._ctor["per_env_counts"] == "wave" and again.kernel_kind == "wave" and again.per_env_counts
    assert (again.particle_counts()[1].cpu().numpy() == (5, 10, 10)).all()
    plain = _mk(2, per_env_counts=False, n_pursuers=3, n_evaders=4)    # pickles of envs built without the flag are unchanged
    assert not {"crowd", "per_env_counts"} & set(plain._ctor) and set(plain._ctor) == set(pickle.loads(pickle.dumps(plain))._ctor)
    with pytest.raises(RuntimeError, match="per_env_counts"):
        plain.set_particle_counts(n_pursuers=2)
    # no fused StandardizedEnv on the live kernel
    assert env.fused_standardize is False and plain.fused_standardize is True
    with pytest.raises(_lib.MadrlError, match="no fused StandardizedEnv"):
        env.bind_standardize()
    one = MAWaterWorld(device=DEV, per_env_counts="wave", **CAP_C3)    # the N == 1 drop-in passes the flag through
    assert one._env.kernel_kind == "wave"
    one._env.set_particle_counts(n_pursuers=2)
    rows = one.reset()
    assert len(rows) == 5 and np.abs(rows[1]).max() > 0 and not np.abs(rows[2]).any()
    _obs, rew, _done, _info = one.step(np.ones((5, 2)))
    assert rew[1] != 0 and not rew[2:].any()


def test_fused_standardize_and_live_counts_refuse_each_other_in_c():
    import ctypes as C
    from madrl_amd import _lib
    L = _lib.lib()
    plain = _mk(4, per_env_counts=False, **CAP_C3)
    st = plain.bind_standardize(enable_obsnorm=True)                   # a fused StandardizedEnv first: the counts are refused
    counts = torch.tensor((5, 10, 10), dtype=torch.int32, device=DEV).repeat(4, 1).contiguous()
    live = counts.clone()
    assert L.madrl_waterworld_set_particle_counts(plain._handle, _lib.ptr(counts), _lib.ptr(live)) != 0
    assert b"StandardizedEnv" in L.madrl_last_error()
    plain.unbind_standardize()
    _lib.check(L.madrl_waterworld_set_particle_counts(plain._handle, _lib.ptr(counts), _lib.ptr(live)))
    a = _lib.StandardizeArgs()                                          # the counts first: the fused StandardizedEnv is refused
    a.struct_size = C.sizeof(_lib.StandardizeArgs)
    a.enable_obsnorm, a.obs_alpha, a.rew_alpha, a.eps, a.scale_reward = 1, 0.001, 0.001, 1e-8, 1.0
    for k, v in st.items():
        setattr(a, k, v.data_ptr())
    assert L.madrl_waterworld_set_standardize(plain._handle, C.byref(a)) != 0 and b"live-count" in L.madrl_last_error()
    _lib.check(L.madrl_waterworld_set_particle_counts(plain._handle, None, None))   # both NULL: the mode is off again
    _lib.check(L.madrl_waterworld_set_standardize(plain._handle, C.byref(a)))
    _lib.check(L.madrl_waterworld_set_standardize(plain._handle, None))
    from madrl_amd.hostage import BatchedContinuousHostageWorld         # the hostage world's one-wavefront handle keeps refusing counts
    hw = BatchedContinuousHostageWorld(3, 4, 2, 2, 2, n_envs=4, device=DEV)
    c3 = torch.tensor((3, 4, 2), dtype=torch.int32, device=DEV).repeat(4, 1).contiguous()
    assert L.madrl_hostage_set_particle_counts(hw._handle, _lib.ptr(c3), _lib.ptr(c3.clone())) != 0
    assert b"crowd kernel (cfg.crowd = 1)" in L.madrl_last_error()


def test_standardized_env_runs_its_epilogue_kernels():
    from madrl_amd.wrappers import StandardizedEnv
    kws = dict(scale_reward=2.0, enable_obsnorm=True, enable_rewnorm=True)
    auto, unfused = StandardizedEnv(_mixed(), **kws), StandardizedEnv(_mixed(), fused=False, **kws)
    assert not auto._fused and not unfused._fused
    assert same_bits(auto.reset(), unfused.reset())
    g = torch.Generator(device="cpu").manual_seed(2)
    for t in range(7):
        a = (torch.rand((8, 5, 2), generator=g) * 2 - 1).to(DEV)
        o1, r1, d1, _ = auto.step(a)
        o2, r2, d2, _ = unfused.step(a)
        assert same_bits(o1, o2) and same_bits(r1, r2) and torch.equal(d1, d2), t
    assert torch.isfinite(o1).all() and torch.isfinite(r1).all()


def test_obs_out_leaves_no_nan_in_an_uninitialised_destination():
    assert_obs_out_leaves_no_nan(_mixed())


def test_rollout_collector_over_a_mixed_batch_equals_stepping_by_hand():
    from madrl_amd.heuristics import WaterworldHeuristicPolicy
    assert_collector_equals_stepping_by_hand(_mixed, WaterworldHeuristicPolicy, H=8, min_dones=8)
