"""GPU parity tests (-m gpu) for the HIP MAWaterWorld path through the C ABI.
(1) teacher-forced against the reference's golden vectors (float64), tolerance 1e-5 as
north_star states; (2) free-running against the float32 build of the C oracle."""
import glob
import os

import numpy as np
import pytest
import torch

from waterworld_parity import DEV, TOL, vs_f32_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "waterworld_*.npz")))
gid = lambda p: os.path.basename(p)[:-4]


def _mk(n_envs, **kw):
    from madrl_amd.waterworld import BatchedMAWaterWorld
    return BatchedMAWaterWorld(n_envs=n_envs, device=DEV, **kw)


@pytest.mark.parametrize("path", FILES, ids=gid)
def test_hip_matches_reference_golden_teacher_forced(path):
    """All recorded steps of a file are independent under teacher forcing -> one batch."""
    from oracle import waterworld as ww
    g = np.load(path)
    T = len(g["pre_t"])
    env = _mk(T, **ww.kwargs_from_golden(g))
    assert env.obs_dim == g["obs"].shape[-1]
    env.set_state(pos=g["pre_pos"], vel=g["pre_vel"], obst=g["obst"], t=g["pre_t"])
    obs, rew, done, info = env.step(g["act"], respawn=g["resp"])
    st = env.get_state()
    flips = 0
    worst = 0.0
    for t in range(T):
        errs = [np.abs(st["pos"][t].cpu().numpy() - g["post_pos"][t]).max(),
                np.abs(st["vel"][t].cpu().numpy() - g["post_vel"][t]).max(),
                np.abs(obs[t].cpu().numpy() - g["obs"][t]).max()]
        if not g["is_reset_step"][t]:
            errs.append(np.abs(rew[t].cpu().numpy() - g["rew"][t]).max())
            assert bool(done[t]) == bool(g["done"][t])
            assert int(info["evcatches"][t]) == int(g["evc"][t]), "evcatches, step %d" % t
            assert int(info["pocatches"][t]) == int(g["poc"][t]), "pocatches, step %d" % t
        assert int(st["t"][t]) == int(g["post_t"][t])
        e = max(errs)
        if e > TOL:
            flips += 1  # a <= / > test decided differently in float32 -- none on the committed fixtures
            print("golden %s step %d: error %.3g beyond %.0e" % (gid(path), t, e, TOL))
        else:
            worst = max(worst, e)
    assert flips == 0, "%d of %d steps beyond %.0e" % (flips, T, TOL)
    assert worst <= TOL


CASES = {
    "c3_default": dict(n_pursuers=5, n_evaders=10),
    "global_randobst": dict(n_pursuers=5, n_evaders=10, obstacle_loc=None, reward_mech="global"),
    "small_nospeed": dict(n_pursuers=3, n_evaders=10, n_coop=2, n_poison=5, n_sensors=12, speed_features=False,
                          addid=False, sensor_range=0.3),
    # runners/run_waterworld.py:16-20 defaults: the second specialised shape (two 64-bit words per collision matrix)
    "runner_default_8v10": dict(n_pursuers=8, n_evaders=10, n_coop=4, n_poison=10),
    "runner_default_8v10_coop1": dict(n_pursuers=8, n_evaders=10, n_coop=1, n_poison=10, ev_speed=0.05, radius=0.03),
    # the other shapes the reference's own scripts construct (specialised: waterworld_specializations.def)
    "gru_test_3_10_2_5": dict(n_pursuers=3, n_evaders=10, n_coop=2, n_poison=5, ev_speed=0.04, radius=0.03),   # rllabwrapper/rllab_gru_test.py:13
    "con_runner_3v5": dict(n_pursuers=3, n_evaders=5, n_coop=2, n_poison=10, ev_speed=0.04, radius=0.03),     # runners/old/rltools/run_con_waterworld.py:57-61
    "coop1_dense": dict(n_pursuers=6, n_evaders=12, n_coop=1, n_poison=12, ev_speed=0.05, action_scale=0.05, n_sensors=20,
                        radius=0.03),
}


# The generic kernel at its limits: 62 particles, so the record is four dwords per lane; 70 sensors, so the passes of 64 (pursuer, sensor)
# pairs straddle pursuers; rows of 7 * 70 + 3 = 493 floats, so the 16-byte row store has a dword tail; about 41 KB of LDS per workgroup
LIMITS = dict(n_pursuers=20, n_evaders=22, n_poison=20, n_sensors=70, obstacle_loc=None, reward_mech="global")


def _vs_f32_oracle(case, teacher_forced, **run):
    """waterworld_parity.vs_f32_oracle (shared with test_waterworld_specialised_gpu.py) on a case of CASES or on constructor arguments"""
    return vs_f32_oracle(CASES[case] if isinstance(case, str) else case, teacher_forced, **run)


@pytest.mark.parametrize("case", sorted(CASES), ids=sorted(CASES))
def test_hip_matches_f32_oracle_free_running(case):
    """truly free-running: no state is ever copied from the oracle to the kernel; every output and the state bit-identical for 60 steps"""
    _vs_f32_oracle(case, teacher_forced=False)


def test_generic_kernel_at_its_limits_free_running_vs_f32_oracle():
    """LIMITS, free-running under auto-reset: every output and the state bit-identical to the float32 oracle"""
    _vs_f32_oracle(LIMITS, teacher_forced=False, N=64, T=40, H=15)


@pytest.mark.parametrize("case", sorted(CASES), ids=sorted(CASES))
def test_hip_matches_f32_oracle_teacher_forced(case):
    """the protocol of rounds 1 - 4 (then named "free running"): the kernel takes the oracle's state before every step; 1e-5"""
    _vs_f32_oracle(case, teacher_forced=True)


def _drawn_case(i):
    from oracle.make_golden_waterworld_fuzz import draw_case
    rng = np.random.RandomState(20260929)
    for _ in range(i + 1):
        (Np, Ne), kw, _run = draw_case(rng)
    kw = dict(kw, n_pursuers=Np, n_evaders=Ne)
    if isinstance(kw.get("obstacle_loc", 0), np.ndarray):
        kw["obstacle_loc"] = tuple(float(v) for v in kw["obstacle_loc"])
    return kw


@pytest.mark.parametrize("i", range(10))
def test_drawn_configurations_free_running_vs_f32_oracle(i):
    """configurations drawn like the recorded ones (oracle/make_golden_waterworld_fuzz.py), another seed, nothing injected (respawns, random
    obstacles, auto-reset from Philox on both sides), truly free-running and bit-identical, on random shapes"""
    CASES["drawn_%d" % i] = _drawn_case(i)
    try:
        _vs_f32_oracle("drawn_%d" % i, teacher_forced=False)
    except AssertionError as e:
        if str(e) != "no catches":
            raise
    finally:
        del CASES["drawn_%d" % i]


# shape -> (constructor arguments, the kernel family that takes them, whether the crafted pairs are the LAST of their classes)
THRESHOLD_SHAPES = {
    "c3_bitrows": (dict(n_pursuers=5, n_evaders=10, n_coop=1), "specialised", False),
    "generic": (dict(n_pursuers=3, n_evaders=10, n_coop=1, n_poison=5, n_sensors=12), "generic", False),
    # test lines of waterworld_specializations.def: four words per ballot matrix (pursuer 7 x evader 29 is bit 239: word 3 of col_ev) and
    # the byte matrices of a specialised kernel (WE = 5)
    "words4": (dict(n_pursuers=8, n_evaders=30, n_coop=1, n_poison=16, n_sensors=8), "specialised", True),
    "spec_bytes": (dict(n_pursuers=10, n_evaders=30, n_coop=1, n_poison=16, n_sensors=6), "specialised", True),
}


@pytest.mark.parametrize("shape", ["c3_bitrows", "generic", "words4", "spec_bytes"])
def test_contact_tests_at_the_threshold_match_the_sqrt_formulation(shape):
    """The kernel tests `dx*dx + dy*dy <= sq_threshold(thr)` where the reference (and the float32 oracle) test `sqrt(...) <= thr`.
    The two must give the same truth value for EVERY input: crafted states put an evader / a poison at the contact distance of a
    pursuer, and an evader at the rebound distance of the obstacle, within +-8 ulps of the threshold along 256 directions.
    words4 / spec_bytes: the touching pursuers are the last two, the evader and the poison the last of their classes -- the highest bits
    of the ballot words, the last bytes of the byte matrices."""
    from oracle import waterworld as ww
    kw, family, last = THRESHOLD_SHAPES[shape]
    Np, Ne = kw["n_pursuers"], kw["n_evaders"]
    Npo = kw.get("n_poison", 10)
    NP = Np + Ne + Npo
    pu_ev, pu_po, ev_hit, po_hit = (Np - 1, Np - 2, Np + Ne - 1, Np + Ne + Npo - 1) if last else (0, 1, Np, Np + Ne)
    N = 17 * 256
    env = _mk(N, seed=3, max_steps=1000, auto_reset=False, **kw)
    orc = ww.WaterworldOracle(n_envs=N, seed=3, max_steps=1000, dtype=np.float32, **kw)
    env.reset(); orc.reset()
    r = np.float32(0.015)
    r_pu, r_ev, r_po, r_ob = r, np.float32(np.float64(r) * 2), np.float32(np.float64(r) * 3 / 4), np.float32(0.2)
    k = np.repeat(np.arange(-8, 9), 256).astype(np.int64)                 # ulps off the threshold
    th = np.tile(np.arange(256) * (2 * np.pi / 256) + 0.001, 17)           # direction
    def at_distance(center, thr, k, th):
        thr = np.full(N, thr, np.float32)
        d = (thr.view(np.int32) + k.astype(np.int32)).view(np.float32)     # thr moved by k ulps
        return np.stack([center[:, 0] + d * np.cos(th).astype(np.float32), center[:, 1] + d * np.sin(th).astype(np.float32)], -1).astype(np.float32)
    pos = np.zeros((N, NP, 2), np.float32)
    if last:   # 54 / 56 particles: the pursuers parked at the left wall, the evaders and poison at the right one, nobody near the obstacle
        pos[:, :Np, 0] = 0.05; pos[:, :Np, 1] = np.linspace(0.3, 0.7, Np).astype(np.float32)[None, :]
        pos[:, Np:, 0] = 0.95; pos[:, Np:, 1] = np.linspace(0.05, 0.95, NP - Np).astype(np.float32)[None, :]
    else:
        far = np.linspace(0.02, 0.12, NP).astype(np.float32)
        pos[:, :, 0] = 0.9; pos[:, :, 1] = far[None, :] * 4 + 0.3           # everything parked away from everything else
    pos[:, pu_ev] = (0.30, 0.12); pos[:, pu_po] = (0.62, 0.12)
    pos[:, ev_hit] = at_distance(pos[:, pu_ev], r_pu + r_ev, k, th)        # an evader at contact distance of a pursuer
    pos[:, po_hit] = at_distance(pos[:, pu_po], r_pu + r_po, k, th)        # a poison at contact distance of another pursuer
    obst = np.tile(np.float32([0.5, 0.7]), (N, 1))
    pos[:, Np + 1] = at_distance(obst, r_ev + r_ob, k, th)                 # evader 1 at rebound distance of the obstacle
    vel = np.zeros((N, NP, 2), np.float32)
    vel[:, Np + 1] = (0.001, -0.002)
    st = orc.get_state()
    for e in (env, orc):
        e.set_state(pos=pos, vel=vel, obst=obst, t=st["t"], tick=np.asarray(st["tick"]).view(np.int32))
    act = np.zeros((N, Np, 2), np.float32)
    obs, rew, done, info = env.step(act)
    assert env.last_launch_kernel == family
    oobs, orew, odone, oinfo = orc.step(act)
    assert np.array_equal(info["evcatches"].cpu().numpy(), oinfo[:, 0])
    assert np.array_equal(info["pocatches"].cpu().numpy(), oinfo[:, 1])
    assert 0 < oinfo[:, 0].sum() < N and 0 < oinfo[:, 1].sum() < N          # both sides of both thresholds were hit
    gst, ost = env.get_state(), orc.get_state()
    assert np.array_equal(gst["vel"].cpu().numpy()[:, Np + 1], ost["vel"][:, Np + 1])   # rebound or not: identical
    flipped = (ost["vel"][:, Np + 1, 0] < 0).sum()
    assert 0 < flipped < N
    assert np.abs(obs.cpu().numpy() - oobs).max() <= TOL


def test_full_batch_invariants_c3():
    """BASELINE C3 size (32 768 envs): properties that do not need the oracle."""
    N, Np = 32768, 5
    env = _mk(N, n_pursuers=5, n_evaders=10, seed=5, auto_reset=True)
    obs = env.reset()
    st = env.get_state()
    assert (st["t"] == 1).all()
    d = (st["pos"][:, :Np] - st["obst"][:, None]).norm(dim=-1)
    assert (d > 0.2).all()                                   # nobody spawns on the obstacle
    g = torch.Generator(device=DEV).manual_seed(0)
    tot_ev = torch.zeros(N, dtype=torch.int64, device=DEV)
    for t in range(50):
        a = torch.rand((N, Np, 2), generator=g, device=DEV) * 2 - 1
        obs, rew, done, info = env.step(a)
        tot_ev += info["evcatches"].long()
    st = env.get_state()
    p = st["pos"][:, :Np]
    assert ((p >= 0) & (p <= 1)).all()                       # pursuers are clipped to the arena (:239-245)
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    K = 30
    assert (obs[..., :K] >= 0).all() and (obs[..., :K] <= 0.2 + 1e-6).all()     # distances within sensor_range
    assert torch.equal(obs[..., 7 * K + 2], torch.arange(1, Np + 1, device=DEV, dtype=torch.float32).expand(N, Np))
    assert set(obs[..., 7 * K].unique().tolist()) <= {0.0, 1.0}
    assert (st["t"] == 51).all()


def test_n1_dropin_api_matches_reference_types():
    from madrl_amd.waterworld import MAWaterWorld
    env = MAWaterWorld(5, 10, obs_loc=None, device=DEV)     # the reference's own __main__ call (:483)
    assert len(env.agents) == 5 and env.agents[0].observation_space.shape == (213,)
    assert env.agents[0].action_space.shape == (2,) and env.timestep_limit == 1000 and env.reward_mech == "local"
    obs = env.reset()
    assert isinstance(obs, list) and len(obs) == 5 and obs[0].shape == (213,) and obs[0].dtype == np.float64
    obs, rew, done, info = env.step(np.random.randn(10) * .5)
    assert isinstance(rew, np.ndarray) and rew.shape == (5,) and isinstance(done, bool)
    assert set(info) == {"evcatches", "pocatches"}
    with pytest.raises(AssertionError):
        env._env.step(np.zeros(7))
