"""GPU tests (-m gpu) of the hostage-world crowd kernel (`crowd=True`: csrc/hostage_crowd.hip, one workgroup of several wavefronts per env,
particles looped over its threads), at shapes beyond one wavefront's worth of particles and at shapes both kernels take:
(a) teacher-forced against the reference recordings, 1e-5, and equal to the float32 oracle; (b) free-running against the float32 oracle,
identical in every bit; (c) against the one-wavefront kernel, identical in every bit; (d) contact tests at their thresholds;
(e) the rest of the env's interface, StreamSharded and RolloutCollector."""
import glob
import os
import pickle

import numpy as np
import pytest
import torch

from helpers import raw, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "hwcrowd_*.npz"))) + sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "hostage_*.npz")))
gid = lambda p: os.path.basename(p)[:-4]
STATE_KEYS = ("pos", "vel", "key", "bomb", "saved", "flags", "t", "tick")


def _mk(*args, n_envs, crowd=True, **kw):
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    return BatchedContinuousHostageWorld(*args, n_envs=n_envs, device=DEV, crowd=crowd, **kw)


def _assert_state_equal(env, orc, where):
    gst, ost = env.get_state(), orc.get_state()
    for k in STATE_KEYS:
        assert np.array_equal(raw(gst[k].cpu().numpy()), raw(ost[k])), "state %s, %s" % (k, where)


@pytest.mark.parametrize("path", FILES, ids=gid)
def test_crowd_matches_reference_golden_teacher_forced(path):
    """Protocol of test_hostage_gpu.py::test_hip_matches_reference_golden_teacher_forced (all recorded steps of a file are independent under
    teacher forcing: one batch).  Observations, rewards of the live steps and the state equal the float32 oracle in every bit; a step is
    within 1e-5 of the recording wherever that oracle is -- in the hwcrowd_ files that is every step."""
    from oracle import hostage as ho
    g = np.load(path)
    T = len(g["pre_t"])
    kw = ho.kwargs_from_golden(g)
    env = _mk(n_envs=T, **kw)
    assert env.kernel_kind == "crowd" and env.obs_dim == g["obs"].shape[-1]
    orc = ho.HostageOracle(n_envs=T, sensors=g["sensors"], dtype=np.float32, **kw)
    Nh = env.n_hostages
    saved = np.array([sum(int(b) << j for j, b in enumerate(g["pre_saved"][t])) for t in range(T)], np.uint64)
    flags = (g["pre_gate"].astype(np.uint8) | (g["pre_bombed"].astype(np.uint8) << 1) | 4).astype(np.uint8)
    for e, tick in ((env, np.arange(T, dtype=np.int32)), (orc, np.arange(T, dtype=np.uint32))):
        e.set_state(pos=g["pre_pos"], vel=g["pre_vel"], key=g["key"], bomb=g["bomb"], saved=saved, flags=flags, t=g["pre_t"].astype(np.int32), tick=tick)
    resp = np.where(g["resp"] >= 0, g["resp"], 0.0)
    obs, rew, done, info = env.step(g["act"], respawn=resp)
    oobs, orew, odone, oinfo = orc.step(g["act"], resp=resp)
    obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
    live = g["is_reset_step"] == 0
    # the kernel IS the float32 oracle (rewards of the reset records are not outputs of reset(): compared where they are)
    assert np.array_equal(obs.view(np.int32), oobs.view(np.int32)), "observations differ from the float32 oracle"
    assert np.array_equal(rew[live].view(np.int32), orew[live].view(np.int32)), "rewards differ from the float32 oracle"
    _assert_state_equal(env, orc, gid(path))
    # ... and the recording, in the reference's float64
    st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    assert np.abs(st["pos"] - g["post_pos"]).max() < 1e-6 and np.abs(st["vel"] - g["post_vel"]).max() < 1e-6
    post_saved = np.array([sum(int(b) << j for j, b in enumerate(g["post_saved"][t])) for t in range(T)], np.uint64)
    assert np.array_equal(st["saved"].view(np.uint64), post_saved) and Nh <= 64
    assert np.array_equal(st["flags"] & 3, g["post_gate"] | (g["post_bombed"] << 1))
    assert np.array_equal(st["t"], g["post_t"])
    err = np.abs(obs - g["obs"]).reshape(T, -1).max(1)
    oerr = np.abs(oobs - g["obs"]).reshape(T, -1).max(1)
    print("golden %s: worst error kernel %.3g, float32 oracle %.3g" % (gid(path), err.max(), oerr.max()))
    beyond = np.nonzero((err > TOL) & (oerr <= TOL))[0]
    assert not len(beyond), "steps beyond %.0e where the float32 oracle is within it: %s" % (TOL, beyond[:5])
    if gid(path).startswith("hwcrowd_"):
        assert err.max() <= TOL and oerr.max() <= TOL, (err.max(), oerr.max())
    assert np.abs(rew[live] - g["rew"][live]).max() < TOL
    assert np.array_equal(done.cpu().numpy()[live], g["done"][live] == 1)
    assert np.array_equal(torch.stack([info["ho_saved"], info["cr_encs"]], 1).cpu().numpy()[live], g["info"][live])


# name -> (constructor arguments, keyword arguments, envs, steps)
BEYOND = {
    # first shape beyond one wavefront
    "62_particles": ((12, 20, 30, 2, 1), dict(n_sensors=16, action_scale=0.03, bad_speed=0.03), 65, 40),
    # first rescuer count beyond 32: local rewards, fixed key, no id, odd K
    "33_rescuers_local": ((33, 5, 7, 2, 1), dict(n_sensors=7, reward_mech="local", key_loc=(0.93, 0.96), addid=False, action_scale=0.03, bad_speed=0.03), 33, 40),
    # every class one past a wavefront multiple (the hostages at their limit)
    "one_past_multiples": ((65, 64, 129, 2, 1), dict(action_scale=0.03, bad_speed=0.04), 17, 30),
    # exact multiples
    "exact_multiples": ((64, 64, 64, 1, 1), dict(n_sensors=12, sensor_range=0.3, radius=0.02, action_scale=0.03), 16, 30),
    # the limits
    "limits": ((128, 64, 831, 3, 1), dict(bad_speed=0.03), 3, 12),
    # rows too long to stage
    "long_rows": ((40, 10, 20, 2, 1), dict(n_sensors=200, sensor_range=0.5, action_scale=0.03), 16, 30),
}


def stage(st, args):
    """Random actions alone never open the gate.  From the state after the first reset (numpy, the oracle's), by env index modulo 5:
    0  all hostages but the last saved, gate open, n_coop_save rescuers on the last hostage  -> a save and an all-saved termination
    1  rescuer 0 at the key                                                                  -> the gate opens
    2  gate open, the last rescuer at the bomb                                               -> a bombing
    3  gate open, n_coop_save rescuers on hostage 0                                          -> a save
    4  as reset                                                                              -> the time limit
    -> the arguments of set_state for both sides"""
    Nr, Nh, _Nc, coop = args[:4]
    pos, saved, flags = np.array(st["pos"], np.float32, copy=True), np.array(st["saved"], np.uint64, copy=True), np.array(st["flags"], np.uint8, copy=True)
    all_h = np.uint64(2 ** Nh - 1)
    for n in range(pos.shape[0]):
        kind = n % 5
        if kind == 0:
            flags[n] |= 1
            saved[n] = all_h & ~np.uint64(1 << (Nh - 1))
            pos[n, :coop] = pos[n, Nr + Nh - 1]
        elif kind == 1:
            pos[n, 0] = st["key"][n]
        elif kind == 2:
            flags[n] |= 1
            pos[n, Nr - 1] = st["bomb"][n]
        elif kind == 3:
            flags[n] |= 1
            pos[n, :coop] = pos[n, Nr]
    return dict(pos=pos, saved=saved, flags=flags)


def free_run_oracle(case, step_env=None):
    """the float32 oracle through a case of BEYOND with auto-reset semantics (reset(mask=done) after a step); step_env(t, act, orc, odone_state)
    is the comparison hook of the GPU test.  -> counts of what occurred, from the oracle's outputs alone"""
    from oracle import hostage as ho
    args, kw, N, T = BEYOND[case]
    H = max(4, T // 3)
    orc = ho.HostageOracle(*args, n_envs=N, seed=77, env_id_base=500, max_steps=H, dtype=np.float32, **kw)
    orc.reset()
    staged = stage(orc.get_state(), args)
    orc.set_state(**staged)
    all_h = np.uint64(2 ** args[1] - 1)
    rng = np.random.RandomState(1)
    ev = dict(saves=0, criminal_hits=0, gate_openings=0, bombings=0, all_saved=0, time_limit=0)
    hook = step_env(orc, staged, H) if step_env else None
    for t in range(T):
        act = rng.uniform(-1, 1, size=(N, args[0], 2)).astype(np.float32)
        gate0 = orc.get_state()["flags"] & 1
        oobs, orew, odone, oinfo = orc.step(act)
        orew, odone, oinfo = orew.copy(), odone.copy(), oinfo.copy()
        mid = orc.get_state()
        ev["saves"] += int(oinfo[:, 0].sum()); ev["criminal_hits"] += int(oinfo[:, 1].sum())
        ev["gate_openings"] += int(((mid["flags"] & 1) & ~gate0 & 1).sum())
        d = odone != 0
        ev["bombings"] += int((d & ((mid["flags"] & 2) != 0)).sum())
        ev["all_saved"] += int((d & ((mid["saved"] & all_h) == all_h)).sum())
        ev["time_limit"] += int((d & (mid["t"] >= H) & ((mid["flags"] & 2) == 0) & ((mid["saved"] & all_h) != all_h)).sum())
        if d.any():
            orc.reset(mask=odone)
        if hook:
            hook(t, act, orew, odone, oinfo)
    return ev


@pytest.mark.parametrize("case", sorted(BEYOND))
def test_crowd_matches_f32_oracle_free_running(case):
    """nothing is ever copied across after the staging: resets, respawns, keys and bombs from Philox on both sides; every output and the
    whole state identical in every bit at every step.  From the oracle's outputs: saves, criminal hits, a gate opening, a bombing, an
    all-saved termination and a time-limit reset all occurred."""
    args, kw, N, T = BEYOND[case]

    def attach(orc, staged, H):
        env = _mk(*args, n_envs=N, seed=77, env_id_base=500, max_steps=H, auto_reset=True, **kw)
        assert env.kernel_kind == "crowd"
        orc2_obs = orc.obs.copy()   # (the oracle was reset before the staging: its reset observations)
        assert np.array_equal(env.reset().cpu().numpy().view(np.int32), orc2_obs.view(np.int32)), "reset observations"
        env.set_state(**staged)
        _assert_state_equal(env, orc, "after staging")

        def hook(t, act, orew, odone, oinfo):
            obs, rew, done, info = env.step(act)
            assert np.array_equal(done.cpu().numpy(), odone != 0), "done step %d" % t
            assert np.array_equal(info["ho_saved"].cpu().numpy(), oinfo[:, 0]), "ho_saved step %d" % t
            assert np.array_equal(info["cr_encs"].cpu().numpy(), oinfo[:, 1]), "cr_encs step %d" % t
            assert np.array_equal(rew.cpu().numpy().view(np.int32), orew.view(np.int32)), "rewards step %d" % t
            got = obs.cpu().numpy()
            assert np.array_equal(got.view(np.int32), orc.obs.view(np.int32)), "obs step %d: %g" % (t, np.abs(got - orc.obs).max())
            _assert_state_equal(env, orc, "step %d" % t)
        return hook

    ev = free_run_oracle(case, attach)
    print("%s: %s" % (case, ev))
    assert all(v > 0 for v in ev.values()), ev


SHARED = {
    "module_specialised": ((3, 10, 5, 2, 2), dict(n_sensors=30)),   # the module's own configuration: the specialised instantiation
    "generic": ((4, 6, 4, 2, 1), dict()),
    "61_particles": ((12, 24, 25, 2, 1), dict(n_sensors=16)),
    "smallest": ((1, 1, 1, 1, 1), dict(n_sensors=1)),
}


@pytest.mark.parametrize("case", sorted(SHARED))
def test_crowd_equals_the_one_wavefront_kernel(case):
    """a shape both kernels run: 40 free-running steps from the same seed, everything equal in every bit"""
    args, kw = SHARED[case]
    N = 65
    kw = dict(kw, seed=5, env_id_base=9, max_steps=15, auto_reset=True, action_scale=0.03, bad_speed=0.03)
    a, b = _mk(*args, n_envs=N, crowd=True, **kw), _mk(*args, n_envs=N, crowd=False, **kw)
    assert (a.kernel_kind, b.kernel_kind) == ("crowd", "wave")
    assert same_bits(a.reset(), b.reset())
    g = torch.Generator(device="cpu").manual_seed(3)
    for t in range(40):
        act = (torch.rand((N, args[0], 2), generator=g) * 2 - 1).to(DEV)
        oa, ra, da, ia = a.step(act)
        ob, rb, db, ib = b.step(act)
        assert same_bits(oa, ob), "obs step %d" % t
        assert same_bits(ra, rb) and torch.equal(da, db), "rewards / done step %d" % t
        assert torch.equal(ia["ho_saved"], ib["ho_saved"]) and torch.equal(ia["cr_encs"], ib["cr_encs"]), "info step %d" % t
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert same_bits(sa[k], sb[k]), "state %s step %d" % (k, t)


def test_contact_tests_at_the_threshold_match_the_sqrt_formulation():
    """test_hostage_gpu.py's construction at 64 particles, with a hostage added: the kernel tests dx*dx + dy*dy <= sq_threshold(thr) where the
    reference and the float32 oracle test sqrt(...) <= thr.  A criminal at 2 radius of rescuer 0, the bomb and the key at their radii of
    rescuers 1 and 2, a hostage at radius + 2 radius of rescuer 3, within +-8 ulps of the threshold along 256 directions (the rescuers
    inside the closed gate's square, so that they stay where they are put): every output equals the oracle's, and both outcomes occur."""
    from oracle import hostage as ho
    N = 17 * 256
    Nr, Nh, Nc = 4, 10, 50
    kw = dict(reward_mech="local", max_steps=1000)
    env = _mk(Nr, Nh, Nc, 1, 1, n_envs=N, seed=2, auto_reset=False, **kw)
    orc = ho.HostageOracle(Nr, Nh, Nc, 1, 1, n_envs=N, seed=2, dtype=np.float32, **kw)
    assert env.kernel_kind == "crowd"
    env.reset(); orc.reset()
    st = orc.get_state()
    radius = np.float32(env.radius)
    k = np.repeat(np.arange(-8, 9), 256).astype(np.int32)
    th = np.tile(np.arange(256) * (2 * np.pi / 256) + 0.001, 17)

    def at_distance(center, thr):
        d = (np.full(N, thr, np.float32).view(np.int32) + k).view(np.float32)
        return np.stack([center[:, 0] + d * np.cos(th).astype(np.float32), center[:, 1] + d * np.sin(th).astype(np.float32)], -1).astype(np.float32)
    pos = np.array(st["pos"], np.float32, copy=True)
    vel = np.zeros_like(pos)
    pos[:, 0] = (0.60, 0.60); pos[:, 1] = (0.60, 0.75); pos[:, 2] = (0.75, 0.90); pos[:, 3] = (0.85, 0.60)
    pos[:, Nr:Nr + Nh] = np.stack([np.full(Nh, 0.97, np.float32), np.linspace(0.05, 0.45, Nh).astype(np.float32)], -1)[None]      # hostages parked
    pos[:, Nr + Nh:] = np.stack([np.full(Nc, 0.05, np.float32), np.linspace(0.05, 0.95, Nc).astype(np.float32)], -1)[None]        # criminals parked
    pos[:, Nr + Nh] = at_distance(pos[:, 0], radius + radius)                          # criminal 0 at contact distance of rescuer 0
    bomb = at_distance(pos[:, 1], radius + np.float32(env.bomb_radius))                # bomb at its radius of rescuer 1
    key = at_distance(pos[:, 2], radius + np.float32(env.key_radius))                  # key at its radius of rescuer 2
    pos[:, Nr] = at_distance(pos[:, 3], radius + np.float32(env.radius * 2))           # hostage 0 at contact distance of rescuer 3
    for e, tick in ((env, st["tick"].astype(np.int32)), (orc, st["tick"])):
        e.set_state(pos=pos, vel=vel, key=key, bomb=bomb, saved=st["saved"], flags=st["flags"], t=st["t"], tick=tick)
    act = np.zeros((N, Nr, 2), np.float32)
    obs, rew, done, info = env.step(act)
    oobs, orew, odone, oinfo = orc.step(act)
    assert np.array_equal(obs.cpu().numpy().view(np.int32), oobs.view(np.int32)) and np.array_equal(rew.cpu().numpy().view(np.int32), orew.view(np.int32))
    assert np.array_equal(done.cpu().numpy(), odone != 0)
    assert np.array_equal(info["cr_encs"].cpu().numpy(), oinfo[:, 1]) and 0 < oinfo[:, 1].sum() < N
    assert np.array_equal(info["ho_saved"].cpu().numpy(), oinfo[:, 0]) and 0 < oinfo[:, 0].sum() < N
    _assert_state_equal(env, orc, "after the step")
    fl = orc.get_state()["flags"]
    assert 0 < (fl & 1).sum() < N and 0 < ((fl >> 1) & 1).sum() < N    # key and bomb reached in some envs and not in others


def test_crowd_env_interface():
    """kernel_kind, the constructor arguments it pickles by, mask reset, set_state / get_state round trip, step(obs_out=) into a second tensor"""
    from oracle import hostage as ho
    args, kw, N, _T = BEYOND["62_particles"]
    Nr, NP = args[0], sum(args[:3])
    env = _mk(*args, n_envs=N, seed=3, max_steps=1000, **kw)
    orc = ho.HostageOracle(*args, n_envs=N, seed=3, max_steps=1000, dtype=np.float32, **kw)
    assert env.kernel_kind == "crowd" and env._ctor["crowd"] is True
    small = _mk(3, 4, 2, 1, 1, n_envs=2, crowd=False)
    assert small.kernel_kind == "wave" and "crowd" not in small._ctor      # pickles of the envs that existed before stay what they were
    assert pickle.loads(pickle.dumps(env)).kernel_kind == "crowd" and pickle.loads(pickle.dumps(small)).kernel_kind == "wave"
    assert np.array_equal(env.reset().cpu().numpy(), orc.reset())
    rng = np.random.RandomState(0)
    act = rng.uniform(-1, 1, (N, Nr, 2)).astype(np.float32)
    # step into a second tensor: the env's own buffer keeps what it held
    own = env._obs.clone()
    dst = torch.full((N * Nr * env.obs_dim,), 7.0, device=DEV)
    obs, rew, done, info = env.step(act, obs_out=dst)
    oobs, orew, _od, _oi = orc.step(act)
    assert obs.data_ptr() == dst.data_ptr() and torch.equal(env._obs, own)
    assert np.array_equal(obs.cpu().numpy(), oobs) and np.array_equal(rew.cpu().numpy(), orew)
    # mask reset: the envs outside the mask keep state and observations
    before, st0 = env.step(act)[0].clone(), env.get_state()
    orc.step(act)
    m = np.zeros(N, np.uint8); m[::3] = 1
    got = env.reset(mask=m).cpu().numpy()
    want = orc.reset(mask=m)
    keep = m == 0
    assert np.array_equal(got[m == 1], want[m == 1]) and np.array_equal(got[keep], before.cpu().numpy()[keep])
    st1 = env.get_state()
    assert torch.equal(st1["pos"][torch.as_tensor(keep)], st0["pos"][torch.as_tensor(keep)]) and (st1["t"].cpu().numpy()[m == 1] == 1).all()
    _assert_state_equal(env, orc, "after the mask reset")
    # set_state / get_state round trip through the record the crowd kernel reads
    pos = rng.uniform(0, 1, (N, NP, 2)).astype(np.float32); vel = rng.uniform(-.01, .01, (N, NP, 2)).astype(np.float32)
    key = rng.uniform(0.9, 1.0, (N, 2)).astype(np.float32); bomb = rng.uniform(0, 0.25, (N, 2)).astype(np.float32)
    saved = rng.randint(0, 2 ** 20, N).astype(np.uint64); flags = (rng.randint(0, 2, N) | 4).astype(np.uint8)
    t = rng.randint(0, 50, N).astype(np.int32); tick = rng.randint(0, 1000, N).astype(np.int32)
    env.set_state(pos=pos, vel=vel, key=key, bomb=bomb, saved=saved, flags=flags, t=t, tick=tick)
    orc.set_state(pos=pos, vel=vel, key=key, bomb=bomb, saved=saved, flags=flags, t=t, tick=tick.view(np.uint32))
    st = env.get_state()
    for k, v in (("pos", pos), ("vel", vel), ("key", key), ("bomb", bomb), ("saved", saved), ("flags", flags), ("t", t), ("tick", tick)):
        assert np.array_equal(raw(st[k].cpu().numpy()), raw(v)), k
    obs, rew, done, info = env.step(act)
    oobs, orew, odone, oinfo = orc.step(act)
    assert np.array_equal(obs.cpu().numpy(), oobs) and np.array_equal(rew.cpu().numpy(), orew) and np.array_equal(done.cpu().numpy(), odone != 0)
    assert np.array_equal(env.get_state()["t"].cpu().numpy(), t + 1) and np.array_equal(info["cr_encs"].cpu().numpy(), oinfo[:, 1])
    _assert_state_equal(env, orc, "after the step from the set state")


def test_terminal_and_gate_properties_at_64_hostages():
    """the saved mask of 64 hostages fills the int64 the state holds it in: "all saved" is the value with the sign bit set"""
    N = 4
    env = _mk(2, 64, 3, 1, 1, n_envs=N, seed=1, max_steps=1000)
    env.reset()
    st = env.get_state()
    full = np.uint64(2 ** 64 - 1)
    saved = np.array([0, full, full & ~np.uint64(1 << 63), np.uint64(1 << 63)], np.uint64)
    flags = np.array([4, 4, 5, 4], np.uint8)
    env.set_state(saved=saved, flags=flags)
    assert env.is_terminal.cpu().tolist() == [False, True, False, False]
    assert env.is_gate_open.cpu().tolist() == [False, False, True, False]
    assert np.array_equal(env.get_state()["saved"].cpu().numpy().view(np.uint64), saved)
    # the kernel agrees: a step of env 1 is done, one of env 2 is not
    _obs, _rew, done, _info = env.step(np.zeros((N, 2, 2), np.float32))
    assert bool(done[1]) and not bool(done[0]) and not bool(done[3])
    assert torch.equal(st["key"], env.get_state()["key"])
    low = _mk(2, 5, 3, 1, 1, n_envs=2, seed=1, max_steps=1000)   # below 64 the comparison is what it was
    low.reset()
    low.set_state(saved=np.array([31, 15], np.uint64))
    assert low.is_terminal.cpu().tolist() == [True, False]


def test_single_env_dropin_with_crowd():
    from madrl_amd.hostage import ContinuousHostageWorld
    env = ContinuousHostageWorld(12, 20, 30, 2, 1, n_sensors=16, device=DEV, crowd=True)
    assert env._env.kernel_kind == "crowd" and env._env.n_envs == 1
    obs = env.reset()
    D = 16 * 5 + 6
    assert len(obs) == 12 and obs[0].shape == (D,) and obs[0].dtype == np.float64 and env.agents[0].observation_space.shape == (D,)
    obs, rew, done, info = env.step(np.zeros(24))
    assert rew.shape == (12,) and isinstance(done, bool) and set(info) == {"ho_saved", "cr_encs"}
    assert env.is_gate_open in (False, True) and env.is_terminal in (False, True)


def test_stream_sharded_halves_equal_the_whole_batch():
    from madrl_amd.sharded import StreamSharded
    args, kw, _N, _T = BEYOND["62_particles"]
    N = 32
    mk = lambda n_envs, env_id_base, device: _mk(*args, n_envs=n_envs, env_id_base=env_id_base, seed=5, max_steps=9, auto_reset=True, **kw)
    full = mk(N, 40, DEV)
    sh = StreamSharded(mk, N, n_streams=2, env_id_base=40, device=DEV)
    assert [e.kernel_kind for e in sh.envs] == ["crowd", "crowd"]
    assert same_bits(full.reset(), torch.cat(sh.reset()))
    g = torch.Generator(device="cpu").manual_seed(1)
    dones = 0
    for t in range(20):
        a = (torch.rand((N, args[0], 2), generator=g) * 2 - 1).to(DEV)
        o, r, d, _ = full.step(a)
        parts = sh.step(a)
        assert same_bits(o, torch.cat([p[0] for p in parts])), t
        assert same_bits(r, torch.cat([p[1] for p in parts])) and torch.equal(d, torch.cat([p[2] for p in parts])), t
        dones += int(d.sum())
    assert dones >= N


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_rollout_collector_over_a_crowd_env(graph):
    """the step kernel writes the observation slots of the trajectory itself: they equal the observations of an eager loop"""
    from madrl_amd.rollout import RolloutCollector
    args, kw, N, _T = BEYOND["33_rescuers_local"]
    H = 8
    mk = lambda: _mk(*args, n_envs=N, seed=4, max_steps=5, auto_reset=True, **kw)
    # a fixed function of the observation: towards / away from what the first sensors see
    policy = lambda obs: torch.tanh(torch.stack([obs[..., :7].sum(-1) * 20.0 - 0.3, obs[..., 21:28].sum(-1) * 20.0 + 0.2], -1))
    col = RolloutCollector(mk(), policy, horizon=H, store_observations=True, graph=graph)
    assert col._slots
    env = mk()
    obs = env.reset()
    for it in range(3):   # (graph: call 1 eager, call 2 captures and replays, call 3 replays)
        traj = col.collect()
        torch.cuda.synchronize()
        for t in range(H):
            assert same_bits(traj.observations[t], obs), (it, t)
            act = policy(obs)
            assert same_bits(traj.actions[t], act), (it, t)
            obs, rew, done, _info = env.step(act)
            assert same_bits(traj.rewards[t], rew) and torch.equal(traj.dones[t] != 0, done), (it, t)
        assert same_bits(traj.last_observation, obs), it
    assert int((traj.dones != 0).sum()) >= N   # max_steps=5: episodes ended and restarted inside the horizon
