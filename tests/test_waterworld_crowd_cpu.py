"""CPU tests (-m "not gpu") of the Waterworld crowd kernel's host side (madrl_waterworld_config.crowd, csrc/waterworld_crowd.hip):
(1) the C oracle replays the reference recordings at shapes beyond one wavefront (tests/golden/wwcrowd_*.npz, recorded by
scripts/record_wwcrowd_goldens.py from the unmodified reference); (2) validation through madrl_waterworld_state_bytes, which needs no
device; (3) the built library holds the ww_crowd_kernel kernels, none with a private segment."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from oracle import waterworld as ww

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "wwcrowd_*.npz")))
gid = lambda p: os.path.basename(p)[:-4]


def test_the_three_recordings_are_there():
    assert [gid(p) for p in FILES] == ["wwcrowd_20_60_40", "wwcrowd_33_100_100", "wwcrowd_40_30_20"]


@pytest.mark.parametrize("path", FILES, ids=gid)
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 1e-5)], ids=["f64", "f32"])
def test_oracle_matches_reference_golden(path, dtype, tol):
    """as tests/test_oracle_waterworld.py does for its files: teacher-forced step by step, no step beyond the tolerance"""
    g = np.load(path)
    kw = ww.kwargs_from_golden(g)
    assert kw["n_pursuers"] + kw["n_evaders"] + kw["n_poison"] > 62 or kw["n_pursuers"] > 32   # a shape only the crowd kernel takes
    o = ww.WaterworldOracle(n_envs=1, dtype=dtype, sensors=g["sensors"], **kw)
    assert o.D == g["obs"].shape[-1]
    worst = 0.0
    for t in range(len(g["pre_t"])):
        o.set_state(pos=g["pre_pos"][t][None], vel=g["pre_vel"][t][None], obst=g["obst"][t][None], t=np.array([g["pre_t"][t]]))
        obs, rew, done, info = o.step(g["act"][t][None], resp=g["resp"][t][None])
        st = o.get_state()
        errs = [np.abs(st["pos"][0] - g["post_pos"][t]).max(), np.abs(st["vel"][0] - g["post_vel"][t]).max(), np.abs(obs[0] - g["obs"][t]).max()]
        assert int(st["t"][0]) == int(g["post_t"][t])
        if not g["is_reset_step"][t]:
            errs.append(np.abs(rew[0] - g["rew"][t]).max())
            assert int(done[0]) == int(g["done"][t])
            assert int(info[0, 0]) == int(g["evc"][t]) and int(info[0, 1]) == int(g["poc"][t])
        assert max(errs) <= tol, "step %d: %g" % (t, max(errs))
        worst = max(worst, max(errs))
    print("%s %s: worst error %.3g" % (gid(path), np.dtype(dtype).name, worst))
    assert np.nansum(g["evc"]) > 0 and np.nansum(g["poc"]) > 0   # catches of both kinds are in every recording


def _cfg(n_pursuers, n_evaders, n_poison, crowd, n_sensors=30):
    from madrl_amd import _lib
    c = _lib.WaterworldConfig()
    c.struct_size = C.sizeof(_lib.WaterworldConfig)
    c.n_pursuers, c.n_evaders, c.n_coop, c.n_poison, c.n_sensors = n_pursuers, n_evaders, 2, n_poison, n_sensors
    c.addid, c.speed_features, c.obstacle_fixed, c.crowd = 1, 1, 1, crowd
    c.radius, c.obstacle_radius, c.ev_speed, c.poison_speed, c.sensor_range, c.action_scale = 0.015, 0.2, 0.01, 0.01, 0.2, 0.01
    c.obstacle_loc[0], c.obstacle_loc[1] = 0.5, 0.5
    return c


def _state_bytes(cfg, n_envs):
    from madrl_amd import _lib
    L = _lib.lib()
    n = C.c_uint64(0)
    rc = L.madrl_waterworld_state_bytes(C.byref(cfg), n_envs, C.byref(n))
    return rc, n.value, (L.madrl_last_error() or b"").decode()


def test_validation_of_the_crowd_flag():
    n_envs = 5
    rc, _n, msg = _state_bytes(_cfg(13, 25, 25, 0), n_envs)          # 63 particles: one more than a wavefront takes
    assert rc == -1 and "62 particles" in msg, (rc, msg)
    rc, n, msg = _state_bytes(_cfg(13, 25, 25, 1), n_envs)
    assert rc == 0 and n == (4 * 63 + 4) * 4 * n_envs, (rc, n, msg)   # the record layout does not depend on the kernel
    rc, n12, _ = _state_bytes(_cfg(12, 25, 25, 0), n_envs)
    assert (rc, n12) == _state_bytes(_cfg(12, 25, 25, 1), n_envs)[:2] == (0, (4 * 62 + 4) * 4 * n_envs)
    rc, _n, msg = _state_bytes(_cfg(13, 25, 25, 2), n_envs)
    assert rc == -1 and "crowd" in msg and "0 or 1" in msg, (rc, msg)
    rc, _n, msg = _state_bytes(_cfg(13, 25, 25, -1), n_envs)
    assert rc == -1 and "crowd" in msg, (rc, msg)
    rc, _n, msg = _state_bytes(_cfg(129, 25, 25, 1), n_envs)
    assert rc == -1 and "n_pursuers" in msg and "128" in msg, (rc, msg)
    rc, _n, msg = _state_bytes(_cfg(128, 512, 384, 1), n_envs)        # 1 024 particles
    assert rc == -1 and "1023 particles" in msg, (rc, msg)
    rc, n, msg = _state_bytes(_cfg(128, 512, 383, 1), n_envs)         # the limits themselves
    assert rc == 0 and n == (4 * 1023 + 4) * 4 * n_envs, (rc, msg)
    for bad, why in ((_cfg(20, 60, 40, 1, n_sensors=257), "n_sensors"), (_cfg(20, 60, 40, 1, n_sensors=0), "n_sensors")):
        rc, _n, msg = _state_bytes(bad, n_envs)
        assert rc == -1 and why in msg, (rc, msg)
    c = _cfg(20, 60, 40, 1)
    c.n_coop = 0
    rc, _n, msg = _state_bytes(c, n_envs)
    assert rc == -1 and "n_coop" in msg, (rc, msg)
    # the refusals of the one-wavefront kernel are what they were
    rc, _n, msg = _state_bytes(_cfg(33, 5, 5, 0), n_envs)
    assert rc == -1 and "n_pursuers must be <= 32" in msg, (rc, msg)


def test_built_library_has_the_crowd_kernels_without_a_private_segment():
    from isa import built_kernels
    ks = {n: k for n, k in built_kernels().items() if "ww_crowd_kernel" in n}
    assert len(ks) >= 2 and any("ILi0E" in n for n in ks) and any("ILi1E" in n for n in ks), sorted(ks)   # reset and step
    for n, k in ks.items():
        assert "waterworld_kernel" not in n and "hostage_kernel" not in n
        assert k["scratch"] == 0, (n, k)
