"""CPU tests (-m "not gpu") of the hostage-world crowd kernel's host side (madrl_hostage_config.crowd, csrc/hostage_crowd.hip):
(1) the C oracle replays the reference recordings at shapes beyond one wavefront (tests/golden/hwcrowd_*.npz, recorded by
scripts/record_hwcrowd_goldens.py from the unmodified reference); (2) validation through madrl_hostage_state_bytes, which needs no
device; (3) the built library holds the hw_crowd_kernel kernels, none with a private segment."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from oracle import hostage as ho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "hwcrowd_*.npz")))
gid = lambda p: os.path.basename(p)[:-4]


def test_the_three_recordings_are_there():
    assert [gid(p) for p in FILES] == ["hwcrowd_20_30_40", "hwcrowd_33_10_20_local", "hwcrowd_8_64_100"]


@pytest.mark.parametrize("path", FILES, ids=gid)
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 1e-5)], ids=["f64", "f32"])
def test_oracle_matches_reference_golden(path, dtype, tol):
    """as tests/test_oracle_hostage.py does for its files: teacher-forced step by step, no step beyond the tolerance; the saved mask, the
    gate / bombed flags and t exactly, done and info on the live steps"""
    g = np.load(path)
    kw = ho.kwargs_from_golden(g)
    assert kw["n_good"] + kw["n_hostages"] + kw["n_bad"] > 61 or kw["n_good"] > 32   # a shape only the crowd kernel takes
    o = ho.HostageOracle(n_envs=1, sensors=g["sensors"], dtype=dtype, **kw)
    assert o.D == g["obs"].shape[-1]
    worst = 0.0
    for t in range(len(g["pre_t"])):
        o.set_state(**ho.golden_pre_state(g, t))
        resp = np.where(g["resp"][t] >= 0, g["resp"][t], 0.0)
        obs, rew, done, info = o.step(g["act"][t][None], resp=resp[None])
        st = o.get_state()
        errs = [np.abs(st["pos"][0] - g["post_pos"][t]).max(), np.abs(st["vel"][0] - g["post_vel"][t]).max(), np.abs(obs[0] - g["obs"][t]).max()]
        assert [(int(st["saved"][0]) >> j) & 1 for j in range(o.Nh)] == list(g["post_saved"][t]), t
        assert int(st["flags"][0]) & 3 == int(g["post_gate"][t]) | (int(g["post_bombed"][t]) << 1), t
        assert int(st["t"][0]) == int(g["post_t"][t])
        if not g["is_reset_step"][t]:
            errs.append(np.abs(rew[0] - g["rew"][t]).max())
            assert int(done[0]) == int(g["done"][t]) and list(info[0]) == list(g["info"][t]), t
        assert max(errs) <= tol, "step %d: %g" % (t, max(errs))
        worst = max(worst, max(errs))
    print("%s %s: worst error %.3g" % (gid(path), np.dtype(dtype).name, worst))
    live = g["is_reset_step"] == 0
    assert (g["resp"][..., 0] >= 0).sum() > 0 and g["info"][live][:, 0].sum() > 0   # a respawn and a save are in every recording


def _cfg(n_good, n_hostages, n_bad, crowd, n_sensors=30, n_coop_save=2):
    from madrl_amd import _lib
    c = _lib.HostageConfig()
    c.struct_size = C.sizeof(_lib.HostageConfig)
    c.n_good, c.n_hostages, c.n_bad, c.n_coop_save, c.n_coop_avoid, c.n_sensors = n_good, n_hostages, n_bad, n_coop_save, 1, n_sensors
    c.addid, c.reward_global, c.key_fixed, c.crowd = 1, 1, 0, crowd
    c.radius, c.bad_speed, c.sensor_range, c.action_scale = 0.015, 0.01, 0.2, 0.01
    c.bomb_radius, c.key_radius = 0.05, 0.0075
    return c


def _state_bytes(cfg, n_envs):
    from madrl_amd import _lib
    L = _lib.lib()
    n = C.c_uint64(0)
    rc = L.madrl_hostage_state_bytes(C.byref(cfg), n_envs, C.byref(n))
    return rc, n.value, (L.madrl_last_error() or b"").decode()


def _align4(v):
    return (v + 3) // 4 * 4


def test_validation_of_the_crowd_flag():
    from madrl_amd import _lib
    n_envs = 5
    rc, _n, msg = _state_bytes(_cfg(12, 20, 30, 0), n_envs)          # 62 particles: one more than a wavefront takes
    assert rc == -1 and "61 particles" in msg, (rc, msg)
    rc, n, msg = _state_bytes(_cfg(12, 20, 30, 1), n_envs)
    assert rc == 0 and n == _align4(4 * 62 + 9) * 4 * n_envs, (rc, n, msg)   # the record layout does not depend on the kernel
    rc, n61, _ = _state_bytes(_cfg(12, 20, 29, 0), n_envs)
    assert (rc, n61) == _state_bytes(_cfg(12, 20, 29, 1), n_envs)[:2] == (0, _align4(4 * 61 + 9) * 4 * n_envs)
    rc, _n, msg = _state_bytes(_cfg(12, 20, 30, 2), n_envs)
    assert rc == -1 and "crowd" in msg and "0 or 1" in msg, (rc, msg)
    rc, _n, msg = _state_bytes(_cfg(12, 20, 30, -1), n_envs)
    assert rc == -1 and "crowd" in msg and "0 or 1" in msg, (rc, msg)
    rc, _n, msg = _state_bytes(_cfg(129, 20, 30, 1), n_envs)
    assert rc == -1 and "n_good" in msg and "128" in msg, (rc, msg)
    rc, _n, msg = _state_bytes(_cfg(20, 65, 30, 1), n_envs)
    assert rc == -1 and "n_hostages" in msg and "64" in msg, (rc, msg)
    rc, _n, msg = _state_bytes(_cfg(128, 64, 832, 1), n_envs)         # 1 024 particles
    assert rc == -1 and "1023 particles" in msg, (rc, msg)
    rc, n, msg = _state_bytes(_cfg(128, 64, 831, 1), n_envs)          # the limits themselves
    assert rc == 0 and n == _align4(4 * 1023 + 9) * 4 * n_envs, (rc, msg)
    for bad in (_cfg(20, 30, 40, 1, n_sensors=257), _cfg(20, 30, 40, 1, n_sensors=0)):
        rc, _n, msg = _state_bytes(bad, n_envs)
        assert rc == -1 and "n_sensors" in msg, (rc, msg)
    rc, _n, msg = _state_bytes(_cfg(20, 30, 40, 1, n_coop_save=0), n_envs)
    assert rc == -1 and "n_coop_save" in msg, (rc, msg)
    # the refusals of the one-wavefront kernel are what they were
    rc, _n, msg = _state_bytes(_cfg(33, 5, 5, 0), n_envs)
    assert rc == -1 and "n_good must be <= 32" in msg, (rc, msg)
    # a caller compiled against the struct without the two trailing words passes its size: a one-wavefront env, whatever lies behind it
    old = _cfg(3, 10, 5, 1)
    old.reserved0 = 0x55555555
    old.struct_size = _lib.HostageConfig.crowd.offset
    assert old.struct_size == C.sizeof(_lib.HostageConfig) - 8
    rc, n, msg = _state_bytes(old, n_envs)
    assert rc == 0 and n == _align4(4 * 18 + 9) * 4 * n_envs, (rc, msg)
    old = _cfg(12, 20, 30, 1)                                         # ... so 62 particles are refused as before
    old.struct_size = _lib.HostageConfig.crowd.offset
    rc, _n, msg = _state_bytes(old, n_envs)
    assert rc == -1 and "61 particles" in msg, (rc, msg)
    bad = _cfg(3, 10, 5, 0)
    bad.struct_size -= 4
    rc, _n, msg = _state_bytes(bad, n_envs)
    assert rc == -1 and "struct_size" in msg, (rc, msg)


def test_built_library_has_the_crowd_kernels_without_a_private_segment():
    from isa import built_kernels
    ks = {n: k for n, k in built_kernels().items() if "hw_crowd_kernel" in n}
    assert len(ks) >= 2 and any("ILi0E" in n for n in ks) and any("ILi1E" in n for n in ks), sorted(ks)   # reset and step
    for n, k in ks.items():
        assert "hostage_kernel" not in n and "waterworld_kernel" not in n
        assert k["scratch"] == 0, (n, k)
