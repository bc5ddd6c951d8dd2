"""CPU tests (-m "not gpu") of per-pursuer sensor ranges in Waterworld (madrl_waterworld_set_sensor_ranges; waterworld_kernel_ranges,
csrc/waterworld.hip, and ww_crowd_kernel_ranges, csrc/waterworld_crowd.hip): the built library holds the ranged entries of both kernel
families, the C function is declared and known to the ctypes layer, the constructor refuses what is out of scope before it touches a
device -- and the recordings tests/golden/wwrange_*.npz (scripts/make_golden_waterworld_ranges.py: the unmodified reference with an array
sensor_range) discriminate and obey the principle the GPU tests stand on: row i of an array run is row i of a uniform run at ranges[i]."""
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "wwrange_*.npz")))
gid = lambda p: os.path.basename(p)[:-4]
TOL = 1e-12   # the float64 oracle against the reference: the tolerance tests/test_oracle_waterworld.py holds every waterworld_*.npz to


def test_built_library_has_the_ranged_kernels_without_a_private_segment():
    from isa import built_kernels
    ks = built_kernels()
    for family in ("waterworld_kernel_ranges", "ww_crowd_kernel_ranges"):
        ranged = {n: k for n, k in ks.items() if family in n}
        assert len(ranged) >= 2 and any("rangesILi0E" in n for n in ranged) and any("rangesILi1E" in n for n in ranged), (family, sorted(ranged))   # reset and step
        for n, k in ranged.items():
            assert k["scratch"] == 0 and k["vgpr_spills"] == 0, (n, k)
            assert len(k["args"]) == 2, (n, k["args"])   # (WwDev, WwIO): the ranges lie behind the sensor table
    assert sum("waterworld_kernel_ranges" in n for n in ks) == 2   # one generic body, no specialised ranged instantiations


def test_set_sensor_ranges_is_declared_and_exported():
    from madrl_amd import _lib
    header = open(os.path.join(ROOT, "include", "madrl_hip.h")).read()
    assert re.search(r"int madrl_waterworld_set_sensor_ranges\(madrl_waterworld \*h, const double \*ranges_host\);", header)
    assert re.search(r"#define MADRL_ABI_VERSION 8\b", header)
    assert len(_lib.SIGNATURES["madrl_waterworld_set_sensor_ranges"][1]) == 2
    fn = _lib.lib().madrl_waterworld_set_sensor_ranges
    assert len(fn.argtypes) == 2
    assert fn(None, None) == -1 and b"NULL" in _lib.lib().madrl_last_error()   # no handle: refused before anything is touched


def test_constructor_refuses_before_a_device_is_touched():
    from madrl_amd.waterworld import BatchedMAWaterWorld, MAWaterWorld
    nodev = "cuda:99"   # never reached
    r3 = np.array([0.2, 0.1, 0.3])
    with pytest.raises(ValueError, match="per_env_counts"):
        BatchedMAWaterWorld(3, 4, n_envs=2, device=nodev, sensor_range=r3, per_env_counts="wave")
    with pytest.raises(ValueError, match="per_env_counts"):
        BatchedMAWaterWorld(3, 4, n_envs=2, device=nodev, sensor_range=r3, crowd=True, per_env_counts=True)
    for bad in (np.nan, np.inf, 0.0, -0.1):
        with pytest.raises(ValueError, match="finite and > 0"):
            BatchedMAWaterWorld(3, 4, n_envs=2, device=nodev, sensor_range=np.array([0.2, bad, 0.3]))
        with pytest.raises(ValueError, match="finite and > 0"):
            BatchedMAWaterWorld(3, 4, n_envs=2, device=nodev, crowd=True, sensor_range=[0.2, 0.3, bad])
    with pytest.raises(ValueError, match="finite and > 0"):   # the drop-in passes the array through
        MAWaterWorld(3, 4, device=nodev, sensor_range=np.array([0.2, -1.0, 0.3]))
    with pytest.raises(ValueError):   # a length other than n_pursuers: numpy's own broadcast error, as in the reference
        BatchedMAWaterWorld(3, 4, n_envs=2, device=nodev, sensor_range=np.array([0.2, 0.1]))


@pytest.mark.parametrize("path", FILES, ids=gid)
def test_recordings_carry_the_ranges(path):
    g = np.load(path)
    r = g["cfg_sensor_ranges"]
    assert r.dtype == np.float64 and r.shape == (int(g["cfg_n_pursuers"]),)
    assert len(np.unique(r)) >= 2 and float(g["cfg_sensor_range"]) == r[0]


def test_the_two_recordings_are_there():
    assert [gid(p) for p in FILES] == ["wwrange_33_12_8_k8", "wwrange_4_8_6_k12"]


def _oracle_run(g, sensor_range):
    """the float64 oracle at one uniform range, teacher-forced over every recorded step -> obs [T][Np][D], and the worst error of
    post-state and rewards (which the range does not enter)"""
    from oracle import waterworld as ww
    kw = dict(ww.kwargs_from_golden(g), sensor_range=float(sensor_range))
    T = len(g["pre_t"])
    o = ww.WaterworldOracle(n_envs=T, dtype=np.float64, sensors=g["sensors"], **kw)   # the steps are independent: one batch
    assert o.D == g["obs"].shape[-1]
    o.set_state(pos=g["pre_pos"], vel=g["pre_vel"], obst=g["obst"], t=g["pre_t"])
    obs, rew, done, info = o.step(g["act"], resp=g["resp"])
    st = o.get_state()
    live = g["is_reset_step"] == 0
    err = max(np.abs(st["pos"] - g["post_pos"]).max(), np.abs(st["vel"] - g["post_vel"]).max(), np.abs(rew[live] - g["rew"][live]).max())
    assert np.array_equal(st["t"], g["post_t"]) and np.array_equal(done[live], g["done"][live])
    assert np.array_equal(info[live, 0], g["evc"][live].astype(np.int64)) and np.array_equal(info[live, 1], g["poc"][live].astype(np.int64))
    return obs.copy(), err


@pytest.mark.parametrize("path", FILES, ids=gid)
def test_recordings_discriminate_and_rows_are_those_of_uniform_runs(path):
    g = np.load(path)
    ranges = g["cfg_sensor_ranges"]
    T = len(g["pre_t"])
    runs = {}
    for r in np.unique(ranges):
        obs, err = _oracle_run(g, r)
        runs[float(r)] = obs
        assert err <= TOL, "post-state / rewards at range %g: %g" % (r, err)
        rows = np.flatnonzero(ranges == r)
        e = np.abs(obs[:, rows] - g["obs"][:, rows]).max()
        print("%s range %g: rows %s, worst |obs - recording| %.3g" % (gid(path), r, rows.tolist(), e))
        assert e <= TOL, "rows of the pursuers with range %g: %g" % (r, e)
    # what the code computed before: every pursuer at ranges[0]
    first = runs[float(ranges[0])]
    for i in np.flatnonzero(ranges != ranges[0]):
        off = (np.abs(first[:, i] - g["obs"][:, i]).max(axis=-1) > 1e-5).sum()
        print("%s pursuer %d (range %g): off at ranges[0] on %d of %d steps" % (gid(path), i, ranges[i], off, T))
        assert 4 * off >= T, "pursuer %d: %d of %d steps" % (i, off, T)
