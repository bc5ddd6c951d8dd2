"""CPU tests (-m "not gpu"): the NumPy wrapper oracle against golden outputs of the unmodified
reference wrappers (oracle/make_golden_wrappers.py)."""
import os

import numpy as np

from oracle import wrappers_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "wrappers_replay.npz")


def test_standardized_env_oracle_matches_reference():
    g = np.load(G)
    T, P, D = g["obs"].shape
    o = wo.StdOracle((P, D), (P,), scale_reward=float(g["std_cfg_scale_reward"]), enable_obsnorm=True, enable_rewnorm=True,
                     obs_alpha=float(g["std_cfg_obs_alpha"]), rew_alpha=float(g["std_cfg_rew_alpha"]), eps=float(g["std_cfg_eps"]))
    for t in range(T):
        so = o.obs(g["obs"][t].astype(np.float64))
        assert np.abs(so - g["std_obs"][t]).max() < 1e-12
        if g["op"][t] == 1:
            assert np.abs(o.rew(g["rew"][t]) - g["std_rew"][t]).max() < 1e-12


def test_masked_statistics_helpers_are_the_oracle_under_a_full_mask_and_the_identity_under_an_empty_one():
    """masked_obs / masked_rew of tests/test_epilogue_geometry_gpu.py (the oracle, then np.where(mask, new, old) on the statistics) are
    what the GPU tests of partial resets compare the kernels with"""
    from test_epilogue_geometry_gpu import masked_obs, masked_rew
    rng = np.random.RandomState(3)
    shape = (6, 5)
    cfg = dict(scale_reward=0.7, enable_obsnorm=True, enable_rewnorm=True, obs_alpha=0.05, rew_alpha=0.05)
    plain, full, none = (wo.StdOracle(shape, shape, **cfg) for _ in range(3))
    stats = lambda o: (o.om, o.ov, o.rm, o.rv)
    for t in range(4):
        x, r = (3 * rng.randn(*shape)).astype(np.float32), rng.randn(*shape).astype(np.float32)
        if t == 0:   # something other than the initial statistics for the identity to keep
            for o in (plain, full, none):
                o.obs(x), o.rew(r)
            continue
        before = [s.copy() for s in stats(none)]
        want_o, want_r = plain.obs(x), plain.rew(r)
        assert np.array_equal(masked_obs(full, x, np.ones(shape, bool)), want_o)
        assert np.array_equal(masked_rew(full, r, np.ones(shape, bool)), want_r)
        masked_obs(none, x, np.zeros(shape, bool)), masked_rew(none, r, np.zeros(shape, bool))
        assert all(np.array_equal(a, b) for a, b in zip(stats(full), stats(plain)))
        assert all(np.array_equal(a, b) for a, b in zip(stats(none), before))
    assert not np.array_equal(plain.om, none.om) and not np.array_equal(plain.rv, none.rv)
    # a mixed mask: each element follows the one or the other
    m = rng.rand(*shape) < 0.5
    om, rv = none.om.copy(), none.rv.copy()
    ref = wo.StdOracle(shape, shape, **cfg)
    ref.om, ref.ov, ref.rm, ref.rv = (s.copy() for s in stats(none))
    ref.obs(x), ref.rew(r)
    masked_obs(none, x, m), masked_rew(none, r, m)
    assert np.array_equal(none.om, np.where(m, ref.om, om)) and np.array_equal(none.rv, np.where(m, ref.rv, rv)) and m.any() and not m.all()


def test_observation_buffer_oracle_matches_reference():
    g = np.load(G)
    T, P, D = g["obs"].shape
    b = wo.BufOracle((P, D), int(g["buf_k"]))
    for t in range(T):
        out = b.reset(g["obs"][t]) if g["op"][t] == 0 else b.step(g["obs"][t])
        assert np.array_equal(out.astype(np.float32), g["buf_obs"][t])


def test_diagnostics_oracle_matches_reference():
    g = np.load(G)
    T, P, D = g["obs"].shape
    d = wo.DiagOracle(1, P, discount=float(g["diag_discount"]), max_traj_len=int(g["diag_max_traj_len"]))
    k = 0
    for t in range(T):
        if g["op"][t] == 0:
            d.reset()
            continue
        out = d.step(g["rew"][t][None], np.array([g["done"][t]]))
        if out["finished"][0]:
            assert t == g["diag_at"][k]
            assert np.abs(out["reward"][0] - g["diag_reward"][k]).max() < 1e-12
            assert abs(out["disc"][0] - g["diag_disc"][k]) < 1e-12 and out["length"][0] == g["diag_len"][k]
            assert abs(out["reward"][0].mean() - g["diag_avg"][k]) < 1e-12
            k += 1
    assert k == len(g["diag_at"]) and k >= 5
