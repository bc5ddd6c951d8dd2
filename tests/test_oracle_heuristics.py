"""CPU tests (-m "not gpu"): the NumPy policy oracle against golden outputs of the unmodified reference policies."""
import os

import numpy as np

from oracle import heuristics_oracle as ho

G = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "heuristics.npz"))


def test_pursuit_policy_oracle():
    for R in (7, 5, 11):
        a = ho.pursuit_actions(G["pursuit_R%d_obs" % R])
        assert np.array_equal(a, G["pursuit_R%d_act" % R]), R
        assert (a == -1).sum() > 50 and len(np.unique(a)) == 6


def test_waterworld_policy_oracle():
    a = ho.waterworld_actions(G["waterworld_obs"])
    assert np.abs(a - G["waterworld_act"]).max() < 1e-12
    assert np.abs(a[-50:]).max() == 0.0


def test_multiwalker_policy_oracle():
    a = ho.multiwalker_actions(G["multiwalker_obs"])
    assert np.abs(a - G["multiwalker_act"]).max() < 1e-12


# ---- heuristics_edges.npz (oracle/make_golden_heuristics.py edges()): window sizes 1 ... 21 with every pair of evader cells up to 9,
# sensor counts 1 ... 33, the MultiWalker thresholds at their float32 neighbours
E = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heuristics_edges.npz"))
EDGE_R = (1, 2, 3, 4, 8, 9, 21)
EDGE_K = (1, 3, 7, 8, 9, 33)


def test_pursuit_policy_oracle_edge_windows():
    for R in EDGE_R:
        ev, ref = E["pursuit_R%d_ev" % R], E["pursuit_R%d_act" % R]
        n_pairs = R * R * (R * R - 1) // 2 if R <= 9 else 0
        assert len(ev) == R * R + 200 + n_pairs and ev.shape[1:] == (R, R)
        a = ho.pursuit_actions(ho.pursuit_edge_windows(ev, 1000 + R))
        assert np.array_equal(a, ref), R
        assert np.array_equal(ref == -1, ev.reshape(len(ev), -1).sum(axis=1) == 0), R    # the reference samples on empty windows only
        assert (ref == -1).sum() > 10
        assert set(np.unique(ref)) == ({-1, 4} if R == 1 else {-1, 0, 3, 4} if R == 2 else {-1, 0, 1, 2, 3, 4}), R


def test_waterworld_policy_oracle_edge_sensor_counts():
    for K in EDGE_K:
        obs, ref = E["waterworld_K%d_obs" % K], E["waterworld_K%d_act" % K]
        assert obs.shape == (120, 7 * K + 3)
        assert sorted(set(zip(obs[:110, 7 * K], obs[:110, 7 * K + 1]))) == [(0, 0), (0, 1), (1, 0), (1, 1)]
        a = ho.waterworld_actions(obs)
        assert np.abs(a - ref).max() < 1e-12, K
        assert not obs[-10:].any() and not a[-10:].any() and not np.signbit(a[-10:]).any()
        n = np.sqrt((ho.waterworld_raw(obs) ** 2).sum(axis=1))
        assert np.abs(np.sqrt((a[:110] ** 2).sum(axis=1)) - 1).max() < 1e-12 and n[:110].min() > 1e-4, K


def test_multiwalker_policy_oracle_thresholds():
    for key, D in (("multiwalker", 32), ("multiwalker71", 71)):
        obs, ref = E[key + "_obs"], E[key + "_act"]
        assert obs.shape == (400, D)
        a = ho.multiwalker_actions(obs)
        assert np.array_equal(np.isnan(a), np.isnan(ref))
        assert np.nanmax(np.abs(a - ref)) < 1e-12
        assert np.isnan(ref).any(axis=1).sum() == 16            # the sixteen rows with a NaN in a column that reaches an action
        assert np.isnan(obs[:, 8]).sum() > 80 and not np.isnan(ref[np.isnan(obs[:, 8]) & ~np.isnan(np.delete(obs, 8, axis=1)).any(axis=1)]).any()
    assert np.array_equal(E["multiwalker71_obs"][:, :32].view(np.int32), E["multiwalker_obs"].view(np.int32))
    assert np.array_equal(E["multiwalker71_act"].view(np.int64), E["multiwalker_act"].view(np.int64))
    o = E["multiwalker_obs"]
    for col, v in ((2, 0.29), (9, 0.10)):                       # float32(v) and both neighbours, on both sides of the float64 threshold
        assert len(np.unique(o[:, col])) == 3 and (o[:, col].astype(np.float64) > v).any() and (o[:, col].astype(np.float64) < v).any()
    assert np.signbit(o[o[:, 8] == 0, 8]).any() and np.signbit(o[o[:, 6] == 0, 6]).any()   # -0.0 is there


def _nearest_cell_key(R):
    """(d^2, row-major index) of every window cell as the one integer the kernels minimise"""
    i, j = np.divmod(np.arange(R * R), R)
    return ((i - R // 2) ** 2 + (j - R // 2) ** 2) * 65536 + np.arange(R * R)


def test_pursuit_decision_table_is_the_argmin_over_sqrt_distances():
    """For every pair of evader cells the reference's action (argmin over float64 sqrt distances, first minimum in row-major order,
    then the atan2 quadrants) is table[the cell with the smaller (d^2, index) key]: exhaustive up to R = 9, 5 000 drawn pairs above."""
    from madrl_amd.heuristics import pursuit_decision_table
    rng = np.random.RandomState(3)
    for R in list(range(1, 22)) + [255]:
        cells = R * R
        table = pursuit_decision_table(R)
        assert table.shape == (cells,) and table.dtype == np.uint8 and table.max() <= 4     # no 255: every cell has an action
        key = _nearest_cell_key(R)
        assert key.max() < 2 ** 32 and cells - 1 < 65536 and len(np.unique(key)) == cells
        if R <= 9:
            a, b = np.triu_indices(cells, 1)
        else:
            a, b = rng.randint(cells, size=(2, 5000))
            a, b = a[a != b], b[a != b]
        if R <= 21:
            assert np.array_equal(_actions_of_evader_channel(np.eye(cells, dtype=np.uint8), R), table), R   # one evader: the table itself
        for s in range(0, len(a), 500):                                                     # (R = 255: 65 025 cells per window)
            ev = np.zeros((len(a[s:s + 500]), cells), np.uint8)
            ev[np.arange(len(ev)), a[s:s + 500]] = 1
            ev[np.arange(len(ev)), b[s:s + 500]] = 2
            want = table[np.where(key[a] < key[b], a, b)[s:s + 500]]
            assert np.array_equal(_actions_of_evader_channel(ev, R), want), R


def _actions_of_evader_channel(ev, R):
    """ho.pursuit_actions of windows whose evader channel is ev [B, R * R] (the other channels repeat it: the policy reads channel 2 only)"""
    return ho.pursuit_actions(np.broadcast_to(ev.reshape(len(ev), R, R, 1), (len(ev), R, R, 3)))
