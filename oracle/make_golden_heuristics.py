#!/usr/bin/env python
"""Golden vectors for the hand-written policies: the UNMODIFIED reference classes
heuristics/pursuit.py:13-56, heuristics/waterworld.py:6-62, heuristics/multi_walker.py:10-86 evaluated on
recorded / synthetic observations.  TEST INFRASTRUCTURE ONLY.

The reference is Python 2 code (`xrange`, integer `/` in `x, y = xs / 2, ys / 2`, heuristics/pursuit.py:23).  It runs here
under Python 3 with the Python 2 meaning restored from the outside: `xrange` is injected into the module globals and the
observation is handed over as an ndarray subclass whose `.shape` entries divide like Python 2 ints."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(os.environ.get("MADRL_GOLDEN_OUT") or os.path.join(os.path.dirname(HERE), "tests", "golden"))


class Py2Int(int):
    def __truediv__(self, o):
        return Py2Int(int(self) // int(o)) if isinstance(o, int) else int(self) / o


class Py2Array(np.ndarray):
    @property
    def shape(self):
        return tuple(Py2Int(v) for v in np.ndarray.shape.__get__(self))


class FixedSpace(object):
    """action_space whose sample() flags the call (the kernels draw from Philox there)"""

    def sample(self):
        return -1


def main():
    ref_loader.load()
    hp = importlib.import_module("heuristics.pursuit")
    hw = importlib.import_module("heuristics.waterworld")
    hm = importlib.import_module("heuristics.multi_walker")
    hm.xrange = range
    rng = np.random.RandomState(7)
    out = {}
    # ---- pursuit: windows (R, R, 4) channel-last like PursuitEvade(flatten=False) hands them out
    for R in (7, 5, 11):
        wins = []
        for i in range(R):           # every single-evader position
            for j in range(R):
                w = np.zeros((R, R, 4)); w[i, j, 2] = 0.1; wins.append(w)
        for _ in range(600):         # sparse random windows, several evaders (ties included), some empty
            w = np.zeros((R, R, 4))
            k = rng.randint(0, 5)
            for _ in range(k):
                w[rng.randint(R), rng.randint(R), 2] += 0.1
            w[..., 1] = (rng.rand(R, R) < 0.1) * 0.1
            w[..., 0] = (rng.rand(R, R) < 0.1) * 0.1
            wins.append(w)
        wins = np.asarray(wins)
        pol = hp.PursuitHeuristicPolicy(None, FixedSpace())
        acts = np.array([pol.sample_actions(w.view(Py2Array))[0] for w in wins], dtype=np.int32)
        out["pursuit_R%d_obs" % R] = wins.astype(np.float32)
        out["pursuit_R%d_act" % R] = acts      # -1: the reference sampled a random action
    # ---- waterworld: recorded observations of the reference env, one agent row at a time (B = 1)
    g = np.load(os.path.join(OUT, "waterworld_c3_catches.npz"))
    obs = g["obs"].reshape(-1, g["obs"].shape[-1])[:1500]
    extra = obs[:50].copy(); extra[:, :] = 0.0   # all-zero sensors: zero action
    obs = np.concatenate([obs, extra])
    pol = hw.WaterworldHeuristicPolicy(None, None)
    out["waterworld_obs"] = obs.astype(np.float32)
    out["waterworld_act"] = np.concatenate([pol.sample_actions(o.astype(np.float32).astype(np.float64)[None])[0] for o in obs])
    # ---- multiwalker: the policy is a pure function of the 32-vector; synthetic vectors around its thresholds
    obs = rng.uniform(-1.2, 1.2, size=(3000, 32))
    obs[:, 8] = rng.rand(3000) < 0.5; obs[:, 13] = rng.rand(3000) < 0.5
    obs[:500, 2] = rng.uniform(0.2, 0.4, 500)      # around SPEED
    obs[500:1000, 9] = rng.uniform(0.0, 0.2, 500)  # supporting leg behind threshold
    obs[1000:1500, 11] = rng.uniform(0.8, 0.95, 500)
    obs = obs.astype(np.float32)
    pol = hm.MultiWalkerHeuristicPolicy(None, None)
    out["multiwalker_obs"] = obs
    out["multiwalker_act"] = pol.sample_actions(obs.astype(np.float64))[0]
    path = os.path.join(OUT, "heuristics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KB", {k: v.shape for k, v in out.items()})
    a = out["pursuit_R7_act"]
    print("pursuit R7 action histogram (-1 = random):", {int(k): int((a == k).sum()) for k in np.unique(a)})


EDGE_R = (1, 2, 3, 4, 8, 9, 21)
EDGE_K = (1, 3, 7, 8, 9, 33)


def f32_neighbours(v):
    """float32(v) between its two float32 neighbours"""
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def edges():
    """heuristics_edges.npz: the sizes and values heuristics.npz leaves out -- window sizes 1 ... 21 with every tie placed on purpose,
    sensor counts around the policy kernel's eight lanes, the MultiWalker thresholds at their float32 neighbours.  An RNG stream of its
    own, so heuristics.npz does not change."""
    from oracle import heuristics_oracle as ho
    ref_loader.load()
    hp = importlib.import_module("heuristics.pursuit")
    hw = importlib.import_module("heuristics.waterworld")
    hm = importlib.import_module("heuristics.multi_walker")
    hm.xrange = range
    rng = np.random.RandomState(2016)
    out = {}
    # ---- pursuit: the evader channel alone is stored (counts, uint8); ho.pursuit_edge_windows adds the other channels from a seed
    for R in EDGE_R:
        evs = []
        for c in range(R * R):                   # every single-evader position
            e = np.zeros(R * R, np.uint8); e[c] = 1; evs.append(e)
        for _ in range(200):                     # sparse random windows, some empty
            e = np.zeros(R * R, np.uint8)
            for _ in range(rng.randint(0, 5)):
                e[rng.randint(R * R)] += 1
            evs.append(e)
        if R <= 9:                               # every unordered pair of cells, different counts in the two: explicit ties and near-ties
            for a in range(R * R):
                for b in range(a + 1, R * R):
                    e = np.zeros(R * R, np.uint8); e[a], e[b] = (1, 2) if (a + b) % 2 else (2, 1); evs.append(e)
        ev = np.asarray(evs).reshape(-1, R, R)
        wins = ho.pursuit_edge_windows(ev, 1000 + R)
        pol = hp.PursuitHeuristicPolicy(None, FixedSpace())
        out["pursuit_R%d_ev" % R] = ev
        out["pursuit_R%d_act" % R] = np.array([pol.sample_actions(w.astype(np.float64).view(Py2Array))[0] for w in wins], dtype=np.int8)
    # ---- waterworld: rand rows, the two collision flags cycling over their four combinations, the last ten rows all zero
    pol = hw.WaterworldHeuristicPolicy(None, None)
    for K in EDGE_K:
        obs = rng.rand(120, 7 * K + 3).astype(np.float32)
        obs[:, 7 * K] = np.arange(120) % 2
        obs[:, 7 * K + 1] = (np.arange(120) // 2) % 2
        obs[-10:] = 0.0
        out["waterworld_K%d_obs" % K] = obs
        out["waterworld_K%d_act" % K] = np.concatenate([pol.sample_actions(o.astype(np.float64)[None])[0] for o in obs])
    # ---- multiwalker: 400 rows at the thresholds.  2 x (3 x 3 x 4 x 5) products of
    # s[2] around SPEED, s[9] around 0.10, the contact flag s[8], the knee angle s[6] (min(s[6], 0.1) == 0.0 counts as no target),
    # then 40 rows drawn from the same sets, 16 of them with a NaN in a column that reaches an action
    s2, s9 = f32_neighbours(0.29), f32_neighbours(0.10)
    s8 = [np.float32(0.0), np.float32(-0.0), np.float32(1.0), np.float32(np.nan)]
    s6 = [np.float32(v) for v in (0.0, -0.0, 0.05, 0.1, 0.2)]
    rows = []
    for base in rng.uniform(-1.2, 1.2, size=(2, 32)).astype(np.float32):
        for a in s2:
            for b in s9:
                for c in s8:
                    for d in s6:
                        r = base.copy(); r[2], r[9], r[8], r[6] = a, b, c, d; rows.append(r)
    for i, r in enumerate(rng.uniform(-1.2, 1.2, size=(40, 32)).astype(np.float32)):
        r[2], r[9], r[8], r[6] = s2[rng.randint(3)], s9[rng.randint(3)], s8[rng.randint(4)], s6[rng.randint(5)]
        if i < 16:
            r[(0, 1, 3, 4, 5, 7, 11, 12)[i % 8]] = np.nan
        rows.append(r)
    obs = np.asarray(rows, np.float32)
    assert obs.shape == (400, 32)
    obs71 = np.zeros((400, 71), np.float32)      # the one-hot rows: 32 columns, then the walker's id among 39
    obs71[:, :32] = obs
    obs71[np.arange(400), 32 + np.arange(400) % 39] = 1.0
    pol = hm.MultiWalkerHeuristicPolicy(None, None)
    out["multiwalker_obs"] = obs
    out["multiwalker_act"] = pol.sample_actions(obs.astype(np.float64))[0]
    out["multiwalker71_obs"] = obs71
    out["multiwalker71_act"] = pol.sample_actions(obs71.astype(np.float64))[0]
    path = os.path.join(OUT, "heuristics_edges.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KB", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
    edges()
