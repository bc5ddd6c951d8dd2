"""Time of a rollout that KEEPS its observations: RolloutCollector(store_observations=True, graph=True) with PursuitHeuristicPolicy, in us per
rollout step (policy launch + step kernel + whatever moves the observations into the trajectory), at
    c2       BASELINE configs[1]: 16 x 16, 8 v 30, obs_range 7, 65 536 envs, T = 16      (one-wavefront kernel)
    cnn      the authors' CNN line: 128 x 128 pool, 100 v 300, obs_range 21, (R, R, 4) rows, 1 024 envs, T = 8   (crowd kernel)
    authors  the authors' 30 v 50 line: 32 x 32 pool, obs_range 11, 16 384 envs, T = 8   (multi-wavefront kernel)
each after 2 000 untimed steps, so that the stale-zero masks are at their equilibrium.

    python scripts/rollout_store_time.py [c2|cnn|authors ...] [--root DIR] [--reps K] [--copy]

--root DIR: time the madrl_amd package of another checkout (e.g. the parent commit built beside this one) with this same script;
--copy: force the collector that copies the observations after every step (obs_slots=False; only this tree has the switch).
Prints one JSON line per configuration."""
import glob, json, os, sys, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
argv = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in argv:
    i = argv.index("--root"); ROOT = os.path.abspath(argv[i + 1]); del argv[i:i + 2]
REPS = 3
if "--reps" in argv:
    i = argv.index("--reps"); REPS = int(argv[i + 1]); del argv[i:i + 2]
COPY = "--copy" in argv
argv = [a for a in argv if a != "--copy"]
sys.path.insert(0, ROOT)
import numpy as np
import torch
from madrl_amd.heuristics import PursuitHeuristicPolicy
from madrl_amd.maps import rectangle_map, resize, synthetic_map_pool
from madrl_amd.pursuit import BatchedPursuitEvade
from madrl_amd.rollout import RolloutCollector

DEV = "cuda:0"


def pool128():
    return list(resize(8, np.load(glob.glob(os.path.join(ROOT, "tests", "golden", "pursuit_pool16_sample_maps.npz"))[0])["maps"]))


CONFIGS = {
    "c2": (lambda: [rectangle_map(16, 16)], 65536, 16, dict(n_pursuers=8, n_evaders=30, obs_range=7, n_catch=2, surround=True, flatten=True)),
    "cnn": (pool128, 1024, 8, dict(n_pursuers=100, n_evaders=300, obs_range=21, n_catch=2, surround=True, flatten=False, sample_maps=True)),
    "authors": (lambda: synthetic_map_pool(10, 32, 32), 16384, 8, dict(n_pursuers=30, n_evaders=50, obs_range=11, n_catch=2, surround=True, flatten=True,
                                                                       sample_maps=True)),
}

for name in argv or ["c2", "cnn", "authors"]:
    maps, N, T, kw = CONFIGS[name]
    env = BatchedPursuitEvade(maps(), n_envs=N, device=DEV, seed=0, max_steps=500, auto_reset=True, reward_mech="local", **kw)
    col = RolloutCollector(env, PursuitHeuristicPolicy(kw["obs_range"], flatten=kw["flatten"], seed=1), T, discount=0.99, store_observations=True, graph=True,
                           **(dict(obs_slots=False) if COPY else {}))
    warm = (2000 + T - 1) // T
    for _ in range(warm):
        col.collect()
    torch.cuda.synchronize()
    K = max(4, 1600 // T)
    us = []
    for rep in range(REPS):
        t0 = time.perf_counter()
        for _ in range(K):
            col.collect()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / (K * T) * 1e6)
    print(json.dumps(dict(config=name, root=ROOT, n_envs=N, horizon=T, kernel=env.kernel_kind, step_to_kernel=getattr(env, "step_to_kernel_kind", None),
                          slots=bool(getattr(col, "_slots", False)), warm_steps=warm * T, timed_steps=K * T,
                          us_per_rollout_step=[round(u, 2) for u in us], obs_mb_per_step=round(N * kw["n_pursuers"] * env.obs_dim * 4 / 1e6, 1))), flush=True)
    del col, env
    torch.cuda.empty_cache()
