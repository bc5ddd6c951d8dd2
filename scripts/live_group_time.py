"""Per-launch cost of per-env agent counts on the multi-wavefront kernel, at the authors' 30 v 50 shape (runners/old/rllab/pursuit.sh:1:
32 x 32 map pool, obs_range 11, --flatten --surround --sample_maps, local reward; auto-reset at 500 steps).

    python scripts/live_group_time.py --mode {fixed30,live30,live20,generic20} [--envs 16384] [--warmup 200] [--steps 100]

  fixed30    the fixed-shape 30 v 50 group kernel (XG line, pursuit_group_kernel<GShape<...>>)
  live30     capacity 30 v 50, every env at live (30, 50): the live-count group kernel (XLG line, LGShape)
  live20     capacity 30 v 50, every env at live (20, 40): the live-count group kernel
  generic20  capacity 30 v 50, every env at live (20, 40): the generic live-count kernel (pursuit_live_kernel<NT>, set_kernel("generic"))

One launch per step.  Warm-up steps bring the stale-zero masks to equilibrium first.  Prints one JSON line with the HIP-event time per
step; run it under `rocprofv3 --kernel-trace --stats -- python scripts/live_group_time.py ...` for the per-kernel figure
(profiles/r08_live_group)."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=("fixed30", "live30", "live20", "generic20"))
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    a = ap.parse_args()
    import numpy as np
    import torch
    from madrl_amd.pursuit import BatchedPursuitEvade
    # TwoDMaps.resize(2, map_pool16), as recorded with the authors' shape golden
    maps = list(np.load(glob.glob(os.path.join(ROOT, "tests", "golden", "pursuit_authors_30v50_obs11.npz"))[0])["maps"])
    N, dev = a.envs, "cuda:0"
    kw = dict(n_pursuers=30, n_evaders=50, obs_range=11, n_catch=2, surround=True, flatten=True, reward_mech="local", sample_maps=True,
              max_steps=500, auto_reset=True)
    live = a.mode != "fixed30"
    env = BatchedPursuitEvade(maps, n_envs=N, device=dev, seed=0, per_env_counts=live,
                              kernel="generic" if a.mode == "generic20" else "auto", **kw)
    if a.mode.endswith("20"):
        env.set_agent_counts(20, 40)
    env.reset()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    acts = [torch.randint(0, 5, (N, 30), device=dev, dtype=torch.int32, generator=gen) for _ in range(8)]
    rew = torch.zeros((N, 30), dtype=torch.float32, device=dev)
    done = torch.zeros(N, dtype=torch.uint8, device=dev)
    for i in range(a.warmup):
        env.step_into(acts[i % 8], rew, done)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(a.steps):
        env.step_into(acts[i % 8], rew, done)
    t1.record()
    torch.cuda.synchronize()
    counts = env.agent_counts()[1][0].tolist() if live else [30, 50]
    print(json.dumps(dict(mode=a.mode, envs=N, kernel=env.kernel_kind, live=counts, us_per_step=round(1e3 * t0.elapsed_time(t1) / a.steps, 2))))


if __name__ == "__main__":
    main()
