"""Per-launch cost of per-env agent counts (BatchedPursuitEvade(per_env_counts=True)) at the headline shape.

    python scripts/live_counts_time.py --mode {fixed8,live8,live7,generic7} [--envs 65536] [--warmup 300] [--steps 200]

  fixed8    the fixed-shape 8 v 30 wave kernel (bench.py's headline workload: 16 x 16, obs_range 7, local reward, auto-reset at 500)
  live8     capacity 8 v 30, every env at live (8, 30): the live-count wave kernel
  live7     capacity 8 v 30, every env at live (7, 29): the live-count wave kernel
  generic7  a fixed 7 v 29 batch: the generic kernel (what a curriculum step used to fall back to)

Warm-up steps bring the stale-zero masks to equilibrium first.  Prints one JSON line with the HIP-event time per step; run it under
`rocprofv3 --kernel-trace --stats -- python scripts/live_counts_time.py ...` for the per-kernel figure (profiles/r07_live_counts)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=("fixed8", "live8", "live7", "generic7"))
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    import torch
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    N, dev = a.envs, "cuda:0"
    kw = dict(n_pursuers=8, n_evaders=30, obs_range=7, reward_mech="local", max_steps=500, auto_reset=True)
    if a.mode == "generic7":
        kw.update(n_pursuers=7, n_evaders=29)
    env = BatchedPursuitEvade([rectangle_map(16, 16)], n_envs=N, device=dev, seed=0, per_env_counts=a.mode.startswith("live"), **kw)
    if a.mode == "live7":
        env.set_agent_counts(7, 29)
    env.reset()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    acts = [torch.randint(0, 5, (N, 8 if a.mode != "generic7" else 7), device=dev, dtype=torch.int32, generator=gen) for _ in range(8)]
    rew = torch.zeros((N, int(env.n_pursuers)), dtype=torch.float32, device=dev)
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
    live = env.agent_counts()[1][0].tolist() if env.per_env_counts else [int(env.n_pursuers), int(env.n_evaders)]
    print(json.dumps(dict(mode=a.mode, envs=N, kernel=env.kernel_kind, live=live, us_per_step=round(1e3 * t0.elapsed_time(t1) / a.steps, 2))))


if __name__ == "__main__":
    main()
