"""Per-launch cost of the two-buffer step on the multi-wavefront kernel, at the authors' 30 v 50 shape (runners/old/rllab/pursuit.sh:1:
32 x 32 map pool, obs_range 11, --flatten --surround --sample_maps, local reward; auto-reset at 500 steps).

    python scripts/step_to_group_time.py --mode {inplace,to,both} [--envs 16384] [--warmup 2000] [--steps 200] [--slots 9]

  inplace   step_into(): the in-place step (pursuit_group_kernel<GShape<...>, 1, false>)
  to        step_into(obs_out=) round a ring of `slots` buffers of 716 MB, as a rollout of horizon slots - 1 that keeps its observations
            does (pursuit_group_kernel<TGShape<...>, 1, true>; a tree without the XG line of pursuit_to_specializations.def: the generic kernel)
  both      the two loops one after the other on envs of their own (one rocprofv3 --kernel-trace --stats run shows both kernels)

One launch per step.  Warm-up steps bring the stale-zero masks to equilibrium first.  Prints one JSON line per loop with the HIP-event
time per step; run it under `rocprofv3 --kernel-trace --stats -- python scripts/step_to_group_time.py ...` for the per-kernel figure and
under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (runs of their own) for the traffic (profiles/r11_step_to_group)."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=("inplace", "to", "both"))
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--slots", type=int, default=9)
    a = ap.parse_args()
    import numpy as np
    import torch
    from madrl_amd.pursuit import BatchedPursuitEvade
    maps = list(np.load(glob.glob(os.path.join(ROOT, "tests", "golden", "pursuit_authors_30v50_obs11.npz"))[0])["maps"])
    N, dev = a.envs, "cuda:0"
    kw = dict(n_pursuers=30, n_evaders=50, obs_range=11, n_catch=2, surround=True, flatten=True, reward_mech="local", sample_maps=True,
              max_steps=500, auto_reset=True)
    for mode in (("inplace", "to") if a.mode == "both" else (a.mode,)):
        env = BatchedPursuitEvade(maps, n_envs=N, device=dev, seed=0, **kw)
        env.reset()
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        acts = [torch.randint(0, 5, (N, 30), device=dev, dtype=torch.int32, generator=gen) for _ in range(8)]
        rew = torch.zeros((N, 30), dtype=torch.float32, device=dev)
        done = torch.zeros(N, dtype=torch.uint8, device=dev)
        ring = [env.obs_buffer] + [torch.zeros_like(env.obs_buffer) for _ in range(a.slots - 1)] if mode == "to" else None
        k = [0]

        def step(i):
            if ring is None:
                env.step_into(acts[i % 8], rew, done)
            else:
                k[0] = (k[0] + 1) % len(ring)
                env.step_into(acts[i % 8], rew, done, obs_out=ring[k[0]])

        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(a.steps):
            step(i)
        t1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(mode=mode, envs=N, kernel=env.kernel_kind, step_to_kernel=env.step_to_kernel_kind, slots=a.slots if ring else 1,
                              us_per_step=round(1e3 * t0.elapsed_time(t1) / a.steps, 2))), flush=True)
        del env, ring
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
