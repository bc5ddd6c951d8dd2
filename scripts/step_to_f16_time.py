"""What half-precision observation slots cost and gain.

    python scripts/step_to_f16_time.py [--shape {c1,authors}] [--envs N] [--warmup 2000] [--steps 400] [--horizon T] [--runs 3]
    python scripts/step_to_f16_time.py --one {f32,f16,f16_generic,rollout_f32,rollout_f16} ...      # one measurement, this process

  --shape c1       BASELINE configs[1]: 16 x 16, 8 v 30, obs_range 7, flatten; 65 536 envs, horizon 16 (one wavefront per env: pursuit_wave_kernel
                   over a TShape / THShape)
  --shape authors  the authors' training shape: a 32 x 32 synthetic_map_pool, 30 v 50, obs_range 11, sample_maps, surround, flatten; 16 384 envs,
                   horizon 8 (four wavefronts per env: pursuit_group_kernel over a TGShape / THGShape)

  f32 / f16     us per launch of the two-buffer step round a ring of horizon + 1 slots, as a rollout that keeps its observations steps:
                madrl_pursuit_step_to against madrl_pursuit_step_to_f16 of the same build
  f16_generic   the half step of the same batch on the generic kernel (kernel="generic"): what the half fast kernel has to beat
  rollout_*     us per step of RolloutCollector(store_observations=True, graph=True) with a policy that replays stored actions

Without --one: every measurement in `--runs` fresh processes each, interleaved (f32, f16, ... then again), one JSON line per run and a
last line with min - max per measurement.  Warm-up steps bring the stale-zero masks to equilibrium first."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("f32", "f16", "f16_generic", "rollout_f32", "rollout_f16")
# name: (envs, horizon, maps, pursuers, env kwargs)
SHAPES = {"c1": (65536, 16, "rectangle16", 8, dict(n_evaders=30, obs_range=7)),
          "authors": (16384, 8, "pool32", 30, dict(n_evaders=50, obs_range=11, sample_maps=True))}


def one(a):
    import torch
    from madrl_amd.maps import rectangle_map, synthetic_map_pool
    from madrl_amd.pursuit import BatchedPursuitEvade
    from madrl_amd.rollout import RolloutCollector
    maps, P, shape_kw = SHAPES[a.shape][2:]
    N, dev = a.envs, "cuda:0"
    half = a.one in ("f16", "f16_generic", "rollout_f16")
    kw = dict(n_pursuers=P, n_catch=2, surround=True, flatten=True, reward_mech="local", max_steps=500, auto_reset=True, **shape_kw)
    if half:
        kw["obs_dtype"] = torch.float16
    if a.one == "f16_generic":
        kw["kernel"] = "generic"
    env = BatchedPursuitEvade({"rectangle16": lambda: [rectangle_map(16, 16)], "pool32": lambda: synthetic_map_pool(10, 32, 32)}[maps](),
                              n_envs=N, device=dev, seed=0, **kw)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    acts = [torch.randint(0, 5, (N, P), device=dev, dtype=torch.int32, generator=gen) for _ in range(8)]
    out = dict(mode=a.one, shape=a.shape, envs=N, step_to_kernel=env.step_to_kernel_kind, obs_dtype=str(env.obs_dtype))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if a.one.startswith("rollout"):
        k = [0]

        def policy(obs):
            k[0] += 1
            return acts[k[0] % 8]

        col = RolloutCollector(env, policy, a.horizon, store_observations=True, graph=True)
        for _ in range(max(3, a.warmup // a.horizon)):
            col.collect()
        torch.cuda.synchronize()
        reps = max(1, a.steps // a.horizon)
        t0.record()
        for _ in range(reps):
            col.collect()
        t1.record()
        torch.cuda.synchronize()
        out.update(horizon=a.horizon, slot_bytes=col._obs_slots[0].numel() * col._obs_slots.element_size(),
                   us_per_step=round(1e3 * t0.elapsed_time(t1) / (reps * a.horizon), 2))
    else:
        env.reset()
        rew = torch.zeros((N, P), dtype=torch.float32, device=dev)
        done = torch.zeros(N, dtype=torch.uint8, device=dev)
        ring = [torch.zeros_like(env.obs_buffer) for _ in range(a.horizon + 1)]
        for i in range(a.warmup):
            env.step_into(acts[i % 8], rew, done, obs_out=ring[i % len(ring)])
        torch.cuda.synchronize()
        t0.record()
        for i in range(a.warmup, a.warmup + a.steps):
            env.step_into(acts[i % 8], rew, done, obs_out=ring[i % len(ring)])
        t1.record()
        torch.cuda.synchronize()
        out.update(slots=len(ring), slot_bytes=ring[0].numel() * ring[0].element_size(), us_per_launch=round(1e3 * t0.elapsed_time(t1) / a.steps, 2))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=MODES)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="c1")
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--horizon", type=int, default=None)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    a.envs = SHAPES[a.shape][0] if a.envs is None else a.envs
    a.horizon = SHAPES[a.shape][1] if a.horizon is None else a.horizon
    if a.one:
        return one(a)
    res = {m: [] for m in MODES}
    for _ in range(a.runs):   # interleaved: a drift of the machine shows in every measurement alike
        for m in MODES:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", m, "--shape", a.shape, "--envs", str(a.envs), "--warmup", str(a.warmup), "--steps", str(a.steps),
                   "--horizon", str(a.horizon)]
            line = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1]
            print(line, flush=True)
            r = json.loads(line)
            res[m].append(r.get("us_per_launch", r.get("us_per_step")))
    print(json.dumps({m: dict(min=min(v), max=max(v), runs=v) for m, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
