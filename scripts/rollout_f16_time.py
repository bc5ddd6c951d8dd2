"""What half-precision observation rows give a rollout with the device chase policy in the loop.

    python scripts/rollout_f16_time.py --build-variant                       # once, no GPU needed: the library whose half flatten rows take the generic kernel
    python scripts/rollout_f16_time.py [--envs 65536] [--warmup 2000] [--steps 400] [--horizon 16] [--runs 3]
    python scripts/rollout_f16_time.py --one {policy_f32,policy_f16,policy_f16_generic,rollout_f32,rollout_f16} ...      # one measurement, this process

BASELINE configs[1]: 16 x 16, 8 v 30, obs_range 7, flatten; 65 536 envs = 524 288 rows, horizon 16.

  policy_f32 / policy_f16   us per launch of PursuitHeuristicPolicy alone on the rows a live env holds after the untimed steps (float32 env and
                            policy: pursuit_policy_rows_kernel; half env and policy: pursuit_policy_rows_f16_kernel)
  policy_f16_generic        the same half rows through pursuit_policy_f16_kernel: what the row-fast half kernel has to beat.  It needs the variant
                            library (heuristics.hip compiled with -DMADRL_POLICY_F16_ROWS=0, scripts/_variants/, loaded through MADRL_HIP_LIB)
  rollout_f32 / rollout_f16 us per step of RolloutCollector(store_observations=True, graph=True) with the chase policy in the loop: float32 env +
                            float32 policy against half env + half policy

Without --one: every measurement in `--runs` fresh processes each, interleaved (policy_f32, policy_f16, ... then again), each under its own
`timeout -k 10`, one JSON line per run and a last line with min - max per measurement; the first process that fails ends the script.  The
untimed steps (the policy driving the env) bring the stale-zero masks and the evader counts to equilibrium first."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("policy_f32", "policy_f16", "policy_f16_generic", "rollout_f32", "rollout_f16")
VARIANT = os.path.join(ROOT, "scripts", "_variants", "libmadrl_hip_policy_f16_generic.so")


def build_variant():
    """libmadrl_hip.so with heuristics.hip compiled -DMADRL_POLICY_F16_ROWS=0, from the objects of the last build"""
    from madrl_amd import build as b
    b.build()
    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    obj = VARIANT[:-3] + ".heuristics.o"
    subprocess.check_call([b.HIPCC] + b.FLAGS + ["-DMADRL_POLICY_F16_ROWS=0", "-c", os.path.join(b.CSRC, "heuristics.hip"), "-o", obj])
    objs = [obj if os.path.basename(s) == "heuristics.hip" else s[:-4] + ".o" for s in b.sources()]
    subprocess.check_call([b.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", VARIANT] + objs)
    print(VARIANT)


def one(a):
    import torch
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    from madrl_amd.rollout import RolloutCollector
    N, P, dev = a.envs, 8, "cuda:0"
    dtype = torch.float32 if a.one.endswith("f32") else torch.float16
    env = BatchedPursuitEvade([rectangle_map(16, 16)], n_envs=N, device=dev, seed=0, n_pursuers=P, n_evaders=30, obs_range=7, n_catch=2, surround=True,
                              flatten=True, reward_mech="local", max_steps=500, auto_reset=True, obs_dtype=dtype)
    pol = PursuitHeuristicPolicy(7, seed=0, obs_dtype=dtype)
    out = dict(mode=a.one, envs=N, rows=N * P, obs_dtype=str(dtype), lib=os.path.basename(os.environ.get("MADRL_HIP_LIB", "libmadrl_hip.so")))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if a.one.startswith("rollout"):
        col = RolloutCollector(env, pol, a.horizon, store_observations=True, graph=True)
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
        obs = env.reset()
        act = torch.empty((N, P), dtype=torch.int32, device=dev)
        for _ in range(a.warmup):
            obs = env.step(pol(obs, out=act))[0]
        empty = float((~(obs[..., 2 * 49:3 * 49] != 0).any(dim=-1)).float().mean())
        for _ in range(20):
            pol(obs, out=act)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.steps):
            pol(obs, out=act)
        t1.record()
        torch.cuda.synchronize()
        out.update(row_bytes=obs.shape[-1] * obs.element_size(), empty_windows=round(empty, 4), us_per_launch=round(1e3 * t0.elapsed_time(t1) / a.steps, 2))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=MODES)
    ap.add_argument("--build-variant", action="store_true")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a measuring process may take")
    a = ap.parse_args()
    if a.build_variant:
        return build_variant()
    if a.one:
        return one(a)
    modes = [m for m in MODES if m != "policy_f16_generic" or os.path.exists(VARIANT)]
    if len(modes) < len(MODES):
        print("no %s: policy_f16_generic is left out (--build-variant makes it)" % os.path.relpath(VARIANT, ROOT), file=sys.stderr, flush=True)
    res = {m: [] for m in modes}
    for _ in range(a.runs):   # interleaved: a drift of the machine shows in every measurement alike
        for m in modes:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", m, "--envs", str(a.envs), "--warmup", str(a.warmup),
                   "--steps", str(a.steps), "--horizon", str(a.horizon)]
            env = dict(os.environ, MADRL_HIP_LIB=VARIANT) if m == "policy_f16_generic" else os.environ
            line = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, env=env).stdout.strip().splitlines()[-1]   # a failure ends the script here
            print(line, flush=True)
            r = json.loads(line)
            res[m].append(r.get("us_per_launch", r.get("us_per_step")))
    print(json.dumps({m: dict(min=min(v), max=max(v), runs=v) for m, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
