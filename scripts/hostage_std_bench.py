"""The hostage world under StandardizedEnv: the wrapper fused into the step kernel (madrl_hostage_set_standardize) against the stand-alone
epilogue launches (madrl_wrap_obsnorm / madrl_wrap_rewnorm), and the unwrapped step next to both.

    python scripts/hostage_std_bench.py [--envs 32768] [--steps 2000] [--reps 3] [--out FILE.json]

32 768 envs of ContinuousHostageWorld(3, 10, 5, 2, 2) with auto_reset, two wrapper configurations: obsnorm + rewnorm, and the authors' own
StandardizedEnv(env) (no normalisation, scale 1).  The variants of a configuration live side by side on one device and are timed in turn,
`--reps` times each (device events around `--steps` steps after a warm-up), so that a drift of the machine hits all of them alike.  Prints
one line per timed window and one JSON summary line (median, minimum and maximum of the repetitions in us per step)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from madrl_amd.hostage import BatchedContinuousHostageWorld  # noqa: E402
from madrl_amd.wrappers import StandardizedEnv  # noqa: E402

CONFIGS = (("obsnorm_rewnorm", dict(scale_reward=0.5, enable_obsnorm=True, enable_rewnorm=True)),
           ("authors_default", dict()))


def window(env, acts, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        env.step(acts[i % len(acts)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3   # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hostage_std_bench: no ROCm device; a time comes from the GPU or not at all")
    dev, N = torch.device("cuda:0"), args.envs
    mk = lambda: BatchedContinuousHostageWorld(3, 10, 5, 2, 2, n_envs=N, device=dev, seed=0, auto_reset=True)
    acts = [(torch.rand((N, 3, 2), device=dev) * 2 - 1).contiguous() for _ in range(8)]
    summary = dict(envs=N, steps=args.steps, warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0), configs={})
    for cname, cfg in CONFIGS:
        envs = (("fused", StandardizedEnv(mk(), fused=True, **cfg)), ("epilogue", StandardizedEnv(mk(), fused=False, **cfg)), ("unwrapped", mk()))
        assert envs[0][1]._fused and not envs[1][1]._fused
        for _, env in envs:
            env.reset()
            for i in range(args.warmup):
                env.step(acts[i % 8])
        torch.cuda.synchronize()
        times = {name: [] for name, _ in envs}
        for rep in range(args.reps):
            for name, env in envs:
                us = window(env, acts, args.steps)
                times[name].append(us)
                print("%-16s %-10s rep %d  %.2f us per step" % (cname, name, rep, us), flush=True)
        summary["configs"][cname] = {name: dict(median_us=statistics.median(t), min_us=min(t), max_us=max(t), all_us=t) for name, t in times.items()}
        del envs
        torch.cuda.empty_cache()
    line = json.dumps(summary, separators=(",", ":"))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
