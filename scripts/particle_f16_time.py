"""Float32 against half-precision observation rows of the particle worlds (obs_dtype=torch.float16: waterworld_kernel_f16, hostage_kernel_f16,
waterworld_policy_f16_kernel) at 32 768 envs: the table of DESIGN 4.4e.

    python scripts/particle_f16_time.py                       # every figure below, float32 and half alternating, three processes each
    python scripts/particle_f16_time.py --rows ww,policy      # some of: ww, wwgeneric, hostage, policy, rollout

Figures
  ww         a step launch of Waterworld 5/10/10 with 30 sensors (rows of 213: the specialised instantiations)
  wwgeneric  ... of 12/25/25 with 16 sensors (rows of 115: the generic instantiations)
  hostage    a step launch of the hostage world 3/10/5 with 30 sensors (rows of 156: the specialised instantiations)
  policy     a launch of the Waterworld potential-field policy over the rows of 5/10/10
  rollout    a step of RolloutCollector(store_observations=True, graph=True) over 5/10/10 with that policy in the loop, horizon 16

The protocol of scripts/ww_crowd_time.py: steady state with auto_reset (max_steps 500) after an untimed warm-up, device events around the
launches alone, one measurement per process (`--one ...`, what the parent starts), one process at a time; the two variants alternate and
each figure is the min - max of three processes.  The verdict follows DESIGN 4.1's rule: "faster" only if every half run is below every
float32 run and the medians are apart by more than twice the float32 runs' max - min; otherwise "no different" or "slower by x".
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 32768
ROWS = ("ww", "wwgeneric", "hostage", "policy", "rollout")


def make(row, half):
    import torch
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    from madrl_amd.waterworld import BatchedMAWaterWorld
    kw = dict(n_envs=N, device="cuda:0", seed=0, max_steps=500, auto_reset=True, **(dict(obs_dtype=torch.float16) if half else {}))
    if row == "hostage":
        return BatchedContinuousHostageWorld(3, 10, 5, 2, 2, **kw)
    if row == "wwgeneric":
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # (the hint that this shape runs on the generic kernel: that is the point)
            return BatchedMAWaterWorld(12, 25, n_poison=25, n_sensors=16, **kw)
    return BatchedMAWaterWorld(5, 10, n_poison=10, n_sensors=30, **kw)


def one(row, half):
    """one measurement in this process -> a JSON line"""
    import torch
    from madrl_amd.heuristics import WaterworldHeuristicPolicy
    from madrl_amd.rollout import RolloutCollector
    dev = torch.device("cuda:0")
    env = make(row, half)
    Na = env._obs.shape[1]
    dt = torch.float16 if half else torch.float32
    if row == "rollout":
        T = 16
        col = RolloutCollector(env, WaterworldHeuristicPolicy(obs_dtype=dt), horizon=T, store_observations=True, graph=True)
        assert col._slots
        run = lambda k: [col.collect() for _ in range(k)]
        per = T
        run(3)   # eager, capture, replay
        assert col._obs_slots.dtype is dt
    elif row == "policy":
        pol = WaterworldHeuristicPolicy(obs_dtype=dt)
        obs = env.reset()
        for _ in range(20):   # rows of a running episode, not of a reset
            obs = env.step(pol(obs))[0]
        run = lambda k: [pol(obs) for _ in range(k)]
        per = 1
    else:
        acts = [torch.rand(N, Na, 2, device=dev) * 2 - 1 for _ in range(8)]
        env.reset()
        run = lambda k: [env.step(acts[i % 8]) for i in range(k)]
        per = 1

    def timed(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(k); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (k * per) * 1e3

    run(10); torch.cuda.synchronize()
    us = timed(10)
    k = int(min(300, max(10, 1.0e6 / (us * per))))   # about a second of launches
    us = timed(k)
    print(json.dumps(dict(row=row, half=int(half), us=us, launches=k * per, obs_bytes=env._obs.numel() * env._obs.element_size())), flush=True)


def measure(row, half):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", row, str(int(half))], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit("measurement %s half=%d failed (%d):\n%s" % (row, half, out.returncode, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def verdict(f, h):
    """DESIGN 4.1's rule over the two variants' runs (us)"""
    med = lambda v: sorted(v)[len(v) // 2]
    spread = max(f) - min(f)
    if max(h) < min(f) and med(f) - med(h) > 2 * spread:
        return "faster by %.1f %%" % (100 * (1 - med(h) / med(f)))
    if min(h) > max(f) and med(h) - med(f) > 2 * spread:
        return "slower by %.1f %%" % (100 * (med(h) / med(f) - 1))
    return "no different"


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        return one(argv[1], int(argv[2]))
    rows = argv[argv.index("--rows") + 1].split(",") if "--rows" in argv else ROWS
    for row in rows:
        runs = ([], [])
        for _ in range(3):   # float32, half: alternating
            for half in (0, 1):
                runs[half].append(measure(row, half))
        f, h = ([r["us"] for r in rs] for rs in runs)
        print("%-10s float32 %8.1f - %8.1f us   half %8.1f - %8.1f us   half is %s   (row buffer %.1f -> %.1f MB)" % (
            row, min(f), max(f), min(h), max(h), verdict(f, h), runs[0][0]["obs_bytes"] / 1e6, runs[1][0]["obs_bytes"] / 1e6), flush=True)


if __name__ == "__main__":
    main()
