"""Step time of the Waterworld crowd kernel (csrc/waterworld_crowd.hip, `crowd=True`) at shapes beyond one wavefront's worth of particles.

    python scripts/ww_crowd_time.py                      # the table of DESIGN 4.4a: every row below, three processes each, min - max
    python scripts/ww_crowd_time.py --rows shapes,cpu    # some of: shapes, cpu, wave, nw8, live
    python scripts/ww_crowd_time.py --live               # the table of DESIGN 4.4b: the `live` row alone
    python scripts/ww_crowd_time.py --rows livewave      # the table of DESIGN 4.4c (not in the default set)
    python scripts/ww_crowd_time.py --rows ranges        # the table of DESIGN 4.4d (not in the default set)

Rows
  shapes  20/60/40, 33/100/100 and 128/512/383 with 30 sensors, at 4 096 envs and at the largest batch whose observations fit 16 GB:
          us per launch, env-steps/s, ray tests/s (n_pursuers * n_sensors * particles per env-step: what the oracle's sensing loop visits)
  cpu     the float32 C oracle (oracle/waterworld_oracle.c, OpenMP) on this box's host cores at the same shapes: bench.py's cpu_baseline
  wave    crowd kernel against the one-wavefront generic instantiation at 12/25/25 (16 sensors), 32 768 envs
  nw8     eight instead of four wavefronts per workgroup on the first two shapes: needs the variant library
          `SRC=waterworld_crowd MACRO=MADRL_WWC_NW scripts/variants.sh 8` builds (scripts/_variants/, git-ignored)
  live    per-env particle counts (per_env_counts=True) at the capacities 20/60/40 and 33/100/100, 4 096 envs: the fixed-shape kernel, the
          live-count kernel with every env at the capacity, and with every env's triple drawn uniformly between (1, 1, 1) and the capacity
          -- the three alternating, three processes each (ray tests/s of the spread row are counted at the capacity: compare its us)
  livewave  per-env particle counts on the one-wavefront kernel (per_env_counts="wave") against the crowd kernel's, at the capacities
          5/10/10 (30 sensors) and 12/25/25 (16 sensors), 32 768 envs: the fixed-shape one-wavefront kernel (specialised at the first
          capacity, generic at the second), the one-wavefront live kernel and the crowd live kernel with every env at the capacity, and
          both live kernels on the same spread of triples -- the five alternating, three processes each
  ranges  per-pursuer sensor ranges (madrl_waterworld_set_sensor_ranges) against the fixed-shape kernel of the same handle kind: one-wavefront
          at 12/25/25 (16 sensors; generic) and 5/10/10 (30 sensors; specialised), 32 768 envs, and crowd at 20/60/40, 4 096 envs.  Three
          variants alternating, three processes each: fixed shape, the ranged entry with every range at 0.2 (the same ray tests and the same
          cull as the fixed kernel: the cost of the entry itself), and with the ranges cycling over 0.1 / 0.2 / 0.3 (the cull runs on 0.3)

Steady state with auto_reset (max_steps 500), after an untimed warm-up; device events around the launches alone.  One measurement per
process (`--one ...`, what the parent starts), one process at a time.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"20/60/40": (20, 60, 40, 30), "33/100/100": (33, 100, 100, 30), "128/512/383": (128, 512, 383, 30), "12/25/25": (12, 25, 25, 16),
          "5/10/10": (5, 10, 10, 30)}
NW8_LIB = os.path.join(ROOT, "scripts", "_variants", "libmadrl_hip.waterworld_crowd.8.so")
OBS_BYTES = 16e9


def obs_dim(K):
    return 7 * K + 3


def largest_batch(shape):
    Np, _Ne, _Npo, K = SHAPES[shape]
    return int(OBS_BYTES // (Np * obs_dim(K) * 4)) // 1024 * 1024


def one(shape, N, crowd, live=0):
    """one measurement in this process -> a JSON line.  live: 0 fixed shape, 1 per-env counts at the capacity, 2 a spread of counts,
    3 per-pursuer sensor ranges all at 0.2, 4 ranges cycling over 0.1 / 0.2 / 0.3"""
    import ctypes
    import numpy as np
    import torch
    from madrl_amd import _lib
    from madrl_amd.waterworld import BatchedMAWaterWorld
    Np, Ne, Npo, K = SHAPES[shape]
    dev = torch.device("cuda:0")
    env = BatchedMAWaterWorld(Np, Ne, n_poison=Npo, n_sensors=K, n_envs=N, device=dev, seed=0, max_steps=500, auto_reset=True, crowd=bool(crowd),
                              per_env_counts=(True if crowd else "wave") if live in (1, 2) else False)
    if live >= 3:   # through the C function: it takes equal values too, which the constructor would hand to the uniform kernel
        r = np.full(Np, 0.2) if live == 3 else np.asarray([(0.1, 0.2, 0.3)[i % 3] for i in range(Np)])
        _lib.check(_lib.lib().madrl_waterworld_set_sensor_ranges(env._handle, r.ctypes.data_as(ctypes.c_void_p)))
    if live == 2:
        g = torch.Generator().manual_seed(0)
        env.set_particle_counts(*[torch.randint(1, c + 1, (N,), generator=g) for c in (Np, Ne, Npo)])
    acts = [torch.rand(N, Np, 2, device=dev) * 2 - 1 for _ in range(8)]
    env.reset()
    L = _lib.lib()
    outs = [_lib.ptr(t) for t in (env._obs, env._rew, env._done, env._info)]

    def run(k):
        for i in range(k):
            _lib.check(L.madrl_waterworld_step(env._handle, _lib.ptr(acts[i % 8]), None, *outs, _lib.current_stream(dev)))

    def timed(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(k); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k * 1e3

    run(10); torch.cuda.synchronize()
    us = timed(10)
    steps = int(min(300, max(20, 1.0e6 / us)))   # about a second of launches
    us = timed(steps)
    print(json.dumps(dict(shape=shape, n_envs=N, kernel=env.kernel_kind + ("", "-live", "-live-spread", "-ranges", "-ranges-spread")[live], us_per_launch=us, env_steps_per_s=N / us * 1e6,
                          ray_tests_per_s=N * Np * K * (Np + Ne + Npo) / us * 1e6, steps=steps)), flush=True)


def cpu(shape):
    import numpy as np
    from oracle import waterworld as ww
    Np, Ne, Npo, K = SHAPES[shape]
    N = 64 if Np + Ne + Npo > 500 else 512
    orc = ww.WaterworldOracle(Np, Ne, n_poison=Npo, n_sensors=K, n_envs=N, seed=0, max_steps=500, dtype=np.float32)
    orc.reset()
    act = np.random.RandomState(0).uniform(-1, 1, (N, Np, 2)).astype(np.float32)
    orc.step(act)
    t0, n = time.time(), 0
    while time.time() - t0 < 3.0:
        orc.step(act); n += 1
    dt = time.time() - t0
    return dict(shape=shape, n_envs=N, env_steps_per_s=N * n / dt, threads=int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count())


def measure(shape, N, crowd, lib=None, live=0):
    env = dict(os.environ)
    if lib:
        env["MADRL_HIP_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", shape, str(N), str(int(crowd)), str(live)], env=env,
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit("measurement %s N=%d crowd=%d live=%d failed (%d):\n%s" % (shape, N, crowd, live, out.returncode, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def child(shape, N, crowd, lib=None, rs=None):
    rs = rs or [measure(shape, N, crowd, lib) for _ in range(3)]
    us = [r["us_per_launch"] for r in rs]
    lo, hi = min(us), max(us)
    r = rs[0]
    scale = lambda key, u: r[key] * r["us_per_launch"] / u
    print("%-12s %-19s N=%8d  %10.1f - %10.1f us/launch  %.3e - %.3e env-steps/s  %.3e - %.3e ray tests/s%s" % (
        shape, r["kernel"], N, lo, hi, scale("env_steps_per_s", hi), scale("env_steps_per_s", lo), scale("ray_tests_per_s", hi),
        scale("ray_tests_per_s", lo), "  [%s]" % os.path.basename(lib) if lib else ""), flush=True)
    return lo, hi


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        return one(argv[1], int(argv[2]), int(argv[3]), int(argv[4]) if len(argv) > 4 else 0)
    rows = argv[argv.index("--rows") + 1].split(",") if "--rows" in argv else ["live"] if "--live" in argv else ["shapes", "cpu", "wave", "nw8"]
    big = ("20/60/40", "33/100/100", "128/512/383")
    if "shapes" in rows:
        for s in big:
            for N in (4096, largest_batch(s)):
                child(s, N, True)
    if "cpu" in rows:
        for s in big:
            r = cpu(s)
            print("%-12s float32 C oracle, %d threads, N=%d: %.3e env-steps/s" % (s, r["threads"], r["n_envs"], r["env_steps_per_s"]), flush=True)
    if "wave" in rows:
        c = child("12/25/25", 32768, True)
        w = child("12/25/25", 32768, False)
        print("12/25/25 at 32 768 envs: crowd / one-wavefront generic = %.2f - %.2f" % (c[0] / w[1], c[1] / w[0]), flush=True)
    if "nw8" in rows:
        if not os.path.exists(NW8_LIB):
            raise SystemExit("no %s: build it with SRC=waterworld_crowd MACRO=MADRL_WWC_NW scripts/variants.sh 8" % NW8_LIB)
        for s in big[:2]:
            for N in (4096, largest_batch(s)):
                child(s, N, True)
                child(s, N, True, lib=NW8_LIB)
    if "live" in rows:
        for s in big[:2]:
            runs = [[], [], []]
            for _ in range(3):   # fixed, live at the capacity, live spread: alternating
                for live in range(3):
                    runs[live].append(measure(s, 4096, True, live=live))
            (f0, f1), (l0, l1), (s0, s1) = [child(s, 4096, True, rs=r) for r in runs]
            print("%s at 4 096 envs: live at the capacity / fixed = %.3f - %.3f, spread / live at the capacity = %.3f - %.3f" % (
                s, l0 / f1, l1 / f0, s0 / l1, s1 / l0), flush=True)
    if "livewave" in rows:
        variants = ((False, 0), (False, 1), (True, 1), (False, 2), (True, 2))   # (crowd, live)
        for s in ("5/10/10", "12/25/25"):
            runs = [[] for _ in variants]
            for _ in range(3):
                for r, (crowd, live) in zip(runs, variants):
                    r.append(measure(s, 32768, crowd, live=live))
            (f0, f1), (w0, w1), (c0, c1), (ws0, ws1), (cs0, cs1) = [child(s, 32768, crowd, rs=r) for r, (crowd, _l) in zip(runs, variants)]
            print("%s at 32 768 envs: one-wavefront live / fixed = %.3f - %.3f; crowd live / one-wavefront live = %.2f - %.2f at the capacity, "
                  "%.2f - %.2f on the spread; gate (one-wavefront live faster than crowd live beyond the spread of the repetitions): %s" % (
                      s, w0 / f1, w1 / f0, c0 / w1, c1 / w0, cs0 / ws1, cs1 / ws0, "holds" if w1 < c0 and ws1 < cs0 else "does NOT hold"),
                  flush=True)
    if "ranges" in rows:
        for s, N, crowd in (("12/25/25", 32768, False), ("5/10/10", 32768, False), ("20/60/40", 4096, True)):
            runs = [[], [], []]
            for _ in range(3):   # fixed, ranged at one value, ranged spread: alternating
                for r, live in zip(runs, (0, 3, 4)):
                    r.append(measure(s, N, crowd, live=live))
            (f0, f1), (r0, r1), (s0, s1) = [child(s, N, crowd, rs=r) for r in runs]
            print("%s at %d envs (%s): ranged at one value / fixed = %.3f - %.3f, ranged spread / fixed = %.3f - %.3f" % (
                s, N, "crowd" if crowd else "one wavefront", r0 / f1, r1 / f0, s0 / f1, s1 / f0), flush=True)


if __name__ == "__main__":
    main()
