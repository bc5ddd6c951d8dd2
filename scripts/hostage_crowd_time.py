"""Step time of the hostage-world crowd kernel (csrc/hostage_crowd.hip, `crowd=True`) at shapes beyond one wavefront's worth of particles.

    python scripts/hostage_crowd_time.py                      # the table of DESIGN 4.5a: every row below, three processes each, min - max
    python scripts/hostage_crowd_time.py --rows shapes,cpu    # some of: shapes, cpu, wave, nw8, live
    python scripts/hostage_crowd_time.py --live               # the table of DESIGN 4.5b: the `live` row alone

Rows
  shapes  20/30/40 at 4 096 and 262 144 envs, 33/10/20 at 4 096, 128/64/831 at 4 096 and 32 768 (30 sensors, n_coop_save 2): us per launch,
          env-steps/s, ray tests/s (n_good * n_sensors * (n_hostages + n_bad + 2) per env-step: what the oracle's sensing loop visits) and
          the share of 8 TB/s the algorithmic bytes of an env-step reach (actions, observations, rewards, done, info, the record read and
          written)
  cpu     the float32 C oracle (oracle/hostage_oracle.c, OpenMP) on this box's host cores at the same shapes
  wave    3/10/5 at 32 768 envs on both kernels, alternating in one process: the cost of the crowd form on a shape both take
  nw8     eight instead of four wavefronts per workgroup on the first two shapes: needs the variant library
          `SRC=hostage_crowd MACRO=MADRL_HWC_NW scripts/variants.sh 8` builds (scripts/_variants/, git-ignored)
  live    per-env particle counts (per_env_counts=True) at the capacities 20/30/40 and 33/10/20, 4 096 envs: the fixed-shape kernel, the
          live-count kernel with every env at the capacity, and with every env's triple drawn uniformly between (1, 1, 1) and the capacity
          -- the three alternating, three processes each (ray tests/s of the spread row are counted at the capacity: compare its us)

Steady state with auto_reset (max_steps 500), after an untimed warm-up; device events around at least 200 launches with no synchronise
between them.  One measurement per process (`--one ...`, what the parent starts), one process at a time.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 30
SHAPES = {"20/30/40": (20, 30, 40), "33/10/20": (33, 10, 20), "128/64/831": (128, 64, 831), "3/10/5": (3, 10, 5)}
ROWS = (("20/30/40", 4096), ("20/30/40", 262144), ("33/10/20", 4096), ("128/64/831", 4096), ("128/64/831", 32768))
NW8_LIB = os.path.join(ROOT, "scripts", "_variants", "libmadrl_hip.hostage_crowd.8.so")
HBM_PEAK = 8e12
STEPS = 200
LIVE_KINDS = ("crowd", "crowd-live", "crowd-live-spread")


def bytes_per_env_step(shape):
    Nr, Nh, Nc = SHAPES[shape]
    rec = (4 * (Nr + Nh + Nc) + 9 + 3) // 4 * 4 * 4
    return Nr * 2 * 4 + Nr * (5 * K + 6) * 4 + Nr * 4 + 1 + 8 + 2 * rec


def _env(shape, N, crowd, live=0):
    """live: 0 fixed shape, 1 per-env counts at the capacity, 2 a spread of counts"""
    import torch
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    Nr, Nh, Nc = SHAPES[shape]
    env = BatchedContinuousHostageWorld(Nr, Nh, Nc, 2, 2, n_sensors=K, n_envs=N, device=torch.device("cuda:0"), seed=0, max_steps=500,
                                        auto_reset=True, crowd=bool(crowd), per_env_counts=bool(live))
    if live == 2:
        g = torch.Generator().manual_seed(0)
        env.set_particle_counts(*[torch.randint(1, c + 1, (N,), generator=g) for c in (Nr, Nh, Nc)])
    return env


def one(shape, N, kernels):
    """one measurement per kernel of `kernels` ("crowd", "wave", "crowd,wave": alternating blocks; "crowd-live" / "crowd-live-spread": the
    live-count kernel at the capacity / over a spread of counts) in this process -> a JSON line each"""
    import torch
    from madrl_amd import _lib
    Nr, Nh, Nc = SHAPES[shape]
    dev = torch.device("cuda:0")
    L = _lib.lib()
    acts = [torch.rand(N, Nr, 2, device=dev) * 2 - 1 for _ in range(8)]
    runs = {}
    for kind in kernels.split(","):
        env = _env(shape, N, kind != "wave", LIVE_KINDS.index(kind) if kind in LIVE_KINDS else 0)
        assert env.kernel_kind == kind.split("-")[0]
        env.reset()
        outs = [_lib.ptr(t) for t in (env._obs, env._rew, env._done, env._info)]

        def run(k, env=env, outs=outs):
            for i in range(k):
                _lib.check(L.madrl_hostage_step(env._handle, _lib.ptr(acts[i % 8]), None, *outs, _lib.current_stream(dev)))
        runs[kind] = (env, run)

    def timed(run, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(k); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k * 1e3

    for _env_, run in runs.values():
        run(10)
    torch.cuda.synchronize()
    best = {}
    for _rep in range(2 if len(runs) > 1 else 1):   # alternating: crowd, wave, crowd, wave
        for kind, (_env_, run) in runs.items():
            us = timed(run, STEPS)
            best[kind] = min(best.get(kind, us), us)
    for kind, us in best.items():
        print(json.dumps(dict(shape=shape, n_envs=N, kernel=kind, us_per_launch=us, env_steps_per_s=N / us * 1e6,
                              ray_tests_per_s=N * Nr * K * (Nh + Nc + 2) / us * 1e6,
                              hbm_share=N * bytes_per_env_step(shape) / (us * 1e-6) / HBM_PEAK, steps=STEPS)), flush=True)


def cpu(shape):
    import numpy as np
    from oracle import hostage as ho
    Nr, Nh, Nc = SHAPES[shape]
    N = 64 if Nr + Nh + Nc > 500 else 512
    orc = ho.HostageOracle(Nr, Nh, Nc, 2, 2, n_sensors=K, n_envs=N, seed=0, max_steps=500, dtype=np.float32)
    orc.reset()
    act = np.random.RandomState(0).uniform(-1, 1, (N, Nr, 2)).astype(np.float32)
    orc.step(act)
    t0, n = time.time(), 0
    while time.time() - t0 < 3.0:
        _o, _r, done, _i = orc.step(act); n += 1
        if done.any():
            orc.reset(mask=done)
    dt = time.time() - t0
    return dict(shape=shape, n_envs=N, env_steps_per_s=N * n / dt, threads=int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count())


def child(shape, N, kernels="crowd", lib=None, separate=False):
    """three processes (separate: three per kernel of `kernels`, the kernels alternating) -> {kernel: (min, max) us per launch}"""
    env = dict(os.environ)
    if lib:
        env["MADRL_HIP_LIB"] = lib
    rs = {}
    for _ in range(3):
        for ks in (kernels.split(",") if separate else [kernels]):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", shape, str(N), ks], env=env, capture_output=True, text=True,
                                 timeout=900)
            if out.returncode != 0:
                raise SystemExit("measurement %s N=%d %s failed (%d):\n%s" % (shape, N, ks, out.returncode, out.stderr[-2000:]))
            for line in out.stdout.strip().splitlines()[-len(ks.split(",")):]:
                r = json.loads(line)
                rs.setdefault(r["kernel"], []).append(r)
    res = {}
    for kind, rr in rs.items():
        us = [r["us_per_launch"] for r in rr]
        lo, hi = min(us), max(us)
        r = rr[0]
        scale = lambda key, u: r[key] * r["us_per_launch"] / u
        print("%-11s %-5s N=%7d  %9.1f - %9.1f us/launch  %.3e - %.3e env-steps/s  %.3e - %.3e ray tests/s  %.4f - %.4f of 8 TB/s%s" % (
            shape, kind, N, lo, hi, scale("env_steps_per_s", hi), scale("env_steps_per_s", lo), scale("ray_tests_per_s", hi),
            scale("ray_tests_per_s", lo), scale("hbm_share", hi), scale("hbm_share", lo), "  [%s]" % os.path.basename(lib) if lib else ""), flush=True)
        res[kind] = (lo, hi)
    return res


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        return one(argv[1], int(argv[2]), argv[3])
    rows = argv[argv.index("--rows") + 1].split(",") if "--rows" in argv else ["live"] if "--live" in argv else ["shapes", "cpu", "wave", "nw8"]
    if "shapes" in rows:
        for s, N in ROWS:
            child(s, N)
    if "cpu" in rows:
        for s in ("20/30/40", "33/10/20", "128/64/831", "3/10/5"):
            r = cpu(s)
            print("%-11s float32 C oracle, %d threads, N=%d: %.3e env-steps/s" % (s, r["threads"], r["n_envs"], r["env_steps_per_s"]), flush=True)
    if "wave" in rows:
        r = child("3/10/5", 32768, "crowd,wave")
        c, w = r["crowd"], r["wave"]
        print("3/10/5 at 32 768 envs: crowd / one-wavefront (specialised) = %.2f - %.2f" % (c[0] / w[1], c[1] / w[0]), flush=True)
    if "nw8" in rows:
        if not os.path.exists(NW8_LIB):
            raise SystemExit("no %s: build it with SRC=hostage_crowd MACRO=MADRL_HWC_NW scripts/variants.sh 8" % NW8_LIB)
        for s, N in ROWS[:3]:
            child(s, N)
            child(s, N, lib=NW8_LIB)
    if "live" in rows:
        for s in ("20/30/40", "33/10/20"):   # fixed, live at the capacity, live spread: alternating, a process each
            r = child(s, 4096, ",".join(LIVE_KINDS), separate=True)
            (f0, f1), (l0, l1), (s0, s1) = [r[k] for k in LIVE_KINDS]
            print("%s at 4 096 envs: live at the capacity / fixed = %.3f - %.3f, spread / live at the capacity = %.3f - %.3f" % (
                s, l0 / f1, l1 / f0, s0 / l1, s1 / l0), flush=True)


if __name__ == "__main__":
    main()
