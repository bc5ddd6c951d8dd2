"""Per-launch cost of a PursuitEvade step above 64 pursuers or evaders: the crowd kernel (pursuit_crowd.hpp, the XC lines of
pursuit_crowd_specializations.def) against the generic kernel the same shapes ran on before.

    python scripts/crowd_time.py --mode {crowd,generic} [--shape {cnn,cnn48,surround24,colocate20,wide24}] [--envs 1024] [--warmup 200] [--steps 200]
                                 [--live P E] [--to SLOTS]

  cnn         the authors' CNN launch line (runners/old/rllab/pursuit_cnn.sh:1): 100 v 300, obs_range 21, (R, R, 4) rows, --surround
              --sample_maps, local reward, on a ten-map 128 x 128 pool.  Their map_pool128.npy is not in their tree: the pool is
              madrl_amd.maps.resize(8, map_pool16), the 16 x 16 pool as recorded in tests/golden/pursuit_pool16_sample_maps.npz
  cnn48       the same rows on rectangle_map(48, 48)
  surround24  20 v 300, obs_range 9, flatten, open 24 x 24 map (windows at the border all the time)
  colocate20  260 v 40, obs_range 5, flatten, open 20 x 20 map, co-location catches, global reward
  wide24      70 v 90, obs_range 9, flatten, open 24 x 24 map

--live P E: the batch is built with per_env_counts=True (the shape's counts are then a capacity) and every env runs P pursuers and E evaders:
--mode crowd is then the live crowd kernel (the XLC lines of pursuit_live_specializations.def), --mode generic pursuit_live_kernel, and the
bytes are those of the live rows.

--to SLOTS: the two-buffer step, step_into(obs_out=) round a ring of SLOTS observation buffers (pursuit_crowd_to_kernel where the shape has
an XC line in pursuit_to_specializations.def, pursuit_to_kernel otherwise and with --mode generic); the JSON line names the kernel kind.

sample_maps as listed, max_steps=500, auto_reset=True; one launch per step through step_into.  Prints one JSON line: the HIP-event time per
step, the kernel that ran, the algorithmic bytes per env-step (bench.algorithmic_bytes_per_env_step: 708 229 B at the CNN shape) and the
share of the 8.0e12 B/s peak they amount to.  It needs a GPU; there is no fallback.  Run it under
`rocprofv3 --kernel-trace --stats -- python scripts/crowd_time.py ...` for the per-kernel figure (profiles/r09_crowd)."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CNN = dict(n_pursuers=100, n_evaders=300, obs_range=21, n_catch=2, surround=True, flatten=False, reward_mech="local")
SHAPES = {
    "cnn": ("pool128", dict(CNN, sample_maps=True)),
    "cnn48": ("rect48", CNN),
    "surround24": ("open24", dict(n_pursuers=20, n_evaders=300, obs_range=9, n_catch=2, surround=True, flatten=True, reward_mech="local")),
    "colocate20": ("open20", dict(n_pursuers=260, n_evaders=40, obs_range=5, n_catch=2, surround=False, flatten=True, reward_mech="global",
                                  catchr=0.1, urgency_reward=-0.05)),
    "wide24": ("open24", dict(n_pursuers=70, n_evaders=90, obs_range=9, n_catch=2, surround=True, flatten=True, reward_mech="local")),
}


def maps_of(name):
    import numpy as np
    from madrl_amd.maps import rectangle_map, resize
    if name == "pool128":
        return list(resize(8, np.load(glob.glob(os.path.join(ROOT, "tests", "golden", "pursuit_pool16_sample_maps.npz"))[0])["maps"]))
    if name == "rect48":
        return [rectangle_map(48, 48)]
    return [np.zeros((int(name[4:]), int(name[4:])), np.int32)]   # open24 / open20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=("crowd", "generic"))
    ap.add_argument("--shape", default="cnn", choices=sorted(SHAPES))
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--live", type=int, nargs=2, metavar=("P", "E"), default=None)
    ap.add_argument("--to", type=int, default=0, metavar="SLOTS")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("crowd_time.py needs a GPU")
    from bench import algorithmic_bytes_per_env_step
    from madrl_amd.pursuit import BatchedPursuitEvade
    mname, kw = SHAPES[a.shape]
    N, dev, P = a.envs, "cuda:0", kw["n_pursuers"]
    env = BatchedPursuitEvade(maps_of(mname), n_envs=N, device=dev, seed=0, max_steps=500, auto_reset=True,
                              kernel="wave" if a.mode == "crowd" else "generic",   # "wave" raises where no crowd kernel was compiled
                              **(dict(kw, per_env_counts=True) if a.live else kw))
    if a.live:
        env.set_agent_counts(a.live[0], a.live[1])   # pending: the reset below takes them
    env.reset()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    acts = [torch.randint(0, 5, (N, P), device=dev, dtype=torch.int32, generator=gen) for _ in range(8)]
    rew = torch.zeros((N, P), dtype=torch.float32, device=dev)
    done = torch.zeros(N, dtype=torch.uint8, device=dev)
    ring = [env.obs_buffer] + [torch.zeros_like(env.obs_buffer) for _ in range(a.to - 1)] if a.to else None

    def step(i):
        if ring is None:
            env.step_into(acts[i % 8], rew, done)
        else:
            env.step_into(acts[i % 8], rew, done, obs_out=ring[(i + 1) % len(ring)])

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(a.steps):
        step(i)
    t1.record()
    torch.cuda.synchronize()
    us = 1e3 * t0.elapsed_time(t1) / a.steps
    nbytes = algorithmic_bytes_per_env_step(a.live[0] if a.live else P, kw["n_evaders"], env.obs_dim, env.record_bytes)
    print(json.dumps(dict(mode=a.mode, shape=a.shape, envs=N, **(dict(live=a.live) if a.live else {}), kernel_kind=env.kernel_kind,
                          **(dict(step_to_kernel=env.step_to_kernel_kind, slots=a.to) if a.to else {}), us_per_step=round(us, 2),
                          algorithmic_bytes_per_env_step=nbytes, share_of_8e12=round(nbytes * N / (us * 1e-6) / 8.0e12, 4))))


if __name__ == "__main__":
    main()
