"""What tests/test_waterworld_gpu.py and tests/test_waterworld_specialised_gpu.py (and the latter's CPU companion) share: a plain module,
not collected.  Importing it needs no GPU.
  * vs_f32_oracle: a seeded rollout of BatchedMAWaterWorld under auto-reset against the float32 build of the C oracle;
  * SPEC_SHAPES: the test lines of csrc/waterworld_specializations.def as configurations, with the physics each one needs for its run
    to catch evaders and poison and to end episodes;
  * oracle_run: the oracle's side of such a run alone, computed once per configuration and shared (left unchanged by its users)."""
import functools

import numpy as np

DEV = "cuda:0"
TOL = 1e-5  # BASELINE.json north_star: "within 1e-5 for Waterworld ... float32 state"


def mk(n_envs, **kw):
    from madrl_amd.waterworld import BatchedMAWaterWorld
    return BatchedMAWaterWorld(n_envs=n_envs, device=DEV, **kw)


def vs_f32_oracle(kw, teacher_forced, N=256, T=60, H=20, env_kw=None, mask_reset_at=None, bits=False, each_launch=None):
    """Seeded rollout with auto-reset against the float32 oracle: same statement order, their own Philox on both sides.
    teacher_forced: the kernel takes the oracle's state at the start of every step (a divergence cannot compound: the comparison of each
    step stands on its own, tolerance 1e-5 as north_star asks).  Otherwise NOTHING is ever copied across: 60 steps, resets, respawns and
    random obstacles included, must stay identical in every bit of every output and of the state -- one flipped `<=` would show.
    What the callers of the specialised shapes add, all off by default: env_kw (constructor arguments of the env alone, max_blocks);
    mask_reset_at (a step index before which both sides reset(mask=) every third env, the rows compared); bits (observations, rewards,
    positions, velocities and the obstacle compared as 32-bit patterns: a zero of the other sign or another NaN fails); each_launch(env,
    where) called after the reset and after every launch.  -> the oracle's totals: evader catches, poison catches, episode ends."""
    from oracle import waterworld as ww
    env = mk(N, seed=77, env_id_base=500, max_steps=H, auto_reset=True, **dict(kw, **(env_kw or {})))
    orc = ww.WaterworldOracle(n_envs=N, seed=77, env_id_base=500, max_steps=H, dtype=np.float32, **kw)
    tol = TOL if teacher_forced else 0.0

    def close(got, want):
        got = np.ascontiguousarray(got.cpu().numpy())
        if bits:
            return np.array_equal(got.view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32))
        return np.abs(got - want).max() <= tol

    obs = env.reset()
    oobs = orc.reset()
    if each_launch:
        each_launch(env, "reset")
    assert close(obs, oobs)
    assert np.abs(obs.cpu().numpy() - oobs).max() <= tol
    rng = np.random.RandomState(1)
    exact = total = 0
    catches = 0
    totals = np.zeros(3, np.int64)
    for t in range(T):
        if t == mask_reset_at:
            mask = np.arange(N) % 3 == 0
            got = env.reset(mask=mask)
            if each_launch:
                each_launch(env, "reset(mask=) before step %d" % t)
            assert close(got, orc.reset(mask=mask)), "reset(mask=) before step %d" % t
        if teacher_forced:
            st = orc.get_state()
            env.set_state(pos=st["pos"], vel=st["vel"], obst=st["obst"], t=st["t"], tick=st["tick"].view(np.int32))
        act = rng.uniform(-1, 1, size=(N, kw["n_pursuers"], 2)).astype(np.float32)
        obs, rew, done, info = env.step(act)
        if each_launch:
            each_launch(env, "step %d" % t)
        oobs, orew, odone, oinfo = orc.step(act)
        assert np.array_equal(done.cpu().numpy(), odone.astype(bool)), "done step %d" % t
        assert np.array_equal(info["evcatches"].cpu().numpy(), oinfo[:, 0]), "evcatches step %d" % t
        assert np.array_equal(info["pocatches"].cpu().numpy(), oinfo[:, 1]), "pocatches step %d" % t
        assert np.abs(rew.cpu().numpy() - orew).max() <= tol, "rewards step %d" % t
        assert close(rew, orew), "rewards step %d" % t
        catches += int(oinfo.sum())
        totals += (int(oinfo[:, 0].sum()), int(oinfo[:, 1].sum()), int(odone.astype(bool).sum()))
        if odone.any():
            orc.reset(mask=odone)
        got = obs.cpu().numpy()
        assert np.abs(got - orc.obs).max() <= tol, "obs step %d: %g" % (t, np.abs(got - orc.obs).max())
        assert close(obs, orc.obs), "obs step %d" % t
        gst = env.get_state()
        ost = orc.get_state()
        assert np.abs(gst["pos"].cpu().numpy() - ost["pos"]).max() <= tol
        assert np.abs(gst["vel"].cpu().numpy() - ost["vel"]).max() <= tol
        assert close(gst["pos"], ost["pos"]) and close(gst["vel"], ost["vel"]), "state step %d" % t
        if bits:
            assert close(gst["obst"], ost["obst"]), "obstacle step %d" % t
        assert np.array_equal(gst["t"].cpu().numpy(), ost["t"])
        assert np.array_equal(gst["tick"].cpu().numpy().view(np.uint32), ost["tick"])
        exact += int(np.array_equal(got, orc.obs)); total += 1
    assert catches > 0, "no catches"
    print("bit-identical observation batches: %d / %d" % (exact, total))
    return tuple(int(v) for v in totals)


# ------------------------------------------------------------------ the test lines of csrc/waterworld_specializations.def
# Every run of a test shape: 64 envs, 40 steps, max_steps 15 under auto-reset (RUN), seed and env ids as vs_f32_oracle sets them.
RUN = dict(N=64, T=40, H=15)
FAST = dict(radius=0.03, ev_speed=0.04, action_scale=0.05)   # large and fast particles: catches and respawns within a few steps
# name -> (the line X(Np, Ne, Npo, K, D), the constructor arguments that give it, physics included)
SPEC_SHAPES = {
    "nospeed_noid_3_9_4_k12": ((3, 9, 4, 12, 50), dict(FAST, n_pursuers=3, n_evaders=9, n_poison=4, n_sensors=12, speed_features=False, addid=False,
                                                        sensor_range=0.3)),
    "k64_noid_2_3_2": ((2, 3, 2, 64, 450), dict(FAST, n_pursuers=2, n_evaders=3, n_poison=2, n_sensors=64, addid=False, n_coop=1)),
    "k1_3_3_3": ((3, 3, 3, 1, 10), dict(FAST, n_pursuers=3, n_evaders=3, n_poison=3, n_sensors=1, n_coop=1)),
    "k256_2_2_2": ((2, 2, 2, 256, 1795), dict(FAST, n_pursuers=2, n_evaders=2, n_poison=2, n_sensors=256, n_coop=1, obstacle_loc=None)),
    "words4_8_30_16": ((8, 30, 16, 8, 59), dict(FAST, n_pursuers=8, n_evaders=30, n_poison=16, n_sensors=8, reward_mech="global")),
    "bytes_10_30_16": ((10, 30, 16, 6, 45), dict(FAST, n_pursuers=10, n_evaders=30, n_poison=16, n_sensors=6, n_coop=3)),
    "class40_2_40_3": ((2, 40, 3, 8, 59), dict(FAST, n_pursuers=2, n_evaders=40, n_poison=3, n_sensors=8, n_coop=1)),
    "full_32_16_14": ((32, 16, 14, 4, 31), dict(FAST, n_pursuers=32, n_evaders=16, n_poison=14, n_sensors=4, reward_mech="global",
                                                obstacle_loc=None)),
    # (n_coop=1: one pursuer alone catches no evader under the default n_coop=2 -- the oracle counts 0 evader catches there, 53 here)
    "ones_1_1_1": ((1, 1, 1, 30, 213), dict(FAST, n_pursuers=1, n_evaders=1, n_poison=1, n_sensors=30, radius=0.06, n_coop=1)),
}
MASK_RESET_AT = 20   # the runs that reset(mask=) every third env do so before this step


@functools.lru_cache(maxsize=None)
def oracle_run(name, mask_reset_at=None):
    """the float32 oracle's side of the run of a test shape, alone and once per process: (actions [T, N, Np, 2], evader catches, poison
    catches, episode ends).  The actions are vs_f32_oracle's draws and mask_reset_at is its argument; nothing of the result may be changed
    by a caller."""
    from oracle import waterworld as ww
    kw = SPEC_SHAPES[name][1]
    N, T, H = RUN["N"], RUN["T"], RUN["H"]
    orc = ww.WaterworldOracle(n_envs=N, seed=77, env_id_base=500, max_steps=H, dtype=np.float32, **kw)
    orc.reset()
    rng = np.random.RandomState(1)
    acts = np.zeros((T, N, kw["n_pursuers"], 2), np.float32)
    ev = po = ends = 0
    for t in range(T):
        if t == mask_reset_at:
            orc.reset(mask=np.arange(N) % 3 == 0)
        acts[t] = rng.uniform(-1, 1, size=acts[t].shape).astype(np.float32)
        _obs, _rew, done, info = orc.step(acts[t])
        ev, po, ends = ev + int(info[:, 0].sum()), po + int(info[:, 1].sum()), ends + int(done.astype(bool).sum())
        if done.any():
            orc.reset(mask=done)
    acts.setflags(write=False)
    return acts, ev, po, ends


def exercised(ev, po, ends, what=""):
    """the conditions every run of a test shape has to meet, on the oracle's numbers: evaders and poison were caught (respawns ran), and at
    least as many episodes ended as there are envs (the fused auto-reset pass ran)"""
    assert ev > 0 and po > 0 and ends >= RUN["N"], "%s: %d evader catches, %d poison catches, %d episode ends" % (what, ev, po, ends)
