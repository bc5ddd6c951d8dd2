"""GPU tests (-m gpu): the Philox counter words of the env kernels and the device policy across 2^31 and 2^32.

The per-env `tick` is a uint32 (get_state / set_state carry it as int32); the global env index env_id_base + env is the other 32-bit
counter word (check_env_ids accepts env_id_base + n_envs up to 2^32 - 1).  Every other test starts ticks at 0 and uses a base of at most
1 000, so neither word ever had bit 31 set, and no tick ever wrapped.

130 envs on 3 workgroups, max_steps 5 with auto-reset, 24 steps of seeded actions, free-running and bit for bit against the C oracle
after every step (observations, rewards, done bits, removed, every state key, the tick as uint32):

  * tick: set_state(tick=) on kernel and oracle alike, start ticks spread over 2^31 - 12 .. 2^31 - 1 in one run and 2^32 - 12 .. 2^32 - 1
    in the other -- different envs cross the line at different steps, some inside a fused reset's second pass;
  * env_id_base: 2^31 - 65 (the global index straddles bit 31 inside the batch, inside one workgroup's walk) and 2^32 - 1 - N, the largest
    base accepted; one more is refused; StreamSharded over a base that puts the 2^31 line between its two sub-batches.

The same for the Waterworld kernels (one wavefront, live counts, per-pursuer ranges, crowd) and the hostage world's (one wavefront, crowd)
against their float32 oracles; for MultiWalker, whose only counter word of this kind is the global env index (terrain and push draws), all
three capacity classes in both launch modes against the CPU build, whole world records; and the device policy's draw counter across its
wrap.  Each case asserts the kernel it ran on."""
import numpy as np
import pytest
import torch

import wide
from wide import PursuitCase

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, BLOCKS, H, T = 130, 3, 5, 24
GENERIC = ("generic", "generic", "generic")
HEAD, AUTHORS = (16, 16, 8, 30, 7, 1), (32, 32, 30, 50, 11, 1)

KERNELS = {
    "wave": PursuitCase("rect", (16, 16, 13, 51, 7, 1)),
    "fixed": PursuitCase("rect", (8, 8, 5, 6, 5, 1), kinds=("wave", "wave", "fixed")),
    "group": PursuitCase("rect", (16, 16, 20, 50, 5, 1)),
    "crowd": PursuitCase("open", (24, 24, 20, 300, 9, 1)),
    "generic": PursuitCase("rect", HEAD, kernel="generic", kinds=GENERIC),
    "wave_two_buffer": PursuitCase("rect", HEAD, mode="step_to"),
    "wave_half": PursuitCase("rect", HEAD, mode="half"),
    "group_two_buffer": PursuitCase("rect", AUTHORS, mode="step_to"),
    "group_half": PursuitCase("rect", AUTHORS, mode="half"),
}


def _free_run(case, monkeypatch, base=None, first_tick=None):
    """-> (the run, the oracle's ticks before the first step and after the last)"""
    run = wide.Run(case, N, 0, H, monkeypatch, base=base, max_blocks=BLOCKS)
    orc = wide.PursuitProbeOracle(case, N, 0, H, base=base)
    run.reset()
    orc.reset(run.env)
    if first_tick is not None:
        tick = ((first_tick + np.arange(N) % 12) & 0xFFFFFFFF).astype(np.uint32)
        run.env.set_state(dict(tick=torch.from_numpy(tick.view(np.int32)).to(DEV)))
        orc.set_tick(tick)
    before = orc.ticks().astype(np.int64)
    rng = np.random.RandomState(9)
    for t in range(T):
        act = rng.randint(5, size=(N, case.P)).astype(np.int32)
        run.step(torch.as_tensor(act, device=DEV))
        run.check_kinds("step %d" % t)
        orc.step(run.env, act, "step %d" % t)   # (every state key and the tick as uint32 among it)
    assert bool((orc.resets >= T // H).all()), "every env went through the fused reset several times"
    return run, before, orc.ticks().astype(np.int64)


@pytest.mark.parametrize("line", [2**31, 2**32], ids=["2^31", "2^32"])
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_tick_crosses_the_line(name, line, monkeypatch):
    run, before, after = _free_run(KERNELS[name], monkeypatch, first_tick=line - 12)
    assert before.min() == line - 12 and before.max() == line - 1
    moved = (after - before) % 2**32
    assert bool((moved >= T + T // H).all()), "a step and a fused reset each advance the tick"
    crossed = (before + moved >= line)
    assert bool(crossed.all()), "%d envs did not cross" % int((~crossed).sum())
    if line == 2**32:
        assert after.max() <= 2 * T, "the tick wraps to small values"
    else:
        assert after.min() >= 2**31
        assert int(run.env.get_state()["tick"].max()) < 0, "get_state() hands the tick out as int32: bit 31 is its sign"
    wide.free_device()


@pytest.mark.parametrize("base", [2**31 - 65, 2**32 - 1 - N], ids=["straddles_2^31", "largest"])
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_global_env_index_with_bit_31_set(name, base, monkeypatch):
    _free_run(KERNELS[name], monkeypatch, base=base)
    wide.free_device()


def test_env_id_base_does_matter_and_one_more_than_the_largest_is_refused(monkeypatch):
    """the cases above would pass on a kernel that dropped env_id_base altogether if the oracle did too: two bases 2^31 apart must differ"""
    from madrl_amd import _lib
    case = KERNELS["wave"]
    lo, hi = wide.Run(case, N, 0, H, monkeypatch, base=7), wide.Run(case, N, 0, H, monkeypatch, base=7 + 2**31)
    assert not wide.bits_equal(lo.reset(), hi.reset()), "bit 31 of the global env index does not reach the Philox counter"
    for name in ("wave", "crowd", "generic"):
        with pytest.raises(_lib.MadrlError, match="global env index must fit 32 bits"):
            KERNELS[name].make(N, 0, H, monkeypatch, base=2**32 - N)
    wide.free_device()


def test_stream_sharded_with_the_2_31_line_between_its_sub_batches(monkeypatch):
    from madrl_amd.sharded import StreamSharded
    case = PursuitCase("rect", HEAD, walk="forward", kinds=("wave", "wave", "fixed"))
    base = 2**31 - N // 2

    def make_env(n_envs, env_id_base, device):
        env = case.make(n_envs, env_id_base - base, H, monkeypatch, base=base)
        env.set_launch(max_blocks=BLOCKS)
        return env

    sh = StreamSharded(make_env, N, n_streams=2, env_id_base=base, device=DEV)
    assert sh.envs[0].env_id_base + sh.per == 2**31 == sh.envs[1].env_id_base
    orcs = [wide.PursuitProbeOracle(case, sh.per, j * sh.per, H, base=base) for j in range(2)]
    sh.reset()
    for env, orc in zip(sh.envs, orcs):
        orc.reset(env)
    rng = np.random.RandomState(3)
    for t in range(T):
        act = rng.randint(5, size=(N, case.P)).astype(np.int32)
        sh.step(torch.as_tensor(act, device=DEV))
        torch.cuda.synchronize()
        for j, (env, orc) in enumerate(zip(sh.envs, orcs)):
            assert env.last_step_entry == "fixed"
            orc.step(env, act[j * sh.per:(j + 1) * sh.per], "step %d, sub-batch %d" % (t, j))
    wide.free_device()


# ------------------------------------------------------------------------------------------------------ Waterworld and the hostage world
WW = dict(n_pursuers=5, n_evaders=10, n_poison=10, n_coop=2, n_sensors=30, radius=0.03, ev_speed=0.03, action_scale=0.03)   # the compiled 5 / 10 / 10 shape
RANGES = np.array([0.2, 0.35, 0.2, 0.35, 0.2])
HW = dict(n_sensors=8, action_scale=0.03, bad_speed=0.03, radius=0.03)
HW_ARGS = (3, 10, 5, 2, 2)


def _ww(kind, base):
    """-> (env, [(oracle, the observation rows it speaks for)]): row i of a ranged batch is row i of a batch with sensor_range[i]"""
    from madrl_amd.waterworld import BatchedMAWaterWorld
    from oracle import waterworld as ww
    extra = {"wave": {}, "wave_live": dict(per_env_counts="wave"), "ranged": dict(sensor_range=RANGES), "crowd": dict(crowd=True)}[kind]
    env = BatchedMAWaterWorld(n_envs=N, device=DEV, seed=77, env_id_base=base, max_steps=H, auto_reset=True, max_blocks=BLOCKS, **dict(WW, **extra))
    assert env.kernel_kind == ("crowd" if kind == "crowd" else "wave") and env.per_env_counts == (kind == "wave_live") and env._ranged == (kind == "ranged")
    mk = lambda **kw: ww.WaterworldOracle(n_envs=N, seed=77, env_id_base=base, max_steps=H, dtype=np.float32, **dict(WW, **kw))
    if kind == "ranged":
        return env, [(mk(sensor_range=float(r)), np.nonzero(RANGES == r)[0]) for r in sorted(set(RANGES.tolist()))]
    return env, [(mk(), np.arange(WW["n_pursuers"]))]


def _hw(kind, base):
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    from oracle import hostage as ho
    env = BatchedContinuousHostageWorld(*HW_ARGS, n_envs=N, device=DEV, seed=77, env_id_base=base, max_steps=H, auto_reset=True, max_blocks=BLOCKS,
                                        crowd=(kind == "crowd"), **HW)
    assert env.kernel_kind == kind
    return env, [(ho.HostageOracle(*HW_ARGS, n_envs=N, seed=77, env_id_base=base, max_steps=H, dtype=np.float32, **HW), np.arange(HW_ARGS[0]))]


PARTICLE = {"waterworld_" + k: (_ww, k) for k in ("wave", "wave_live", "ranged", "crowd")}
PARTICLE.update({"hostage_" + k: (_hw, k) for k in ("wave", "crowd")})


def _particle_free_run(name, base=500, first_tick=None):
    """the free-running comparison of tests/wide.py (particle_oracle_step) on a small batch.  -> the env, the ticks (int64) before the first
    step and after the last, the info events"""
    make, kind = PARTICLE[name]
    env, orcs = make(kind, base)
    n_agents = env._obs.shape[1]
    env.reset()
    for orc, _rows in orcs:
        orc.reset()
    wide.assert_particle_probe_equals_oracle(env, orcs, "reset")
    if first_tick is not None:
        tick = ((first_tick + np.arange(N) % 12) & 0xFFFFFFFF).astype(np.uint32)
        env.set_state(tick=torch.from_numpy(tick.view(np.int32)).to(DEV))
        for orc, _rows in orcs:
            orc.set_state(tick=tick)
    before = orcs[0][0].get_state()["tick"].astype(np.int64)
    rng = np.random.RandomState(1)
    n_done = events = 0
    for t in range(T):
        act = rng.uniform(-1, 1, size=(N, n_agents, 2)).astype(np.float32)
        env.step(act)
        d, ev = wide.particle_oracle_step(env, orcs, act, "step %d" % t)
        n_done, events = n_done + d, events + ev
    assert n_done >= N * (T // H), "every env went through the fused reset several times"
    return env, before, orcs[0][0].get_state()["tick"].astype(np.int64), events


@pytest.mark.parametrize("line", [2**31, 2**32], ids=["2^31", "2^32"])
@pytest.mark.parametrize("name", sorted(PARTICLE))
def test_particle_world_tick_crosses_the_line(name, line):
    env, before, after, _events = _particle_free_run(name, first_tick=line - 12)
    assert before.min() == line - 12 and before.max() == line - 1
    moved = (after - before) % 2**32
    assert bool((moved >= T + T // H).all()), "a step and a fused reset each advance the tick"
    assert bool((before + moved >= line).all()), "an env did not cross"
    if line == 2**32:
        assert after.max() <= 2 * T, "the tick wraps to small values"
    else:
        assert after.min() >= 2**31 and int(env.get_state()["tick"].max()) < 0
    wide.free_device()


@pytest.mark.parametrize("base", [2**31 - 65, 2**32 - 1 - N], ids=["straddles_2^31", "largest"])
@pytest.mark.parametrize("name", sorted(PARTICLE))
def test_particle_world_global_env_index_with_bit_31_set(name, base):
    _particle_free_run(name, base=base)
    wide.free_device()


def test_particle_worlds_refuse_one_more_than_the_largest_base_and_bit_31_matters():
    from madrl_amd import _lib
    for name in ("waterworld_wave", "waterworld_crowd", "hostage_wave", "hostage_crowd"):
        make, kind = PARTICLE[name]
        with pytest.raises(_lib.MadrlError, match="global env index must fit 32 bits"):
            make(kind, 2**32 - N)
        lo, hi = make(kind, 7)[0], make(kind, 7 + 2**31)[0]
        assert not wide.bits_equal(lo.reset(), hi.reset()), name + ": bit 31 of the global env index does not reach the Philox counter"
    wide.free_device()


# ------------------------------------------------------------------------------------------------------------------ MultiWalker
@pytest.mark.parametrize("base", [2**31 - 65, 2**32 - 1 - N], ids=["straddles_2^31", "largest"])
@pytest.mark.parametrize("fused", [False, True], ids=["three_launches", "one_launch"])
@pytest.mark.parametrize("n_walkers", sorted(wide.MW_LANES))
def test_multiwalker_global_env_index_with_bit_31_set(n_walkers, fused, base):
    """all three capacity classes against the CPU build of the same source created with the same base (which tests/test_wide_counters_cpu.py
    holds against the independent restatement there): whole world records byte for byte, auto-reset through spares"""
    env, orc = wide.mw_make(N, n_walkers, fused, H, base), wide.MwProbeOracle(N, n_walkers, H, base)
    env.reset()
    orc.reset(env)
    rng = np.random.RandomState(6)
    for t in range(T):
        act = rng.uniform(-1, 1, (N, n_walkers, 4)).astype(np.float32)
        env.step(act)
        orc.step(env, act, "step %d" % t)
    assert orc.resets >= N * (T // H)
    wide.free_device()


def test_multiwalker_refuses_one_more_than_the_largest_base_and_bit_31_matters():
    from madrl_amd import _lib
    with pytest.raises(_lib.MadrlError, match="global env index must fit 32 bits"):
        wide.mw_make(N, 3, False, H, 2**32 - N)
    lo, hi = wide.mw_make(N, 3, False, H, 7), wide.mw_make(N, 3, False, H, 7 + 2**31)
    lo.reset(), hi.reset()
    assert not torch.equal(lo.get_state()["terrain"], hi.get_state()["terrain"]), "bit 31 of the global env index does not reach the terrain draws"
    wide.free_device()


# ------------------------------------------------------------------------------------------------------------------ the device policy
@pytest.mark.parametrize("flatten", [True, False])
def test_policy_draw_counter_wraps_at_2_32_with_row_ids_that_straddle_2_31(flatten):
    """PursuitHeuristicPolicy keeps its draw counter on the device (int32 words): set to -3, that is 2^32 - 3, six calls draw at ticks
    2^32 - 3 .. 2^32 - 1, 0, 1, 2.  row_id_base puts the 2^31 line of the row id's low word inside the launch.  Against the host
    recomputation of tests/test_policy_edges_gpu.py (oracle/heuristics_oracle.py for the rows that do not draw, Philox on the host for
    those that do)."""
    import test_policy_edges_gpu as pe
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    n, seed = 400, (7 << 32) | 5
    base = 2**31 - n // 2
    win, ref = pe._draw_windows(n, 300)
    drawn = np.flatnonzero(ref < 0)
    assert base + drawn[0] < 2**31 <= base + drawn[-1]
    obs = pe._pursuit_obs(win, flatten)
    pol = PursuitHeuristicPolicy(7, flatten=flatten, seed=seed, row_id_base=base)
    pe._pursuit_call(pol, obs)   # (the counter exists after the first call)
    pol._tick[0] = -3
    seen = []
    for k in range(6):
        tick = (2**32 - 3 + k) % 2**32
        want = ref.copy()
        want[drawn] = pe._draws(seed, base, drawn, tick)
        a = pe._pursuit_call(pol, obs)
        assert np.array_equal(a, want), (tick, np.flatnonzero(a != want)[:5])
        seen.append(want[drawn])
    assert int(pol._tick[0]) == 3 and len(set(map(bytes, seen))) == 6
