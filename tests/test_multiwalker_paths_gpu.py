"""GPU tests (-m gpu) for the MultiWalker kernels in the configuration bench.py measures and the collector drives -- beyond whole
wavefronts, one stream, noise 0 and the env's own buffers, which is where tests/test_multiwalker_gpu.py stays:

(1) ragged and tiny batches (part of a wavefront gone in the live-step path) against the CPU build of the same source;
(2) observation noise on, through the three routes that produce an episode's first observation (reset / reset(mask), the spare record built
    ahead of time, the second launch of a step): the draws are keyed by (env id, episode, tick, walker, draw), and all routes must use one key;
(3) four sub-batches on their own HIP streams (StreamSharded) against one batch and the CPU build;
(4) a whole horizon as a replayed hipGraph against the eager collector, and the spare cycle's bookkeeping at the end of the state tensor;
(5) caller destinations of step() (rew_out / done_out / obs_out).

The oracle is oracle.multiwalker.MultiWalkerOracle (oracle/multiwalker_oracle.cpp: the kernel source compiled for the host, the lanes one
after the other); auto-reset is emulated with orc.reset(mask=ends).  Each oracle run is made once per case and shared by the launch forms
and spare modes compared against it; every event count asserted here is computed from the oracle alone.

Tolerances.  World records, rewards, done bits and every observation column the noise does not enter: equal in every bit.  The seven noisy
columns (24 .. 30 of a 32-wide row: neighbour offsets, package offset and angle) are compared within 1e-6 * max(1, |oracle|), the bound
tests/test_multiwalker_envlayer.py uses for the kernels' float32 outputs: the draws go through logf / sqrtf, whose last place may differ
between the host's libm and the device's.  The largest difference seen is printed by every noisy test."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPW = {3: 16, 6: 8, 10: 4}            # envs per wavefront of the capacity class a walker count runs on (64 / lanes per env)
RAGGED = {W: (1, e - 1, e + 1, 2 * e + 3) for W, e in EPW.items()}   # 1/15/17/35, 1/7/9/19, 1/3/5/11
NOISY = slice(24, 31)
NOISE = 0.05                          # fifty times the constructor's default: a draw from a wrong key is off by ~1e-2, not ~1e-4
T_STEPS = 40
_worst = [0.0]                        # largest |kernel - oracle| seen in the noisy columns


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _actions(rng, t, N, W):
    act = rng.uniform(-1, 1, (N, W, 4)).astype(np.float32)
    if t % 25 > 17:
        act[:] = 0
    return act


class Trace(object):
    """one oracle run: per step the actions, rewards, (fell | 2 * time limit), and -- after reset(mask=ends) -- observations and world records"""


@functools.lru_cache(maxsize=4)
def _trace(W, N, horizon, noise, seed, base, act_seed, T=T_STEPS):
    from oracle import multiwalker as mwo
    orc = mwo.MultiWalkerOracle(n_walkers=W, position_noise=noise, angle_noise=noise, n_envs=N, seed=seed, env_id_base=base)
    tr = Trace()
    tr.W, tr.N, tr.horizon, tr.world_bytes = W, N, horizon, orc.world_bytes
    tr.obs0, tr.worlds0 = orc.reset().copy(), orc.worlds()
    rng = np.random.RandomState(act_seed)
    tstep = np.zeros(N, np.int64)
    last = np.zeros(N, bool)
    tr.steps, tr.n_ends, tr.n_falls, tr.n_back_to_back = [], 0, 0, 0
    for t in range(T):
        act = _actions(rng, t, N, W)
        _, orew, odone = orc.step(act)
        tstep += 1
        fell = odone.astype(bool)
        cut = (tstep >= horizon) if horizon else np.zeros(N, bool)
        ends = fell | cut
        rew = orew.copy()
        if ends.any():
            orc.reset(mask=ends.astype(np.uint8))
            tstep[ends] = 0
        tr.n_ends += int(ends.sum()); tr.n_falls += int(fell.sum()); tr.n_back_to_back += int((ends & last).sum())
        last = ends
        tr.steps.append((act, rew, fell.astype(np.uint8) | (cut.astype(np.uint8) << 1), orc.obs.copy(), orc.worlds()))
    return tr


def _check_obs(got, want, noisy, what):
    """noise-free columns in every bit; the noisy ones (when noise is on) within 1e-6 * max(1, |oracle|)"""
    if not noisy:
        assert np.array_equal(_bits(got), _bits(want)), "%s: observations" % what
        return
    quiet = np.ones(got.shape[-1], bool)
    quiet[NOISY] = False
    assert np.array_equal(_bits(got[..., quiet]), _bits(want[..., quiet])), "%s: observation columns the noise does not enter" % what
    d = np.abs(got[..., NOISY].astype(np.float64) - want[..., NOISY].astype(np.float64))
    _worst[0] = max(_worst[0], float(d.max()))
    bound = 1e-6 * np.maximum(1.0, np.abs(want[..., NOISY].astype(np.float64)))
    assert (d <= bound).all(), "%s: noisy observation columns, max |d| = %g" % (what, d.max())


def _check_step(what, step, obs, rew, done_bits, worlds, noisy):
    act, orew, obits, oobs, oworlds = step
    assert np.array_equal(done_bits & 3, obits), "%s: which episodes ended (bit 0) / ran into the time limit (bit 1)" % what
    assert np.array_equal(_bits(rew), _bits(orew)), "%s: rewards" % what
    _check_obs(obs, oobs, noisy, what)
    if worlds is not None:
        same = (worlds[:, :oworlds.shape[1]] == oworlds).all(axis=1)
        assert same.all(), "%s: world records of envs %s differ" % (what, np.nonzero(~same)[0].tolist())


def _mk(W, N, **kw):
    from madrl_amd.multiwalker import BatchedMultiWalkerEnv
    return BatchedMultiWalkerEnv(n_walkers=W, n_envs=N, device=DEV, **kw)


def _spare_tail(env):
    """(ready_step [N], dirty_list [2, N], the four dwords behind them) from the end of the env's state tensor, as mw_layout (madrl_amd/csrc/multiwalker_layout.hpp)
    lays it out -- after checking that layout against madrl_multiwalker_state_bytes"""
    from madrl_amd import _lib
    N, W = env.n_envs, int(env.n_walkers)
    up16 = lambda x: (x + 15) // 16 * 16
    tail = 12 * N + 16
    total = C.c_uint64()
    cfg = env._config()
    _lib.check(_lib.lib().madrl_multiwalker_state_bytes(C.byref(cfg), N, C.byref(total)))
    assert total.value == env._state.numel() == 2 * N * env.record_stride + up16(N) + up16(4 * N * W * env.obs_dim) + tail, "layout of the state tensor"
    t = env._state[-tail:].view(torch.int32).cpu().numpy().view(np.uint32)
    return t[:N], t[N:3 * N].reshape(2, N), t[3 * N:]


def _check_spare_cycle(env, ended_now, ended_before, what):
    """after a step() call, an env whose episode ended in neither of the last two calls has a finished spare: ready_step neither 0 (stale,
    waiting on a list) nor 0xFFFFFFFF (being built)"""
    ready = _spare_tail(env)[0]
    settled = ~(ended_now | ended_before)
    bad = settled & ((ready == 0) | (ready == 0xFFFFFFFF))
    assert not bad.any(), "%s: envs %s are out of the spare cycle (ready_step %s)" % (what, np.nonzero(bad)[0].tolist(), ready[bad].tolist())


def _run_auto_reset(env, tr, noisy, what, T=None, spare_cycle=False):
    """env (auto_reset=True) through the trace's actions, every output and the world records against the trace at every step"""
    obs = env.reset()
    _check_obs(obs.cpu().numpy(), tr.obs0, noisy, what + " reset")
    assert (env.state_buffer.cpu().numpy()[:, :tr.world_bytes] == tr.worlds0).all(), what + ": world records after reset"
    before = np.zeros(tr.N, bool)
    for t, step in enumerate(tr.steps[:T]):
        obs, rew, done, info = env.step(torch.as_tensor(step[0], device=DEV))
        bits = info["done_bits"].cpu().numpy()
        assert np.array_equal(done.cpu().numpy(), (bits & 1) != 0)
        _check_step("%s step %d" % (what, t), step, obs.cpu().numpy(), rew.cpu().numpy(), bits, env.state_buffer.cpu().numpy(), noisy)
        now = step[2] != 0
        if spare_cycle:
            _check_spare_cycle(env, now, before, "%s step %d" % (what, t))
        before = now


# ------------------------------------------------------------------------------------------------ 1. ragged and tiny batches
# Under these actions no walker falls before its episode is about 30 steps old (counted on the oracle), so a short horizon alone ends every
# episode by the time limit.  Each class therefore also runs its largest ragged batch WITHOUT a horizon, for T_LONG steps: episodes that end by
# a fall, at different steps in different envs, each taking a spare that has been ready for a long time.
T_LONG = 64
P1 = dict(seed=21, base=5, act_seed=6)
CASES1 = [(W, N, 7, T_STEPS) for W in (3, 6, 10) for N in RAGGED[W]] + [(W, RAGGED[W][-1], 0, T_LONG) for W in (3, 6, 10)]
# (a horizon of 7 does not divide the step count: spares are consumed and rebuilt in ragged groups)


def _trace1(W, N, H, T):
    return _trace(W, N, H, 0.0, P1["seed"], P1["base"], P1["act_seed"] + N, T)


@pytest.mark.parametrize("use_spares", [True, False], ids=["spares", "second-launch"])
@pytest.mark.parametrize("fused", [False, True], ids=["three-launches", "one-launch"])
@pytest.mark.parametrize("W,N,H,T", CASES1)
def test_ragged_batches_match_the_cpu_build(W, N, H, T, fused, use_spares):
    """N in {1, EPW - 1, EPW + 1, 2 EPW + 3}: the last wavefront of the live blocks -- and, behind a horizon of 7, of the spare blocks -- runs
    the solver, the continuous pass and (sixteen-lane class) the record lookup by lane id with groups of lanes gone"""
    tr = _trace1(W, N, H, T)
    assert H == 0 or tr.n_ends >= N * (T // H)
    env = _mk(W, N, position_noise=0.0, angle_noise=0.0, seed=P1["seed"], env_id_base=P1["base"], auto_reset=True, max_steps=H)
    env.set_mode(fused=fused, use_spares=use_spares)
    _run_auto_reset(env, tr, False, "W=%d N=%d" % (W, N), spare_cycle=use_spares)


@pytest.mark.parametrize("W", [3, 6, 10])
def test_ragged_cases_hold_fall_ended_episodes(W):
    """the oracle alone: over the cases of a class, episodes end by a fall (or a dropped package) too, not by the time limit only"""
    assert sum(_trace1(*c).n_falls for c in CASES1 if c[0] == W) >= 1


# ------------------------------------------------------------------------------------------------ 2. noise through the reset routes
# Which route gives an episode its first observation, with spares on:
#   horizon 2   every env takes its spare in the call after the one that rebuilt it;
#   horizon 7   the same in ragged groups, several calls after the rebuild;
#   no horizon  (T_LONG steps) episodes end by falls, each env on its own;
#   horizon 1   every episode ends in the call right after its predecessor ended: the spare, being rebuilt by that same call, is never ready
#               and every auto-reset takes the second launch WHILE spares are rebuilt.  (A fall within an episode's first step would do the same;
#               under these actions the oracle shows none -- the earliest fall comes about 30 steps into an episode.)
# With use_spares=False every auto-reset takes the second launch.
P2 = dict(seed=33, base=9, act_seed=12)
N2 = {3: 17, 6: 19, 10: 11}    # one ragged batch per class
HORIZONS2 = (1, 2, 7, 0)


def _trace2(W, H):
    return _trace(W, N2[W], H, NOISE, P2["seed"], P2["base"], P2["act_seed"] + H, T_STEPS if H else T_LONG)


@pytest.mark.parametrize("use_spares", [True, False], ids=["spares", "second-launch"])
@pytest.mark.parametrize("fused", [False, True], ids=["three-launches", "one-launch"])
@pytest.mark.parametrize("H", HORIZONS2)
@pytest.mark.parametrize("W", [3, 6, 10])
def test_noisy_observations_through_spares_and_second_launch(W, H, fused, use_spares):
    """the draws of an episode's first observation are the same whichever route produced it, and equal to reset(mask)'s on the CPU build"""
    tr = _trace2(W, H)
    assert H == 0 or tr.n_ends >= tr.N * (len(tr.steps) // H)
    env = _mk(W, tr.N, position_noise=NOISE, angle_noise=NOISE, seed=P2["seed"], env_id_base=P2["base"], auto_reset=True, max_steps=H)
    env.set_mode(fused=fused, use_spares=use_spares)
    _run_auto_reset(env, tr, True, "W=%d horizon=%d" % (W, H), spare_cycle=use_spares)
    print("largest host/device difference in the noisy columns so far: %g" % _worst[0])


@pytest.mark.parametrize("W", [3, 6, 10])
def test_noisy_cases_hold_an_episode_without_a_ready_spare(W):
    """the oracle alone: in the runs above episodes end in the call right after their predecessor ended (no spare ready), and by falls"""
    assert sum(_trace2(W, H).n_back_to_back for H in HORIZONS2) >= 1
    assert sum(_trace2(W, H).n_falls for H in HORIZONS2) >= 1


@pytest.mark.parametrize("H", [7, 0])
@pytest.mark.parametrize("W", [3, 6, 10])
def test_noisy_observations_through_host_driven_reset(W, H):
    """the same comparison with reset(mask) called from the host where the episodes end (auto_reset off)"""
    tr = _trace2(W, H)
    env = _mk(W, tr.N, position_noise=NOISE, angle_noise=NOISE, seed=P2["seed"], env_id_base=P2["base"], auto_reset=False, max_steps=H)
    _check_obs(env.reset().cpu().numpy(), tr.obs0, True, "reset")
    for t, step in enumerate(tr.steps):
        obs, rew, done, info = env.step(torch.as_tensor(step[0], device=DEV))
        bits = info["done_bits"].cpu().numpy()
        rew = rew.cpu().numpy()
        if (bits & 3).any():
            obs = env.reset(mask=torch.as_tensor((bits & 3) != 0, device=DEV))
        _check_step("W=%d step %d" % (W, t), step, obs.cpu().numpy(), rew, bits, env.state_buffer.cpu().numpy(), True)
    print("largest host/device difference in the noisy columns so far: %g" % _worst[0])


@pytest.mark.parametrize("W", [3, 6, 10])
def test_env_of_a_batch_equals_a_one_env_batch_at_its_id(W):
    """sharding invariance with noise on: env n of a batch at env_id_base b is env 0 of a one-env batch at b + n -- same device, same code, so
    every bit of the observations too; over a reset, ten steps and (horizon 4) two auto-resets"""
    N, b = N2[W], 40
    kw = dict(position_noise=NOISE, angle_noise=NOISE, seed=8, auto_reset=True, max_steps=4)
    rng = np.random.RandomState(2)
    acts = [torch.as_tensor(rng.uniform(-1, 1, (N, W, 4)).astype(np.float32), device=DEV) for _ in range(10)]
    batch = _mk(W, N, env_id_base=b, **kw)
    ref = [[batch.reset().cpu().numpy().copy()]]
    for a in acts:
        obs, rew, done, info = batch.step(a)
        ref.append([x.cpu().numpy().copy() for x in (obs, rew, info["done_bits"], batch.state_buffer[:, :batch.world_bytes])])
    for n in (0, N // 2, N - 1):
        one = _mk(W, 1, env_id_base=b + n, **kw)
        assert np.array_equal(_bits(one.reset().cpu().numpy()[0]), _bits(ref[0][0][n])), "env %d: reset observation" % n
        for t, a in enumerate(acts):
            obs, rew, done, info = one.step(a[n:n + 1])
            got = [x.cpu().numpy() for x in (obs, rew, info["done_bits"], one.state_buffer[:, :one.world_bytes])]
            for g, r, name in zip(got, ref[t + 1], ("observations", "rewards", "done bits", "world record")):
                assert np.array_equal(_bits(g[0]), _bits(r[n])), "env %d step %d: %s" % (n, t, name)


# ------------------------------------------------------------------------------------------------ 3. sub-batches on streams
@pytest.mark.parametrize("W,per", [(3, 19), (6, 9), (10, 5)])
def test_four_sub_batches_on_streams_equal_one_batch(W, per):
    """StreamSharded over MultiWalker in bench.py's settings (auto-reset, the constructor's default noise, the one-launch step on the four-
    and eight-lane classes): the sub-batches' outputs, concatenated, are the single batch's in every bit and the CPU build's under the rules
    above -- 30 joined steps, then 10 steps that only enqueue and one join()"""
    from madrl_amd.sharded import StreamSharded
    N, H, base, fused = 4 * per, 9, 50, W < 9
    kw = dict(n_walkers=W, seed=17, auto_reset=True, max_steps=H)
    tr = _trace(W, N, H, 1e-3, 17, base, 23)

    def make(n_envs, env_id_base, device):
        from madrl_amd.multiwalker import BatchedMultiWalkerEnv
        e = BatchedMultiWalkerEnv(n_envs=n_envs, env_id_base=env_id_base, device=device, **kw)
        e.set_mode(fused=fused)
        return e

    sh = StreamSharded(make, N, n_streams=4, env_id_base=base, device=DEV)
    whole = make(N, base, DEV)
    cat = lambda parts: torch.cat(list(parts)).cpu().numpy()
    sh_worlds = lambda: cat(e.state_buffer[:, :e.world_bytes] for e in sh.envs)
    wobs = whole.reset().cpu().numpy()
    sobs = cat(sh.reset())
    assert np.array_equal(_bits(sobs), _bits(wobs)), "reset observations"
    _check_obs(sobs, tr.obs0, True, "reset")
    for t, step in enumerate(tr.steps):
        a = torch.as_tensor(step[0], device=DEV)
        joined = t < 30
        out = sh.step(a, join=joined)
        wobs, wrew, wdone, winfo = whole.step(a)
        if not joined and t < T_STEPS - 1:
            continue
        if not joined:
            sh.join()
        got = [cat(o[0] for o in out), cat(o[1] for o in out), cat(o[3]["done_bits"] for o in out), sh_worlds()]
        ref = [x.cpu().numpy() for x in (wobs, wrew, winfo["done_bits"], whole.state_buffer[:, :whole.world_bytes])]
        for g, r, name in zip(got, ref, ("observations", "rewards", "done bits", "world records")):
            assert np.array_equal(_bits(g), _bits(r)), "step %d: %s of the sub-batches against the single batch" % (t, name)
        _check_step("step %d" % t, step, got[0], got[1], got[2], got[3], True)
    assert tr.n_ends >= N * (T_STEPS // H)
    print("largest host/device difference in the noisy columns so far: %g" % _worst[0])


# ------------------------------------------------------------------------------------------------ 4. hipGraph replay and the spare cycle
def _policy(obs):   # a pure function of the observation: capturable, and any difference in an observation shows in the next action
    return torch.sin(obs[..., :4] * 50)


GRAPH_CASES = [(3, 35, 5, 5), (3, 35, 6, 4), (6, 19, 5, 2), (10, 11, 7, 3)]   # odd / even horizons, the time limit aligned to them or not
FIELDS = ("actions", "rewards", "dones", "observations", "last_observation", "returns")


@pytest.mark.parametrize("W,N,T,H", GRAPH_CASES)
def test_collector_hipgraph_replay_matches_eager_on_multiwalker(W, N, T, H):
    """(a) six collect() calls -- one eager, one that captures, four that only replay -- give the eager collector's trajectories and leave the
    eager env's world records; (c) afterwards every env is still in the spare cycle.  A replay repeats whatever the captured launches carried
    by value, so the step counter that picks the dirty list by parity and stamps finished spares has to advance on the device."""
    from madrl_amd.rollout import RolloutCollector
    envs = [_mk(W, N, seed=5, env_id_base=3, auto_reset=True, max_steps=H) for _ in range(2)]
    cols = [RolloutCollector(e, _policy, T, store_observations=True, graph=g) for e, g in zip(envs, (False, True))]
    n_ends = 0
    for it in range(6):
        a, b = cols[0].collect(), cols[1].collect()
        for k in FIELDS:
            assert torch.equal(getattr(a, k), getattr(b, k)), "collect() %d: %s of the replayed graph against the eager collector" % (it, k)
        n_ends += int(((a.dones & 3) != 0).sum())
    assert cols[1]._graph is not None and n_ends >= N * (6 * T // H)
    torch.cuda.synchronize()
    assert torch.equal(envs[0].state_buffer[:, :envs[0].world_bytes], envs[1].state_buffer[:, :envs[1].world_bytes]), "world records after six horizons"
    zero = torch.zeros((N, W, 4), device=DEV)
    for env, name in zip(envs, ("eager", "graph")):
        ended = []
        for _ in range(2):
            ended.append((env.step(zero)[3]["done_bits"].cpu().numpy() & 3) != 0)
        if H > 2:   # (a horizon of two ends every episode within these two calls)
            assert not (ended[0] | ended[1]).all()
        _check_spare_cycle(env, ended[1], ended[0], "%s env after six horizons and two steps" % name)


@pytest.mark.parametrize("W,N,T,H", [GRAPH_CASES[0], GRAPH_CASES[3]])
def test_collector_trajectory_slots_equal_the_copy_per_step(W, N, T, H):
    """(b) store_observations through obs_out= (the step kernel of step t writes slot t + 1) against obs_slots=False (a copy per step)"""
    from madrl_amd.rollout import RolloutCollector
    cols = [RolloutCollector(_mk(W, N, seed=5, env_id_base=3, auto_reset=True, max_steps=H), _policy, T, store_observations=True, obs_slots=s)
            for s in (None, False)]
    assert cols[0]._slots and not cols[1]._slots
    for it in range(3):
        a, b = cols[0].collect(), cols[1].collect()
        for k in FIELDS:
            assert torch.equal(getattr(a, k), getattr(b, k)), "collect() %d: %s" % (it, k)
    assert ((a.dones & 3) != 0).any()


# ------------------------------------------------------------------------------------------------ 5. caller destinations
def _framed(shape, dtype, pad):
    """an interior, contiguous slice [pad : pad + shape[0]] of a larger tensor filled with the byte 0xA5 -> (the larger tensor's bytes, the slice)"""
    rows = shape[0] + 2 * pad
    row_bytes = int(np.prod(shape[1:], dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((rows * row_bytes,), 0xA5, dtype=torch.uint8, device=DEV)
    return raw.view(rows, row_bytes), raw.view(dtype).view((rows,) + tuple(shape[1:]))[pad:pad + shape[0]]


@pytest.mark.parametrize("use_spares", [True, False], ids=["spares", "second-launch"])
@pytest.mark.parametrize("fused", [False, True], ids=["three-launches", "one-launch"])
@pytest.mark.parametrize("W", [3, 10])
def test_step_writes_caller_destinations_and_nothing_else(W, fused, use_spares):
    """step(act, rew_out=, done_out=, obs_out=) with a horizon of 2: on every other step each observation row comes from the copy out of
    spare_obs (or, use_spares=False, from the second launch), on the others from env_observe -- all three must write the caller's rows, and
    only those"""
    tr = _trace2(W, 2)
    N, D, pad, T = tr.N, 32, 3, 12
    kw = dict(position_noise=NOISE, angle_noise=NOISE, seed=P2["seed"], env_id_base=P2["base"], auto_reset=True, max_steps=2)
    env, twin = _mk(W, N, **kw), _mk(W, N, **kw)
    for e in (env, twin):
        e.set_mode(fused=fused, use_spares=use_spares)
    frames = [_framed((N, W, D), torch.float32, pad), _framed((N, W), torch.float32, pad), _framed((N,), torch.uint8, pad)]
    (obs_raw, obs_dst), (rew_raw, rew_dst), (done_raw, done_dst) = frames
    assert obs_dst.is_contiguous() and obs_dst.data_ptr() == obs_raw.data_ptr() + pad * W * D * 4
    env.reset(); twin.reset()
    own = (env._obs, env._rew, env._done)
    for x in own:
        x.view(torch.uint8).fill_(0x5A)
    for t, step in enumerate(tr.steps[:T]):
        a = torch.as_tensor(step[0], device=DEV)
        if t == 3:   # refused before any launch: the env stays in step with its twin below
            for bad in (torch.empty((N, W, 2 * D), device=DEV)[..., ::2], torch.empty((N + 1, W, D), device=DEV), torch.empty((N, W, D - 1), device=DEV)):
                with pytest.raises(ValueError):
                    env.step(a, rew_out=rew_dst, done_out=done_dst, obs_out=bad)
        obs, rew, done, info = env.step(a, rew_out=rew_dst, done_out=done_dst, obs_out=obs_dst)
        tobs, trew, tdone, tinfo = twin.step(a)
        assert obs.data_ptr() == obs_dst.data_ptr() and obs.shape == (N, W, D), "the returned observation is a view of the destination"
        assert rew.data_ptr() == rew_dst.data_ptr() and info["done_bits"].data_ptr() == done_dst.data_ptr()
        for raw, name in ((obs_raw, "obs_out"), (rew_raw, "rew_out"), (done_raw, "done_out")):
            assert (raw[:pad] == 0xA5).all() and (raw[pad + N:] == 0xA5).all(), "step %d: bytes around %s" % (t, name)
        for x, name in zip(own, ("observation", "reward", "done")):
            assert (x.view(torch.uint8) == 0x5A).all(), "step %d: the env's own %s buffer" % (t, name)
        for g, r, name in ((obs_dst, tobs, "observations"), (rew_dst, trew, "rewards"), (done_dst, tinfo["done_bits"], "done bits")):
            assert np.array_equal(_bits(g.cpu().numpy()), _bits(r.cpu().numpy())), "step %d: %s against the twin env" % (t, name)
        assert torch.equal(env.state_buffer[:, :env.world_bytes], twin.state_buffer[:, :twin.world_bytes]), "step %d: world records against the twin env" % t
        _check_step("step %d" % t, step, obs_dst.cpu().numpy(), rew_dst.cpu().numpy(), done_dst.cpu().numpy(), env.state_buffer.cpu().numpy(), True)
    assert sum(int((s[2] != 0).sum()) for s in tr.steps[:T]) >= N * (T // 2)
