"""Per-env agent counts on the PursuitEvade crowd kernel (pursuit_live_crowd_kernel over an LCShape, the XLC lines of
pursuit_live_specializations.def): the authors' CNN capacity (100 v 300, obs_range 21, (R, R, 4) rows) on the 128 x 128 pool and on a
48 x 48 map, 20 v 300 on an open 24 x 24 map and 260 v 40 with the global reward on an open 20 x 20 map.

An env at live counts (p, e) of a capacity must compute bit for bit what env n of a fixed-shape (p, e) batch computes -- observations,
rewards, done bits, `removed`, the flag plane, positions and RNG ticks -- on the live crowd kernel ("wave") and on the generic kernel.
Rows k >= p of the observation buffer stay untouched and rewards k >= p are 0.  The fixed batch below the capacity runs the generic
kernel: that is the established result."""
import pickle

import numpy as np
import pytest
import torch

from live_pursuit import assert_live_equals_fixed, assert_pending_counts_history, counts_tensor
from pursuit_cases import CNN, FREE_RUNS, SURROUND_24, named_maps as _maps

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COLOCATE = FREE_RUNS["colocate_global_260v40"][1]
CAPS = {
    # name: (maps, config, max_steps, steps of the free run)
    "cnn48": ("rect48", CNN, 25, 60),
    "20v300": ("open24", SURROUND_24, 25, 60),
    "260v40": ("open20", COLOCATE, 100, 120),
}
# full capacity, capacity - 1, a mid count, the curriculum floor (pursuit_evade.py:268-270 stops removing at 4 pursuers); 130 and 200
# pursuers take numpy's split above 128 elements in the global reward's mean on a run-time count
COUNTS = {
    "cnn48": ((100, 300), (99, 299), (70, 270), (4, 204)),
    "20v300": ((20, 300), (19, 299), (12, 292), (4, 284)),
    "260v40": ((260, 40), (259, 39), (200, 30), (130, 20)),
}
LISTED = {"cnn128": ("pool128", dict(CNN, sample_maps=True)), "cnn48": ("rect48", CNN), "20v300": ("open24", SURROUND_24),
          "260v40": ("open20", COLOCATE)}


def _mk(maps, n, kernel="auto", **kw):
    from madrl_amd.pursuit import BatchedPursuitEvade
    return BatchedPursuitEvade(maps, n_envs=n, device=DEV, kernel=kernel, **kw)


def _env(cap, n, kernel="auto", **kw):
    return _mk(_maps(CAPS[cap][0]), n, kernel, **dict(CAPS[cap][1], **kw))


def _oracle(cap, n, p, e, **kw):
    from oracle import pursuit as po
    return po.PursuitOracle(_maps(CAPS[cap][0]), n_envs=n, **dict(CAPS[cap][1], n_pursuers=p, n_evaders=e, **kw))


@pytest.mark.parametrize("cap", sorted(LISTED))
def test_listed_capacities_run_the_live_crowd_kernel(cap):
    mname, kw = LISTED[cap]
    env = _mk(_maps(mname), 8, per_env_counts=True, **kw)
    assert env.kernel_kind == "wave"
    env.set_kernel("generic")
    assert env.kernel_kind == "generic"
    env.set_kernel("wave")
    assert env.kernel_kind == "wave"


@pytest.mark.parametrize("kernel", ["wave", "generic"])
@pytest.mark.parametrize("which", range(4), ids=["full", "cap_minus_1", "mid", "floor"])
@pytest.mark.parametrize("cap", sorted(CAPS))
def test_live_counts_match_a_fixed_shape_batch(cap, which, kernel):
    """every env at one live count against a fixed batch of that count: same seed and env_id_base, auto-reset, free-running steps"""
    p, e = COUNTS[cap][which]
    P = CAPS[cap][1]["n_pursuers"]
    N = 32 if cap == "cnn48" else 64
    kw = dict(seed=13, env_id_base=1000, max_steps=CAPS[cap][2], auto_reset=True)
    env = _env(cap, N, kernel, per_env_counts=True, **kw)
    fix = _env(cap, N, "auto", n_pursuers=p, n_evaders=e, **kw)
    assert env.kernel_kind == kernel
    assert_live_equals_fixed(env, fix, p, e, P, CAPS[cap][3], np.random.RandomState(which), state_every=20, last_too=True)
    assert env.kernel_kind == kernel


# name: capacity, extra config, envs per block, blocks, blocks with removed > 0, blocks with episodes ended by catches.
# The catch assertions are kept to what the C oracle ALONE gives in this layout (run on the CPU: one oracle per block at env_id_base
# 7 + block * envs per block, seed 3, one RandomState(5) action array [N, P] of which block j takes rows j and columns :p).  Evaders removed
# over the run, per block: 48 x 48 17 / 19 / 13 / 0; 48 x 48 with constraint_window 0.5 4 508 / 3 814 / 1 468 / 262; 24 x 24 18 / 12 / 6 / 0;
# 24 x 24 with random_opponents 9 / 4 / 1 / 0; 20 x 20 7 663 / 7 815 / 4 384 / 1 921 with 138 / 150 / 90 / 26 episodes ended by catches.
# Nothing about catches is asserted at (4, 204), (4, 284) and (40, 240).
MIXED = {
    "cnn48": ("cnn48", {}, 32, COUNTS["cnn48"], COUNTS["cnn48"][:3], ()),
    "cnn48_constraint_window": ("cnn48", dict(constraint_window=0.5), 32, COUNTS["cnn48"][:3] + ((40, 240),), COUNTS["cnn48"][:3], ()),
    "20v300": ("20v300", {}, 64, COUNTS["20v300"], COUNTS["20v300"][:3], ()),
    "20v300_random_opponents": ("20v300", dict(random_opponents=True, max_opponents=250), 64, COUNTS["20v300"], COUNTS["20v300"][:3], ()),
    "260v40": ("260v40", {}, 64, COUNTS["260v40"], COUNTS["260v40"], COUNTS["260v40"]),
}


@pytest.mark.parametrize("kernel", ["wave", "generic"])
@pytest.mark.parametrize("case", sorted(MIXED))
def test_mixed_batch_matches_the_oracle_per_block(case, kernel):
    """blocks of envs at different live counts in ONE batch, each block against a C oracle of its count at the block's env_id_base, with
    fused auto-reset; seed 3, env_id_base 7, RandomState(5) actions"""
    cap, extra, B, blocks, want_removed, want_done = MIXED[case]
    _mname, _kw, H, T = CAPS[cap]
    P = CAPS[cap][1]["n_pursuers"]
    N = B * len(blocks)
    env = _env(cap, N, kernel, per_env_counts=True, seed=3, env_id_base=7, max_steps=H, auto_reset=True, **extra)
    assert env.kernel_kind == kernel
    counts = counts_tensor(blocks, B)
    env.set_agent_counts(counts[:, 0], counts[:, 1])
    obs = env.reset().cpu().numpy().reshape(N, P, -1)
    orcs = [_oracle(cap, B, p, e, seed=3, env_id_base=7 + j * B, **extra) for j, (p, e) in enumerate(blocks)]
    for j, (p, e) in enumerate(blocks):
        oo = orcs[j].reset()
        assert np.array_equal(obs[j * B:(j + 1) * B, :p], oo.reshape(B, p, -1)), j
    rng = np.random.RandomState(5)
    tstep = np.zeros(N, np.int64)
    removed, ended = np.zeros(len(blocks), np.int64), np.zeros(len(blocks), np.int64)
    for it in range(T):
        act = rng.randint(5, size=(N, P))
        obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
        obs, rew = obs.cpu().numpy().reshape(N, P, -1), rew.cpu().numpy()
        dbits, rem = info["done_bits"].cpu().numpy(), info["removed"].cpu().numpy()
        tstep += 1
        for j, (p, e) in enumerate(blocks):
            s = slice(j * B, (j + 1) * B)
            orc = orcs[j]
            _oo, orew, odone, orem = orc.step(act[s, :p])
            bits = odone.astype(np.uint8) | ((tstep[s] >= H).astype(np.uint8) << 1)
            assert np.array_equal(dbits[s], bits) and np.array_equal(rem[s], orem), (it, j)
            assert np.array_equal(rew[s, :p], orew.astype(np.float32)) and not rew[s, p:].any(), (it, j)
            mask = (bits != 0).astype(np.uint8)
            if mask.any():
                orc.reset(mask=mask)
            assert np.array_equal(obs[s, :p], orc.obs.reshape(B, p, -1)), (it, j)
            assert not obs[s, p:].any(), (it, j)
            removed[j] += int(orem.sum())
            ended[j] += int((bits & 1).sum())
        tstep[dbits != 0] = 0
    print("%s: removed %s, episodes ended by catches %s" % (case, removed.tolist(), ended.tolist()))
    assert env.kernel_kind == kernel
    for j, c in enumerate(blocks):
        if c in want_removed:
            assert removed[j] > 0, (c, removed.tolist())
        if c in want_done:
            assert ended[j] > 0, (c, ended.tolist())


@pytest.mark.parametrize("cap", sorted(CAPS))
def test_pending_counts_take_effect_at_each_envs_own_reset(cap):
    """Counts change mid-episode (down, then back UP: rows that were not written for a while come back) and take effect at each env's own
    reset, explicit or fused.  The live crowd kernel and the generic kernel run the same history and must agree on every output.  The
    history starts on freshly zeroed buffers (the crowd kernel knows channel 3 of the (R, R, 4) rows to be +0.0 and stores whole float4s)
    and goes on after an in-place edit of the returned observations (it no longer knows, and must leave the edited values alone)."""
    B = 8
    blocks = COUNTS[cap]
    P = CAPS[cap][1]["n_pursuers"]
    N = B * len(blocks)
    envs = [_env(cap, N, k, per_env_counts=True, seed=3, max_steps=25, auto_reset=True) for k in ("wave", "generic")]
    assert_pending_counts_history(envs, counts_tensor(blocks, B), P)


@pytest.mark.parametrize("masked", [True, False])
def test_reference_curriculum_keeps_the_handle_and_the_fast_path(masked):
    """pursuit_evade.py:264-272 through update_curriculum on the 20 v 300 capacity, one pursuer and one evader removed every 3 iterations:
    down to 4 v 284 by iteration 48 and no further, on the live crowd kernel with one handle.  At each of the 17 counts reached the envs
    are reset and stepped against a C oracle of that count."""
    N, every = 16, 3
    env = _env("20v300", N, per_env_counts=True, seed=8, curriculum_remove_every=every)
    assert env.kernel_kind == "wave"
    gen0 = env.handle_generation
    mask = (torch.arange(N, device=DEV) % 2 == 0) if masked else None
    sel = mask if masked else torch.ones(N, dtype=torch.bool, device=DEV)
    rng = np.random.RandomState(0)
    checked = set()
    for itr in range(60):
        env.update_curriculum(itr, mask=mask)
        assert env.kernel_kind == "wave" and env.handle_generation == gen0, itr
        pend = env.agent_counts()[0]
        p = max(20 - itr // every, 4)
        want = torch.tensor([p, p + 280], dtype=torch.int32, device=DEV)
        assert bool((pend[sel] == want).all()), itr
        assert bool((pend[~sel] == torch.tensor([20, 300], dtype=torch.int32, device=DEV)).all()), itr
        if p not in checked:   # every count the rule reaches, 20 included: each gives the np * DV row loop a different tail
            checked.add(p)
            cw_env, cr_env = env.curriculum_state()
            orc = _oracle("20v300", N, p, p + 280, seed=8, catchr=float(cr_env[0]), constraint_window=float(cw_env[0]))
            orc.set_curriculum(cw_env.cpu().numpy(), cr_env.cpu().numpy())
            st = env.get_state()
            ost = orc.get_state()
            ost["tick"] = st["tick"].cpu().numpy().view(np.uint32)
            orc.set_state(ost)
            env.obs_buffer.zero_()
            s = sel.cpu().numpy()
            obs = env.reset().cpu().numpy()
            assert np.array_equal(obs[s, :p], orc.reset()[s]), itr
            assert torch.equal(env.agent_counts()[1][sel], want.expand(int(sel.sum()), 2))
            for _ in range(4):
                act = rng.randint(5, size=(N, 20))
                obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
                oobs, orew, _, _ = orc.step(act[:, :p])
                assert np.array_equal(obs.cpu().numpy()[s, :p], oobs[s]), itr
                assert np.array_equal(rew.cpu().numpy()[s, :p], orew.astype(np.float32)[s]), itr
                assert not rew[sel][:, p:].any(), itr
            assert env.kernel_kind == "wave"
    assert checked == set(range(4, 21))
    assert bool((env.agent_counts()[0][sel] == torch.tensor([4, 284], dtype=torch.int32, device=DEV)).all())


@pytest.mark.parametrize("cap", ["cnn48", "260v40"])
def test_state_pickle_and_kernel_switch_round_trips(cap):
    B = 6
    blocks = COUNTS[cap]
    P = CAPS[cap][1]["n_pursuers"]
    N = B * len(blocks)
    env = _env(cap, N, "auto", per_env_counts=True, seed=4, max_steps=20, auto_reset=True)
    counts = counts_tensor(blocks, B)
    env.set_agent_counts(counts[:, 0], counts[:, 1])
    env.reset()
    rng = np.random.RandomState(4)
    for _ in range(5):
        env.step(torch.as_tensor(rng.randint(5, size=(N, P)), device=DEV))
    env.set_agent_counts(5, 7, mask=torch.arange(N, device=DEV) % 3 == 0)
    st = {k: v.clone() for k, v in env.get_state().items()}
    obs0 = env.obs_buffer.clone()
    acts = [torch.as_tensor(rng.randint(5, size=(N, P)), device=DEV) for _ in range(25)]
    ref = [tuple(t.clone() for t in env.step(a)[:2]) for a in acts]
    assert env.kernel_kind == "wave"

    def replay(e, switch=False):
        e.obs_buffer.copy_(obs0)
        e.invalidate_obs()
        e.set_state(st)
        for i, (a, (o, r)) in enumerate(zip(acts, ref)):
            if switch:
                e.set_kernel("generic" if i % 2 else "wave")
            obs, rew, _, _ = e.step(a)
            assert torch.equal(obs, o) and torch.equal(rew, r), i

    replay(env)
    twin = pickle.loads(pickle.dumps(env))
    assert twin.per_env_counts and torch.equal(twin.agent_counts()[0], st["pending"])
    assert twin.kernel_kind == "wave"
    replay(twin)
    replay(twin, switch=True)   # generic <-> wave every step: the two kernels share the record, the results do not change


def test_stream_sharded_sub_batches_give_the_results_of_one_launch():
    from madrl_amd.sharded import StreamSharded
    cap, N = "20v300", 64
    blocks = COUNTS[cap]
    kw = dict(CAPS[cap][1], per_env_counts=True, seed=9, max_steps=8, auto_reset=True)
    maps = _maps(CAPS[cap][0])
    counts = counts_tensor(blocks, N // len(blocks))
    envs = [_mk(maps, N, "wave", max_blocks=b, **kw) for b in (0, 1, 7)]
    sh = StreamSharded(lambda n_envs, env_id_base, device: _mk(maps, n_envs, "wave", env_id_base=env_id_base, **kw), N, n_streams=2, device=DEV)
    for e in envs:
        e.set_agent_counts(counts[:, 0], counts[:, 1])
    for j, e in enumerate(sh.envs):
        c = counts[j * sh.per:(j + 1) * sh.per]
        e.set_agent_counts(c[:, 0], c[:, 1])
    assert all(e.kernel_kind == "wave" for e in envs + sh.envs)
    obs = [e.reset() for e in envs]
    so = sh.reset()
    assert torch.equal(obs[0], obs[1]) and torch.equal(obs[0], obs[2]) and torch.equal(obs[0], torch.cat(so))
    g = torch.Generator(device="cpu").manual_seed(1)
    for t in range(20):
        act = torch.randint(0, 5, (N, 20), generator=g, dtype=torch.int32).to(DEV)
        res = [e.step(act) for e in envs]
        parts = sh.step(act)
        for r in res[1:]:
            assert torch.equal(r[0], res[0][0]) and torch.equal(r[1], res[0][1]) and torch.equal(r[2], res[0][2]), t
        assert torch.equal(res[0][0], torch.cat([p[0] for p in parts])) and torch.equal(res[0][1], torch.cat([p[1] for p in parts])), t
        assert torch.equal(res[0][2], torch.cat([p[2] for p in parts])), t
    assert torch.equal(envs[0].agent_counts()[1], torch.cat([e.agent_counts()[1] for e in sh.envs]))


def test_every_env_of_a_1024_env_cnn_batch_at_live_90v290_matches_the_oracle():
    from oracle import pursuit as po
    maps, N, p, e = _maps("pool128"), 1024, 90, 290
    kw = dict(CNN, sample_maps=True)
    env = _mk(maps, N, "wave", per_env_counts=True, seed=11, max_steps=500, auto_reset=True, **kw)
    assert env.kernel_kind == "wave"
    env.set_agent_counts(p, e)
    orc = po.PursuitOracle(maps, n_envs=N, seed=11, **dict(kw, n_pursuers=p, n_evaders=e))
    obs = env.reset()
    assert np.array_equal(obs[:, :p].reshape(orc.obs.shape).cpu().numpy(), orc.reset()) and not bool(obs[:, p:].any())
    rng = np.random.RandomState(2)
    for t in range(10):
        act = rng.randint(5, size=(N, 100))
        obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
        oobs, orew, odone, orem = orc.step(act[:, :p])
        assert np.array_equal(obs[:, :p].reshape(oobs.shape).cpu().numpy(), oobs), "step %d obs" % t
        assert not bool(obs[:, p:].any()) and not bool(rew[:, p:].any())
        assert np.array_equal(rew[:, :p].cpu().numpy(), orew.astype(np.float32)) and np.array_equal(info["removed"].cpu().numpy(), orem)
        assert not odone.any() and not bool(done.any())
    st, ref = env.get_state(), orc.get_state()
    assert np.array_equal(st["pos_p"][:, :p].cpu().numpy(), ref["pos_p"]) and np.array_equal(st["pos_e"][:, :e].cpu().numpy(), ref["pos_e"])
    assert np.array_equal(st["gone"][:, :e].cpu().numpy(), ref["gone"]) and np.array_equal(st["map_id"].cpu().numpy(), ref["map_id"])
    assert np.array_equal(st["tick"].cpu().numpy().view(np.uint32), ref["tick"])
