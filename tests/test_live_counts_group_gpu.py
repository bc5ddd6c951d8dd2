"""Per-env agent counts on the multi-wavefront Pursuit kernel (pursuit_group_kernel over an LGShape, the XLG lines of
pursuit_live_specializations.def): the authors' 30 v 50 and 30 v 30 capacities (32 x 32 map pool, obs_range 11, the long-row slot table)
and the two-wavefront 20 v 50 test capacity (no table).

An env at live counts (p, e) of a capacity must compute bit for bit what env n of a fixed-shape (p, e) batch computes -- observations,
rewards, the flag plane, positions and RNG ticks -- on the live group kernel ("wave") and on the generic kernel.  Rows k >= p of the
observation buffer stay untouched and rewards k >= p are 0."""
import pickle

import numpy as np
import pytest
import torch

from helpers import golden_id, pursuit_golden_files
from live_pursuit import assert_live_equals_fixed, assert_pending_counts_history, counts_tensor, pursuit_state_equal

DEV = "cuda:0"
AUTHORS = dict(n_catch=2, surround=True, flatten=True, reward_mech="local", sample_maps=True, obs_range=11)
CAPS = {
    "30v50": dict(maps="pool32", n_pursuers=30, n_evaders=50, **AUTHORS),
    "30v30": dict(maps="pool32", n_pursuers=30, n_evaders=30, **AUTHORS),
    "20v50": dict(maps="pool16", n_pursuers=20, n_evaders=50, obs_range=5, n_catch=2, surround=True, flatten=True, reward_mech="local",
                  sample_maps=True),
}
# full capacity, capacity - 1, a mid count, the curriculum floor (pursuit_evade.py:268-270 stops removing at 4 pursuers)
COUNTS = {
    "30v50": ((30, 50), (29, 49), (17, 37), (4, 24)),
    "30v30": ((30, 30), (29, 29), (17, 17), (4, 4)),
    "20v50": ((20, 50), (19, 49), (12, 42), (4, 34)),
}


def _case_maps(name):
    # pool32: TwoDMaps.resize(2, map_pool16), as recorded in the authors' shape goldens; pool16: the reference's 16 x 16 pool
    gid = {"pool32": "pursuit_authors_30v50_obs11", "pool16": "pursuit_pool16_sample_maps"}[name]
    files = pursuit_golden_files()
    return list(np.load(files[[golden_id(f) for f in files].index(gid)])["maps"])


def _cfg(cap, **kw):
    args = dict(CAPS[cap])
    maps = _case_maps(args.pop("maps"))
    args.update(kw)
    return maps, args


def _env(cap, n, kernel="auto", **kw):
    from madrl_amd.pursuit import BatchedPursuitEvade
    maps, args = _cfg(cap, **kw)
    return BatchedPursuitEvade(maps, n_envs=n, device=DEV, kernel=kernel, **args)


def _oracle(cap, n, p, e, **kw):
    from oracle import pursuit as po
    maps, args = _cfg(cap, n_pursuers=p, n_evaders=e, **kw)
    return po.PursuitOracle(maps, n_envs=n, **args)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", sorted(CAPS))
def test_listed_capacities_run_the_live_group_kernel(cap):
    env = _env(cap, 8, per_env_counts=True)
    assert env.kernel_kind == "wave"
    env.set_kernel("generic")
    assert env.kernel_kind == "generic"
    env.set_kernel("wave")
    assert env.kernel_kind == "wave"


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "generic"])
@pytest.mark.parametrize("which", range(4), ids=["full", "cap_minus_1", "mid", "floor"])
@pytest.mark.parametrize("cap", sorted(CAPS))
def test_live_counts_match_a_fixed_shape_batch(cap, which, kernel):
    """every env at one live count against a fixed batch of that count: same seed and env_id_base, auto-reset, 150 free-running steps"""
    p, e = COUNTS[cap][which]
    P = CAPS[cap]["n_pursuers"]
    N = 256
    kw = dict(seed=13, env_id_base=1000, max_steps=40, auto_reset=True)
    env = _env(cap, N, kernel, per_env_counts=True, **kw)
    fix = _env(cap, N, "auto", n_pursuers=p, n_evaders=e, **kw)
    assert env.kernel_kind == kernel
    assert_live_equals_fixed(env, fix, p, e, P, 150, np.random.RandomState(which), state_every=50)
    assert env.kernel_kind == kernel


def _blocks(cap):
    return COUNTS[cap]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "generic"])
@pytest.mark.parametrize("cap", sorted(CAPS))
def test_mixed_batch_matches_the_oracle_per_block(cap, kernel):
    B = 12
    blocks = _blocks(cap)
    P = CAPS[cap]["n_pursuers"]
    env = _env(cap, B * len(blocks), kernel, per_env_counts=True, seed=5)
    counts = counts_tensor(blocks, B)
    env.set_agent_counts(counts[:, 0], counts[:, 1])
    obs = env.reset().cpu().numpy()
    orcs = [_oracle(cap, B, p, e, seed=5, env_id_base=j * B) for j, (p, e) in enumerate(blocks)]
    oobs = [o.reset().copy() for o in orcs]
    for j, (p, e) in enumerate(blocks):
        assert np.array_equal(obs[j * B:(j + 1) * B, :p], oobs[j]), j
    rng = np.random.RandomState(9)
    for it in range(30):
        act = rng.randint(5, size=(B * len(blocks), P))
        obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
        obs, rew, dbits = obs.cpu().numpy(), rew.cpu().numpy(), info["done_bits"].cpu().numpy()
        for j, (p, e) in enumerate(blocks):
            s = slice(j * B, (j + 1) * B)
            oo, orew, odone, _ = orcs[j].step(act[s, :p])
            assert np.array_equal(obs[s, :p], oo) and np.array_equal(rew[s, :p], orew.astype(np.float32)), (it, j)
            assert not rew[s, p:].any() and np.array_equal(dbits[s] & 1, odone), (it, j)
    assert env.kernel_kind == kernel
    assert torch.equal(env.agent_counts()[1], counts)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", sorted(CAPS))
def test_pending_counts_take_effect_at_each_envs_own_reset(cap):
    """Counts change mid-episode (down, then back up: rows written earlier come back through the stale-zero masks) and take effect at
    each env's own reset, explicit or fused.  The live group kernel and the generic kernel run the same history and must agree on every
    output; an in-place edit of the returned observation tensor is part of that history."""
    B = 16
    blocks = _blocks(cap)
    P = CAPS[cap]["n_pursuers"]
    N = B * len(blocks)
    envs = [_env(cap, N, k, per_env_counts=True, seed=3, max_steps=25, auto_reset=True) for k in ("wave", "generic")]
    assert_pending_counts_history(envs, counts_tensor(blocks, B), P)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [True, False])
def test_authors_curriculum_keeps_the_handle_and_the_fast_path(masked):
    """runners/old/rltools/pursuit.sh:1: 30 v 30, --update_curriculum --cur_remove 15.  update_curriculum removes one pursuer and one
    evader every 15 iterations, down to 4 v 4 by iteration 390: the whole run stays on the live group kernel with one handle."""
    N = 24
    env = _env("30v30", N, per_env_counts=True, seed=8, curriculum_remove_every=15)
    assert env.kernel_kind == "wave"
    gen0 = env.handle_generation
    mask = (torch.arange(N, device=DEV) % 2 == 0) if masked else None
    sel = mask if masked else torch.ones(N, dtype=torch.bool, device=DEV)
    rng = np.random.RandomState(0)
    checked = set()
    for itr in range(400):
        env.update_curriculum(itr, mask=mask)
        assert env.kernel_kind == "wave" and env.handle_generation == gen0, itr
        pend = env.agent_counts()[0]
        p = max(30 - itr // 15, 4)
        want = torch.tensor([p, p], dtype=torch.int32, device=DEV)
        assert bool((pend[sel] == want).all()), itr
        assert bool((pend[~sel] == torch.tensor([30, 30], dtype=torch.int32, device=DEV)).all()), itr
        if p in (29, 16, 4) and p not in checked:
            checked.add(p)
            cw_env, cr_env = env.curriculum_state()
            orc = _oracle("30v30", N, p, p, seed=8, catchr=float(cr_env[0]), constraint_window=float(cw_env[0]))
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
                act = rng.randint(5, size=(N, 30))
                obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
                oobs, orew, _, _ = orc.step(act[:, :p])
                assert np.array_equal(obs.cpu().numpy()[s, :p], oobs[s]), itr
                assert np.array_equal(rew.cpu().numpy()[s, :p], orew.astype(np.float32)[s]), itr
                assert not rew[sel][:, p:].any(), itr
            assert env.kernel_kind == "wave"
    assert checked == {29, 16, 4}


VARIANTS = {
    "random_opponents": dict(random_opponents=True, max_opponents=40),
    "global": dict(reward_mech="global"),
    "colocate": dict(surround=False, n_catch=1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "generic"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_variants_match_a_fixed_shape_batch(variant, kernel):
    N, p, e = 512, 13, 41
    kw = dict(VARIANTS[variant], seed=21, max_steps=30, auto_reset=True)
    env = _env("20v50", N, kernel, per_env_counts=True, **kw)
    fix = _env("20v50", N, "auto", n_pursuers=p, n_evaders=e, **kw)
    assert env.kernel_kind == kernel
    env.set_agent_counts(p, e)
    obs_c, obs_f = env.reset(), fix.reset()
    assert torch.equal(obs_c[:, :p], obs_f)
    rng = np.random.RandomState(2)
    caught = 0
    for it in range(120):
        act = torch.as_tensor(rng.randint(5, size=(N, 20)), device=DEV, dtype=torch.int32)
        obs_c, rew_c, _, info_c = env.step(act)
        obs_f, rew_f, _, info_f = fix.step(act[:, :p].contiguous())
        assert torch.equal(obs_c[:, :p], obs_f) and not bool(obs_c[:, p:].any()), it
        assert torch.equal(rew_c[:, :p], rew_f) and not bool(rew_c[:, p:].any()), it
        assert torch.equal(info_c["done_bits"], info_f["done_bits"]) and torch.equal(info_c["removed"], info_f["removed"]), it
        caught += int(info_c["removed"].sum())
    pursuit_state_equal(env, fix, p, e)
    assert caught > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cap", ["30v50", "20v50"])
def test_state_pickle_and_kernel_switch_round_trips(cap):
    B = 8
    blocks = _blocks(cap)
    P = CAPS[cap]["n_pursuers"]
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
