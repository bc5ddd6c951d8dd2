"""Per-env agent counts within a compiled capacity (BatchedPursuitEvade(per_env_counts=True), madrl_pursuit_set_agent_counts).

An env at live counts (p, e) of a capacity (Pcap, Ecap) must compute bit for bit what env n of a fixed-shape (p, e) batch computes
(same seed, env_id_base + n): observations, rewards, done bits, positions and RNG ticks -- on the one-wavefront live-count kernel and on
the generic kernel.  Rows k >= p of the observation buffer stay untouched and rewards k >= p are 0."""
import pickle

import numpy as np
import pytest
import torch

from live_pursuit import assert_live_equals_fixed, counts_tensor

DEV = "cuda:0"
CAP = dict(n_pursuers=8, n_evaders=30, obs_range=7)


def _maps():
    from madrl_amd.maps import rectangle_map
    return [rectangle_map(16, 16)]


def _env(n, kernel, **kw):
    from madrl_amd.pursuit import BatchedPursuitEvade
    args = dict(CAP)
    args.update(kw)
    return BatchedPursuitEvade(_maps(), n_envs=n, device=DEV, kernel=kernel, **args)


VARIANTS = {
    "default": dict(),
    "random_opponents": dict(random_opponents=True, max_opponents=12),
    "global_colocate": dict(reward_mech="global", surround=False, n_catch=1),
    "hwc": dict(flatten=False, reward_mech="local"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "generic"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_live_counts_match_a_fixed_shape_batch(variant, kernel):
    """capacity (8, 30), every env at live (7, 29), auto-reset at 50 steps, 200 free-running steps against a fixed (7, 29) batch"""
    N, p, e = 4096, 7, 29
    kw = dict(VARIANTS[variant], seed=11, max_steps=50, auto_reset=True)
    cap = _env(N, kernel, per_env_counts=True, **kw)
    fix = _env(N, "auto", **dict(kw, n_pursuers=p, n_evaders=e))
    assert cap.kernel_kind == kernel
    assert_live_equals_fixed(cap, fix, p, e, 8, 200, np.random.RandomState(3), state_every=50)
    assert cap.kernel_kind == kernel


BLOCKS = ((8, 30), (7, 29), (6, 28), (4, 26))


def _mixed(kernel, B, **kw):
    cap = _env(B * len(BLOCKS), kernel, per_env_counts=True, seed=5, **kw)
    counts = counts_tensor(BLOCKS, B)
    cap.set_agent_counts(counts[:, 0], counts[:, 1])
    return cap, counts


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "generic"])
def test_mixed_batch_matches_the_oracle_per_block(kernel):
    from oracle import pursuit as po
    B = 32
    cap, counts = _mixed(kernel, B, reward_mech="local")
    obs = cap.reset().cpu().numpy()
    orcs = [po.PursuitOracle(_maps(), n_envs=B, seed=5, env_id_base=j * B, n_pursuers=p, n_evaders=e, obs_range=7, reward_mech="local")
            for j, (p, e) in enumerate(BLOCKS)]
    oobs = [o.reset().copy() for o in orcs]
    for j, (p, e) in enumerate(BLOCKS):
        assert np.array_equal(obs[j * B:(j + 1) * B, :p], oobs[j]), j
    rng = np.random.RandomState(9)
    for it in range(40):
        act = rng.randint(5, size=(B * len(BLOCKS), 8))
        obs, rew, done, info = cap.step(torch.as_tensor(act, device=DEV))
        obs, rew, dbits = obs.cpu().numpy(), rew.cpu().numpy(), info["done_bits"].cpu().numpy()
        for j, (p, e) in enumerate(BLOCKS):
            s = slice(j * B, (j + 1) * B)
            oo, orew, odone, _ = orcs[j].step(act[s, :p])
            assert np.array_equal(obs[s, :p], oo) and np.array_equal(rew[s, :p], orew.astype(np.float32)), (it, j)
            assert not rew[s, p:].any() and np.array_equal(dbits[s] & 1, odone), (it, j)
    assert cap.kernel_kind == kernel
    assert torch.equal(cap.agent_counts()[1], counts)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "generic"])
def test_pending_counts_take_effect_at_each_envs_own_reset(kernel):
    B = 64
    cap, counts = _mixed(kernel, B, max_steps=30, auto_reset=True)
    cap.reset()
    rng = np.random.RandomState(1)
    N = B * len(BLOCKS)
    for _ in range(7):
        cap.step(torch.as_tensor(rng.randint(5, size=(N, 8)), device=DEV))
    new = counts.flip(0).contiguous()   # every block moves to another count, mid-episode
    cap.set_agent_counts(new[:, 0], new[:, 1])
    switched = torch.zeros(N, dtype=torch.bool, device=DEV)
    k = torch.arange(8, device=DEV)[None, :]
    live = counts
    for it in range(40):
        _, rew, _, info = cap.step(torch.as_tensor(rng.randint(5, size=(N, 8)), device=DEV))
        assert not bool(rew[k >= live[:, :1]].any()), it   # the rewards of the episode that ran this step
        switched |= info["done_bits"] != 0
        pend, live = cap.agent_counts()
        assert torch.equal(pend, new)
        assert torch.equal(live, torch.where(switched[:, None], new, counts)), it
        st = cap.get_state()
        ghost = k >= live[:, :1]
        assert bool((st["pos_p"][ghost] == -1).all()) and bool((st["pos_p"][~ghost] >= 0).all())
        assert torch.equal(cap.live_agents(), ~ghost)
    assert bool(switched.all())   # max_steps 30: every env has reset at least once
    assert cap.kernel_kind == kernel


def _golden():
    import os
    from helpers import GOLDEN
    return np.load(os.path.join(GOLDEN, "curriculum_pursuit.npz"))


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [True, False])
def test_curriculum_per_env_keeps_the_handle_and_the_fast_path(masked):
    from oracle import pursuit as po
    g = _golden()
    cfg = {k[4:]: (float(g[k]) if g[k].dtype.kind == "f" else int(g[k])) for k in g.files if k.startswith("cfg_")}
    N = 64
    env = _env(N, "auto", per_env_counts=True, seed=8, reward_mech="local", **cfg)
    assert env.kernel_kind == "wave"
    gen0 = env.handle_generation
    mask = (torch.arange(N, device=DEV) % 2 == 0) if masked else None
    sel = mask if masked else torch.ones(N, dtype=torch.bool, device=DEV)
    rng = np.random.RandomState(0)
    checked = set()
    for itr in range(len(g["cw"])):
        env.update_curriculum(itr, mask=mask)
        assert env.kernel_kind == "wave" and env.handle_generation == gen0, itr
        pend = env.agent_counts()[0]
        want = torch.tensor([int(g["n_pursuers"][itr]), int(g["n_evaders"][itr])], dtype=torch.int32, device=DEV)
        assert bool((pend[sel] == want).all()), itr
        assert bool((pend[~sel] == torch.tensor([8, 30], dtype=torch.int32, device=DEV)).all()), itr
        cw_env, cr_env = env.curriculum_state()
        if not masked:
            assert (env.constraint_window, env.catchr) == (g["cw"][itr], g["catchr"][itr]), itr
        else:
            assert bool((cw_env[sel] == float(g["cw"][itr])).all()) and bool((cr_env[sel] == float(g["catchr"][itr])).all()), itr
        p, e = int(want[0]), int(want[1])
        if (p, e) in ((7, 29), (4, 26)) and (p, e) not in checked:
            checked.add((p, e))
            orc = po.PursuitOracle(_maps(), n_envs=N, seed=8, n_pursuers=p, n_evaders=e, obs_range=7, reward_mech="local",
                                   catchr=float(cr_env[0]), constraint_window=float(cw_env[0]))
            orc.set_curriculum(cw_env.cpu().numpy(), cr_env.cpu().numpy())
            st = env.get_state()
            ost = orc.get_state()
            ost["tick"] = st["tick"].cpu().numpy().view(np.uint32)
            orc.set_state(ost)
            env._obs.zero_()
            env.invalidate_obs()
            s = sel.cpu().numpy()
            obs = env.reset().cpu().numpy()
            assert np.array_equal(obs[s, :p], orc.reset()[s]), itr
            assert torch.equal(env.agent_counts()[1][sel], want.expand(int(sel.sum()), 2))
            for _ in range(3):
                act = rng.randint(5, size=(N, 8))
                obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
                oobs, orew, _, _ = orc.step(act[:, :p])
                assert np.array_equal(obs.cpu().numpy()[s, :p], oobs[s]), itr
                assert np.array_equal(rew.cpu().numpy()[s, :p], orew.astype(np.float32)[s]), itr
            assert env.kernel_kind == "wave"
    assert checked == {(7, 29), (4, 26)}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "generic"])
def test_state_and_pickle_round_trips_reproduce_the_next_step(kernel):
    B = 16
    cap, counts = _mixed(kernel, B, max_steps=20, auto_reset=True)
    N = B * len(BLOCKS)
    cap.reset()
    rng = np.random.RandomState(4)
    for _ in range(5):
        cap.step(torch.as_tensor(rng.randint(5, size=(N, 8)), device=DEV))
    cap.set_agent_counts(5, 27, mask=torch.arange(N, device=DEV) % 3 == 0)
    st = {k: v.clone() for k, v in cap.get_state().items()}
    obs0 = cap.obs_buffer.clone()
    acts = [torch.as_tensor(rng.randint(5, size=(N, 8)), device=DEV) for _ in range(25)]
    ref = [tuple(t.clone() for t in cap.step(a)[:2]) for a in acts]

    def replay(env):
        env.obs_buffer.copy_(obs0)
        env.invalidate_obs()
        env.set_state(st)
        for a, (o, r) in zip(acts, ref):
            obs, rew, _, _ = env.step(a)
            assert torch.equal(obs, o) and torch.equal(rew, r)

    replay(cap)
    twin = pickle.loads(pickle.dumps(cap))
    assert twin.per_env_counts and torch.equal(twin.agent_counts()[0], st["pending"])
    replay(twin)
    assert twin.kernel_kind == kernel


@pytest.mark.gpu
def test_out_of_scope_combinations_are_refused():
    from madrl_amd import _lib
    with pytest.raises(NotImplementedError):
        _env(8, "auto", per_env_counts=True, train_pursuit=False)
    ev = _env(8, "auto", train_pursuit=False, n_pursuers=8, n_evaders=12)
    with pytest.raises(_lib.MadrlError, match="control_evaders"):
        _lib.check(_lib.lib().madrl_pursuit_set_agent_counts(ev._handle, _lib.ptr(torch.zeros((8, 2), dtype=torch.int32, device=DEV))))
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    big = BatchedPursuitEvade([rectangle_map(32, 32)], n_envs=8, device=DEV, per_env_counts=True, n_pursuers=16, n_evaders=60, obs_range=7)
    assert big.kernel_kind == "generic"   # a capacity with only a multi-wavefront entry: the generic kernel
    with pytest.raises(_lib.MadrlError, match="live-count"):
        big.set_kernel("wave")
    fixed = _env(8, "auto")
    with pytest.raises(RuntimeError):
        fixed.set_agent_counts(7, 29)
    cap = _env(8, "auto", per_env_counts=True)
    with pytest.raises(ValueError):
        cap.set_agent_counts(9, 29)
    with pytest.raises(ValueError):
        cap.set_agent_counts(0, 29)
