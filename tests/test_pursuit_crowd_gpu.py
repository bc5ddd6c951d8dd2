"""GPU tests (-m gpu) of the PursuitEvade crowd kernel (madrl_amd/csrc/pursuit_crowd.hpp, the XC lines of
pursuit_crowd_specializations.def): shapes with more than 64 pursuers or evaders.  Every comparison is bit for bit -- observations (the
never-stored cells included), rewards, done bits, `removed` and the whole state -- against the reference's recorded goldens, the C oracle
and the generic kernel."""
import numpy as np
import pytest
import torch

from pursuit_cases import CNN, FREE_RUNS, SURROUND_24, golden as _golden, named_maps as _maps

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _mk(maps, n_envs, **kw):
    from madrl_amd.pursuit import BatchedPursuitEvade
    return BatchedPursuitEvade(maps, n_envs=n_envs, device=DEV, **kw)


STATE_KEYS = ("pos_p", "pos_e", "gone", "term_p", "term_e", "map_id", "tick", "t")


def _same_state(a, b, msg):
    sa, sb = a.get_state(), b.get_state()
    for k in STATE_KEYS:
        assert torch.equal(sa[k], sb[k]), "%s: state[%s]" % (msg, k)


def _cmp_oracle_state(env, orc, msg):
    st, ref = env.get_state(), orc.get_state()
    for k in ("pos_p", "pos_e", "gone", "term_p", "term_e", "map_id"):
        assert np.array_equal(st[k].cpu().numpy(), ref[k]), "%s: state[%s]" % (msg, k)
    assert np.array_equal(st["tick"].cpu().numpy().view(np.uint32), ref["tick"]), msg + ": tick"


@pytest.mark.parametrize("name", ["pursuit_crowd_20v300", "pursuit_crowd_260v40_global", "pursuit_wide_70v90"])
def test_crowd_kernel_replays_the_reference_goldens(name):
    """the reference's own recordings above 64 of a kind (injected positions and evader actions), three identical env copies"""
    from oracle import pursuit as po
    g = _golden(name)
    N = 3
    env = _mk(list(g["maps"]), N, kernel="wave", **po.config_from_golden(g))
    assert env.kernel_kind == "wave"
    rep = lambda a: np.repeat(np.asarray(a)[None], N, axis=0)
    for t in range(len(g["op"])):
        want_obs = g["obs_f32"][t].reshape(env.n_pursuers, -1)
        if g["op"][t] == 0:
            pos = np.concatenate([g["init_p"][t], g["init_e"][t]])
            obs = env.reset(positions=rep(pos), map_ids=np.full(N, g["map_id"][t]))
            got = obs.reshape(N, env.n_pursuers, -1).cpu().numpy()
            for n in range(N):
                assert np.array_equal(got[n], want_obs), "%s reset obs op %d env %d" % (name, t, n)
        else:
            obs, rew, done, info = env.step(rep(g["act_p"][t]), evader_actions=rep(g["act_e"][t]))
            got = obs.reshape(N, env.n_pursuers, -1).cpu().numpy()
            st = env.get_state()
            for n in range(N):
                tag = "%s op %d env %d" % (name, t, n)
                assert np.array_equal(got[n], want_obs), tag + ": obs (%d cells differ)" % int((got[n] != want_obs).sum())
                assert np.array_equal(rew[n].cpu().numpy(), g["rew_f64"][t].astype(np.float32)), tag + ": rewards"
                assert bool(done[n]) == bool(g["done"][t]), tag + ": done"
                assert int(info["removed"][n]) == int(g["removed"][t]), tag + ": removed"
                assert np.array_equal(st["pos_p"][n].cpu().numpy(), g["pos_p"][t]), tag + ": pursuer positions"
                assert np.array_equal(st["pos_e"][n].cpu().numpy(), g["pos_e"][t]), tag + ": evader positions"
                assert np.array_equal(st["gone"][n].cpu().numpy(), g["gone_e"][t]), tag + ": evaders_gone"


@pytest.mark.parametrize("case", sorted(FREE_RUNS), ids=sorted(FREE_RUNS))
def test_crowd_kernel_free_running_vs_oracle_and_generic(case):
    """seeded free-running rollouts with fused auto-reset: the crowd kernel, the generic kernel and the C oracle each run their own Philox;
    every output and the whole state agree on every step"""
    from oracle import pursuit as po
    mname, kw, N, T, H, want_removed, want_done = FREE_RUNS[case]
    maps = _maps(mname)
    env = _mk(maps, N, seed=3, env_id_base=7, max_steps=H, auto_reset=True, kernel="wave", **kw)
    assert env.kernel_kind == "wave"
    gen = _mk(maps, N, seed=3, env_id_base=7, max_steps=H, auto_reset=True, kernel="generic", **kw)
    assert gen.kernel_kind == "generic"
    orc = po.PursuitOracle(maps, n_envs=N, seed=3, env_id_base=7, **kw)
    obs, gobs = env.reset(), gen.reset()
    oobs = orc.reset().copy()
    assert np.array_equal(obs.reshape(oobs.shape).cpu().numpy(), oobs), "reset obs"
    assert torch.equal(obs, gobs), "reset obs, generic kernel"
    _cmp_oracle_state(env, orc, "after reset")
    rng = np.random.RandomState(5)
    tstep = np.zeros(N, np.int64)
    n_done = n_removed = 0
    for t in range(T):
        act = rng.randint(5, size=(N, env.n_pursuers))
        a = torch.as_tensor(act, device=DEV)
        obs, rew, done, info = env.step(a)
        gobs, grew, gdone, ginfo = gen.step(a)
        oobs, orew, odone, orem = orc.step(act)
        tstep += 1
        bits = odone.astype(np.uint8) | ((tstep >= H).astype(np.uint8) << 1)
        assert np.array_equal(info["done_bits"].cpu().numpy(), bits), "step %d done bits" % t
        assert np.array_equal(info["removed"].cpu().numpy(), orem), "step %d removed" % t
        assert np.array_equal(rew.cpu().numpy(), orew.astype(np.float32)), "step %d rewards" % t
        mask = (bits != 0).astype(np.uint8)
        if mask.any():
            orc.reset(mask=mask)
            tstep[mask != 0] = 0
        n_done += int((bits & 1).sum())
        n_removed += int(orem.sum())
        got = obs.reshape(orc.obs.shape).cpu().numpy()
        assert np.array_equal(got, orc.obs), "step %d obs: %d cells differ" % (t, int((got != orc.obs).sum()))
        assert torch.equal(obs, gobs) and torch.equal(rew, grew) and torch.equal(done, gdone), "step %d: generic kernel" % t
        assert torch.equal(info["done_bits"], ginfo["done_bits"]) and torch.equal(info["removed"], ginfo["removed"]), "step %d: generic kernel" % t
        if t % 10 == 0 or t == T - 1:
            _cmp_oracle_state(env, orc, "step %d" % t)
            _same_state(env, gen, "step %d" % t)
            assert np.array_equal(env.get_state()["t"].cpu().numpy(), tstep), "episode step counter"
    print("%s: removed %d, episodes ended by catches %d" % (case, n_removed, n_done))
    if want_removed:
        assert n_removed > 0
    if want_done:
        assert n_done > 0


def test_all_reset_rules_together_free_running_vs_oracle():
    """every reset rule at once on the smallest crowd shape (XC(24, 24, 20, 300, 9, 1, 1)): the episode's map drawn from a pool of three,
    random_opponents, a constraint window inside the map, the fused auto-reset -- 9 envs on 3 workgroups, max_steps 7, 40 steps"""
    from madrl_amd.maps import synthetic_map_pool
    from oracle import pursuit as po
    maps = list(synthetic_map_pool(3, 24, 24, seed=1))
    kw = dict(SURROUND_24, sample_maps=True, random_opponents=True, max_opponents=250, constraint_window=0.5)
    N, T, H = 9, 40, 7
    env = _mk(maps, N, seed=3, env_id_base=7, max_steps=H, auto_reset=True, kernel="wave", **kw)
    env.set_launch(max_blocks=3)   # a workgroup walks three envs
    assert env.kernel_kind == "wave"
    orc = po.PursuitOracle(maps, n_envs=N, seed=3, env_id_base=7, **kw)
    assert np.array_equal(env.reset().reshape(orc.obs.shape).cpu().numpy(), orc.reset()), "reset obs"
    _cmp_oracle_state(env, orc, "after reset")
    assert len(set(orc.get_state()["map_id"].tolist())) >= 2
    rng = np.random.RandomState(5)
    tstep = np.zeros(N, np.int64)
    for t in range(T):
        act = rng.randint(5, size=(N, env.n_pursuers))
        obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
        _oobs, orew, odone, orem = orc.step(act)
        tstep += 1
        bits = odone.astype(np.uint8) | ((tstep >= H).astype(np.uint8) << 1)
        assert np.array_equal(info["done_bits"].cpu().numpy(), bits), "step %d done bits" % t
        assert np.array_equal(info["removed"].cpu().numpy(), orem), "step %d removed" % t
        assert np.array_equal(rew.cpu().numpy(), orew.astype(np.float32)), "step %d rewards" % t
        mask = (bits != 0).astype(np.uint8)
        if mask.any():
            orc.reset(mask=mask)
            tstep[mask != 0] = 0
        got = obs.reshape(orc.obs.shape).cpu().numpy()
        assert np.array_equal(got, orc.obs), "step %d obs: %d cells differ" % (t, int((got != orc.obs).sum()))
        _cmp_oracle_state(env, orc, "step %d" % t)


def test_every_env_of_a_1024_env_cnn_batch_matches_the_oracle():
    from oracle import pursuit as po
    maps, N = _maps("pool128"), 1024
    kw = dict(CNN, sample_maps=True)
    env = _mk(maps, N, seed=11, max_steps=500, auto_reset=True, kernel="wave", **kw)
    assert env.kernel_kind == "wave"
    orc = po.PursuitOracle(maps, n_envs=N, seed=11, **kw)
    assert np.array_equal(env.reset().reshape(orc.obs.shape).cpu().numpy(), orc.reset())
    rng = np.random.RandomState(2)
    for t in range(10):
        act = rng.randint(5, size=(N, 100))
        obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
        oobs, orew, odone, orem = orc.step(act)
        assert np.array_equal(obs.reshape(oobs.shape).cpu().numpy(), oobs), "step %d obs" % t
        assert np.array_equal(rew.cpu().numpy(), orew.astype(np.float32)) and np.array_equal(info["removed"].cpu().numpy(), orem)
        assert not odone.any() and not bool(done.any())
    _cmp_oracle_state(env, orc, "after 10 steps")


@pytest.mark.parametrize("case", ["cnn_rows_48x48", "colocate_global_260v40"])
def test_switching_kernels_on_one_handle_and_state_round_trip(case):
    """10 steps crowd, 5 generic, 10 crowd on ONE handle against a handle that stays generic: the record is shared, and what the crowd
    kernel remembers about the observation buffer is forgotten when another kernel wrote it.  Then get_state -> set_state into a fresh env."""
    mname, kw, N, _T, H, _r, _d = FREE_RUNS[case]
    maps, N = _maps(mname), 48
    a = _mk(maps, N, seed=4, max_steps=12, auto_reset=True, kernel="wave", **kw)
    b = _mk(maps, N, seed=4, max_steps=12, auto_reset=True, kernel="generic", **kw)
    assert torch.equal(a.reset(), b.reset())
    g = torch.Generator(device="cpu").manual_seed(3)
    t = 0
    for kind, n in (("wave", 10), ("generic", 5), ("wave", 10)):
        a.set_kernel(kind)
        assert a.kernel_kind == kind and b.kernel_kind == "generic"
        for _ in range(n):
            act = torch.randint(0, 5, (N, a.n_pursuers), generator=g, dtype=torch.int32).to(DEV)
            oa, ra, da, ia = a.step(act)
            ob, rb, db, ib = b.step(act)
            assert torch.equal(oa, ob), "step %d (%s): obs, %d cells differ" % (t, kind, int((oa != ob).sum()))
            assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ia["removed"], ib["removed"]), "step %d (%s)" % (t, kind)
            _same_state(a, b, "step %d (%s)" % (t, kind))
            t += 1
    c = _mk(maps, N, seed=4, max_steps=12, auto_reset=True, kernel="wave", **kw)
    c.reset()
    c.set_state(a.get_state())
    c.obs_buffer.copy_(a.obs_buffer)   # the persistent IN / OUT buffer belongs to the state of a run (never-stored cells)
    _same_state(a, c, "after set_state")
    for _ in range(8):
        act = torch.randint(0, 5, (N, a.n_pursuers), generator=g, dtype=torch.int32).to(DEV)
        oa, ra, da, ia = a.step(act)
        oc, rc, dc, ic = c.step(act)
        assert torch.equal(oa, oc) and torch.equal(ra, rc) and torch.equal(da, dc) and torch.equal(ia["removed"], ic["removed"])
    _same_state(a, c, "8 steps after set_state")


def test_in_place_edits_of_the_returned_observations_are_noticed_by_the_crowd_kernel():
    """(R, R, 4) rows on the 48 x 48 map: after `obs.add_(0.25)` the never-stored cells -- channel 3 off the centre, count cells outside the
    map -- keep the edited values exactly as the oracle's local_obs does; the crowd kernel must not go on storing +0.0 into channel 3 of
    a buffer it was once told to be zero"""
    from oracle import pursuit as po
    maps = _maps("rect48")
    N, P, R = 12, 100, 21
    env = _mk(maps, N, seed=5, kernel="wave", **CNN)
    assert env.kernel_kind == "wave"
    orc = po.PursuitOracle(maps, n_envs=N, seed=5, **CNN)
    obs, oobs = env.reset(), orc.reset()
    assert np.array_equal(obs.reshape(oobs.shape).cpu().numpy(), oobs)
    rng = np.random.RandomState(4)
    edits = 0

    def mirror():   # the oracle's persistent buffer [N, P, 4, R, R] takes the values the edited (R, R, 4) rows hold
        orc.set_local_obs(obs.cpu().numpy().reshape(N, P, R, R, 4).transpose(0, 1, 4, 2, 3).astype(np.float64))

    for t in range(24):
        if t % 7 == 3:
            obs.add_(0.25); mirror(); edits += 1
        if t % 7 == 5:
            obs.mul_(2.0); mirror(); edits += 1
        if t == 13:
            obs[:, 0].zero_(); mirror(); edits += 1
        act = rng.randint(5, size=(N, P))
        obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
        oobs, orew, odone, orem = orc.step(act)
        got = obs.reshape(oobs.shape).cpu().numpy()
        assert np.array_equal(got, oobs), "step %d: observations (never-stored cells included), %d cells differ" % (t, int((got != oobs).sum()))
        assert np.array_equal(rew.cpu().numpy(), orew.astype(np.float32))
        if odone.any():
            m = odone.astype(np.uint8)
            obs, oobs = env.reset(mask=m), orc.reset(mask=m)
            assert np.array_equal(obs.reshape(oobs.shape).cpu().numpy(), oobs)
    ch3 = obs.cpu().numpy().reshape(N, P, R, R, 4)[..., 3]
    assert edits >= 6 and (np.abs(ch3) > 1.5).any(), "edited values survive in channel 3 (an id is at most 0.99)"


def test_count_overflow_mark_equals_the_generic_kernels():
    """260 pursuers injected onto one cell: info['count_overflow'], the flag plane and record word 3 as on the generic kernel; a reset
    clears the mark"""
    N, P, E = 3, 260, 40
    kw = dict(n_pursuers=P, n_evaders=E, obs_range=5, n_catch=2, surround=False, flatten=True, reward_mech="global", seed=0)
    pos = np.zeros((N, P + E, 2), np.int32)
    spread = np.stack([np.arange(P) % 20, (np.arange(P) // 20) % 20], 1)
    pos[0, :P] = [9, 9]                                    # env 0: all 260 pursuers on one cell
    pos[1, :P] = spread                                    # env 1: spread out
    pos[2, :253] = [3, 3]; pos[2, 253:P] = spread[253:]    # env 2: exactly 253 on one cell -- still inside the byte's range
    pos[:, P:] = np.stack([np.arange(E) % 20, 19 - np.arange(E) // 20], 1)
    stay = torch.full((N, P), 4, dtype=torch.int32, device=DEV)
    out = []
    for kernel in ("wave", "generic"):
        env = _mk([np.zeros((20, 20), np.int32)], N, kernel=kernel, **kw)
        assert env.kernel_kind == kernel
        env.reset(positions=pos)
        _, _, _, info = env.step(stay, evader_actions=np.full((N, E), 4, np.int32))
        rec = env._state[:N * env.record_bytes].view(N, env.record_bytes)[:, 12:16].clone()
        first = (info["count_overflow"].cpu().numpy().tolist(), info["done_bits"].cpu().clone(), env._flags.cpu().clone(), rec.cpu())
        env.reset(mask=np.array([1, 0, 0], np.uint8), positions=pos[[1, 1, 1]])
        _, _, _, info = env.step(stay, evader_actions=np.full((N, E), 4, np.int32))
        rec = env._state[:N * env.record_bytes].view(N, env.record_bytes)[:, 12:16].clone()
        out.append(first + (info["count_overflow"].cpu().numpy().tolist(), env._flags.cpu().clone(), rec.cpu()))
    w, g = out
    assert w[0] == g[0] == [True, False, False]
    assert torch.equal(w[1], g[1]) and torch.equal(w[2], g[2]) and torch.equal(w[3], g[3])
    assert bool(w[3][0].any()) and not bool(w[3][1:].any())
    assert w[4] == g[4] == [False, False, False]
    assert torch.equal(w[5], g[5]) and torch.equal(w[6], g[6]) and not bool(w[6].any())


def test_launch_shape_and_stream_sharding_do_not_change_results():
    from madrl_amd.sharded import StreamSharded
    maps, N = _maps("pool128"), 96
    kw = dict(CNN, sample_maps=True, seed=9, max_steps=8, auto_reset=True)
    envs = [_mk(maps, N, kernel="wave", max_blocks=b, **kw) for b in (0, 1, 7)]
    sh = StreamSharded(lambda n_envs, env_id_base, device: _mk(maps, n_envs, env_id_base=env_id_base, kernel="wave", **kw), N, n_streams=2,
                       device=DEV)
    assert all(e.kernel_kind == "wave" for e in envs)
    obs = [e.reset() for e in envs]
    so = sh.reset()
    assert torch.equal(obs[0], obs[1]) and torch.equal(obs[0], obs[2]) and torch.equal(obs[0], torch.cat(so))
    g = torch.Generator(device="cpu").manual_seed(1)
    for t in range(20):
        act = torch.randint(0, 5, (N, 100), generator=g, dtype=torch.int32).to(DEV)
        res = [e.step(act) for e in envs]
        parts = sh.step(act)
        for r in res[1:]:
            assert torch.equal(r[0], res[0][0]) and torch.equal(r[1], res[0][1]) and torch.equal(r[2], res[0][2]), t
        assert torch.equal(res[0][0], torch.cat([p[0] for p in parts])) and torch.equal(res[0][1], torch.cat([p[1] for p in parts])), t
        assert torch.equal(res[0][2], torch.cat([p[2] for p in parts])), t
    for e in envs[1:]:
        _same_state(envs[0], e, "launch shapes")


def test_evader_control_and_per_env_counts_stay_on_the_generic_kernel():
    from madrl_amd import _lib
    maps = _maps("open24")
    kw = dict(n_pursuers=70, n_evaders=90, obs_range=9, n_catch=2, surround=True, flatten=True, reward_mech="local")
    assert _mk(maps, 4, **kw).kernel_kind == "wave"
    for extra in (dict(per_env_counts=True), dict(train_pursuit=False)):
        env = _mk(maps, 4, **kw, **extra)
        assert env.kernel_kind == "generic"
        with pytest.raises(_lib.MadrlError, match="specialisation"):
            env.set_kernel("wave")
        assert env.kernel_kind == "generic"
        env.reset()
