"""One twin harness for per-env particle counts (test_waterworld_live_counts_gpu.py, test_waterworld_wave_live_counts_gpu.py,
test_hostage_live_counts_gpu.py).  The definition of right: an env at live counts (a, b, c) computes what env n of a fixed-shape
(a, b, c) batch with the same seed and env_id_base + n computes.  So a run has one float32 oracle twin of N envs per distinct triple, env
n is compared with env n of its triple's twin, nothing is copied across, and every output and the whole state, slotted at the capacity,
are compared in every bit at every step.

compare_step() and compare_state() are the comparisons, over numpy arrays alone; LiveTwins is the protocol that keeps the twins in step
with a GPU batch; a World says what differs between the worlds.  The scenarios at the end are the tests that the three files share."""
import collections

import numpy as np
import torch

from helpers import bits, i32, raw, same_bits, slots

# cap: the capacity's triple; make_env(N, H, **env_kw): the GPU batch; make_twin(tri, N, H): the oracle twin of a triple;
# counters: the names of the two info counters; state_keys: the state compared beyond pos / vel; kernel_kind: what the env must report;
# events: the names tallied per triple in LiveTwins.ev; tally(run), called before a step, returns after(q, twin, idx), called when twin q
# has stepped (idx: the envs that run triple q) -- or None
World = collections.namedtuple("World", "cap make_env make_twin counters state_keys kernel_kind events tally")


def _np(t):
    return t.cpu().numpy()


def compare_step(twins, triples, cur, rew, done, count0, count1, tag):
    """what a step returned beside the observations, env n against env n of twin cur[n]"""
    for q, (o, tri) in enumerate(zip(twins, triples)):
        idx, a = cur == q, tri[0]
        assert np.array_equal(done[idx], o.done[idx].astype(bool)), "done %s" % tag
        assert np.array_equal(count0[idx], o.info[idx, 0]) and np.array_equal(count1[idx], o.info[idx, 1]), "info %s" % tag
        assert np.array_equal(i32(rew[idx, :a]), i32(o.rew[idx])), "rewards %s: %s" % (tag, np.abs(rew[idx, :a] - o.rew[idx]).max())
        assert not i32(rew[idx, a:]).any(), "rewards of absent agents %s" % tag


def compare_state(twins, cap, triples, cur, pend, st, live, pending, state_keys, tag, obs=None):
    """the counts, the state (st: get_state() as arrays) and, if given, the observations, env n against env n of twin cur[n]"""
    assert np.array_equal(live, np.asarray(triples)[cur]), "live counts %s" % tag
    assert np.array_equal(pending, np.asarray(triples)[pend]), "pending counts %s" % tag
    assert np.array_equal(st["counts"], live)
    for q, (o, tri) in enumerate(zip(twins, triples)):
        idx, a = cur == q, tri[0]
        if not idx.any():
            continue
        if obs is not None:
            assert np.array_equal(i32(obs[idx, :a]), i32(o.obs[idx])), "obs %s: %g" % (tag, np.abs(obs[idx, :a] - o.obs[idx]).max())
            assert not i32(obs[idx, a:]).any(), "rows of absent agents are not +0.0, %s" % tag
        ost, s = o.get_state(), slots(cap, tri)
        gone = np.setdiff1d(np.arange(sum(cap)), s)
        assert np.array_equal(i32(st["pos"][idx][:, s]), i32(ost["pos"][idx])), "pos %s" % tag
        assert np.array_equal(i32(st["vel"][idx][:, s]), i32(ost["vel"][idx])), "vel %s" % tag
        assert (st["pos"][idx][:, gone] == -1.0).all() and not i32(st["vel"][idx][:, gone]).any(), "absent slots %s" % tag
        for k in state_keys:
            assert np.array_equal(raw(st[k][idx]), raw(ost[k][idx])), "state %s, %s" % (k, tag)


class LiveTwins(object):
    """a per-env-counts batch and its oracle twins; `cur[n]` is the index of the triple env n runs, `pend[n]` of the one its next reset
    takes; `ev[q]` tallies, from the oracle's outputs alone, what happened among the envs that ran triple q"""

    def __init__(self, world, triples, N, H, deal=None, max_blocks=0, **env_kw):
        self.world, self.cap, self.triples, self.N, self.H = world, tuple(world.cap), [tuple(t) for t in triples], N, H
        self.env = world.make_env(N, H, **env_kw)
        assert self.env.kernel_kind == world.kernel_kind and self.env.per_env_counts
        if max_blocks:
            self.env.set_launch(max_blocks)   # one wavefront then walks envs of different triples one after the other
        self.twins = [world.make_twin(tri, N, H) for tri in self.triples]
        self.started = False   # live counts start at the capacity; the first reset deals the triples
        self.cur = np.full(N, -1)
        self.pend = self.cur.copy()
        self.set_pending(np.arange(N) % len(self.triples) if deal is None else deal)
        self.ev = [dict.fromkeys(world.events, 0) for _ in self.triples]
        self.resets = 0

    def total(self, event):
        return sum(ev[event] for ev in self.ev)

    def set_pending(self, idx, mask=None):
        idx = np.broadcast_to(np.asarray(idx), (self.N,))
        tri = np.asarray(self.triples)[idx]
        self.env.set_particle_counts(tri[:, 0], tri[:, 1], tri[:, 2], mask=mask)
        self.pend = np.where(np.ones(self.N, bool) if mask is None else np.asarray(mask, bool), idx, self.pend)

    def _reset_twins(self, env_mask, own_done=False):
        """the envs of env_mask take their pending triple: the twin an env moves to gets the env's tick first and then resets it (what
        else a reset draws from is the env's already: every twin had its first reset at tick 0).  own_done: every twin also resets the
        envs its own step ended (its envs that no batch env is compared with run along)"""
        new = np.where(env_mask, self.pend, self.cur)
        ticks = [o.get_state()["tick"] for o in self.twins]
        for q, o in enumerate(self.twins):
            arrive = env_mask & (new == q)
            tk = ticks[q].copy()
            for n in np.nonzero(arrive & (self.cur != q))[0]:
                tk[n] = ticks[self.cur[n]][n]
            o.set_state(tick=tk)
            m = arrive | (o.done.astype(bool) if own_done else False)
            if m.any():
                o.reset(mask=m.astype(np.uint8))
        self.cur = new

    def reset(self, mask=None):
        m = np.ones(self.N, bool) if mask is None else np.asarray(mask, bool)
        if not self.started:
            assert mask is None   # the first reset: every env leaves the capacity for its dealt triple; all ticks are 0
            self.started, self.cur = True, self.pend.copy()
            for o in self.twins:
                o.reset()
        else:
            self._reset_twins(m)
        self.obs = _np(self.env.reset(mask=None if mask is None else m.astype(np.uint8)))
        self.check("reset")

    def step(self, act, tag):
        after = self.world.tally(self) if self.world.tally else None
        obs, rew, done, info = self.env.step(act)
        done = _np(done)
        for q, (o, tri) in enumerate(zip(self.twins, self.triples)):
            o.step(act[:, :tri[0]])
            if after:
                after(q, o, self.cur == q)
        compare_step(self.twins, self.triples, self.cur, _np(rew), done, *[_np(info[k]) for k in self.world.counters], tag=tag)
        self.resets += int(done.sum())
        self._reset_twins(done, own_done=True)
        self.obs = _np(obs)
        self.check(tag)
        return done

    def check(self, tag, obs=True):
        st = {k: _np(v) for k, v in self.env.get_state().items()}
        pending, live = (_np(c) for c in self.env.particle_counts())
        compare_state(self.twins, self.cap, self.triples, self.cur, self.pend, st, live, pending, self.world.state_keys, tag,
                      obs=self.obs if obs else None)


# ---------------------------------------------------------------- the two worlds
def _catches(run):
    def after(q, o, idx):
        run.ev[q]["evc"] += int(o.info[idx, 0].sum())
        run.ev[q]["poc"] += int(o.info[idx, 1].sum())
    return after


def waterworld(kw, seed, base, kernel_kind=None, mk=None):
    """kw: the constructor arguments of the capacity; mk(n_envs, **kw): the per-env-counts GPU batch"""
    from oracle import waterworld as ww
    shared = dict(seed=seed, env_id_base=base, dtype=np.float32)
    return World(cap=(kw["n_pursuers"], kw["n_evaders"], kw["n_poison"]),
                 make_env=lambda N, H, **env_kw: mk(N, seed=seed, env_id_base=base, max_steps=H, auto_reset=True, **dict(kw, **env_kw)),
                 make_twin=lambda tri, N, H: ww.WaterworldOracle(n_envs=N, max_steps=H, **dict(kw, n_pursuers=tri[0], n_evaders=tri[1],
                                                                                                 n_poison=tri[2], **shared)),
                 counters=("evcatches", "pocatches"), state_keys=("obst", "t", "tick"), kernel_kind=kernel_kind, events=("evc", "poc"),
                 tally=_catches)


HOSTAGE_EVENTS = ("saves", "criminal_hits", "gate_openings", "bombings", "all_saved", "time_limit")


def all_h(h):
    """the saved mask of h hostages"""
    return np.uint64(2 ** int(h) - 1)


def _hostage_events(run):
    gate0 = [o.get_state()["flags"] & 1 for o in run.twins]

    def after(q, o, idx):   # the tallies of test_hostage_crowd_gpu.py::free_run_oracle, per triple
        mid, ev, d, full = o.get_state(), run.ev[q], idx & (o.done != 0), all_h(run.triples[q][1])
        ev["saves"] += int(o.info[idx, 0].sum())
        ev["criminal_hits"] += int(o.info[idx, 1].sum())
        ev["gate_openings"] += int(((mid["flags"] & 1) & ~gate0[q] & 1)[idx].sum())
        ev["bombings"] += int((d & ((mid["flags"] & 2) != 0)).sum())
        ev["all_saved"] += int((d & ((mid["saved"] & full) == full)).sum())
        ev["time_limit"] += int((d & (mid["t"] >= run.H) & ((mid["flags"] & 2) == 0) & ((mid["saved"] & full) != full)).sum())
    return after


def hostage(cap, coop, kw, seed, base, kernel_kind=None, mk=None):
    """cap: (rescuers, hostages, criminals); mk(*counts, n_coop_save, n_coop_avoid, n_envs=, **kw): the GPU batch"""
    from oracle import hostage as ho
    shared = dict(seed=seed, env_id_base=base)
    return World(cap=tuple(cap),
                 make_env=lambda N, H, **env_kw: mk(*cap, coop, 1, n_envs=N, per_env_counts=True, max_steps=H,
                                                    **dict(dict(kw, auto_reset=True, **shared), **env_kw)),
                 make_twin=lambda tri, N, H: ho.HostageOracle(*tri, coop, 1, n_envs=N, max_steps=H, dtype=np.float32, **dict(kw, **shared)),
                 counters=("ho_saved", "cr_encs"), state_keys=("key", "bomb", "saved", "flags", "t", "tick"), kernel_kind=kernel_kind,
                 events=HOSTAGE_EVENTS, tally=_hostage_events)


# ---------------------------------------------------------------- scenarios the three files share
def lockstep(a, b, shape, T, counters, counts=False):
    """two batches stepped with the same actions (shape: [N, agents, 2]): outputs and state equal in every bit.  A generator: it yields
    after every step, for a caller that changes something between two steps"""
    assert same_bits(a.reset(), b.reset())
    g = torch.Generator(device="cpu").manual_seed(3)
    for t in range(T):
        act = (torch.rand(shape, generator=g) * 2 - 1).to(a.device)
        oa, ra, da, ia = a.step(act)
        ob, rb, db, ib = b.step(act)
        assert same_bits(oa, ob), "obs step %d" % t
        assert same_bits(ra, rb) and torch.equal(da, db), "rewards / done step %d" % t
        assert all(torch.equal(ia[k], ib[k]) for k in counters), "info step %d" % t
        sa, sb = a.get_state(), b.get_state()
        assert set(sa) - set(sb) == (set() if counts else {"counts"})
        for k in sb:
            assert same_bits(sa[k], sb[k]), "state %s step %d" % (k, t)
        if counts:
            for ca, cb in zip(a.particle_counts(), b.particle_counts()):
                assert torch.equal(ca, cb), "counts step %d" % t
        yield t


def assert_obs_out_leaves_no_nan(env, steps=1):
    """env: a mixed batch; its step writes every element of an uninitialised observation destination, +0.0 in the rows of absent agents"""
    env.reset()
    N, Na = env.live_agents().shape
    dst = torch.empty(N * Na * env.obs_dim, device=env.device).fill_(float("nan"))
    act = torch.rand((N, Na, 2), device=env.device) * 2 - 1
    for t in range(steps):
        obs, rew, _done, _info = env.step(act, obs_out=dst)
        assert obs.data_ptr() == dst.data_ptr() and not torch.isnan(dst).any()
        absent = ~env.live_agents()
        assert absent.any() and not bits(obs[absent]).any() and not bits(rew[absent]).any() and (obs[~absent].abs().amax(dim=1) > 0).all()
        dst.fill_(float("nan"))


def assert_collector_equals_stepping_by_hand(make_env, make_policy, H, min_dones):
    """a RolloutCollector over a mixed batch, two horizons, against a second batch and policy stepped by hand"""
    from madrl_amd.rollout import RolloutCollector
    col = RolloutCollector(make_env(), make_policy(), horizon=H, store_observations=True)
    assert col._slots
    env, pol = make_env(), make_policy()
    obs = env.reset()
    for it in range(2):
        traj = col.collect()
        torch.cuda.synchronize()
        for t in range(H):
            assert same_bits(traj.observations[t], obs), (it, t)
            act = pol(obs)
            act = act[0] if isinstance(act, tuple) else act
            assert same_bits(traj.actions[t], act), (it, t)
            obs, rew, done, _info = env.step(act)
            assert same_bits(traj.rewards[t], rew) and torch.equal(traj.dones[t] != 0, done), (it, t)
        assert same_bits(traj.last_observation, obs), it
    assert not torch.isnan(traj.observations).any() and int((traj.dones != 0).sum()) >= min_dones
