"""What the tests at the 32-bit edges share (test_wide_buffers_gpu.py, test_wide_counters_gpu.py; DESIGN.md "index widths").

The kernels carry env indices, Philox counters and per-row offsets in 32-bit registers; buffer bases and byte offsets are 64-bit.  A
row base, an action pointer or a mask offset narrowed to 32 bits computes the same values on every batch below 4 GiB.  The check here
makes it fail:

  * `big`: one handle whose observation buffer passes the byte (or element) line, at least 64 whole envs beyond it;
  * `parts`: K handles of N / K envs each, same seed, env_id_base advanced by the part's offset, every buffer below 2^31 bytes -- a part
    cannot overflow anything, and sharding is invisible (test_sharding_is_invisible_env_id_base), so big == concatenation of the parts
    checks every byte of the big buffers without a host reference of that size;
  * `probe`: 48 envs whose env_id_base puts them on big's last 48 envs, compared with the C oracle after every call -- big's tail must
    equal the probe, which ties the envs beyond the line to the reference itself and not only to another run of the same kernel.

Sizes come from the handle (rows of n_agents * obs_dim * itemsize bytes), never from literals."""
import gc

import numpy as np
import pytest
import torch

DEV = "cuda:0"
PROBE = 48      # envs of the probe: big's last ones
BEYOND = 64     # whole envs that must lie beyond the line
STATE_KEYS = ("pos_p", "pos_e", "gone", "term_p", "term_e", "map_id", "tick", "t")


def free_device():
    gc.collect()
    torch.cuda.empty_cache()


def need_device_bytes(n):
    """the one reason a case may skip: less free device memory than it needs"""
    free_device()
    free, _total = torch.cuda.mem_get_info()
    if free < n:
        pytest.skip("%.1f GiB of device memory free, the case needs %.1f GiB" % (free / 2.0**30, n / 2.0**30))


def plan(row_bytes, line_bytes=2**32, parts=None):
    """(N, K): N the smallest multiple of K with N * row_bytes >= line_bytes + BEYOND * row_bytes; K = `parts`, or the smallest count
    that keeps a part's buffer below 2^31 bytes"""
    n_min = -(-(line_bytes + BEYOND * row_bytes) // row_bytes)
    K = parts or 1
    while True:
        N = -(-n_min // K) * K
        if (N // K) * row_bytes < 2**31:
            break
        assert parts is None, "%d parts of %d bytes each" % (K, (N // K) * row_bytes)
        K += 1
    assert N * row_bytes >= line_bytes + BEYOND * row_bytes and (N - K) * row_bytes < line_bytes + BEYOND * row_bytes
    return N, K


def zm16_eligible(P, R, flatten):
    """csrc/pursuit_zm16.hpp, eligible(): the one-wavefront shapes whose stale-zero masks are kept as 16 bits per lane, 128 B per env"""
    dv = (3 * R * R + 1) // 4
    ns = -(-P * dv // 64)
    if flatten != 1 or ns > 5:
        return False

    def useful(q):
        m = q % dv
        return q < P * dv and 4 * m + 3 >= R * R and 4 * m < 3 * R * R
    return all(sum(useful(lane + 64 * s) for s in range(ns)) <= 4 for lane in range(64))


def bits_equal(a, b):
    """every bit of two tensors of one shape and type (float32 / float16 compared as integers: NaN and -0.0 count)"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
    a, b = a.contiguous(), b.contiguous()
    as_int = {torch.float32: torch.int32, torch.float16: torch.int16, torch.float64: torch.int64, torch.bool: torch.uint8}.get(a.dtype)
    return torch.equal(a.view(as_int), b.view(as_int)) if as_int is not None else torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ PursuitEvade
class PursuitCase(object):
    """one kernel of BatchedPursuitEvade at one shape.  mode: 'step' (in place), 'step_to' (two float32 buffers, alternating) or 'half'
    (obs_dtype float16: step() goes between the env's two internal buffers).  counts: per-env (pursuers, evaders), env n takes entry
    n % len(counts) -- of its GLOBAL index, so that a part's envs get what big's envs got.  kinds: what kernel_kind, step_to_kernel_kind
    and last_step_entry must say."""

    def __init__(self, maps, shape, mode="step", kernel="auto", walk="auto", counts=None, kinds=("wave", "wave", "wave"), fixed=None, **kw):
        self.maps, self.shape, self.mode, self.kernel, self.walk, self.counts, self.kinds, self.fixed = maps, shape, mode, kernel, walk, counts, kinds, fixed
        xs, ys, P, E, R, fl = shape
        self.kw = dict(n_pursuers=P, n_evaders=E, obs_range=R, n_catch=2, surround=True, flatten=bool(fl), reward_mech="local", **kw)
        self.P, self.E = P, E
        self.dtype = torch.float16 if mode == "half" else torch.float32

    def map_pool(self):
        from madrl_amd.maps import rectangle_map
        return [rectangle_map(self.shape[0], self.shape[1])] if self.maps == "rect" else [np.zeros(self.shape[:2], np.int32)]

    def row_bytes(self):
        """(bytes of one env's observation rows, bytes per env of everything else a handle and a comparison hold), from a 1 024-env handle"""
        env = self.make(1024, 0, 1)
        P, E = self.P, self.E
        row = int(env.n_pursuers) * int(env.obs_dim) * env._obs.element_size()
        held = env._state.numel() // 1024 + 4 * P + 5   # state buffer, rewards, done, removed
        passing = 4 * P + 8 * (P + E) + P + 2 * E + 12 + 16   # the actions; one get_state(): positions, gone / terminal bytes, map id, tick, t, counts
        del env
        return row, held, passing

    def counts_of(self, base, n):
        c = torch.tensor(self.counts, dtype=torch.int32, device=DEV)
        return c[(torch.arange(n, device=DEV) + base) % len(self.counts)].contiguous()

    def make(self, n_envs, offset, max_steps, monkeypatch=None, base=None):
        from madrl_amd.pursuit import BatchedPursuitEvade
        if monkeypatch is not None:
            if self.fixed is False:
                monkeypatch.setenv("MADRL_PURSUIT_FIXED", "0")   # read when the handle is created
            else:
                monkeypatch.delenv("MADRL_PURSUIT_FIXED", raising=False)
        extra = dict(per_env_counts=True) if self.counts is not None else {}
        if self.mode == "half":
            extra["obs_dtype"] = torch.float16
        env = BatchedPursuitEvade(self.map_pool(), n_envs=n_envs, device=DEV, seed=SEED, env_id_base=(ID_BASE if base is None else base) + offset,
                                  max_steps=max_steps, auto_reset=True, kernel=self.kernel, **dict(self.kw, **extra))
        if monkeypatch is not None:
            monkeypatch.delenv("MADRL_PURSUIT_FIXED", raising=False)
        if self.walk != "auto":
            env.set_walk(self.walk)
        if self.counts is not None:
            c = self.counts_of(offset, n_envs)
            env.set_agent_counts(c[:, 0], c[:, 1])
        return env


SEED, ID_BASE = 2024, 1000


class Run(object):
    """a handle and the second buffer of the two-buffer modes (zero-filled, like the handle's own)"""

    def __init__(self, case, n_envs, offset, max_steps, monkeypatch, base=None, max_blocks=0):
        self.case, self.n, self.offset = case, n_envs, offset
        self.env = case.make(n_envs, offset, max_steps, monkeypatch, base=base)
        if max_blocks:
            self.env.set_launch(max_blocks=max_blocks)
        self.other = torch.zeros_like(self.env._obs) if case.mode == "step_to" else None

    def reset(self, mask=None, last=True):
        """last: no reset follows directly.  A half reset runs on a float32 copy of twice the buffer's bytes, which the env keeps for its next
        reset; it is dropped here.  (Not between two resets in a row: the library remembers which buffer its masks describe by address, and
        whether a new copy comes back at the old address -- masks kept -- or elsewhere -- masks start from "nothing known" -- is the
        allocator's choice: both are right, but they are not the same bits.)"""
        out = self.env.reset(mask=mask)
        if self.case.mode == "half" and last:
            self.env._obs32 = None
        return out

    def step(self, act):
        if self.case.mode == "step_to":
            prev = self.env._obs
            out = self.env.step_to(act, self.other)
            self.other = prev
            return out
        return self.env.step(act)

    def check_kinds(self, what):
        env, (kind, to_kind, entry) = self.env, self.case.kinds
        assert env.kernel_kind == kind, "%s: kernel_kind %s" % (what, env.kernel_kind)
        if self.case.mode != "step":
            assert env.step_to_kernel_kind == to_kind, "%s: step_to_kernel_kind %s" % (what, env.step_to_kernel_kind)
        assert env.last_step_entry == entry, "%s: last_step_entry %s" % (what, env.last_step_entry)
        # the library reports generic / wave / fixed only; which fast kernel a shape's line belongs to shows in the mask region it sizes:
        # 256 B per env for one wavefront, 256 B per wavefront and mask word for a group, one word for the crowd kernel
        xs, ys, P, E, R, fl = self.case.shape
        region = (env._flags.data_ptr() - env._state.data_ptr() - (-(-int(env.record_bytes) * self.n // 256) * 256)) // self.n
        family = "crowd" if max(P, E) > 64 else ("wave" if P + E <= 64 else "group")
        assert (region == 4) if family == "crowd" else (region == 256) if family == "wave" else (region >= 512 and region % 256 == 0), \
            "%s: a mask region of %d B per env is not the %s kernel's" % (what, region, family)
        assert env.per_env_counts == (self.case.counts is not None), what + ": per-env counts"

    def layout(self):
        """(record bytes per env, offset of the stale-zero masks, the bytes per env the kernels use of them, offset of the flag plane) of the
        state buffer: [records][pad to 256 B][mask region][flag plane] (csrc/pursuit.hip, "caller-owned state buffer").  The region has
        256 B per env, wavefront and mask word (the crowd kernel: one word per env); the one-wavefront kernels of a shape with 16 mask bits
        per lane use the first n_envs * 128 bytes of it, [n_envs][32] dwords, and only memsets touch the rest."""
        env = self.env
        rec = int(env.record_bytes)
        zoff = -(-rec * self.n // 256) * 256
        foff = env._flags.data_ptr() - env._state.data_ptr()
        assert (foff - zoff) % self.n == 0 and foff + 4 * self.n == env._state.numel()
        region = (foff - zoff) // self.n
        xs, ys, P, E, R, fl = self.case.shape
        one_wavefront = region == 256 and P + E <= 64
        return rec, zoff, 128 if one_wavefront and zm16_eligible(P, R, fl) else region, foff


def assert_slice_equals(big, small, at, what, result_big=None, result_small=None):
    """envs at .. at + small.n of `big` against the whole of `small`: every buffer a reset or a step writes, whole"""
    a, b, n = big.env, small.env, small.n
    sl = slice(at, at + n)
    assert bits_equal(a._obs[sl], b._obs), "%s: observation buffer" % what
    assert bits_equal(a._rew[sl], b._rew), "%s: rewards" % what
    assert torch.equal(a._done[sl], b._done), "%s: done bytes" % what
    assert torch.equal(a._removed[sl], b._removed), "%s: removed" % what
    assert torch.equal(a._flags[sl], b._flags), "%s: flag plane" % what
    (rec, zoff_a, mb, _fa), (rec_b, zoff_b, mb_b, _fb) = big.layout(), small.layout()
    assert rec == rec_b and mb == mb_b
    assert torch.equal(a._state[at * rec:(at + n) * rec], b._state[:n * rec]), "%s: state buffer, records" % what
    if mb:
        assert torch.equal(a._state[zoff_a + at * mb:zoff_a + (at + n) * mb], b._state[zoff_b:zoff_b + n * mb]), "%s: state buffer, stale-zero masks" % what
    sa, sb = a.get_state(), b.get_state()
    assert set(sa) == set(sb) and set(STATE_KEYS) <= set(sa)
    for k in sa:
        assert torch.equal(sa[k][sl], sb[k]), "%s: get_state()[%s]" % (what, k)
    if result_big is not None:
        (oa, ra, da, ia), (ob, rb, db, ib) = result_big, result_small
        assert bits_equal(oa[sl], ob) and bits_equal(ra[sl], rb) and torch.equal(da[sl], db), "%s: what step() returned" % what
        assert set(ia) == set(ib)
        for k in ia:
            assert torch.equal(ia[k][sl], ib[k]), "%s: info[%s]" % (what, k)


class PursuitProbeOracle(object):
    """the C oracle free-running beside a handle (tests/test_pursuit_fixed_gpu.py, _Oracle): its own Philox, reset(mask) after every
    step that ends an episode.  With per-env counts: one fixed-shape oracle batch per distinct (p, e), each env compared with the batch of
    its counts (tests/live_pursuit.py: an env at live (p, e) of a capacity is the (p, e) env; rows and rewards past p stay zero)."""

    def __init__(self, case, n_envs, offset, max_steps, counts=None, seed=None, base=None, tick=None):
        from oracle import pursuit as po
        self.case, self.N, self.H = case, n_envs, max_steps
        self.counts = None if counts is None else counts.cpu().numpy()
        groups = [(case.P, case.E)] if counts is None else sorted(set(map(tuple, self.counts.tolist())))
        self.orcs = {}
        for (p, e) in groups:
            kw = dict(case.kw, n_pursuers=p, n_evaders=e)
            self.orcs[(p, e)] = po.PursuitOracle(case.map_pool(), n_envs=n_envs, seed=SEED if seed is None else seed,
                                                 env_id_base=(ID_BASE if base is None else base) + offset, **kw)
        self.tstep = {g: np.zeros(n_envs, np.int64) for g in self.orcs}
        self.resets, self.removed = np.zeros(n_envs, np.int64), 0
        if tick is not None:
            self.set_tick(tick)

    def set_tick(self, tick):
        for o in self.orcs.values():
            st = o.get_state()
            st["tick"] = np.asarray(tick, np.uint32)
            o.set_state(st)

    def rows(self, g):
        return np.arange(self.N) if self.counts is None else np.nonzero((self.counts == np.asarray(g)).all(axis=1))[0]

    def _obs(self, env, g, what):
        p, o = g[0], self.orcs[g]
        rows = self.rows(g)
        got = env._obs.reshape(self.N, self.case.P, -1)[torch.as_tensor(rows, device=env._obs.device)].cpu()
        want = torch.from_numpy(o.obs[rows])
        if env._obs.dtype is torch.float16:   # each element the round-to-nearest-even half of the float32 value
            want = want.to(torch.float16)
        assert bits_equal(got[:, :p], want), "%s: %d observation cells differ from the oracle's" % (what, int((got[:, :p] != want).sum()))
        assert not bool(got[:, p:].any()), what + ": rows of pursuers that do not exist were written"

    def _state(self, env, g, what):
        (p, e), rows = g, self.rows(g)
        sg, so = env.get_state(), self.orcs[g].get_state()
        for k, n in (("pos_p", p), ("pos_e", e), ("gone", e), ("term_p", p), ("term_e", e)):
            assert np.array_equal(sg[k].cpu().numpy()[rows][:, :n], so[k][rows]), "%s: state[%s]" % (what, k)
        assert np.array_equal(sg["map_id"].cpu().numpy()[rows], so["map_id"][rows]), what + ": state[map_id]"
        assert np.array_equal(sg["tick"].cpu().numpy().view(np.uint32)[rows], so["tick"][rows]), what + ": tick"
        assert np.array_equal(sg["t"].cpu().numpy()[rows], self.tstep[g][rows]), what + ": episode step counter"

    def ticks(self):
        """uint32 [N]: every env's tick, from the oracle batch of its counts"""
        out = np.zeros(self.N, np.uint32)
        for g, o in self.orcs.items():
            out[self.rows(g)] = o.get_state()["tick"][self.rows(g)]
        return out

    def reset(self, env, what="reset", mask=None):
        for g, o in self.orcs.items():
            o.reset(mask=mask)
            if mask is None:
                self.tstep[g][:] = 0
            else:
                self.tstep[g][np.asarray(mask) != 0] = 0
            self._obs(env, g, what)
            self._state(env, g, what)

    def step(self, env, act, what):
        done_any = np.zeros(self.N, bool)
        for g, o in self.orcs.items():
            p, rows = g[0], self.rows(g)
            _oobs, orew, odone, orem = o.step(np.ascontiguousarray(act[:, :p]))
            self.tstep[g] += 1
            dbits = odone.astype(np.uint8) | ((self.tstep[g] >= self.H).astype(np.uint8) << 1)
            assert np.array_equal(env._done.cpu().numpy()[rows], dbits[rows]), what + ": done bits"
            assert np.array_equal(env._removed.cpu().numpy()[rows], orem[rows]), what + ": removed"
            rew = env._rew.cpu().numpy()
            assert np.array_equal(rew[rows][:, :p].view(np.int32), orew.astype(np.float32)[rows].view(np.int32)), what + ": rewards"
            assert not rew[rows][:, p:].any(), what + ": rewards of pursuers that do not exist"
            mask = (dbits != 0).astype(np.uint8)
            if mask.any():
                o.reset(mask=mask)
                self.tstep[g][mask != 0] = 0
            done_any[rows] = mask[rows] != 0
            self.removed += int(orem[rows].sum())
            self._obs(env, g, what)
            self._state(env, g, what)
        self.resets += done_any


M32 = 0xFFFFFFFF


def pursuit_policy_check(case, big, part, probe, N, per):
    """PursuitHeuristicPolicy over big's observation buffer as the steps left it: against the parts' policies (row_id_base advanced by the
    part's first row), on the tail against the probe's, and the probe's against oracle/heuristics_oracle.py -- rows that see no evader draw
    (Philox on the host: counter (row id low, tick, row id high, 3), as tests/test_policy_edges_gpu.py restates it).  Two calls on the
    buffers as the run left them, then two with the evader channel of every other env blanked, so that half the rows draw: four ticks.
    It edits the observation buffers and is therefore the last thing a case does."""
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    from oracle import heuristics_oracle as ho
    from oracle.pursuit import philox
    xs, ys, P, E, R, fl = case.shape
    assert not fl, "the oracle takes (R, R, 4) windows"
    seed = (7 << 32) | 5
    mk = lambda off: PursuitHeuristicPolicy(R, flatten=False, seed=seed, row_id_base=off * P)
    pol_big, pol_probe, pol_part = mk(0), mk(N - PROBE), [mk(j * per) for j in range(len(part))]
    tick = n_drawn = 0
    for phase in ("as the steps left it", "evader channel of every other env blanked"):
        if phase != "as the steps left it":   # (the last use of these buffers: the rows of those envs see no evader and draw)
            for r in [big] + part + [probe]:
                sel = (torch.arange(r.n, device=DEV) + r.offset) % 2 == 0
                r.env._obs.view(r.n, P, R, R, 4)[sel, :, :, :, 2] = 0
        win = probe.env._obs.cpu().numpy().reshape(PROBE * P, R, R, 4)
        ref = ho.pursuit_actions(win)
        drawn = np.flatnonzero(ref < 0)
        n_drawn += len(drawn)
        for _call in range(2):
            ab = pol_big(big.env._obs_view()).clone()
            assert tuple(ab.shape) == (N, P) and int(ab.min()) >= 0 and int(ab.max()) <= 4
            for j, r in enumerate(part):
                assert torch.equal(ab[j * per:(j + 1) * per], pol_part[j](r.env._obs_view())), "policy, %s, call %d: part %d" % (phase, tick, j)
            ap = pol_probe(probe.env._obs_view())
            assert torch.equal(ab[N - PROBE:], ap), "policy, %s, call %d: big's tail against the probe" % (phase, tick)
            want = ref.copy()
            for i in drawn:
                rid = (N - PROBE) * P + int(i)
                want[i] = (int(philox((rid & M32, tick, rid >> 32, 3), (seed & M32, seed >> 32))[0]) * 5) >> 32
            assert np.array_equal(ap.cpu().numpy().reshape(-1), want), "policy, %s, call %d: the probe against the oracle" % (phase, tick)
            tick += 1
    assert n_drawn >= PROBE * P // 2, "the rows without an evader in sight draw"
    return n_drawn


def assert_big_equals_parts(case, monkeypatch, line_bytes=2**32, parts=None, steps=8, max_steps=3, mask_reset_first=False, policy=False):
    """The three comparisons of one case, after reset(), after each of `steps` steps (max_steps 3 with auto-reset: every env goes through
    fused resets) and after one reset(mask=) on every third env: big against its parts over the whole buffers, big's last 48 envs against
    the probe, the probe against the oracle.  mask_reset_first: the masked reset follows the first reset directly (the half-precision
    cases: a half reset needs a float32 copy of twice the buffer's bytes, which is affordable only while the parts do not exist yet).
    Returns (N, K, bytes of big's observation buffer)."""
    row, held, passing = case.row_bytes()
    N, K = plan(row, line_bytes, parts)
    per = N // K
    n_bufs = {"step": 1, "step_to": 2, "half": 2}[case.mode]
    # big and the parts: n_bufs observation buffers each and their small buffers; a half reset: one float32 copy of twice the buffer's
    # bytes (big's while no part exists, later one part's); the actions and get_state() copies of big and of one part; 64 MiB to spare
    peak = 2 * n_bufs * N * row + (2 * per * row if case.mode == "half" else 0) + 2 * N * held + (N + per) * passing + 2**26
    assert peak < 20 * 2**30, "the case is planned at %.2f GiB, above 20 GiB" % (peak / 2.0**30)
    need_device_bytes(peak)
    torch.cuda.reset_peak_memory_stats()
    third = (torch.arange(N, device=DEV) % 3 == 0)
    big = Run(case, N, 0, max_steps, monkeypatch)
    assert big.env._obs.numel() * big.env._obs.element_size() == N * row >= line_bytes + BEYOND * row
    assert not bool(big.env._obs.any())
    big.reset(last=not mask_reset_first)
    if mask_reset_first:
        big.reset(mask=third)
    part = [Run(case, per, j * per, max_steps, monkeypatch) for j in range(K)]
    probe = Run(case, PROBE, N - PROBE, max_steps, monkeypatch)
    orc = PursuitProbeOracle(case, PROBE, N - PROBE, max_steps, counts=None if case.counts is None else case.counts_of(N - PROBE, PROBE))
    for j, r in enumerate(part + [probe]):
        assert r.env._obs.numel() * r.env._obs.element_size() < 2**31
        r.reset(last=not mask_reset_first)
        if r is probe:
            orc.reset(probe.env)
        if mask_reset_first:
            r.reset(mask=third[r.offset:r.offset + r.n])
    if mask_reset_first:
        orc.reset(probe.env, "reset(mask=)", mask=third[N - PROBE:].cpu().numpy().astype(np.uint8))

    def compare(what, results=None):
        for j, r in enumerate(part):
            assert_slice_equals(big, r, j * per, "%s, part %d of %d" % (what, j, K), *(() if results is None else (results[0], results[1 + j])))
        assert_slice_equals(big, probe, N - PROBE, what + ", the probe", *(() if results is None else (results[0], results[-1])))

    compare("after reset")
    gen = torch.Generator(device=DEV).manual_seed(7)
    for t in range(steps):
        act = torch.randint(0, 5, (N, case.P), generator=gen, device=DEV, dtype=torch.int32)
        results = [big.step(act)]
        for r in part + [probe]:
            results.append(r.step(act[r.offset:r.offset + r.n].contiguous()))
        for r in [big, probe] + part:
            r.check_kinds("step %d" % t)
        compare("step %d" % t, results)
        orc.step(probe.env, act[N - PROBE:].cpu().numpy(), "step %d, the probe" % t)
    assert bool((orc.resets >= steps // max_steps).all()), "every probe env went through the fused reset"
    if not mask_reset_first:
        for r in [big] + part + [probe]:
            r.reset(mask=third[r.offset:r.offset + r.n])
        compare("after reset(mask=)")
        orc.reset(probe.env, "reset(mask=)", mask=third[N - PROBE:].cpu().numpy().astype(np.uint8))
    if policy:
        print("policy: %d probe rows drew" % pursuit_policy_check(case, big, part, probe, N, per))
    used = torch.cuda.max_memory_allocated()
    assert used < 20 * 2**30, "%.1f GiB of device memory at the peak" % (used / 2.0**30)
    print("N=%d K=%d row=%d B buffer=%.3f GiB peak=%.2f GiB removed=%d" % (N, K, row, N * row / 2.0**30, used / 2.0**30, orc.removed))
    del big, part, probe, results
    free_device()
    return N, K, N * row


# ------------------------------------------------------------------------------------------------- Waterworld and the hostage world
class ParticleCase(object):
    """one kernel of a particle world at one shape.  world: 'waterworld' | 'hostage'; args / kw: the constructor's; kind: 'wave' | 'crowd'"""

    def __init__(self, world, args, kind, **kw):
        self.world, self.args, self.kind, self.kw = world, tuple(args), kind, kw

    def _classes(self):
        if self.world == "waterworld":
            from madrl_amd.waterworld import BatchedMAWaterWorld as Env
            from oracle.waterworld import WaterworldOracle as Orc
        else:
            from madrl_amd.hostage import BatchedContinuousHostageWorld as Env
            from oracle.hostage import HostageOracle as Orc
        return Env, Orc

    def make(self, n_envs, offset, max_steps):
        env = self._classes()[0](*self.args, n_envs=n_envs, device=DEV, seed=SEED, env_id_base=ID_BASE + offset, max_steps=max_steps, auto_reset=True,
                                 crowd=(self.kind == "crowd"), **self.kw)
        assert env.kernel_kind == self.kind, env.kernel_kind
        return env

    def oracle(self, n_envs, offset, max_steps):
        return self._classes()[1](*self.args, n_envs=n_envs, seed=SEED, env_id_base=ID_BASE + offset, max_steps=max_steps, dtype=np.float32, **self.kw)


def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_particle_slice_equals(a, b, at, what, result_a=None, result_b=None):
    """envs at .. at + b.n_envs of handle `a` against the whole of handle `b`: every buffer a reset or a step writes, whole"""
    n = b.n_envs
    sl = slice(at, at + n)
    assert bits_equal(a._obs[sl], b._obs), "%s: observation buffer" % what
    assert bits_equal(a._rew[sl], b._rew), "%s: rewards" % what
    assert torch.equal(a._done[sl], b._done), "%s: done bytes" % what
    assert torch.equal(a._info[sl], b._info), "%s: info counters" % what
    rec = b._state.numel() // n
    assert b._state.numel() == n * rec and a._state.numel() == a.n_envs * rec
    assert torch.equal(a._state[at * rec:(at + n) * rec], b._state), "%s: state buffer" % what
    sa, sb = a.get_state(), b.get_state()
    assert set(sa) == set(sb)
    for k in sa:
        assert bits_equal(sa[k][sl], sb[k]), "%s: get_state()[%s]" % (what, k)
    if result_a is not None:
        (oa, ra, da, ia), (ob, rb, db, ib) = result_a, result_b
        assert bits_equal(oa[sl], ob) and bits_equal(ra[sl], rb) and torch.equal(da[sl], db), "%s: what step() returned" % what
        assert set(ia) == set(ib)
        for k in ia:
            assert torch.equal(ia[k][sl], ib[k]), "%s: info[%s]" % (what, k)


def assert_particle_probe_equals_oracle(env, orcs, what):
    """orcs: [(oracle, the observation rows it speaks for)] -- one oracle and every row, except for a batch with per-pursuer sensor
    ranges, whose row i is row i of a batch with sensor_range[i]"""
    got, gst = env._obs.cpu().numpy(), env.get_state()
    for orc, rows in orcs:
        assert np.array_equal(_raw(got[:, rows]), _raw(orc.obs[:, rows])), "%s: observations differ from the oracle's" % what
        ost = orc.get_state()
        for k in ost:
            g = gst[k].cpu().numpy()   # (the tick: int32 here, uint32 in the oracle -- the same 32 bits)
            assert np.array_equal(_raw(g), _raw(np.asarray(ost[k]).astype(g.dtype))), "%s: state[%s]" % (what, k)


def particle_oracle_step(env, orcs, act, what):
    """one free-running step of the oracles beside a handle that has just stepped on `act` (tests/test_hostage_gpu.py,
    test_waterworld_crowd_gpu.py): the oracle has no auto-reset of its own and resets the envs the step ended; then observations and
    every state key must be equal in every bit.  -> (episodes ended, info events)"""
    for orc, _rows in orcs:
        _oo, orew, odone, oinfo = orc.step(act)
        assert np.array_equal(env._done.cpu().numpy() != 0, odone != 0), what + ": done"
        assert np.array_equal(_raw(env._rew.cpu().numpy()), _raw(orew)), what + ": rewards"
        assert np.array_equal(env._info.cpu().numpy(), oinfo), what + ": info counters"
        if (odone != 0).any():
            orc.reset(mask=(odone != 0).astype(np.uint8))
    assert_particle_probe_equals_oracle(env, orcs, what)
    return int((odone != 0).sum()), int(oinfo.sum())


def waterworld_policy_check(big, part, probe, N, per):
    """WaterworldHeuristicPolicy over big's observation buffer: against the parts', the probe's, and oracle/heuristics_oracle.py (the
    1e-5 of tests/test_heuristics_gpu.py: float32 actions of a float64 expression)"""
    from madrl_amd.heuristics import WaterworldHeuristicPolicy
    from oracle import heuristics_oracle as ho
    ab = WaterworldHeuristicPolicy()(big._obs).clone()
    assert tuple(ab.shape) == (N, big._obs.shape[1], 2) and bool(torch.isfinite(ab).all())
    for j, p in enumerate(part):
        assert bits_equal(ab[j * per:(j + 1) * per], WaterworldHeuristicPolicy()(p._obs)), "policy: part %d" % j
    ap = WaterworldHeuristicPolicy()(probe._obs)
    assert bits_equal(ab[N - PROBE:], ap), "policy: big's tail against the probe"
    want = ho.waterworld_actions(probe._obs.cpu().numpy().reshape(-1, probe._obs.shape[-1]))
    err = np.abs(ap.cpu().numpy().reshape(-1, 2) - want).max()
    assert err < 1e-5 and np.abs(want).max() > 0.5, "policy: the probe against the oracle, max error %r" % err


def assert_big_equals_parts_particle(case, steps=8, max_steps=3, policy=False):
    """assert_big_equals_parts for a particle world, against the float32 oracle bit for bit (as tests/test_edge_cases_gpu.py uses it).
    Returns (N, K, bytes of big's observation buffer)."""
    one = case.make(1024, 0, 1)
    Na, D = one._obs.shape[1], one._obs.shape[2]
    row = Na * D * one._obs.element_size()
    held = one._state.numel() // 1024 + 4 * Na + 1 + 8
    passing = 8 * Na + sum(v[0].numel() * v.element_size() for v in one.get_state().values())
    del one
    N, K = plan(row)
    per = N // K
    peak = 2 * N * row + 2 * N * held + (N + per) * passing + 2**26
    assert peak < 20 * 2**30, "the case is planned at %.2f GiB, above 20 GiB" % (peak / 2.0**30)
    need_device_bytes(peak)
    torch.cuda.reset_peak_memory_stats()
    big = case.make(N, 0, max_steps)
    assert big._obs.numel() * 4 == N * row >= 2**32 + BEYOND * row and not bool(big._obs.any())
    part = [case.make(per, j * per, max_steps) for j in range(K)]
    probe, orcs = case.make(PROBE, N - PROBE, max_steps), [(case.oracle(PROBE, N - PROBE, max_steps), np.arange(Na))]
    assert all(p._obs.numel() * 4 < 2**31 for p in part)
    third = torch.arange(N, device=DEV) % 3 == 0

    def compare(what, results=None):
        for j, p in enumerate(part):
            assert_particle_slice_equals(big, p, j * per, "%s, part %d of %d" % (what, j, K), *(() if results is None else (results[0], results[1 + j])))
        assert_particle_slice_equals(big, probe, N - PROBE, what + ", the probe", *(() if results is None else (results[0], results[-1])))

    for e in [big] + part + [probe]:
        e.reset()
    orcs[0][0].reset()
    compare("after reset")
    assert_particle_probe_equals_oracle(probe, orcs, "after reset")
    gen = torch.Generator(device=DEV).manual_seed(7)
    n_done = events = 0
    for t in range(steps):
        act = torch.rand((N, Na, 2), generator=gen, device=DEV, dtype=torch.float32) * 2 - 1
        results = [big.step(act)] + [p.step(act[j * per:(j + 1) * per]) for j, p in enumerate(part)] + [probe.step(act[N - PROBE:])]
        for e in [big] + part + [probe]:
            assert e.kernel_kind == case.kind
        compare("step %d" % t, results)
        d, ev = particle_oracle_step(probe, orcs, act[N - PROBE:].cpu().numpy(), "step %d, the probe" % t)
        n_done, events = n_done + d, events + ev
    assert n_done >= PROBE * (steps // max_steps), "every probe env went through the fused reset"
    if policy:
        waterworld_policy_check(big, part, probe, N, per)
    for e, at in [(big, 0)] + [(p, j * per) for j, p in enumerate(part)] + [(probe, N - PROBE)]:
        e.reset(mask=third[at:at + e.n_envs])
    orcs[0][0].reset(mask=third[N - PROBE:].cpu().numpy().astype(np.uint8))
    compare("after reset(mask=)")
    assert_particle_probe_equals_oracle(probe, orcs, "after reset(mask=)")
    used = torch.cuda.max_memory_allocated()
    assert used < 20 * 2**30, "%.1f GiB of device memory at the peak" % (used / 2.0**30)
    print("N=%d K=%d row=%d B buffer=%.3f GiB peak=%.2f GiB events=%d" % (N, K, row, N * row / 2.0**30, used / 2.0**30, events))
    del big, part, probe, results
    free_device()
    return N, K, N * row


STD = dict(scale_reward=0.7, enable_obsnorm=True, enable_rewnorm=True, obs_alpha=0.05, rew_alpha=0.05)
STD_NAMES = ("obs_mean", "obs_var", "obs_out", "rew_mean", "rew_var", "rew_out")


def assert_fused_std_big_equals_parts(case, steps=6, max_steps=3):
    """The fused StandardizedEnv step and reset of a particle world (bind_standardize: the FUSED instantiations, whose std_obs_row takes a
    base of its own, env * n_el).  The float64 statistics [N][agents][D] of big pass 2^32 bytes, its standardised float32 rows 2^31 -- a
    row buffer past 2^32 bytes would take 26 GiB with its statistics, above what a test may use.  The parts run one after the other on
    the same seeded actions: rewards, done bytes and info counters are compared per step (big's are kept), everything else -- statistics,
    standardised rows, raw state, every get_state() key -- after the last step and after the reset(mask=) that follows it.  The probe
    also runs beside an unfused 48-env twin whose raw outputs go through oracle/wrappers_oracle.py (the 1e-5 of tests/test_hostage_std_gpu.py)."""
    from oracle import wrappers_oracle as wo
    one = case.make(64, 0, 1)
    Na, D = one._obs.shape[1], one._obs.shape[2]
    del one
    N, K = plan(Na * D * 8)
    per = N // K
    need_device_bytes((N + per) * Na * D * 28 + 2**30)
    torch.cuda.reset_peak_memory_stats()
    gen = torch.Generator(device=DEV).manual_seed(7)
    acts = [torch.rand((N, Na, 2), generator=gen, device=DEV, dtype=torch.float32) * 2 - 1 for _ in range(steps)]
    third = torch.arange(N, device=DEV) % 3 == 0

    def run(n, at, keep=None, twin=None):
        """-> (env, its bound tensors, [(rewards, done, info) per step]); keep: big's history, compared as the steps go"""
        env = case.make(n, at, max_steps)
        st = env.bind_standardize(**STD)
        assert env._std is st and env.kernel_kind == case.kind and env.fused_standardize
        if twin is not None:
            raw, so = twin
            ref = so.obs(raw.reset().cpu().numpy())
        o = env.reset()
        assert o.data_ptr() == st["obs_out"].data_ptr()
        if twin is not None:
            assert np.abs(o.cpu().numpy() - ref).max() < 1e-5, "reset: the probe against the wrapper oracle"
        hist = []
        for t, a in enumerate(acts):
            o, r, _d, _i = env.step(a[at:at + n])
            assert o.data_ptr() == st["obs_out"].data_ptr() and r.data_ptr() == st["rew_out"].data_ptr()
            if keep is None:
                hist.append((r.clone(), env._done.clone(), env._info.clone()))
            else:
                for name, mine, theirs in zip(("rewards", "done bytes", "info counters"), (r, env._done, env._info), keep[t]):
                    assert bits_equal(theirs[at:at + n], mine), "step %d, envs from %d: %s" % (t, at, name)
            if twin is not None:
                ro, rr, _rd, _ri = raw.step(a[at:at + n])
                assert np.abs(o.cpu().numpy() - so.obs(ro.cpu().numpy())).max() < 1e-5, "step %d: the probe's rows against the wrapper oracle" % t
                want = so.rew(rr.cpu().numpy())
                assert np.abs(r.cpu().numpy() - want).max() < 1e-5 * max(1.0, np.abs(want).max()), "step %d: the probe's rewards" % t
        return env, st, hist

    def same(a_env, a_st, b_env, b_st, at, what):
        n = b_env.n_envs
        for name in STD_NAMES:
            assert bits_equal(a_st[name][at:at + n], b_st[name]), "%s: %s" % (what, name)
        rec = b_env._state.numel() // n
        assert torch.equal(a_env._state[at * rec:(at + n) * rec], b_env._state), what + ": state buffer"
        sa, sb = a_env.get_state(), b_env.get_state()
        for k in sa:
            assert bits_equal(sa[k][at:at + n], sb[k]), "%s: get_state()[%s]" % (what, k)

    big, bst, hist = run(N, 0)
    assert bst["obs_mean"].numel() * 8 >= 2**32 + BEYOND * Na * D * 8 and bst["obs_out"].numel() * 4 > 2**31
    n_done = int(sum(int((h[1] != 0).sum()) for h in hist))
    assert n_done >= N * (steps // max_steps), "every env went through the fused reset"
    # (the comparison after the last step needs big as it was then: the parts are compared first, then everybody resets under the mask)
    runs = []
    for j in range(K + 1):
        at, n = (j * per, per) if j < K else (N - PROBE, PROBE)
        twin = None
        if j == K:
            twin = (case.make(PROBE, N - PROBE, max_steps), wo.StdOracle((PROBE, Na, D), (PROBE, Na), **STD))
        env, st, _ = run(n, at, keep=hist, twin=twin)
        assert all(st[name].numel() * st[name].element_size() < 2**31 for name in STD_NAMES)
        same(big, bst, env, st, at, "after the last step, envs from %d" % at)
        env.reset(mask=third[at:at + n])
        if j < K:   # what the part holds after its masked reset, for the comparison once big has had its own
            runs.append((at, {name: st[name].cpu() for name in ("rew_mean", "rew_var", "rew_out")}, env._state.cpu(), st["obs_out"][:PROBE].clone(),
                         st["obs_mean"][-PROBE:].clone()))
            del env, st
            free_device()
        else:
            probe, pst = env, st
    big.reset(mask=third)
    same(big, bst, probe, pst, N - PROBE, "after reset(mask=), the probe")
    for at, small, state, head_out, tail_mean in runs:
        for name, v in small.items():
            assert bits_equal(bst[name][at:at + per].cpu(), v), "after reset(mask=), envs from %d: %s" % (at, name)
        rec = state.numel() // per
        assert torch.equal(big._state[at * rec:(at + per) * rec].cpu(), state), "after reset(mask=), envs from %d: state buffer" % at
        assert bits_equal(bst["obs_out"][at:at + PROBE], head_out) and bits_equal(bst["obs_mean"][at + per - PROBE:at + per], tail_mean), \
            "after reset(mask=), envs from %d: rows / statistics at the part's ends" % at
    used = torch.cuda.max_memory_allocated()
    assert used < 20 * 2**30, "%.1f GiB of device memory at the peak" % (used / 2.0**30)
    print("fused std N=%d K=%d statistics=%.3f GiB each, rows=%.3f GiB, peak=%.2f GiB" % (N, K, N * Na * D * 8 / 2.0**30, N * Na * D * 4 / 2.0**30, used / 2.0**30))
    del big, bst, probe, pst, hist, runs, acts
    free_device()
    return N, K


# ------------------------------------------------------------------------------------------------------------------ MultiWalker
MW_LANES = {3: 4, 7: 8, 10: 16}   # lanes per env of the three capacity classes


def mw_make(n_envs, n_walkers, fused, max_steps, base):
    from madrl_amd.multiwalker import BatchedMultiWalkerEnv
    env = BatchedMultiWalkerEnv(n_envs=n_envs, device=DEV, n_walkers=n_walkers, position_noise=0.0, angle_noise=0.0, seed=SEED, env_id_base=base,
                                auto_reset=True, max_steps=max_steps)
    if fused:
        env.set_mode(fused=True)
    assert env.lanes_per_env == MW_LANES.get(n_walkers, env.lanes_per_env) and getattr(env, "_mode", (0, 1)) == (int(fused), 1)
    return env


class MwProbeOracle(object):
    """the CPU build of the product's source free-running beside a handle with auto-reset through spares
    (tests/test_multiwalker_gpu.py, test_auto_reset_through_spares_matches_mask_resets): whole world records byte for byte"""

    def __init__(self, n_envs, n_walkers, max_steps, base):
        from oracle import multiwalker as mwo
        self.orc = mwo.MultiWalkerOracle(n_walkers=n_walkers, position_noise=0.0, angle_noise=0.0, n_envs=n_envs, seed=SEED, env_id_base=base)
        self.H, self.tstep, self.resets = max_steps, np.zeros(n_envs, np.int64), 0

    def same_worlds(self, env, what):
        same = (env.state_buffer.cpu().numpy()[:, :self.orc.world_bytes] == self.orc.worlds()).all(axis=1)
        assert same.all(), "%s: %d world records differ from the CPU build's" % (what, int((~same).sum()))

    def reset(self, env, what="reset", mask=None):
        self.orc.reset(mask=mask)
        self.tstep[:] = 0 if mask is None else np.where(np.asarray(mask) != 0, 0, self.tstep)
        assert np.array_equal(env._obs.cpu().numpy(), self.orc.obs), what + ": observations"
        self.same_worlds(env, what)

    def step(self, env, act, what):
        _oobs, orew, odone = self.orc.step(act)
        self.tstep += 1
        ends = odone.astype(bool) | (self.tstep >= self.H)
        assert np.array_equal(env._done.cpu().numpy() != 0, ends), what + ": which episodes ended"
        assert np.array_equal(env._rew.cpu().numpy(), orew), what + ": rewards"
        if ends.any():
            self.orc.reset(mask=ends.astype(np.uint8))
            self.tstep[ends] = 0
        self.resets += int(ends.sum())
        assert np.array_equal(env._obs.cpu().numpy(), self.orc.obs), what + ": observations (the next episode's first one where an episode ended)"
        self.same_worlds(env, what)
