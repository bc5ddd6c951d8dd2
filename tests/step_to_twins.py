"""One twin harness for the two-buffer Pursuit step (test_step_to_gpu.py, test_step_to_group_gpu.py, test_step_to_f16_gpu.py,
test_step_to_group_f16_gpu.py): step_to / madrl_pursuit_step_to / madrl_pursuit_step_to_f16.  A plain module, not collected.  Nothing in
it needs a GPU: the device is an argument, and tests/test_step_to_twins_cpu.py runs every comparison below over a stand-in env on CPU
tensors and shows that a single wrong bit fails it.

A Case says what a pair of twins runs; make_env() builds one env of it, prefill() fills its buffer with 7.0 (no observation value, exact
in binary16) and tells the env so, a Ring is three slots with guard bands between them.  Both twin classes draw their actions alike
(Twins.actions) and compare rewards, done, the four info keys (Twins.check_outputs) and the state (Twins.check_state) alike.

InPlaceTwins: `ref` steps in place -- the yardstick, which the rest of the suite pins to the reference's goldens and the C oracle --
and `env` through a ring of three buffers whose first slot is its own buffer; the other slots start as 101.0 and 102.0.  It asserts
  * __init__: the reset observations are equal in bits;
  * hop: observations, rewards, done, done_bits, removed, truncated, count_overflow are equal; the returned tensor and obs_buffer are the
    slot (data_ptr); the slot equals the in-place buffer in bits; the previous slot is unchanged;
  * in_place: the same outputs, and the current slot equals the in-place buffer in bits;
  * check_state: every key of get_state() is equal.

HalfTwins: `f`, a float32 env on a guarded float32 Ring, and `h`, a half env on a guarded half Ring.  The half of a float32 twin's
element is its `.to(float16)` (round to nearest even); a kept element is 16 bits carried over.  It asserts
  * __init__: the dtypes of the two buffers; the reset's dtype, shape and same16; both buffers hold as many 7.0 after the reset;
  * hop: the guard bands of both rings are intact; dtype, shape and pointer identity (slot, obs_buffer) of the returned tensor; same16 of
    the slot, with the count of differing elements in the message; rewards as int32 bits; done; the four info keys; obs_prev unchanged as
    16-bit words;
  * finish: every env ended an episode (counted per env); the state is equal; changed per-env counts were taken; in both envs
    0 < elements that still read 7.0 < those after the reset; the sightings the case asks for (rne, subnormal)."""
import collections

import numpy as np
import torch

from helpers import same_bits
from pursuit_cases import maps

DEV = "cuda:0"
GUARD, GUARD_BYTE = 4096, 0xA5
F16, F32 = torch.float16, torch.float32
INFO_KEYS = ("done_bits", "removed", "truncated", "count_overflow")

# maps: a kind of pursuit_cases.maps; size: (xs, ys); env: constructor kwargs; counts: per-env (pursuers, evaders) or None;
# twin: make_env kwargs of this case (seed, max_steps, max_blocks, walk) and evader_actions / rne / subnormal of the twins;
# a file's own columns: n envs, steps, the step_to_kernel_kind it expects
Case = collections.namedtuple("Case", "maps size env counts twin n steps kind", defaults=({}, None, None, None))


def agents(p, e, r, fl, **kw):
    return dict(n_pursuers=p, n_evaders=e, obs_range=r, flatten=bool(fl), **kw)


def make_env(case, obs_dtype=F32, n=7, seed=21, max_steps=3, max_blocks=2, walk=None, device=DEV, **kw):
    from madrl_amd.pursuit import BatchedPursuitEvade
    env = BatchedPursuitEvade(maps(case.maps, *case.size), n_envs=n, device=device, seed=seed, max_steps=max_steps, auto_reset=True,
                              obs_dtype=obs_dtype, **dict(case.env, **kw))
    if max_blocks is not None:
        env.set_launch(max_blocks=max_blocks)   # 2: a workgroup walks several envs, the loop-carried state is exercised
    if walk is not None:
        env.set_walk(walk)
    return env


def prefill(env, counts=None):
    env.obs_buffer.fill_(7.0)
    env.invalidate_obs()
    if counts is not None:
        c = torch.tensor(counts, dtype=torch.int32, device=env.obs_buffer.device)
        env.set_agent_counts(c[:, 0], c[:, 1])


def b16(t):
    return t.contiguous().view(torch.int16)


def as_half_bits(t):
    """the bits the half twin must hold where the float32 twin holds t"""
    return b16(t.to(F16)) if t.dtype is F32 else b16(t)


def same16(half, ref):
    assert half.dtype is F16
    return torch.equal(b16(half).reshape(-1), as_half_bits(ref).reshape(-1))


class Ring(object):
    """n slots of `shape` carved from one byte tensor: [guard][slot 0][guard][slot 1] ... [guard]"""

    def __init__(self, shape, dtype, n=3, device=DEV):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        stride = (nbytes + 15) // 16 * 16 + GUARD
        self.raw = torch.full((GUARD + n * stride,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.is_guard = torch.ones(self.raw.numel(), dtype=torch.bool, device=device)
        self.slots = []
        for k in range(n):
            off = GUARD + k * stride
            self.slots.append(self.raw[off:off + nbytes].view(dtype).view(shape))
            self.is_guard[off:off + nbytes] = False
            assert self.slots[-1].data_ptr() % 16 == 0
        for s in self.slots:
            s.fill_(7.0)

    def intact(self):
        return bool((self.raw[self.is_guard] == GUARD_BYTE).all())


class Twins(object):
    """what the two kinds of twins share: the envs of a case, the action draws, the pending counts, the comparisons beside the
    observations"""

    def __init__(self, case, n, device, make, mk):
        tkw = dict(case.twin)
        self.with_eact = tkw.pop("evader_actions", False)
        self.want_rne, self.want_subnormal = tkw.pop("rne", False), tkw.pop("subnormal", False)
        self.case, self.counts, self.kind, self.dev = case, case.counts, case.kind, torch.device(device)
        self.n = case.n if n is None else n
        self._make, self._mk = make, dict(mk, **tkw)
        self.at = 0
        self.gen = torch.Generator(device="cpu").manual_seed(5)

    def make(self, obs_dtype=F32):
        return self._make(self.case, obs_dtype, n=self.n, device=self.dev, **self._mk)

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()

    def actions(self):
        """(pursuer actions, evader actions or None)"""
        act = torch.randint(0, 5, (self.n, self.P), generator=self.gen).to(torch.int32).to(self.dev)
        eact = torch.randint(0, 5, (self.n, self.E), generator=self.gen).to(torch.int32).to(self.dev) if self.with_eact else None
        return act, eact

    def recount(self):
        """per-env counts: other pending counts, taken at each env's next fused reset (the row count of an env changes between the passes)"""
        if self.counts is None:
            return
        c = torch.tensor(self.counts[::-1], dtype=torch.int32, device=self.dev)
        for e in self.envs:
            e.set_agent_counts(c[:, 0], c[:, 1])

    def check_outputs(self, ra, rb, what):
        (_oa, rwa, da, ia), (_ob, rwb, db, ib) = ra, rb
        assert same_bits(rwa, rwb), (what, "rewards")
        assert torch.equal(da, db), (what, "done")
        for k in INFO_KEYS:
            assert torch.equal(ia[k], ib[k]), (what, k)

    def check_state(self):
        a, b = (e.get_state() for e in self.envs)
        for k in a:
            assert torch.equal(a[k], b[k]), k


class InPlaceTwins(Twins):
    """`ref` steps in place; `env` steps through `ring`, whose first slot is its own buffer"""

    def __init__(self, case, n=None, device=DEV, make=make_env, **mk):
        Twins.__init__(self, case, n, device, make, mk)
        self.ref, self.env = self.envs = self.make(), self.make()
        self.P, self.E = int(self.ref.n_pursuers), int(self.ref.n_evaders)
        for e in self.envs:
            prefill(e, self.counts)
        first = self.env.obs_buffer
        self.ring = [first, torch.full_like(first, 101.0), torch.full_like(first, 102.0)]
        a, b = self.ref.reset(), self.env.reset()
        assert same_bits(a, b)

    def check_results(self, ra, rb, what):
        assert same_bits(ra[0], rb[0]), (what, "observations")
        self.check_outputs(ra, rb, what)

    def hop(self, what):
        act, eact = self.actions()
        nxt = (self.at + 1) % 3
        prev_before = self.ring[self.at].clone()
        ra = self.ref.step(act, evader_actions=eact)
        rb = self.env.step_to(act, self.ring[nxt], evader_actions=eact)
        self.check_results(ra, rb, what)
        assert rb[0].data_ptr() == self.ring[nxt].data_ptr() and self.env.obs_buffer.data_ptr() == self.ring[nxt].data_ptr()
        assert same_bits(self.ring[nxt], self.ref.obs_buffer), (what, "slot")
        assert same_bits(self.ring[self.at], prev_before), (what, "the previous slot was written")
        self.at = nxt

    def in_place(self, what):
        act, eact = self.actions()
        self.check_results(self.ref.step(act, evader_actions=eact), self.env.step(act, evader_actions=eact), what)
        assert same_bits(self.ring[self.at], self.ref.obs_buffer), (what, "slot")


class HalfTwins(Twins):
    """`f`: the float32 twin and its ring `fr`; `h`: the half env and its ring `hr`"""

    def __init__(self, case, n=None, half_kernel=None, device=DEV, make=make_env, **mk):
        Twins.__init__(self, case, n, device, make, mk)
        self.f, self.h = self.envs = self.make(), self.make(F16)
        if half_kernel is not None:
            self.h.set_kernel(half_kernel)
        assert self.f.obs_buffer.dtype is F32 and self.h.obs_buffer.dtype is F16
        self.P, self.E = int(self.f.n_pursuers), int(self.f.n_evaders)
        for e in self.envs:
            prefill(e, self.counts)
        shape = tuple(self.f.obs_buffer.shape)
        self.fr, self.hr = Ring(shape, F32, device=self.dev), Ring(shape, F16, device=self.dev)
        a, b = self.f.reset(), self.h.reset()
        assert b.dtype is F16 and b.shape == a.shape
        assert same16(b, a), "reset() of the half env is not the float32 twin's reset .to(float16)"
        self.sevens_at_start = int((self.h.obs_buffer == 7.0).sum())
        assert self.sevens_at_start == int((self.f.obs_buffer == 7.0).sum())
        self.rne_differs = self.subnormal = False   # seen: an element whose nearest-even and truncated halves differ / a subnormal half
        self.dones = torch.zeros(self.n, dtype=torch.int64, device=self.dev)   # episodes ended, per env

    def hop(self, what, act=None):
        act, eact = self.actions() if act is None else (act, None)
        k = self.at
        prev = self.h.obs_buffer
        prev_before = prev.clone()
        fo, frew, fdone, finfo = rf = self.f.step_to(act, self.fr.slots[k], evader_actions=eact)
        ho, hrew, hdone, hinfo = rh = self.h.step_to(act, self.hr.slots[k], evader_actions=eact)
        self.sync()
        assert self.hr.intact() and self.fr.intact(), (what, "a guard band was written")
        assert ho.dtype is F16 and ho.shape == fo.shape and ho.data_ptr() == self.hr.slots[k].data_ptr() == self.h.obs_buffer.data_ptr()
        fs, hs = self.fr.slots[k], self.hr.slots[k]
        assert same16(hs, fs), (what, "slot", int((b16(hs) != as_half_bits(fs)).sum()))
        self.check_outputs(rf, rh, what)
        assert torch.equal(b16(prev), b16(prev_before)), (what, "obs_prev was written")
        # positive float32 values whose half was rounded UP: truncation would have given the half below
        self.rne_differs = self.rne_differs or bool((hs.to(F32) > fs).any())
        bits = b16(hs).to(torch.int32) & 0xFFFF
        self.subnormal = self.subnormal or bool(((bits > 0) & (bits < 0x0400)).any())
        self.dones += (finfo["done_bits"] != 0).to(torch.int64)
        self.at = (k + 1) % 3
        self.last_rew = hrew
        return hs

    def run(self, hops):
        for k in range(hops):
            if k == hops // 2:
                self.recount()
            self.hop(k)

    def finish(self):
        assert bool((self.dones >= 1).all()) and int(self.dones.sum()) >= self.n, "every env ended an episode: the second pass of a fused auto-reset ran"
        self.check_state()
        if self.counts is not None:
            assert not torch.equal(self.h.agent_counts()[1].cpu(), torch.tensor(self.counts, dtype=torch.int32)), "the changed counts were never taken"
        for env in self.envs:
            left = int((env.obs_buffer == 7.0).sum())
            assert left > 0, "no kept cell still reads 7.0"
            assert left < self.sevens_at_start, "every cell that read 7.0 after the reset still does: no kept cell was ever stored"
        if self.want_rne:
            assert self.rne_differs, "no element whose round-to-nearest-even and truncated halves differ occurred"
        if self.want_subnormal:
            assert self.subnormal, "1 / 30000 is subnormal in binary16: none seen"


# ---------------------------------------------------------------- the rollout tests of the two half files
def nonzero_count_policy(obs):
    """depends only on which cells are non-zero: the count of non-zero cells of a row mod 5"""
    return ((obs != 0).sum(dim=-1) % 5).to(torch.int32)


def rollout_env(case, obs_dtype=F32, counts=None, **kw):
    """seed 9, the default launch shape; `counts`: the buffer filled with 7.0 and per-env counts dealt"""
    env = make_env(case, obs_dtype, seed=9, max_blocks=0, **kw)
    if counts is not None:
        prefill(env, counts)
    return env
