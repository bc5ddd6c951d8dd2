"""GPU tests (-m gpu): "zeros over known zeros" in the in-place observation pass of the one-wavefront Pursuit kernel
(madrl_amd/csrc/pursuit_wave.hpp, Shape::ZSKIP): a 64-byte chunk whose sixteen cells are known to hold +0.0f and would get +0.0f again is
not stored.  The rule trusts the stale-zero masks, so every test here is about a chunk skipped over contents the masks do not describe:

  * free-running against the C oracle, bit for bit, both walks;
  * a twin of the same seed whose masks are reset to "nothing known" before every step (it can never skip), both buffers filled with 1.0
    first: a chunk skipped over unknown contents keeps its 1.0 in one buffer only;
  * a caller's in-place edit half way; two alternating buffers through the C ABI; in-place steps mixed with two-buffer steps;
  * evader control (rows of absent observers) and per-env agent counts (rows past the live pursuers).

130 envs on 2 workgroups (one wavefront walks 65 envs: the record / mask prefetch and the loop-carried mask run), max_steps 5 with the
episode clocks staggered, so fused auto-resets -- two passes, the second trusting what the first learned -- happen at every step.
"""
import numpy as np
import pytest
import torch

import helpers
from helpers import same_bits
from live_pursuit import assert_live_equals_fixed

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, BLOCKS, H, T = 130, 2, 5, 40

# name -> (map side, pursuers, evaders, obs_range): one-wavefront shapes with the 16-bit mask form (pursuit_specializations.def)
SHAPES = {
    "c2_8v30_r7": (16, 8, 30, 7),    # the headline: 5 slots per lane, every lane drops one mask position; the last slot ends at lane 40
    "2v2_r3": (10, 2, 2, 3),         # 1 slot in 14 lanes: nothing dropped, a quad with two lanes past the end of the rows
    "c2_8v12_r7": (16, 8, 12, 7),    # evader control (n_evaders >= n_pursuers)
}
TO_SHAPES = ("c2_8v30_r7", "2v2_r3")   # ... that have a line in pursuit_to_specializations.def


def _kw(name, **kw):
    side, P, E, R = SHAPES[name]
    args = dict(n_pursuers=P, n_evaders=E, obs_range=R, n_catch=2, surround=True, flatten=True, reward_mech="local")
    args.update(kw)
    return side, args


def _env(name, seed=3, **kw):
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    side, args = _kw(name, **kw)
    env = BatchedPursuitEvade([rectangle_map(side, side)], n_envs=N, device=DEV, seed=seed, env_id_base=900, max_steps=H, auto_reset=True,
                              kernel="auto", **args)
    env.set_launch(max_blocks=BLOCKS)
    assert env.kernel_kind == "wave"
    return env


def _oracle(name, seed=3, **kw):
    from madrl_amd.maps import rectangle_map
    from oracle import pursuit as po
    side, args = _kw(name, **kw)
    return po.PursuitOracle([rectangle_map(side, side)], n_envs=N, seed=seed, env_id_base=900, **args)


AGES = (np.arange(N) * 3) % H   # episode clocks after the reset: 1/5 of the envs end at every step


def _stagger(env):
    env.set_state(dict(t=AGES))   # (clocks alone: what the fast path knows about the buffer stays)


def _vs_oracle(t, a):
    """a tensor of the env's and the oracle's array of the same elements, both for same_bits / _differ"""
    return t.detach().cpu().reshape(a.shape), a


def _differ(a, b):
    """in how many elements two buffers differ in some bit (the figure of a failure's message)"""
    return int((helpers.bits(a) != helpers.bits(b)).sum())


class OracleRun(object):
    """an env against the oracle, free-running: step(kind) runs one step of either side and compares every output bit for bit"""

    def __init__(self, name, **kw):
        self.env, self.orc = _env(name, **kw), _oracle(name, **kw)
        self.P = SHAPES[name][1]
        obs, oobs = self.env.reset(), self.orc.reset()
        assert same_bits(*_vs_oracle(obs, oobs)), "reset obs"
        _stagger(self.env)
        self.tstep = AGES.astype(np.int64).copy()
        self.rng = np.random.RandomState(5)
        self.n_resets = 0

    def step(self, t, obs_out=None):
        act = self.rng.randint(5, size=(N, self.P))
        a = torch.as_tensor(act, device=DEV, dtype=torch.int32)
        obs, rew, done, info = self.env.step(a) if obs_out is None else self.env.step_to(a, obs_out)
        oobs, orew, odone, orem = self.orc.step(act)
        self.tstep += 1
        bits = odone.astype(np.uint8) | ((self.tstep >= H).astype(np.uint8) << 1)
        assert np.array_equal(info["done_bits"].cpu().numpy(), bits), "step %d done bits" % t
        assert np.array_equal(info["removed"].cpu().numpy(), orem), "step %d removed" % t
        assert np.array_equal(rew.cpu().numpy(), orew.astype(np.float32)), "step %d rewards" % t
        mask = (bits != 0).astype(np.uint8)
        if mask.any():
            self.orc.reset(mask=mask)
            self.tstep[mask != 0] = 0
            self.n_resets += int(mask.sum())
        got, want = _vs_oracle(self.env.obs_buffer, self.orc.obs)
        assert same_bits(got, want), "step %d obs: %d elements differ" % (t, _differ(got, want))
        return obs


@pytest.mark.parametrize("walk", ["forward", "alternate"])
@pytest.mark.parametrize("name", ["c2_8v30_r7", "2v2_r3"])
def test_free_running_equals_the_oracle_bit_for_bit(name, walk):
    run = OracleRun(name)
    run.env.set_walk(walk)
    for t in range(T):
        run.step(t)
    assert run.n_resets >= N * (T // H - 1)   # fused resets: the second pass ran in every env, several times


def _twin_run(make, P, edit_at=None):
    """env a keeps what it knows; env b, same seed, is told before every step that its buffer was edited (an in-place write that changes no
    bit moves the tensor's version counter): its masks go back to "nothing known" and it can never skip.  Both buffers hold 1.0 at the start."""
    a, b = make(), make()
    for e in (a, b):
        e.obs_buffer.fill_(1.0)
    assert same_bits(a.reset(), b.reset())
    for e in (a, b):
        _stagger(e)
    g = torch.Generator(device="cpu").manual_seed(4)
    for t in range(T):
        if edit_at == t:   # the caller edits the returned tensors in place
            a.obs_buffer.fill_(0.5)
            b.obs_buffer.fill_(0.5)
        buf = b.obs_buffer
        version = buf._version
        buf.copy_(buf.clone())
        assert buf._version != version
        act = torch.randint(0, 5, (N, P), generator=g, dtype=torch.int32).to(DEV)
        (oa, ra, da, ia), (ob, rb, db, ib) = a.step(act), b.step(act)
        got, want = a.obs_buffer, b.obs_buffer
        assert same_bits(got, want), "step %d: %d elements differ from the twin that never skips" % (t, _differ(got, want))
        assert torch.equal(ra, rb) and torch.equal(ia["done_bits"], ib["done_bits"]) and torch.equal(ia["removed"], ib["removed"]), t
    return a, b


@pytest.mark.parametrize("name", ["c2_8v30_r7", "2v2_r3"])
def test_twin_that_never_skips_agrees_on_buffers_that_held_ones(name):
    a, b = _twin_run(lambda: _env(name), SHAPES[name][1])
    assert bool((a.obs_buffer == 0.0).any())


@pytest.mark.parametrize("name", ["c2_8v30_r7", "2v2_r3"])
def test_twin_agrees_after_a_caller_edit_half_way(name):
    a, b = _twin_run(lambda: _env(name), SHAPES[name][1], edit_at=20)
    if name == "c2_8v30_r7":
        assert bool((a.obs_buffer == 0.5).any())   # the edit stays in the cells no step stores


@pytest.mark.parametrize("name", ["c2_8v30_r7", "2v2_r3"])
def test_two_alternating_buffers_through_the_c_abi(name):
    """madrl_pursuit_step with two observation buffers in turn, both holding 1.0: the masks describe the buffer of the call before, never
    the one a call is given.  The twin steps into buffers of its own and is told "nothing known" before every call."""
    from madrl_amd import _lib
    L = _lib.lib()
    P = SHAPES[name][1]
    a, b = _env(name), _env(name)
    assert same_bits(a.reset(), b.reset())
    for e in (a, b):
        _stagger(e)
    shape = tuple(a.obs_buffer.shape)
    bufs = {id(e): [torch.full(shape, 1.0, dtype=torch.float32, device=DEV) for _ in range(2)] for e in (a, b)}
    for e in (a, b):   # both buffers start from the reset's observations where it stored, 1.0 elsewhere: the same on both sides
        for x in bufs[id(e)]:
            x.copy_(torch.where(e.obs_buffer != 0, e.obs_buffer, x))
    g = torch.Generator(device="cpu").manual_seed(6)
    stream = _lib.current_stream(a.device)
    for t in range(T):
        act = torch.randint(0, 5, (N, P), generator=g, dtype=torch.int32).to(DEV)
        _lib.check(L.madrl_pursuit_invalidate_obs(b._handle))
        for e in (a, b):
            _lib.check(L.madrl_pursuit_step(e._handle, _lib.ptr(act), None, _lib.ptr(bufs[id(e)][t % 2]), _lib.ptr(e._rew), _lib.ptr(e._done),
                                            _lib.ptr(e._removed), stream))
        for k in range(2):
            got, want = bufs[id(a)][k], bufs[id(b)][k]
            assert same_bits(got, want), "call %d, buffer %d: %d elements differ" % (t, k, _differ(got, want))
        assert torch.equal(a._rew, b._rew) and torch.equal(a._done, b._done), t


@pytest.mark.parametrize("name", TO_SHAPES)
def test_in_place_steps_mixed_with_two_buffer_steps_equal_the_oracle(name):
    """in place, step_to into a trajectory slot (which becomes the current buffer), in place again on that slot, ...: the two-buffer kernel
    never skips and must leave masks that are true for the slot, or the in-place step after it skips a chunk of the 3.0 the slot held."""
    run = OracleRun(name)
    assert run.env.step_to_kernel_kind == "wave"
    shape = tuple(run.env.obs_buffer.shape)
    ring = [torch.empty(shape, dtype=torch.float32, device=DEV) for _ in range(3)]
    k = 0
    for t in range(T):
        if t % 3 == 1:
            slot = ring[k % 3]
            k += 1
            assert slot.data_ptr() != run.env.obs_buffer.data_ptr()
            slot.fill_(3.0)
            run.step(t, obs_out=slot)
            assert run.env.obs_buffer.data_ptr() == slot.data_ptr()
        else:
            run.step(t)   # t % 3 == 2: in place on the slot the step before wrote
    assert k >= T // 3


def test_evader_control_rows_of_absent_observers():
    """train_pursuit=False on the 8 v 12 shape (co-location catches by one pursuer, so that observers disappear): against the oracle, and
    against the twin that never skips on buffers that held 1.0 -- the rows past the last observer keep their contents and their flags."""
    kw = dict(train_pursuit=False, surround=False, n_catch=1)
    run = OracleRun("c2_8v12_r7", **kw)
    absent = 0
    for t in range(T):
        run.step(t)
        absent += int((~run.env.obs_rows_valid()).sum())
    assert absent > 0, "no observer was ever absent: the run does not reach the rows the test is about"
    _twin_run(lambda: _env("c2_8v12_r7", **kw), 8)


def test_per_env_agent_counts_rows_past_the_live_pursuers():
    """capacity (8, 30) at live (5, 17): row 5 starts in the middle of an aligned group of four float4 slots (slot 185), so one chunk holds
    cells of a live row and of an absent one.  Against a fixed-shape (5, 17) batch (tests/live_pursuit.py; rows >= 5 stay zero), then the
    never-skipping twin on buffers that held 1.0."""
    p, e = 5, 17
    cap = _env("c2_8v30_r7", seed=8, per_env_counts=True)
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    fix = BatchedPursuitEvade([rectangle_map(16, 16)], n_envs=N, device=DEV, seed=8, env_id_base=900, max_steps=H, auto_reset=True,
                              **dict(_kw("c2_8v30_r7")[1], n_pursuers=p, n_evaders=e))
    assert_live_equals_fixed(cap, fix, p, e, 8, T, np.random.RandomState(3), state_every=10, last_too=True)
    assert cap.kernel_kind == "wave"

    def make():
        env = _env("c2_8v30_r7", seed=8, per_env_counts=True)
        env.set_agent_counts(p, e)
        return env
    a, b = _twin_run(make, 8)
    assert bool((a.obs_buffer[:, p:] == 1.0).all())   # rows of pursuers that do not exist are never written
