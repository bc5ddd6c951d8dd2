"""Half-precision observation slots: madrl_pursuit_step_to_f16 / BatchedPursuitEvade(obs_dtype=torch.float16).

The yardstick everywhere is a float32 twin with the same seed that steps through a float32 ring of three buffers, while the half env steps
through a half ring of three: after every step the half slot equals the float32 slot's `.to(torch.float16)` in every bit (a stored element
is the round-to-nearest-even half of the float32 value; a kept element is 16 bits carried over, and half(7.0) carried over is what
half(float 7.0 carried over) gives), and rewards, done bits, removed counts and the state records are equal.

All slots of a ring are carved from ONE tensor with guard bands of 4 KiB between them and at both ends, filled with a byte no result holds
and checked after every step: a store past the end of a slot -- a float32-sized address in the half kernel -- fails a test here instead of
faulting.  Slots and the envs' first buffers are pre-filled with 7.0 (exact in binary16), so every kept cell is visible."""
import ctypes as C
import functools
import pickle

import pytest
import torch

from step_to_twins import DEV, F16, F32, Case, HalfTwins, agents, b16, make_env, prefill, rollout_env, same16
from step_to_twins import nonzero_count_policy as _policy

pytestmark = pytest.mark.gpu

X_2V2 = Case("rect16", (10, 10), agents(2, 2, 3, 1), None, {})
X_8V30 = Case("rect16", (16, 16), agents(8, 30, 7, 1), None, {})
X_8V30_SURROUND = Case("rect16", (16, 16), agents(8, 30, 7, 1, surround=True, n_catch=2), None, {})
# Every case: seed 21 unless it names one, max_steps 3, two workgroups (make_env's defaults).  The steps (and seeds) are few enough that
# some never-stored cell is left at the end: on a 3 x 3 window every cell has been inside the map once after a handful of steps and resets.
COUNTS = [(8, 30), (7, 29), (3, 5), (1, 1)]
RING_CASES = {
    "X_smallest": X_2V2._replace(twin=dict(seed=23), n=5, steps=5, kind="wave"),
    "X_window_wider_than_map": Case("rect16", (6, 6), agents(3, 5, 11, 0), None, {}, n=5, steps=12, kind="wave"),
    "XL_live_counts": Case("rect16", (16, 16), agents(8, 30, 7, 1, per_env_counts=True), [COUNTS[i % 4] for i in range(8)], {},
                           n=8, steps=12, kind="wave"),
    "generic_evader_control": Case("rect16", (16, 16), agents(8, 12, 7, 1, train_pursuit=False), None, {}, n=5, steps=8, kind="generic"),
    "generic_2_byte_path": Case("rect16", (12, 12), agents(3, 4, 4, 1), None, {}, n=5, steps=12, kind="generic"),
    "XG_runs_generic": Case("rect16", (32, 32), agents(16, 60, 7, 1), None, {}, n=4, steps=8, kind="generic"),
    "XC_runs_generic": Case("rect16", (24, 24), agents(20, 300, 9, 1, surround=True, n_catch=2), None, {}, n=4, steps=8, kind="generic"),
    "X_subnormal_values": Case("rect16", (10, 10), agents(2, 2, 3, 1, layer_norm=30000.0), None, dict(seed=23), n=5, steps=5, kind="wave"),
}


@pytest.mark.parametrize("name", sorted(RING_CASES))
def test_half_ring_equals_the_float32_ring(name):
    case = RING_CASES[name]
    tw = HalfTwins(case)
    assert tw.h.step_to_kernel_kind == case.kind
    if name in ("XG_runs_generic", "XC_runs_generic"):
        assert tw.f.step_to_kernel_kind == "wave"   # (the float32 form of the same handle has its fast kernel)
    tw.run(case.steps)   # (half way: other pending counts, taken at each env's next fused reset)
    if name == "X_subnormal_values":
        sub = b16(tw.h.obs_buffer).to(torch.int32) & 0xFFFF
        assert bool(((sub > 0) & (sub < 0x0400)).any()), "1 / 30000 is subnormal in binary16: none seen"
    tw.finish()   # (max_steps=3: every env ended an episode; the changed counts were taken)


def test_consecutive_envs_of_a_wavefront_and_round_to_nearest_even():
    """X(16,16,8,30,7,1): 130 envs on 3 workgroups, auto_reset with max_steps=12, 40 steps -- a wavefront's consecutive envs, the second
    pass of a fused auto-reset on the half buffer, and elements whose round-to-nearest-even and truncated halves differ (three agents on a
    cell at layer_norm 10: 0.3f is 0x34CD in binary16, the packed round-toward-zero conversion gives 0x34CC)"""
    assert b16(torch.tensor([0.3], dtype=F32).to(F16)).item() == 0x34CD
    tw = HalfTwins(X_8V30_SURROUND, n=130, max_steps=12, max_blocks=3)
    assert tw.h.step_to_kernel_kind == "wave"
    saw_03 = False
    for k in range(40):
        hs = tw.hop(k)
        saw_03 = saw_03 or bool((b16(hs) == 0x34CD).any())
    assert int(tw.dones.sum()) >= 2 * 130
    assert tw.rne_differs, "no element whose round-to-nearest-even and truncated halves differ occurred"
    assert saw_03, "0.3 (three agents on a cell) never occurred"
    tw.finish()


def test_step_ping_pong_in_place_edit_and_pickle():
    """step() of a half env ping-pongs between two internal buffers and gives what the ring gives; an in-place edit of the returned tensor
    (to a value exact in binary16) is noticed and persists in the kept cells as on a float32 twin that steps in place; a pickle keeps
    the dtype"""
    case = RING_CASES["X_window_wider_than_map"]   # every row has kept cells
    tw = HalfTwins(case)
    pp, ip = make_env(case, F16, n=5), make_env(case, n=5)   # half step() / float32 step() in place
    for e in (pp, ip):
        prefill(e)
        e.reset()
    seen = set()
    for k in range(6):
        act = tw.actions()[0]
        hs = tw.hop(k, act)
        o = pp.step(act)[0]
        assert o.dtype is F16 and o.shape == (5, 3, 11, 11, 4) and o.data_ptr() == pp.obs_buffer.data_ptr()
        assert torch.equal(b16(o).reshape(-1), b16(hs).reshape(-1)), k
        assert same16(o, ip.step(act)[0]), k
        seen.add(o.data_ptr())
    assert len(seen) == 2
    for k in range(4):   # the edit: every element 5.0, through the returned tensors
        act = tw.actions()[0]
        if k == 0:
            pp.obs_buffer.view(-1)[:] = 5.0
            ip.obs_buffer.view(-1)[:] = 5.0
        o, r = pp.step(act)[0], ip.step(act)[0]
        assert same16(o, r), ("after the edit", k)
        assert bool((o == 5.0).any()) and not bool((o == 5.0).all())
    clone = pickle.loads(pickle.dumps(pp))
    assert clone.obs_dtype is F16 and clone.reset().dtype is F16 and clone.step_to_kernel_kind == "wave"
    assert "obs_dtype" not in ip.__getstate__() and pickle.loads(pickle.dumps(ip)).obs_dtype is F32


def test_mismatched_destination_dtypes_raise():
    h, f = make_env(X_2V2, F16, n=5), make_env(X_2V2, n=5)
    h.reset(), f.reset()
    act = torch.zeros((5, 2), dtype=torch.int32, device=DEV)
    shape = tuple(f.obs_buffer.shape)
    rew, dn = torch.zeros((5, 2), dtype=F32, device=DEV), torch.zeros(5, dtype=torch.uint8, device=DEV)
    for env, bad in ((h, F32), (f, F16), (h, torch.float64), (f, torch.float64)):
        dest = torch.zeros(shape, dtype=bad, device=DEV)
        with pytest.raises(ValueError):
            env.step_to(act, dest)
        with pytest.raises(ValueError):
            env.step_into(act, rew, dn, obs_out=dest)
    with pytest.raises(ValueError):   # there is no in-place half step
        h.step_to(act, h.obs_buffer)
    o = h.step_into(act, rew, dn, obs_out=torch.zeros(shape, dtype=F16, device=DEV))
    assert o.dtype is F16 and same16(o, f.step_into(act, rew, dn, obs_out=torch.zeros(shape, dtype=F32, device=DEV)))


def test_c_abi_argument_checks_and_format_switch():
    from madrl_amd import _lib
    L = _lib.lib()
    N, P = 6, 8
    e1 = make_env(X_8V30, n=N, max_steps=0)
    D = e1.obs_dim
    n = N * P * D
    e1.reset()
    act = torch.randint(0, 5, (N, P), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)
    rew, dn, rem = torch.zeros((N, P), dtype=F32, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    hA = e1.obs_buffer.to(F16)
    region = torch.zeros(4 * n + 64, dtype=torch.uint8, device=DEV)   # holds a half buffer -- and, at the same address, a float32 one
    region[2 * n:4 * n].view(F32).fill_(7.0)   # (7.0 as float32: the second half of the float32 view)
    hB = region[:2 * n].view(F16)
    stream = _lib.current_stream(e1.device)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(prev, nxt, h=e1):
        return L.madrl_pursuit_step_to_f16(h._handle, p(act), None, prev, nxt, p(rew), p(dn), p(rem), stream)

    EINVAL = -1
    assert call(None, p(hB)) == EINVAL and call(p(hA), None) == EINVAL                 # NULL
    assert call(p(hA), p(region, 8)) == EINVAL and call(p(region, 2 * n + 8), p(hB)) == EINVAL   # not 16-byte aligned
    assert call(p(region), p(region, 16)) == EINVAL and call(p(region, 2 * n - 16), p(region)) == EINVAL   # overlapping
    assert call(p(hB), p(hB)) == EINVAL                                                # equal: no in-place half step
    torch.cuda.synchronize()
    assert bool((region[:2 * n] == 0).all()), "a refused call wrote"
    kind = C.c_int32()
    assert L.madrl_pursuit_step_to_f16_kernel_kind(e1._handle, C.byref(kind)) == 0 and kind.value == _lib.KERNEL_WAVE
    # two half steps: the handle's knowledge now describes hB as a binary16 buffer (its kept cells: zero)
    hC = torch.zeros(n, dtype=F16, device=DEV)
    _lib.check(call(p(hA), p(hC)))
    _lib.check(call(p(hC), p(hB)))
    st = e1.get_state()
    # the same address as a float32 buffer: element i is halves 2 i and 2 i + 1 of hB, then the 7.0s -- an unknown buffer
    as_f32 = region[:4 * n].view(F32)
    got, want = torch.zeros(n, dtype=F32, device=DEV), torch.zeros(n, dtype=F32, device=DEV)
    g_rew, w_rew = torch.zeros_like(rew), torch.zeros_like(rew)
    _lib.check(L.madrl_pursuit_step_to(e1._handle, p(act), None, p(as_f32), p(got), p(g_rew), p(dn), p(rem), stream))
    e2 = make_env(X_8V30, n=N, max_steps=0)
    e2.reset()
    e2.set_state(st)
    _lib.check(L.madrl_pursuit_step_to(e2._handle, p(act), None, p(as_f32.clone()), p(want), p(w_rew), p(dn), p(rem), stream))
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the format switch kept the half buffer's knowledge"
    assert torch.equal(g_rew.view(torch.int32), w_rew.view(torch.int32))
    assert bool((got == 7.0).any())   # kept cells of the float32 view did hold non-zero values


T, NR = 6, 32


_rollout_env = functools.partial(rollout_env, X_8V30_SURROUND, n=NR, max_steps=5)


def test_rollout_collector_keeps_half_slots():
    from madrl_amd.rollout import RolloutCollector
    f = RolloutCollector(_rollout_env(), _policy, T, store_observations=True)
    h = RolloutCollector(_rollout_env(obs_dtype=F16), _policy, T, store_observations=True)
    g = RolloutCollector(_rollout_env(obs_dtype=F16), _policy, T, store_observations=True, graph=True)
    assert f._slots and h._slots and g._slots
    for it in range(3):   # (graph: call 1 eager, call 2 captures and replays, call 3 replays)
        a, b, c = f.collect(), h.collect(), g.collect()
        torch.cuda.synchronize()
        for tr in (b, c):
            assert tr.observations.dtype is F16 and tr.last_observation.dtype is F16
            assert tr.observations.shape == a.observations.shape
            assert same16(tr.observations, a.observations), it
            assert same16(tr.last_observation, a.last_observation), it
            for key in ("actions", "rewards", "dones", "returns"):
                x, y = getattr(a, key), getattr(tr, key)
                assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (it, key)
    assert g._graph is not None
    assert int((a.dones != 0).sum()) >= NR
    assert h._obs_slots.element_size() == 2


def test_wrappers_and_the_device_policy_refuse_a_half_env():
    """what reads float32 rows through the raw pointer raises over a half env instead of reading past its buffers"""
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    from madrl_amd.rollout import RolloutCollector
    from madrl_amd.wrappers import ObservationBuffer, StandardizedEnv
    with pytest.raises(TypeError, match="float32"):
        RolloutCollector(_rollout_env(obs_dtype=F16), PursuitHeuristicPolicy(7, seed=3), T, store_observations=True).collect()
    with pytest.raises(TypeError, match="float32"):
        ObservationBuffer(_rollout_env(obs_dtype=F16), 2).reset()
    with pytest.raises(TypeError, match="float32"):
        StandardizedEnv(_rollout_env(obs_dtype=F16), enable_obsnorm=True).reset()
    env = StandardizedEnv(_rollout_env(obs_dtype=F16), enable_rewnorm=True)   # rewards are float32: nothing to refuse
    assert env.reset().dtype is F16


def test_stream_sharded_half_envs_step_one_by_one():
    """madrl_pursuit_step_sharded writes float32 rows in place: a StreamSharded over half envs must stay off that one-call path, and gives
    what the float32 sharded batch gives; so does the sharded collector"""
    from madrl_amd.rollout import RolloutCollector, ShardedRolloutCollector
    from madrl_amd.sharded import StreamSharded

    def make(dtype):
        return lambda n_envs, env_id_base, device: rollout_env(X_8V30_SURROUND, dtype, n=n_envs, max_steps=5, env_id_base=env_id_base)

    f, h = StreamSharded(make(F32), NR, n_streams=2, device=DEV), StreamSharded(make(F16), NR, n_streams=2, device=DEV)
    assert f._native_pursuit() and not h._native_pursuit()
    cat = lambda parts: torch.cat(list(parts), dim=0)
    a, b = cat(f.reset()), cat(h.reset())
    assert b.dtype is F16 and same16(b, a)
    gen = torch.Generator(device="cpu").manual_seed(5)
    for k in range(7):
        act = torch.randint(0, 5, (NR, 8), generator=gen).to(torch.int32).to(DEV)
        ra, rb = f.step(act), h.step(act)
        torch.cuda.synchronize()
        assert h._nat is None, "the half batch took the one-call float32 path"
        oa, ob = cat([r[0] for r in ra]), cat([r[0] for r in rb])   # (one (obs, rew, done, info) per sub-batch)
        assert ob.dtype is F16 and same16(ob, oa), k
        assert torch.equal(cat([r[1] for r in ra]).view(torch.int32), cat([r[1] for r in rb]).view(torch.int32)), k
    fc = ShardedRolloutCollector(StreamSharded(make(F32), NR, n_streams=2, device=DEV), [_policy, _policy], T, store_observations=True)
    hc = ShardedRolloutCollector(StreamSharded(make(F16), NR, n_streams=2, device=DEV), [_policy, _policy], T, store_observations=True)
    for it in range(2):
        pa, pb = fc.collect(), hc.collect()
        torch.cuda.synchronize()
        for x, y in zip(pa, pb):
            assert y.observations.dtype is F16 and same16(y.observations, x.observations), it
            assert torch.equal(x.actions, y.actions) and torch.equal(x.rewards.view(torch.int32), y.rewards.view(torch.int32)), it
