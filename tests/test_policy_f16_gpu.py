"""GPU tests (-m gpu): the chase policy over half-precision observation rows, PursuitHeuristicPolicy(obs_dtype=torch.float16) /
madrl_heuristic_pursuit_f16 -- pursuit_policy_rows_f16_kernel for flatten rows with 4 ... 64 window cells (obs_range 2 ... 8),
pursuit_policy_f16_kernel for everything else.

The yardstick for actions is the float32 policy on the widened rows (`half.float()`, exact), which tests/test_policy_edges_gpu.py pins to the
reference's recorded actions, and those recorded actions themselves (tests/golden/heuristics_edges.npz, heuristics.npz); drawn actions are
Philox on the host.  Actions are integers and compared exactly.

Every action buffer is filled with -7 and carries a guard element on either side.  The half rows of sections 1 - 3 end where their allocation
ends (no element behind the last row) and, in sections 1 and 3, begin one element into it: every row, odd obs_range included, is then only
2-byte aligned, and the element in front is a NaN, an evader if a kernel looked at it."""
import os

import numpy as np
import pytest
import torch

from oracle import heuristics_oracle as ho
from oracle.pursuit import philox

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32 = torch.float16, torch.float32
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(_GOLDEN, "heuristics.npz"))
E = np.load(os.path.join(_GOLDEN, "heuristics_edges.npz"))
M32 = 0xFFFFFFFF
NEG_ZERO, SUBNORMAL, NAN16, ONE = 0x8000, 0x0001, 0x7E00, 0x3C00


# ---------------------------------------------------------------- helpers
class _Out(object):
    """int32 actions of `shape` inside an allocation of one element more on either side, everything set to -7"""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2,), -7, dtype=torch.int32, device=DEV)
        self.t = self.full[1:1 + n].view(*shape)

    def np(self):
        g = self.full[[0, -1]].cpu().numpy()
        assert (g == -7).all(), "guard element overwritten: %r" % g
        a = self.t.cpu().numpy()
        assert a.min() >= 0 and a.max() <= 4, "a row without an action"
        return a


def _call(pol, obs):
    """one call of a policy object on [n, 1, ...] rows into a guarded buffer -> int32 [n]"""
    out = _Out((obs.shape[0], obs.shape[1]))
    assert pol(obs, out=out.t) is out.t
    return out.np().reshape(-1)


def _half_rows(bits, lead):
    """uint16 bit patterns [n, ...] -> the same as a float16 tensor [n, 1, ...] on the device whose last element is the last element of its
    allocation, with `lead` NaN elements in front of the first row"""
    bits = np.ascontiguousarray(bits, np.uint16)
    full = torch.empty(lead + bits.size, dtype=torch.int16, device=DEV)
    full[:lead] = NAN16
    full[lead:] = torch.as_tensor(bits.reshape(-1).view(np.int16), device=DEV)
    t = full.view(F16)[lead:].view(bits.shape[0], 1, *bits.shape[1:])
    assert t.is_contiguous() and t.data_ptr() == full.data_ptr() + 2 * lead
    assert t.data_ptr() + 2 * t.numel() == full.data_ptr() + full.numel() * 2
    return t


def _bits(win, flatten):
    """float32 windows [n, R, R, 4] -> the uint16 bits of the half rows in either layout (round to nearest even, as the half step kernels
    store them; no non-zero value of the test data rounds to zero, so the recorded actions hold for the half rows)"""
    x = np.ascontiguousarray(ho.pursuit_flatten_rows(win) if flatten else win)
    h = x.astype(np.float16)
    assert np.array_equal(h != 0, x != 0)
    return h.view(np.uint16)


def _draws(seed, row_id_base, rows, tick):
    """the action the policy draws for `rows`: Philox-4x32-10 on the host, counter (row id low, tick, row id high, tag 3), key (seed low, seed
    high), first word scaled to 0 ... 4"""
    out = np.empty(len(rows), np.int32)
    for i, r in enumerate(rows):
        rid = row_id_base + int(r)
        out[i] = (int(philox((rid & M32, tick, rid >> 32, 3), (seed & M32, seed >> 32))[0]) * 5) >> 32
    return out


def _policies(R, flatten, **kw):
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    return PursuitHeuristicPolicy(R, flatten=flatten, obs_dtype=F16, **kw), PursuitHeuristicPolicy(R, flatten=flatten, **kw)


# ---------------------------------------------------------------- 1. recorded windows at every obs_range
def _recorded_windows(R):
    if ("pursuit_R%d_ev" % R) in E.files:
        return ho.pursuit_edge_windows(E["pursuit_R%d_ev" % R], 1000 + R), E["pursuit_R%d_act" % R].astype(np.int32)
    return G["pursuit_R%d_obs" % R], G["pursuit_R%d_act" % R]


RECORDED = sorted({int(f.split("_")[1][1:]) for f in list(E.files) + list(G.files) if f.startswith("pursuit_R") and f.endswith("_act")})


def test_the_recorded_window_sets_cover_both_kernels_and_both_alignments():
    """obs_range 1 ... 9 and 21 (and 11): flatten R = 2 ... 8 is the row-fast kernel, even R the rows that are 2-byte aligned by their length"""
    assert RECORDED == [1, 2, 3, 4, 5, 7, 8, 9, 11, 21], RECORDED


@pytest.mark.parametrize("R", RECORDED)
def test_recorded_windows_both_layouts(R):
    """Flatten rows of R = 2 ... 8 take the row-fast half kernel (even R: rows 2-byte aligned by their length; odd cell counts: the last
    lanes step back onto a 2-byte boundary), everything else the generic half kernel: the actions the unmodified reference gave, ties
    included, and the host's Philox draw where it samples."""
    win, ref = _recorded_windows(R)
    det = ref >= 0
    assert det.sum() > 0 and (~det).sum() > 0
    want = ref.copy()
    want[~det] = _draws(5, 0, np.flatnonzero(~det), 0)
    for flatten in (True, False):
        half, f32 = _policies(R, flatten, seed=5)
        obs = _half_rows(_bits(win, flatten), lead=1)
        got = _call(half, obs)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "R %d, flatten %s: %d of %d rows differ, first row %d (got %d, want %d, drawn: %s)" % (
            R, flatten, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]], not det[bad[0]])
        assert np.array_equal(got, _call(f32, obs.float()))


def test_obs_range_255_equals_the_float32_policy():
    """65 025 cells, the (d^2 << 16 | cell) key at its largest: evaders in the corners, at the edge midpoints and in the centre"""
    R, c, z = 255, 127, 254
    spots = [(0, 0), (0, z), (z, 0), (z, z), (0, c), (c, 0), (c, z), (z, c), (c, c)]
    rng = np.random.RandomState(255)
    sets = [[s] for s in spots] + [[], [], []] + [spots[:4], spots[4:8], spots[:8], spots[1:4], [spots[3], spots[2]], [spots[7], spots[6]]]
    ev = np.zeros((len(sets), R, R), np.uint8)
    for e, s in zip(ev, sets):
        for (i, j) in s:
            e[i, j] = rng.randint(1, 4)
    win = ho.pursuit_edge_windows(ev, 255)
    for flatten in (True, False):
        half, f32 = _policies(R, flatten, seed=9)
        obs = _half_rows(_bits(win, flatten), lead=1)
        got, want = _call(half, obs), _call(f32, obs.float())
        assert np.array_equal(got, want), (flatten, got, want)
        assert len(np.unique(got[:9])) == 5 and np.array_equal(got[9:12], _draws(9, 0, [9, 10, 11], 0))


# ---------------------------------------------------------------- 2. row counts, draws and the draw counter
@pytest.mark.parametrize("R,n_rows", [(7, 7), (7, 16), (7, 1000), (7, 70000), (3, 1000), (8, 1000)])
def test_row_counts_draws_and_the_draw_counter(R, n_rows):
    """fewer rows than lane groups, odd tails, more rows than one sweep of the grid (2 048 workgroups of 32 rows); a 64-bit seed and row ids
    whose high word changes inside the batch; five calls, every one equal to the float32 policy's, the first and the fifth checked against
    Philox on the host"""
    from madrl_amd import _lib
    seed, base = (7 << 32) | 11, 2 ** 32 - 5
    rng = np.random.RandomState(n_rows + R)
    win = np.zeros((n_rows, R, R, 4), np.float32)
    win[..., 2] = (rng.rand(n_rows, R, R) < (0.04 if R > 3 else 0.15)) * rng.randint(1, 4, (n_rows, R, R))   # sparse evader counts, many empty windows
    win[..., 0] = rng.rand(n_rows, R, R) < 0.2
    win[..., 1] = rng.randint(0, 3, (n_rows, R, R))
    drawn = np.flatnonzero(~win[..., 2].any(axis=(1, 2)))
    assert len(drawn) > 0 and len(drawn) < n_rows
    some = drawn if len(drawn) <= 600 else np.concatenate([drawn[:400], drawn[-200:]])
    half, f32 = _policies(R, True, seed=seed, row_id_base=base)
    obs = _half_rows(_bits(win, True), lead=0)
    wide = obs.float()
    ref = ho.pursuit_actions(win[:2000])
    for tick in range(5):
        got, want = _call(half, obs), _call(f32, wide)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (tick, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
        if tick in (0, 4):
            assert np.array_equal(got[some], _draws(seed, base, some, tick)), tick
        assert np.array_equal(got[:len(ref)][ref >= 0], ref[ref >= 0])
    for pol in (half, f32):
        t = pol._tick.cpu().numpy()
        assert len(t) == _lib.POLICY_COUNTER_WORDS and t[0] == 5 and not t[1:].any(), (t[0], np.flatnonzero(t[1:])[:8] + 1)


# ---------------------------------------------------------------- 3. bit patterns
def _pattern_rows(R, flatten, cells):
    """one row per entry of `cells` (a list of {cell: bits}): every evader cell +0 except the given ones; the channels the policy must not
    look at hold clutter, -0.0, subnormals and NaN among it"""
    n = len(cells)
    rng = np.random.RandomState(R)
    clutter = np.array([0, NEG_ZERO, SUBNORMAL, NAN16, ONE, 0x4000], np.uint16)
    win = clutter[rng.randint(len(clutter), size=(n, R, R, 4))]
    win[..., 2] = 0
    for r, d in enumerate(cells):
        for k, b in d.items():
            win[r, k // R, k % R, 2] = b
    if not flatten:
        return win
    return np.concatenate([np.transpose(win[..., :3], (0, 3, 1, 2)).reshape(n, -1), np.full((n, 1), 0x3400, np.uint16)], axis=1)


@pytest.mark.parametrize("R,flatten", [(7, True), (5, False), (21, True)])
def test_bit_patterns_decide_as_the_float32_comparison_does(R, flatten):
    """a cell holds an evader iff its 16 bits are not +-0: -0.0 alone is an empty window (a drawn action), the smallest subnormal alone and a
    NaN alone are evaders at their cell, and a -0.0 next to the centre does not hide a farther evader -- with the lone cell at every
    position of the window"""
    from madrl_amd.heuristics import pursuit_decision_table
    table = pursuit_decision_table(R).astype(np.int32)
    C, near = R * R, (R // 2) * R + R // 2 + 1          # the cell beside the centre
    others = [k for k in range(C) if k != near]
    cases = ([{k: NEG_ZERO} for k in range(C)] + [{k: SUBNORMAL} for k in range(C)] + [{k: NAN16} for k in range(C)] +
             [{near: NEG_ZERO, k: ONE} for k in others])
    want = np.concatenate([_draws(13, 0, np.arange(C), 0), table, table, table[others]])
    half, f32 = _policies(R, flatten, seed=13)
    obs = _half_rows(_pattern_rows(R, flatten, cases), lead=1)
    got = _call(half, obs)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(got, _call(f32, obs.float()))
    assert len(np.unique(want[:C])) == 5 and not np.array_equal(want[:C], table)


# ---------------------------------------------------------------- 4. live env, both layouts
def _env(n, flatten=True, seed=9, env_id_base=0, device=DEV, **kw):
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    return BatchedPursuitEvade([rectangle_map(16, 16)], n_envs=n, device=device, seed=seed, env_id_base=env_id_base, auto_reset=True,
                               n_pursuers=8, n_evaders=30, obs_range=7, flatten=flatten, **kw)


@pytest.mark.parametrize("flatten", [True, False])
def test_live_env_equals_the_float32_twin(flatten):
    N = 64
    h, f = _env(N, flatten, max_steps=7, obs_dtype=F16), _env(N, flatten, max_steps=7)
    half, f32 = _policies(7, flatten, seed=3)
    oh, of = h.reset(), f.reset()
    seen = set()
    for step in range(21):
        assert oh.dtype is F16 and of.dtype is F32
        a, b = half(oh), f32(of)
        assert torch.equal(a, b), (step, int((a != b).sum()))
        seen.update(np.unique(b.cpu().numpy()).tolist())
        if step < 20:
            act = b.clone()
            oh, of = h.step(act)[0], f.step(act)[0]
    assert seen == {0, 1, 2, 3, 4}


# ---------------------------------------------------------------- 5. collectors
NC, T = 64, 8
KEYS = ("actions", "rewards", "dones", "returns")


def _rollout_env(n_envs=NC, env_id_base=0, device=DEV, **kw):
    return _env(n_envs, True, seed=9, env_id_base=env_id_base, device=device, max_steps=5, n_catch=2, surround=True, **kw)


def _half_env(n_envs=NC, env_id_base=0, device=DEV):
    return _rollout_env(n_envs, env_id_base, device, obs_dtype=F16)


def _same16(half, ref):
    """the half tensor holds, bit for bit, the float32 tensor's `.to(float16)` (or the same bits as another half tensor)"""
    assert half.dtype is F16
    want = ref.to(F16) if ref.dtype is F32 else ref
    return torch.equal(half.contiguous().view(torch.int16).reshape(-1), want.contiguous().view(torch.int16).reshape(-1))


def _same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def test_rollout_collector_with_the_half_policy_in_the_loop():
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    from madrl_amd.rollout import RolloutCollector
    pol = lambda dtype: PursuitHeuristicPolicy(7, seed=3, obs_dtype=dtype)
    f = RolloutCollector(_rollout_env(), pol(F32), T, store_observations=True)
    h = RolloutCollector(_half_env(), pol(F16), T, store_observations=True)
    g = RolloutCollector(_half_env(), pol(F16), T, store_observations=True, graph=True)
    for it in range(3):   # (graph: call 1 eager, call 2 captures and replays, call 3 replays)
        a, b, c = f.collect(), h.collect(), g.collect()
        torch.cuda.synchronize()
        for tr in (b, c):
            assert tr.observations.dtype is F16 and tr.last_observation.dtype is F16 and tr.observations.shape == a.observations.shape
            assert _same16(tr.observations, a.observations) and _same16(tr.last_observation, a.last_observation), it
            for key in KEYS:
                assert _same_bits(getattr(a, key), getattr(tr, key)), (it, key)
    assert f._slots and h._slots and g._slots and g._graph is not None and h._obs_slots.element_size() == 2
    assert int((a.dones != 0).sum()) >= NC and len(torch.unique(a.actions)) == 5


def test_sharded_half_collector_equals_the_one_batch_half_collector():
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    from madrl_amd.rollout import RolloutCollector, ShardedRolloutCollector
    from madrl_amd.sharded import StreamSharded
    per = NC // 2
    one = RolloutCollector(_half_env(), PursuitHeuristicPolicy(7, seed=3, obs_dtype=F16), T, store_observations=True)
    col = ShardedRolloutCollector(StreamSharded(_half_env, NC, n_streams=2, device=DEV),
                                  [PursuitHeuristicPolicy(7, seed=3, row_id_base=j * per * 8, obs_dtype=F16) for j in range(2)], T,
                                  store_observations=True)
    for it in range(2):
        a, parts = one.collect(), col.collect()
        torch.cuda.synchronize()
        for key in KEYS:
            assert _same_bits(getattr(a, key), torch.cat([getattr(p, key) for p in parts], dim=1)), (it, key)
        assert all(p.observations.dtype is F16 for p in parts)
        assert _same16(torch.cat([p.observations for p in parts], dim=1), a.observations), it
        assert _same16(torch.cat([p.last_observation for p in parts], dim=0), a.last_observation), it


# ---------------------------------------------------------------- 6. refusals on the device
def test_refusals_on_the_device():
    half, f32 = _policies(7, True, seed=3)
    oh, of = _half_env(4).reset(), _rollout_env(4).reset()
    with pytest.raises(TypeError, match="obs_dtype"):
        half(of)
    with pytest.raises(TypeError, match="float32"):
        f32(oh)
    assert half._tick is None and f32._tick is None   # neither got as far as its device state
    assert torch.equal(half(oh), f32(of))
