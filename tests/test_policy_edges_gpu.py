"""GPU tests (-m gpu): the three device policies of heuristics.hip at every window size, sensor count and draw.

What a replacement of the chase policy's window scan has to reproduce, tie for tie and draw for draw: the recorded actions of the
unmodified reference at obs_range 1 ... 21 (tests/golden/heuristics_edges.npz: every pair of evader cells up to 9), the oracle at 255,
every drawn action as Philox on the host, the draw counter after launches whose 64 workgroup groups have unequal sizes.  The Waterworld
policy runs at sensor counts around its eight lanes per row, the MultiWalker policy at its thresholds' float32 neighbours.

Every output buffer is filled with NaN (integers: -7) before a launch and carries a guard element on either side that must keep its
fill (the output tensors the policy classes allocate themselves, section 5, cannot).

Tolerances.  Pursuit actions are integers and compared exactly.  The Waterworld unit vector keeps the project's bound for this policy,
1e-5 absolute (the kernel sums in float64 in another order than NumPy and rounds to float32: 6e-8); rows whose action before it is
normalised is shorter than 1e-4 in the oracle have no defined direction and are left out, at most 1 % of a case.  MultiWalker: 1e-6."""
import os

import numpy as np
import pytest
import torch

from oracle import heuristics_oracle as ho
from oracle.pursuit import philox

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(_GOLDEN, "heuristics.npz"))
E = np.load(os.path.join(_GOLDEN, "heuristics_edges.npz"))
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- helpers
class _Out(object):
    """an output of `shape` inside an allocation of one element more on either side, everything set to `fill`"""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2,), fill, dtype=dtype, device=DEV)
        self.fill, self.t = fill, self.full[1:1 + n].view(*shape)

    def np(self):
        """the output on the host, after checking that both guards kept their fill"""
        g = self.full[[0, -1]].cpu().numpy()
        assert (np.isnan(g) if self.fill != self.fill else g == self.fill).all(), "guard element overwritten: %r" % g
        return self.t.cpu().numpy()


def _L():
    from madrl_amd import _lib
    return _lib, _lib.lib(), _lib.ptr, _lib.current_stream(torch.device(DEV))


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _pursuit_obs(win, flatten):
    """windows [n, R, R, 4] on the device as the [n, 1, ...] observations of BatchedPursuitEvade in either layout"""
    n = len(win)
    return _d(ho.pursuit_flatten_rows(win)).view(n, 1, -1) if flatten else _d(win).view(n, 1, *win.shape[1:])


def _pursuit_call(pol, obs):
    """one call of a policy object into a guarded, -7-filled buffer -> int32 [n]; every row must have been given an action"""
    out = _Out((obs.shape[0], 1), torch.int32, -7)
    assert pol(obs, out=out.t) is out.t
    a = out.np()[:, 0]
    assert a.min() >= 0 and a.max() <= 4, "a row without an action"
    return a


def _draws(seed, row_id_base, rows, tick):
    """the action the policy draws for `rows` (indices into a launch): Philox-4x32-10 on the host, counter (row id low, tick, row id high,
    tag 3), key (seed low, seed high), first word scaled to 0 ... 4"""
    out = np.empty(len(rows), np.int32)
    for i, r in enumerate(rows):
        rid = row_id_base + int(r)
        out[i] = (int(philox((rid & M32, tick, rid >> 32, 3), (seed & M32, seed >> 32))[0]) * 5) >> 32
    return out


def _table_windows(R, n, rng, p_empty):
    """n windows with one evader each (or none, with probability p_empty) -> (windows, the evader's cell or -1): the action of a
    non-empty one is the decision table's entry for that cell, so every row of a large launch has its expected action without a
    per-row oracle call"""
    cell = np.where(rng.rand(n) < p_empty, -1, rng.randint(R * R, size=n))
    ev = np.zeros((n, R * R), np.uint8)
    ev[np.flatnonzero(cell >= 0), cell[cell >= 0]] = rng.randint(1, 4, (cell >= 0).sum())
    return ho.pursuit_edge_windows(ev.reshape(n, R, R), n), cell


# ---------------------------------------------------------------- 2. the chase policy
def _recorded_windows(R):
    if ("pursuit_R%d_ev" % R) in E.files:
        return ho.pursuit_edge_windows(E["pursuit_R%d_ev" % R], 1000 + R), E["pursuit_R%d_act" % R].astype(np.int32)
    return G["pursuit_R%d_obs" % R], G["pursuit_R%d_act" % R]


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 7, 8, 9, 11, 21])
def test_pursuit_recorded_windows_both_layouts(R):
    """Both kernels (flatten rows: pursuit_policy_rows_kernel for R = 2 ... 8; everything else: pursuit_policy_kernel) against the actions
    the unmodified reference gave: every single evader, every pair of evader cells up to R = 9, sparse windows; where the reference samples,
    the host's Philox draw."""
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    win, ref = _recorded_windows(R)
    det = ref >= 0
    assert det.sum() > R * R and (~det).sum() > 10
    want = ref.copy()
    want[~det] = _draws(5, 0, np.flatnonzero(~det), 0)
    a = _pursuit_call(PursuitHeuristicPolicy(R, flatten=True, seed=5), _pursuit_obs(win, True))
    b = _pursuit_call(PursuitHeuristicPolicy(R, flatten=False, seed=5), _pursuit_obs(win, False))
    for name, got in (("flatten", a), ("windows", b)):
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "R %d, %s layout: %d of %d rows differ, first row %d (got %d, want %d, drawn: %s)" % (
            R, name, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]], not det[bad[0]])
    assert np.array_equal(a, b)


def test_pursuit_obs_range_255():
    """The largest window the C ABI accepts: 65 025 cells, d^2 up to 32 258 -- the (d^2 << 16 | cell) key at its largest.  Evaders only
    in the corners, at the edge midpoints and in the centre; the far corner alone is the largest key there is."""
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    R, c, z = 255, 127, 254
    spots = [(0, 0), (0, z), (z, 0), (z, z), (0, c), (c, 0), (c, z), (z, c), (c, c)]
    rng = np.random.RandomState(255)
    sets = [[s] for s in spots] + [[], [], []] + [spots[:4], spots[4:8], spots[:8], spots[1:4], [spots[3], spots[2]], [spots[7], spots[6]]]
    while len(sets) < 33:
        sets.append([spots[i] for i in np.flatnonzero(rng.rand(9) < 0.4)])
    ev = np.zeros((33, R, R), np.uint8)
    for e, s in zip(ev, sets):
        for (i, j) in s:
            e[i, j] = rng.randint(1, 4)
    win = ho.pursuit_edge_windows(ev, 255)
    ref = ho.pursuit_actions(win)
    det = ref >= 0
    assert 3 <= (~det).sum() <= 8 and ref[3] >= 0 and len(np.unique(ref[det])) == 5
    want = ref.copy()
    want[~det] = _draws(9, 0, np.flatnonzero(~det), 0)
    for flatten in (True, False):
        a = _pursuit_call(PursuitHeuristicPolicy(R, flatten=flatten, seed=9), _pursuit_obs(win, flatten))
        assert np.array_equal(a, want), (flatten, a, want)


def _draw_windows(n, seed):
    """R = 7 windows, about half of them empty, the rest sparse"""
    rng = np.random.RandomState(seed)
    ev = ((rng.rand(n, 7, 7) < 0.05) * rng.randint(1, 4, (n, 7, 7))).astype(np.uint8)
    ev[rng.rand(n) < 0.45] = 0
    win = ho.pursuit_edge_windows(ev, seed)
    ref = ho.pursuit_actions(win)
    assert 0.3 < (ref < 0).mean() < 0.7
    return win, ref


DRAW_CASES = [(11, 0), ((7 << 32) | 5, 0), (11, 2 ** 32 - 100)]


@pytest.mark.parametrize("flatten", [True, False])
@pytest.mark.parametrize("seed,row_id_base", DRAW_CASES)
def test_pursuit_draws_are_philox_on_the_host(seed, row_id_base, flatten):
    """Every counter and key word of the draw: the row id's low and high word (the high word changes inside the batch in the third case),
    the tick of five consecutive calls, the tag, both halves of the seed."""
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    n = 300
    win, ref = _draw_windows(n, 300)
    drawn = np.flatnonzero(ref < 0)
    obs = _pursuit_obs(win, flatten)
    pol = PursuitHeuristicPolicy(7, flatten=flatten, seed=seed, row_id_base=row_id_base)
    seen = []
    for tick in range(5):
        want = ref.copy()
        want[drawn] = _draws(seed, row_id_base, drawn, tick)
        a = _pursuit_call(pol, obs)
        assert np.array_equal(a, want), (tick, np.flatnonzero(a != want)[:5])
        seen.append(want[drawn])
    assert len(set(map(bytes, seen))) == 5 and len(np.unique(np.concatenate(seen))) == 5
    if row_id_base:
        assert (row_id_base + drawn[0]) >> 32 == 0 and (row_id_base + drawn[-1]) >> 32 == 1


@pytest.mark.parametrize("flatten", [True, False])
def test_pursuit_c_abi_host_tick_and_a_table_that_says_draw(flatten):
    """What a C caller uses: no device counter and the tick as an argument -- the actions of the fifth call of a policy object; and a
    decision table with 255 ("draw") entries, which pursuit_decision_table never produces."""
    from madrl_amd.heuristics import PursuitHeuristicPolicy, pursuit_decision_table
    _lib, L, P, st = _L()
    R, n, seed = 7, 300, (7 << 32) | 5
    win, ref = _draw_windows(n, 300)
    obs = _pursuit_obs(win, flatten)
    stride, cell_stride, ch_off = (3 * R * R + 1, 1, 2 * R * R) if flatten else (4 * R * R, 4, 2)
    table = pursuit_decision_table(R)

    def launch(obs_d, n_rows, table_host, tick):
        out, table_d = _Out((n_rows,), torch.int32, -7), _d(table_host)
        _lib.check(L.madrl_heuristic_pursuit(P(obs_d), n_rows, R, stride, cell_stride, ch_off, P(table_d), seed, 0, tick, None, P(out.t), st))
        return out.np()

    want = ref.copy()
    want[ref < 0] = _draws(seed, 0, np.flatnonzero(ref < 0), 4)
    a = launch(obs, n, table, 4)
    assert np.array_equal(a, want)
    pol = PursuitHeuristicPolicy(R, flatten=flatten, seed=seed)
    for _ in range(5):
        fifth = _pursuit_call(pol, obs)
    assert np.array_equal(a, fifth)
    # one evader per window, every cell once; the table says "draw" for window row 2
    t255 = table.copy()
    t255[2 * R:3 * R] = 255
    one = ho.pursuit_edge_windows(np.eye(R * R, dtype=np.uint8).reshape(R * R, R, R), 49)
    a = launch(_pursuit_obs(one, flatten), R * R, t255, 0)
    want = table.astype(np.int32)
    want[2 * R:3 * R] = _draws(seed, 0, np.arange(2 * R, 3 * R), 0)
    assert np.array_equal(a, want)
    assert not np.array_equal(want[2 * R:3 * R], table[2 * R:3 * R])


@pytest.mark.parametrize("flatten", [True, False])
def test_pursuit_shards_draw_as_one_batch(flatten):
    """two policy objects with row_id_base 0 and n / 2 on the halves of a batch = one object on the whole batch, for two ticks"""
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    n = 600
    win, ref = _draw_windows(n, 600)
    whole = PursuitHeuristicPolicy(7, flatten=flatten, seed=21)
    lo, hi = (PursuitHeuristicPolicy(7, flatten=flatten, seed=21, row_id_base=b) for b in (0, n // 2))
    for tick in range(2):
        a = _pursuit_call(whole, _pursuit_obs(win, flatten))
        b = np.concatenate([_pursuit_call(lo, _pursuit_obs(win[:n // 2], flatten)), _pursuit_call(hi, _pursuit_obs(win[n // 2:], flatten))])
        assert np.array_equal(a, b), tick
        want = ref.copy()
        want[ref < 0] = _draws(21, 0, np.flatnonzero(ref < 0), tick)
        assert np.array_equal(a, want), tick


@pytest.mark.parametrize("flatten", [True, False])
@pytest.mark.parametrize("blocks", [63, 64, 65, 101, 127, 129, 2047])
def test_pursuit_draw_counter_with_unequal_workgroup_groups(blocks, flatten):
    """policy_retire counts the workgroups of a launch in min(64, grid) groups; with a grid above 64 that is no multiple of 64 the groups
    have unequal sizes.  A group that never completes would leave the draw counter where it is: after five calls the counter is 5, every
    other counter word is zero, and the fifth call drew at tick 4."""
    from madrl_amd import _lib
    from madrl_amd.heuristics import PursuitHeuristicPolicy, pursuit_decision_table
    R = 7
    n = (32 if flatten else 16) * blocks - 3        # rows per workgroup of the rows kernel (two per lane group) / the generic kernel
    win, cell = _table_windows(R, n, np.random.RandomState(blocks), 0.04)
    obs = _pursuit_obs(win, flatten)
    pol = PursuitHeuristicPolicy(R, flatten=flatten, seed=13)
    for _ in range(5):
        a = _pursuit_call(pol, obs)
    t = pol._tick.cpu().numpy()
    assert len(t) == _lib.POLICY_COUNTER_WORDS
    assert t[0] == 5 and not t[1:].any(), (t[0], np.flatnonzero(t[1:])[:8] + 1)
    want = pursuit_decision_table(R).astype(np.int32)[np.maximum(cell, 0)]
    want[cell < 0] = _draws(13, 0, np.flatnonzero(cell < 0), 4)
    assert (cell < 0).sum() > 20 and np.array_equal(a, want), np.flatnonzero(a != want)[:5]


# ---------------------------------------------------------------- 3. the Waterworld policy
def _waterworld_device(obs):
    """obs float32 [n, D] -> float32 [n, 2] through the C ABI into a guarded, NaN-filled buffer"""
    _lib, L, P, st = _L()
    n, D = obs.shape
    K = D // 7
    ang = np.linspace(0., 2. * np.pi, K + 1)[:-1]
    obs_d, cs = _d(obs), _d(np.c_[np.cos(ang), np.sin(ang)])
    out = _Out((n, 2), torch.float32, NAN)
    _lib.check(L.madrl_heuristic_waterworld(P(obs_d), n, D, P(cs), P(out.t), st))
    return out.np()


def _waterworld_check(obs, ref, label):
    """device actions of obs against ref within 1e-5, leaving out the rows without a direction (module docstring); all-zero rows: +0.0"""
    got = _waterworld_device(obs)
    assert got.dtype == np.float32 and not np.isnan(got).any(), "a row without an action"
    zero = ~obs.any(axis=1)
    norm = np.sqrt((ho.waterworld_raw(obs) ** 2).sum(axis=1))
    out = (norm < 1e-4) & ~zero
    diff = np.abs(got.astype(np.float64) - ref)[~out]
    print("waterworld %s: %d rows, largest difference %.3g, %d rows (%.2f %%) left out, smallest norm %.3g" % (
        label, len(obs), diff.max(), out.sum(), 100.0 * out.mean(), norm[~zero].min() if (~zero).any() else NAN))
    assert out.sum() <= 0.01 * len(obs)
    assert diff.max() < 1e-5
    assert np.array_equal(got[zero].view(np.int32), np.zeros((zero.sum(), 2), np.int32)), "an all-zero row gives exactly +0.0, +0.0"
    return got


@pytest.mark.parametrize("K", [1, 3, 7, 8, 9, 33])
def test_waterworld_recorded_sensor_counts(K):
    """eight lanes per row: fewer sensors than lanes, exactly as many, one more, and a count that is no multiple of eight -- the rows
    the unmodified reference was given, all 120 and the first one alone"""
    obs, ref = E["waterworld_K%d_obs" % K], E["waterworld_K%d_act" % K]
    assert not obs[-10:].any()
    got = _waterworld_check(obs, ref, "recorded K %d" % K)
    one = _waterworld_check(obs[:1], ref[:1], "recorded K %d, one row" % K)
    assert np.array_equal(one.view(np.int32), got[:1].view(np.int32))


@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 4099])
@pytest.mark.parametrize("K", [30, 256])
def test_waterworld_drawn_rows(K, n_rows):
    """the authors' 30 sensors and the crowd kernel's limit of 256, with thread counts on, before and after a multiple of 256"""
    rng = np.random.RandomState(1000 * K + n_rows)
    obs = rng.rand(n_rows, 7 * K + 3).astype(np.float32)
    obs[:, 7 * K] = np.arange(n_rows) % 2
    obs[:, 7 * K + 1] = (np.arange(n_rows) // 2) % 2
    obs[7::10] = 0.0
    _waterworld_check(obs, ho.waterworld_actions(obs), "drawn K %d" % K)


# ---------------------------------------------------------------- 4. the MultiWalker policy
@pytest.mark.parametrize("n_rows", [1, 255, 256, 257])
@pytest.mark.parametrize("D", [32, 71])
def test_multiwalker_recorded_thresholds(D, n_rows):
    """SPEED and the 0.10 of the supporting leg at their float32 neighbours, 0.0 / -0.0 / NaN contact flags, a knee target of 0.0 (unset
    for the reference's `if target:`), NaN where it reaches an action; 32-wide rows and the 71-wide one-hot rows.  The rows taken are the
    40 drawn ones and then the first n_rows - 40 of the products, so that 255 and more rows hold one full product."""
    _lib, L, P, st = _L()
    key = "multiwalker" if D == 32 else "multiwalker71"
    idx = np.roll(np.arange(400), 40)[:n_rows]
    obs, ref = E[key + "_obs"][idx], E[key + "_act"][idx]
    out, obs_d = _Out((n_rows, 4), torch.float32, NAN), _d(obs)
    _lib.check(L.madrl_heuristic_multiwalker(P(obs_d), n_rows, D, P(out.t), st))
    got = out.np()
    assert np.isnan(ref).any()
    assert np.array_equal(np.isnan(ref), np.isnan(got)), np.argwhere(np.isnan(ref) != np.isnan(got))[:5]
    assert np.nanmax(np.abs(got - ref), initial=0.0) < 1e-6


# ---------------------------------------------------------------- 5. the output tensors the policy classes keep
def test_cached_output_tensors_follow_the_observation_shape():
    """one object called with [4, 6, ...] and then [6, 4, ...] observations: the second result has the second shape and a fresh object's
    values; out= of the Pursuit policy neither uses nor disturbs the cached tensor"""
    from madrl_amd.heuristics import PursuitHeuristicPolicy, WaterworldHeuristicPolicy, MultiWalkerHeuristicPolicy
    rng = np.random.RandomState(46)
    win, cell = _table_windows(7, 24, rng, 0.0)                   # no empty window: nothing is drawn, so the tick does not matter
    cases = [(lambda: PursuitHeuristicPolicy(7, flatten=False, seed=1), _d(win), ()),
             (lambda: PursuitHeuristicPolicy(7, flatten=True, seed=1), _d(ho.pursuit_flatten_rows(win)), ()),
             (WaterworldHeuristicPolicy, _d(rng.rand(24, 7 * 9 + 3).astype(np.float32)), (2,)),
             (MultiWalkerHeuristicPolicy, _d(rng.uniform(-1, 1, (24, 32)).astype(np.float32)), (4,))]
    for make, rows, tail in cases:
        pol = make()
        first = pol(rows.view(4, 6, *rows.shape[1:]))
        assert tuple(first.shape) == (4, 6) + tail
        first = first.clone()
        second = pol(rows.view(6, 4, *rows.shape[1:]))
        assert tuple(second.shape) == (6, 4) + tail, (make, tuple(second.shape))
        fresh = make()(rows.view(6, 4, *rows.shape[1:]))
        assert tuple(fresh.shape) == (6, 4) + tail
        assert torch.equal(second.view(torch.int32), fresh.view(torch.int32)) and torch.equal(second.reshape(-1), first.reshape(-1))
        if not tail:
            out = _Out((3, 8), torch.int32, -7)
            assert pol(rows.view(3, 8, *rows.shape[1:]), out=out.t) is out.t
            assert np.array_equal(out.np().reshape(-1), first.cpu().numpy().reshape(-1))
            again = pol(rows.view(6, 4, *rows.shape[1:]))
            assert again is second and tuple(again.shape) == (6, 4) and torch.equal(again, fresh)
