"""CPU checks of tests/pursuit_walk.py, the conditions that keep tests/test_pursuit_walk_gpu.py from being empty: the walks are
deterministic, hold every ordered pair of op kinds, and -- replayed on the model alone -- reach fused resets, catches, kept and overwritten
sentinels, masked resets of running episodes and all three kernel entries; the model's half rule is PyTorch's conversion; and the model's
load / step / store round trip reproduces a committed golden, so it is not a second untested thing."""
import functools
import os

import numpy as np
import pytest

import pursuit_walk as pw

CASES = [(name, seed) for name in pw.HANDLES for seed in pw.HANDLES[name]["seeds"]]
PY_CASES = [(half, seed) for half in (False, True) for seed in pw.PY_SEEDS]


def _walk(name, seed, python_half=None):
    return pw.walk(pw.kinds_of(name) if python_half is None else pw.PY_KINDS, seed, name, python_half)


@functools.lru_cache(maxsize=None)
def _run(name, seed, python_half=None):
    ops = _walk(name, seed, python_half)
    return ops, pw.run_model(pw.model_for(name, seed, python_half), ops)


@pytest.fixture(scope="module", autouse=True)
def _drop_the_models_at_the_end():
    yield
    _run.cache_clear()


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def _pairs(ops):
    return [(a["kind"], b["kind"]) for a, b in zip(ops, ops[1:])]


@pytest.mark.parametrize("name,seed", CASES)
def test_walk_is_deterministic_and_holds_every_ordered_pair_once(name, seed):
    ops, again = _run(name, seed)[0], _walk(name, seed)
    assert _same(ops, again)
    assert not _same(ops, _walk(name, seed + 100))
    kinds = pw.kinds_of(name)
    assert ("pending" in kinds) == bool(pw.HANDLES[name].get("live"))
    pairs = _pairs(ops)
    assert len(pairs) == len(kinds) ** 2 and set(pairs) == {(a, b) for a in kinds for b in kinds}


@pytest.mark.parametrize("name,seed", CASES)
def test_walk_on_the_model_reaches_what_the_gpu_test_is_about(name, seed):
    ops, m = _run(name, seed)   # (no buffer ever held a NaN: run_model asserts it after every op)
    assert (m.fused >= 2).all(), "fused resets per env: %r" % (m.fused,)
    assert m.catches >= 1, "no catch was reported in `removed`"
    assert m.sentinels_left("f") > 0 and m.sentinels_left("h") > 0, "no sentinel survives in a float32 / half slot"
    assert m.overwritten > 0, "no sentinel was overwritten by a store"
    assert m.mid_episode_resets > 0, "no masked reset hit an env with t > 0"
    if name == "XF_c1":
        for entry in (pw.ENTRY_FIXED, pw.ENTRY_WAVE, pw.ENTRY_GENERIC):
            assert m.entries.count(entry) >= 5, (entry, m.entries.count(entry))
    else:
        assert pw.ENTRY_FIXED not in m.entries
    if pw.HANDLES[name].get("live"):
        assert len(set(m.live)) > 1, "the envs never ran different counts"


@pytest.mark.parametrize("half,seed", PY_CASES)
def test_python_level_walk_on_the_model(half, seed):
    ops, m = _run("XF_c1", seed, half)
    pairs = _pairs(ops)
    assert len(pairs) == len(pw.PY_KINDS) ** 2 and set(pairs) == {(a, b) for a in pw.PY_KINDS for b in pw.PY_KINDS}
    assert _same(ops, _walk("XF_c1", seed, half))
    assert (m.fused >= 2).all() and m.overwritten > 0 and m.mid_episode_resets > 0
    assert m.sentinels_left("h" if half else "f") > 0
    if not half:
        assert m.entries.count(pw.ENTRY_FIXED) >= 3 and pw.ENTRY_WAVE in m.entries and pw.ENTRY_GENERIC in m.entries


def test_sentinels_are_exact_in_binary16_distinct_per_slot_and_never_a_stored_value():
    idx = np.arange(5000)
    seen = []
    for slot in range(6):
        for salt in (0, 1, 7):
            v = pw.sentinels(slot, idx, salt)
            assert v.dtype == np.float32 and pw.is_sentinel(v).all()   # negative: a step stores |count| / layer_norm, ids and map cells, all >= 0
            assert np.array_equal(pw.widen(pw.half_bits(v)), v)
            assert (v[1:] != v[:-1]).all()
            seen.append(set(v.tolist()))
    for a in range(0, 18, 3):
        for b in range(a + 3, 18, 3):
            assert not (seen[a] & seen[b])


def test_half_rule_is_the_float32_to_float16_tensor_conversion():
    import torch
    rng = np.random.RandomState(11)
    some_halves = rng.randint(0, 0x7BFF, size=2500).astype(np.uint16)   # finite, non-negative, not the largest
    lo, hi = pw.widen(some_halves).astype(np.float64), pw.widen(some_halves + 1).astype(np.float64)
    ties = ((lo + hi) / 2).astype(np.float32)                            # exactly half way between two neighbouring halves
    assert np.array_equal(ties.astype(np.float64), (lo + hi) / 2)
    x = np.concatenate([
        rng.standard_normal(2500).astype(np.float32) * 10.0,
        (rng.rand(2000).astype(np.float32) * 2 - 1) * np.float32(6.0e-5),   # subnormal results (below 2 ** -14) and underflow
        ties, -ties[:500],
        np.float32([0.0, -0.0, 0.3, 65504.0, 65519.99, 65520.0, 1e6, -1e6, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, np.inf, -np.inf]),
        (rng.rand(2487).astype(np.float32) * 70000.0)])
    assert x.size == 10000
    got = pw.half_bits(x)
    want = torch.from_numpy(x).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    mag = got & 0x7FFF
    assert ((mag > 0) & (mag < 0x0400)).sum() > 500, "subnormal results"
    assert (mag == 0x7C00).sum() > 100, "overflow to infinity"
    assert np.array_equal(pw.half_bits(ties), some_halves + (some_halves & 1)), "ties go to the even neighbour"


def test_model_reset_and_step_reproduce_a_golden(golden_dir):
    """tests/golden/pursuit_tiny5_dense through Model.reset / Model.step (load the buffer into local_obs, run, store), in place and hopping
    between two float32 slots and two half slots: every env of the model is the golden's env"""
    from oracle import pursuit as po
    g = np.load(os.path.join(golden_dir, "pursuit_tiny5_dense.npz"))
    cfg = po.config_from_golden(g)
    shape = (int(g["cfg_xs"]), int(g["cfg_ys"]), cfg.pop("n_pursuers"), cfg.pop("n_evaders"), cfg.pop("obs_range"), int(cfg.pop("flatten")))
    spec = dict(shape=shape, kw=cfg, fixed=True, to=True, f16=True)
    m = pw.Model("tiny5_dense", 0, spec=spec, maps=list(g["maps"]), max_steps=0, auto_reset=False)
    for s in ("f0", "f1"):
        m.apply(("zero", s))   # the golden starts from the reference's zeroed local_obs
    for s in ("h0", "h1"):
        m.view(s, "h")[:] = 0
    at, at16, steps = "f0", "h0", 0
    for t in range(len(g["op"])):
        want = g["obs_f32"][t].reshape(m.P, m.D)
        if g["op"][t] == 0:
            pos = np.concatenate([g["init_p"][t], g["init_e"][t]])[None]
            m.reset(at, "f", None, inj_pos=pos, inj_map=np.array([g["map_id"][t]]))
            m.view(at16, "h")[:] = pw.half_bits(m.view(at, "f"))   # (the half ring restarts from the float32 reset, as a caller would)
        else:
            m.inj = True
            act, inj = np.repeat(g["act_p"][t][None], pw.N, 0), np.repeat(g["act_e"][t][None], pw.N, 0)
            nxt16 = "h1" if at16 == "h0" else "h0"
            m.step("f16", at16, nxt16, "h", act, inj)
            at16 = nxt16
            states = [o.get_state() for o in m.orcs]
            for o, st in zip(m.orcs, states):   # (the half step moved the agents: put the float32 step's start back)
                o.set_state(prev_state[m.orcs.index(o)])
            nxt = at if steps % 2 else ("f1" if at == "f0" else "f0")
            m.step("inplace" if nxt == at else "to", at, nxt, "f", act, inj)
            at, steps = nxt, steps + 1
            for n in range(pw.N):
                assert np.array_equal(m.rew[n], g["rew_f64"][t].astype(np.float32)), "rewards, op %d" % t
            assert (m.done == int(g["done"][t])).all() and (m.removed == int(g["removed"][t])).all(), "done / removed, op %d" % t
            for o, st in zip(m.orcs, states):
                for k in st:
                    assert np.array_equal(o.get_state()[k], st[k]), (t, k)
            got16 = m.view(at16, "h").reshape(pw.N, m.P, m.D)
            assert all(np.array_equal(got16[n], pw.half_bits(want)) for n in range(pw.N)), "half slot, op %d" % t
        prev_state = [o.get_state() for o in m.orcs]
        got = m.view(at, "f").reshape(pw.N, m.P, m.D)
        for n in range(pw.N):
            assert np.array_equal(got[n], want), "observations of env %d, op %d" % (n, t)
    assert steps > 100
