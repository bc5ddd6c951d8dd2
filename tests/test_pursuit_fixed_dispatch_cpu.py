"""CPU test (-m "not gpu"): which step launches take the Pursuit kernel with its launch constants folded in (pw::FShape, the XF lines of
csrc/pursuit_fixed_specializations.def).  madrl_pursuit_fixed_choice is the host's own decision -- launch() in pursuit.hip calls the same
function (takes_fixed: the line's XF kernel, fixed_contract) -- answered without a device: every XF line in the contract's form takes the fixed kernel,
and each clause of the contract flipped ALONE sends the launch to the plain kernel of the line."""
import ctypes as C
import os

import pytest

import isa

XF_LINES = isa.def_lines("pursuit_fixed_specializations.def", ("XF",))["XF"]
HEADLINE = (16, 16, 8, 30, 7, 1)
# the launch bits of include/madrl_hip.h
PER_ENV_COUNTS, CURRICULUM_ARRAYS, INJECTED_ACTIONS, WALK_ALTERNATE, WALK_FORWARD, STEP_TO, HALF, RESET, KERNEL_GENERIC = (1 << k for k in range(9))


def _cfg(line, **over):
    from madrl_amd import _lib
    c = _lib.PursuitConfig()
    c.struct_size = C.sizeof(_lib.PursuitConfig)
    c.xs, c.ys, c.n_pursuers, c.n_evaders, c.obs_range, c.flatten = line[:6]
    c.n_catch, c.surround, c.include_id, c.n_maps = 2, 1, 1, 1
    c.layer_norm, c.constraint_window = 10.0, 1.0
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _choice(cfg, bits=0, n_envs=32768):
    from madrl_amd import _lib
    out = C.c_int32(-1)
    assert _lib.lib().madrl_pursuit_fixed_choice(C.byref(cfg), n_envs, bits, C.byref(out)) == 0, _lib.lib().madrl_last_error()
    assert out.value in (0, 1)
    return bool(out.value)


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    monkeypatch.delenv("MADRL_PURSUIT_FIXED", raising=False)


@pytest.mark.parametrize("line", XF_LINES, ids=lambda l: "-".join(map(str, l)))
def test_every_xf_line_takes_the_fixed_kernel_in_the_contracts_form(line):
    assert _choice(_cfg(line))
    assert _choice(_cfg(line), WALK_FORWARD)
    assert _choice(_cfg(line, max_steps=500, auto_reset=1, n_catch=3, catchr=0.1, term_pursuit=5.0, urgency_reward=-0.1))   # run-time values


def test_the_headline_is_the_first_line_and_a_shape_without_a_line_is_not_fixed():
    assert XF_LINES[0] == HEADLINE
    unlisted = (10, 10, 2, 2, 3, 1)   # an X line without an XF line
    assert unlisted in isa.def_lines("pursuit_specializations.def", ("X",))["X"] and unlisted not in XF_LINES
    assert not _choice(_cfg(unlisted))
    assert not _choice(_cfg((16, 16, 7, 30, 7, 1)))   # no fast line at all
    assert not _choice(_cfg(HEADLINE, include_id=0))   # off its X line: a flatten row without the id


CLAUSES = {
    "surround=False": (dict(surround=0), 0),
    "global reward": (dict(reward_global=1), 0),
    "a two-map pool with sample_maps": (dict(n_maps=2, sample_maps=1), 0),
    "a two-map pool": (dict(n_maps=2), 0),
    "sample_maps on one map": (dict(sample_maps=1), 0),
    "train_pursuit=False": (dict(control_evaders=1), 0),
    "random_opponents": (dict(max_opponents=6), 0),
    "per_env_counts": ({}, PER_ENV_COUNTS),
    "per-env curriculum arrays": ({}, CURRICULUM_ARRAYS),
    "injected evader actions": ({}, INJECTED_ACTIONS),
    'set_walk("alternate")': ({}, WALK_ALTERNATE),
    "step_to": ({}, STEP_TO),
    "half-precision observations": ({}, STEP_TO | HALF),
    "a reset launch": ({}, RESET),
    'kernel="generic"': ({}, KERNEL_GENERIC),
}


@pytest.mark.parametrize("clause", sorted(CLAUSES))
def test_each_contract_clause_flipped_alone_selects_the_plain_kernel(clause):
    over, bits = CLAUSES[clause]
    assert _choice(_cfg(HEADLINE))
    assert not _choice(_cfg(HEADLINE, **over), bits), clause


def test_the_override_variable(monkeypatch):
    monkeypatch.setenv("MADRL_PURSUIT_FIXED", "0")
    assert not _choice(_cfg(HEADLINE))
    monkeypatch.setenv("MADRL_PURSUIT_FIXED", "1")
    assert _choice(_cfg(HEADLINE))


def test_the_automatic_walk_alternates_above_its_threshold():
    """walk mode auto: forward up to ~375 MB of rows and records per launch (the benchmark's 32 768-env launches: 158 MB), alternating
    above -- those launches stay on the plain kernel, unless the walk is set forward"""
    assert _choice(_cfg(HEADLINE), n_envs=65536)
    assert not _choice(_cfg(HEADLINE), n_envs=131072)
    assert _choice(_cfg(HEADLINE), WALK_FORWARD, n_envs=131072)


def test_bad_arguments_are_refused():
    from madrl_amd import _lib
    out = C.c_int32()
    L = _lib.lib()
    assert L.madrl_pursuit_fixed_choice(C.byref(_cfg(HEADLINE)), 0, 0, C.byref(out)) != 0
    assert L.madrl_pursuit_fixed_choice(C.byref(_cfg(HEADLINE)), 8, 1 << 9, C.byref(out)) != 0
    assert L.madrl_pursuit_fixed_choice(C.byref(_cfg(HEADLINE)), 8, 0, None) != 0
    assert L.madrl_pursuit_last_step_entry(None, C.byref(out)) != 0
