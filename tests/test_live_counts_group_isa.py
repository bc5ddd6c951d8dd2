"""CPU test (-m "not gpu"): the live-count instantiations of the group kernel (pursuit_group_kernel over an LGShape, the XLG lines of
pursuit_live_specializations.def) keep the contracts of the fixed-shape group kernel of the same shape, compiled for gfx950 with the
build's own flags:
  * no scratch and no VGPR spills;
  * the env loop holds exactly as many global stores as the fixed kernel's (rows past an env's live pursuer count keep their store
    instructions; no lane takes them) and the same s_waitcnt vmcnt(...) waits -- the group kernel's record prefetch is waited for at the
    pipeline hinge with compiler-made waits, which must not turn into more or other waits;
  * the static SALU count of the env loop stays within a stated budget of the fixed kernel's;
  * scripts/find_masked_spills.py finds no spill copy under a narrowed exec mask.
Also: the .def lists are consistent, and the build tool forms the right lines."""
import re

import pytest

import isa

CAPS = [(32, 32, 30, 50, 11, 1, 4), (32, 32, 30, 30, 11, 1, 4), (16, 16, 20, 50, 5, 1, 2)]
# static SALU of the env loop (rare paths included) above the fixed kernel's.  Measured: 554 against 381 (30 v 50), 537 against 360
# (30 v 30), 470 against 350 (20 v 50).  About 130 of the extra are the global reward's numpy-order sum over a run-time count (np_sum_first:
# a scalar compare and select per pursuer, only run with reward_mech="global"); the rest are the four ballot popcounts of the live counts
# from the record, the reset's pending-count loads and clamps and the id-cell refresh.
SALU_EXTRA = 190
TU = isa.group_tu([(kind, cap) for kind in ("GShape", "LGShape") for cap in CAPS], inject=False)


@pytest.fixture(scope="module")
def asm():
    return isa.compile_asm(TU)


@pytest.mark.parametrize("cap", CAPS, ids=lambda c: "%dv%d" % (c[2], c[3]))
def test_live_group_kernel_keeps_the_fixed_kernels_contracts(asm, cap):
    live, fix = (isa.store_env_loop(asm, isa.group_kernel(kind, cap)) for kind in ("LGShape", "GShape"))
    stores = lambda loop: [i.split()[0] for i in loop if re.match(r"global_store_\w+", i)]
    assert sorted(stores(live)) == sorted(stores(fix)), (len(stores(live)), len(stores(fix)))
    assert sum(1 for i in live if i.startswith("global_store_dwordx4") and i.endswith(" nt")) == \
        sum(1 for i in fix if i.startswith("global_store_dwordx4") and i.endswith(" nt"))
    waits = lambda loop: sorted(re.sub(r"\s+", " ", i) for i in loop if re.match(r"s_waitcnt vmcnt\(\d+\)$", i))
    assert waits(live) == waits(fix) and waits(fix), (waits(live), waits(fix))
    salu = lambda loop: len(isa.salu(loop))
    assert salu(live) <= salu(fix) + SALU_EXTRA, (salu(live), salu(fix))


@pytest.mark.parametrize("cap", CAPS, ids=lambda c: "%dv%d" % (c[2], c[3]))
def test_live_group_kernel_no_scratch(asm, cap):
    meta = isa.kernel_meta(asm, isa.group_kernel("LGShape", cap))
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta


def test_live_group_kernels_have_no_masked_spills(asm):
    assert isa.masked_spills(asm, "LGShape") == []


def test_def_lists_are_consistent():
    fixed_lines = isa.def_lines("pursuit_specializations.def", ("X", "XG"))
    live = isa.def_lines("pursuit_live_specializations.def", ("XL", "XLG"))
    assert set(CAPS) <= set(live["XLG"])
    for line in live["XLG"]:
        assert line in fixed_lines["XG"], line   # same shape, same NW
    for line in live["XL"]:
        assert line in fixed_lines["X"], line
    assert not any(line[:6] == (32, 32, 16, 60, 7, 1) for line in live["XLG"])   # BASELINE configs[4]: generic with per-env counts


def test_build_tool_forms_the_live_lines():
    from madrl_amd import build as B
    assert B.pursuit_live_lines(32, 32, 30, 50, 11, 1) == ("XLG(32, 32, 30, 50, 11, 1, 4)", "XG(32, 32, 30, 50, 11, 1, 4)")
    assert B.pursuit_live_lines(16, 16, 20, 50, 5, 1) == ("XLG(16, 16, 20, 50, 5, 1, 2)", "XG(16, 16, 20, 50, 5, 1, 2)")
    assert B.pursuit_live_lines(16, 16, 8, 30, 7, 1) == ("XL(16, 16, 8, 30, 7, 1)", "X(16, 16, 8, 30, 7, 1)")
    assert B.pursuit_live_lines(20, 20, 12, 40, 9, 0) == ("XLG(20, 20, 12, 40, 9, 0, 2)", "XG(20, 20, 12, 40, 9, 0, 2)")
    # what pursuit_fast_path refuses, the live form refuses too -- and add_pursuit_live_shape raises with the same reason
    for bad, why in (((16, 16, 8, 30, 6, 1), "even obs_range"), ((16, 16, 100, 30, 7, 1), "more than 64"),
                     ((16, 16, 8, 30, 7, 1, False), "flatten without the id")):
        assert B.pursuit_live_lines(*bad) is None
        assert why in B.pursuit_fast_path(*bad)[1]
    with pytest.raises(ValueError, match="even obs_range"):
        B.add_pursuit_live_shape(16, 16, 8, 30, 6, 1)


def test_live_hint_names_the_group_line():
    """the per-env-counts hint of a large batch on the generic kernel names the XLG line and the build command for a capacity whose
    fixed shape runs on the group kernel"""
    import types
    import warnings
    from madrl_amd.pursuit import BatchedPursuitEvade
    fake = types.SimpleNamespace(xs=20, ys=20, n_pursuers=12, n_evaders=40, obs_range=9, flatten=False, include_id=True, train_pursuit=True,
                                 per_env_counts=True, kernel_kind="generic")
    BatchedPursuitEvade._hinted.discard((20, 20, 12, 40, 9, 0))
    with warnings.catch_warnings(record=True) as got:
        warnings.simplefilter("always")
        BatchedPursuitEvade._hint_fast_path(fake)
    msg = " ".join(str(w.message) for w in got)
    assert "XLG(20,20,12,40,9,0,2)" in msg and "--pursuit-live-shape 20 20 12 40 9 0" in msg, msg
