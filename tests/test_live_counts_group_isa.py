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
import os
import re
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_wave_isa_budget as fixed   # noqa: E402  (NOT_SALU)

CSRC = os.path.join(ROOT, "madrl_amd", "csrc")
CAPS = [(32, 32, 30, 50, 11, 1, 4), (32, 32, 30, 30, 11, 1, 4), (16, 16, 20, 50, 5, 1, 2)]
# static SALU of the env loop (rare paths included) above the fixed kernel's.  Measured: 554 against 381 (30 v 50), 537 against 360
# (30 v 30), 470 against 350 (20 v 50).  About 130 of the extra are the global reward's numpy-order sum over a run-time count (np_sum_first:
# a scalar compare and select per pursuer, only run with reward_mech="global"); the rest are the four ballot popcounts of the live counts
# from the record, the reset's pending-count loads and clamps and the id-cell refresh.
SALU_EXTRA = 190


def _lines(name):
    text = open(os.path.join(CSRC, name)).read()
    return {kind: {tuple(int(v) for v in m.group(1).split(",")) for m in re.finditer(r"^\s*%s\(([^)]*)\)" % kind, text, re.M)}
            for kind in ("X", "XG", "XL", "XLG")}


def _compile():
    from madrl_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    tu = '#include "common.hpp"\n#include "pursuit_group.hpp"\nnamespace madrl { namespace pw {\n'
    for kind in ("GShape", "LGShape"):
        for cap in CAPS:
            tu += "template __global__ void pursuit_group_kernel<%s<%d, %d, %d, %d, %d, %d, %d>, 1, false>(const WaveDev, const WaveIO);\n" % (
                (kind,) + cap)
    tu += "} }\n"
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "group_live.hip"), os.path.join(tmp, "group_live.s")
        with open(src, "w") as f:
            f.write(tu)
        subprocess.run([B.HIPCC] + [f for f in B.FLAGS if f != "-Wall"] + ["-I", CSRC, "--cuda-device-only", "-S", src, "-o", out],
                       check=True, capture_output=True)
        import find_masked_spills
        masked = find_masked_spills.scan(out, "LGShape")
        text = open(out).read()
    return text, masked


@pytest.fixture(scope="module")
def asm():
    return _compile()


def _mangled(kind, cap):
    return "_ZN5madrl2pw20pursuit_group_kernelINS0_%d%sI%sEELi1ELb0EEEvNS0_7WaveDevENS0_6WaveIOE" % (
        len(kind), kind, "".join("Li%dE" % v for v in cap))


def _body(text, name):
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def _meta(text, name):
    i = text.index(".name:           " + name)
    j, k = text.rfind("  - .agpr_count", 0, i), text.find("  - .agpr_count", i)
    return text[j:k if k > 0 else len(text)]


def _env_loop(body):
    """instructions of the env loop: the outermost loop around the observation stores (global_store_dwordx4 ... nt), inner loops included"""
    blocks, cur = [], None
    for l in body:
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)", l)
        if m:
            cur = dict(name=m.group(1), notes=l, insts=[], open=True)
            blocks.append(cur)
        elif cur is not None:
            t = l.strip()
            if t.startswith(";") and cur["open"]:
                cur["notes"] += " " + t
            elif t and not t.startswith((";", ".")):
                cur["open"] = False
                cur["insts"].append(t.split(";")[0].strip())
    home = next(b for b in blocks if any(i.startswith("global_store_dwordx4") and i.endswith(" nt") for i in b["insts"]))
    parents = re.findall(r"Parent Loop (BB\d+_\d+) Depth=1", home["notes"])
    hm = re.search(r"Header=(BB\d+_\d+)", home["notes"])
    header = parents[0] if parents else (hm.group(1) if hm else home["name"])
    if not parents and hm:   # the block sits in an inner loop: its header names the outermost loop among its parents
        hb = next(b for b in blocks if b["name"] == hm.group(1))
        header = (re.findall(r"Parent Loop (BB\d+_\d+) Depth=1", hb["notes"]) or [hm.group(1)])[0]
    headers, grown = {header}, True
    while grown:
        grown = False
        for b in blocks:
            if b["name"] and b["name"] not in headers and any(p in headers for p in re.findall(r"Parent Loop (BB\d+_\d+)", b["notes"])):
                headers.add(b["name"])
                grown = True
    own = lambda b: b["name"] in headers or any(h in headers for h in re.findall(r"Header=(BB\d+_\d+)", b["notes"]))
    return [i for b in blocks if own(b) for i in b["insts"]]


@pytest.mark.parametrize("cap", CAPS, ids=lambda c: "%dv%d" % (c[2], c[3]))
def test_live_group_kernel_keeps_the_fixed_kernels_contracts(asm, cap):
    text, _ = asm
    live, fix = _env_loop(_body(text, _mangled("LGShape", cap))), _env_loop(_body(text, _mangled("GShape", cap)))
    stores = lambda loop: [i.split()[0] for i in loop if re.match(r"global_store_\w+", i)]
    assert sorted(stores(live)) == sorted(stores(fix)), (len(stores(live)), len(stores(fix)))
    assert sum(1 for i in live if i.startswith("global_store_dwordx4") and i.endswith(" nt")) == \
        sum(1 for i in fix if i.startswith("global_store_dwordx4") and i.endswith(" nt"))
    waits = lambda loop: sorted(re.sub(r"\s+", " ", i) for i in loop if re.match(r"s_waitcnt vmcnt\(\d+\)$", i))
    assert waits(live) == waits(fix) and waits(fix), (waits(live), waits(fix))
    salu = lambda loop: len([i for i in loop if i.startswith("s_") and not i.startswith(fixed.NOT_SALU)])
    assert salu(live) <= salu(fix) + SALU_EXTRA, (salu(live), salu(fix))


@pytest.mark.parametrize("cap", CAPS, ids=lambda c: "%dv%d" % (c[2], c[3]))
def test_live_group_kernel_no_scratch(asm, cap):
    meta = _meta(asm[0], _mangled("LGShape", cap))
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta
    assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), meta


def test_live_group_kernels_have_no_masked_spills(asm):
    assert asm[1] == []


def test_def_lists_are_consistent():
    fixed_lines, live = _lines("pursuit_specializations.def"), _lines("pursuit_live_specializations.def")
    assert set(CAPS) <= live["XLG"]
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
