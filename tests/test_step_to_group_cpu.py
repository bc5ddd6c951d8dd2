"""CPU test (-m "not gpu"): the two-buffer step of the multi-wavefront family (pursuit_group_kernel over a TGShape / TLGShape, the XG / XLG
lines of pursuit_to_specializations.def) -- the lists, the build tool's lines and refusals, and the emitted code of the two-buffer
kernels, compiled for gfx950 with the build's own flags beside their in-place counterparts:
  * no scratch and no VGPR spills, and scripts/find_masked_spills.py finds no spill copy under a narrowed exec mask;
  * as many s_barrier as the in-place kernel of the same shape (the two-buffer row pass is per thread);
  * the env loop loads float4s (the kept elements come from the previous buffer in whole float4s)."""
import os
import re
import subprocess
import sys

import pytest

import isa
from isa import CSRC, ROOT

CAPS = [(32, 32, 16, 60, 7, 1, 2), (32, 32, 30, 50, 11, 1, 4), (16, 16, 20, 50, 5, 1, 2)]
IN_PLACE = {"TGShape": "GShape", "TLGShape": "LGShape"}
REQUIRED = {
    "XG": [(32, 32, 16, 60, 7, 1, 2), (32, 32, 30, 50, 11, 1, 4), (32, 32, 30, 30, 11, 1, 4)],
    "XLG": [(32, 32, 30, 50, 11, 1, 4), (32, 32, 30, 30, 11, 1, 4), (16, 16, 20, 50, 5, 1, 2)],
}


def test_committed_group_lines_stand_on_their_fast_lines():
    to = isa.def_lines("pursuit_to_specializations.def")
    for kind, shapes in REQUIRED.items():
        for s in shapes:
            assert s in to.get(kind, []), (kind, s)
    fixed = isa.def_lines("pursuit_specializations.def", ("XG",))["XG"]
    live = isa.def_lines("pursuit_live_specializations.def", ("XLG",))["XLG"]
    for s in to.get("XG", []) + to.get("XLG", []):
        assert s in fixed, s          # (the same NW: the tuple holds it)
    for s in to.get("XLG", []):
        assert s in live, s
    assert (16, 16, 20, 50, 5, 1, 2) not in to.get("XG", [])   # the fixed handle of the test shape stays on the generic step_to


def test_every_includer_defines_the_six_kinds():
    for name in ("pursuit_to.hip", "pursuit_to_group.hip", "pursuit.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "pursuit_to_specializations.def"' in text, name
        head = text[:text.rindex('#include "pursuit_to_specializations.def"')]
        for kind in ("X", "XL", "XC", "XLC", "XG", "XLG"):
            assert re.search(r"^#define %s\(" % kind, head, re.M), (name, kind)


def test_pursuit_to_group_lines():
    from madrl_amd import build as B
    assert B.pursuit_to_group_lines(32, 32, 30, 50, 11, 1) == ("XG(32, 32, 30, 50, 11, 1, 4)", "XG(32, 32, 30, 50, 11, 1, 4)")
    assert B.pursuit_to_group_lines(32, 32, 30, 50, 11, 1, live=True) == ("XLG(32, 32, 30, 50, 11, 1, 4)", "XG(32, 32, 30, 50, 11, 1, 4)")
    assert B.pursuit_to_group_lines(32, 32, 16, 60, 7, 1) == ("XG(32, 32, 16, 60, 7, 1, 2)", "XG(32, 32, 16, 60, 7, 1, 2)")
    line, why = B.pursuit_to_group_lines(16, 16, 8, 30, 7, 1)          # one wavefront per env
    assert line is None and "--pursuit-to-shape" in why
    line, why = B.pursuit_to_group_lines(24, 24, 20, 300, 9, 1)        # the crowd kernel
    assert line is None and "--pursuit-to-shape" in why
    line, why = B.pursuit_to_group_lines(16, 16, 8, 30, 6, 1)          # no fast path at all
    assert line is None and "even obs_range" in why
    # the one-wavefront / crowd tool still refuses an XG shape, and names the option that takes it
    line, why = B.pursuit_to_lines(32, 32, 30, 50, 11, 1)
    assert line is None and "multi-wavefront" in why and "--pursuit-to-group-shape" in why


@pytest.mark.parametrize("shape,reason", [((16, 16, 8, 30, 7, 1), "--pursuit-to-shape"), ((16, 16, 8, 30, 6, 1), "even obs_range"),
                                          ((16, 16, 8, 30, 6, 1, 1), "even obs_range")])
def test_build_refuses_a_shape_without_a_group_fast_path(shape, reason):
    """python -m madrl_amd.build --pursuit-to-group-shape: refused with the reason, before anything is written or compiled"""
    local = [os.path.join(CSRC, n) for n in ("pursuit_to_specializations.local.def", "pursuit_specializations.local.def",
                                             "pursuit_live_specializations.local.def")]
    had = [os.path.exists(f) and open(f).read() for f in local]
    r = subprocess.run([sys.executable, "-m", "madrl_amd.build", "--pursuit-to-group-shape"] + [str(v) for v in shape], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode != 0
    assert "no two-buffer multi-wavefront kernel" in r.stdout and reason in r.stdout
    assert [os.path.exists(f) and open(f).read() for f in local] == had


# ------------------------------------------------------------------ emitted code
TU = isa.group_tu([(kind, cap) for kind in ("GShape", "TGShape", "LGShape", "TLGShape") for cap in CAPS], inject=True)


@pytest.fixture(scope="module")
def asm():
    return isa.compile_asm(TU)


KERNELS = [(kind, cap) for kind in ("TGShape", "TLGShape") for cap in CAPS]
_id = lambda v: v if isinstance(v, str) else "%dv%d" % (v[2], v[3])
_mangled = lambda kind, cap: isa.group_kernel(kind, cap, inject=True)


@pytest.mark.parametrize("kind,cap", KERNELS, ids=_id)
def test_two_buffer_group_kernel_no_scratch(asm, kind, cap):
    meta = isa.kernel_meta(asm, _mangled(kind, cap))
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta


def test_two_buffer_group_kernels_have_no_masked_spills(asm):
    assert isa.masked_spills(asm, "TGShape") + isa.masked_spills(asm, "TLGShape") == []


@pytest.mark.parametrize("kind,cap", KERNELS, ids=_id)
def test_two_buffer_group_kernel_adds_no_barrier_and_loads_float4s(asm, kind, cap):
    to, ip = _mangled(kind, cap), _mangled(IN_PLACE[kind], cap)
    barriers = lambda name: sum(1 for i in isa.kernel_insts(asm, name) if i.startswith("s_barrier"))
    assert barriers(to) == barriers(ip) and barriers(ip) > 0, (barriers(to), barriers(ip))
    loop, ip_loop = isa.store_env_loop(asm, to), isa.store_env_loop(asm, ip)
    assert any(i.startswith("global_load_dwordx4") for i in loop)
    assert not any(i.startswith("global_load_dwordx4") for i in ip_loop)   # (the in-place pass loads no float4: the check above sees the new loads)
    # whole stores only: the two-buffer kernel adds non-temporal float4 stores, and no dword store, to the in-place kernel's
    dword = lambda l: sum(1 for i in l if re.match(r"global_store_dword\s", i))
    assert dword(loop) == dword(ip_loop)
