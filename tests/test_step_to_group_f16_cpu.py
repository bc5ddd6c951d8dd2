"""CPU test (-m "not gpu"): the half-precision two-buffer step of the multi-wavefront family (pursuit_group_kernel over a THGShape /
TLHGShape, the HG / HLG lines of pursuit_to_f16_group_specializations.def) -- the list, the kernels of the built library, the emitted code
of the instantiations compiled for gfx950 with the build's own flags beside their in-place counterparts, and the build tool's lines and
refusals."""
import os
import re
import subprocess
import sys

import pytest

import isa
from isa import CSRC, ROOT

DEF = "pursuit_to_f16_group_specializations.def"
REQUIRED = {
    "HG": [(32, 32, 30, 50, 11, 1, 4), (32, 32, 30, 30, 11, 1, 4), (10, 10, 36, 12, 11, 1, 4), (12, 12, 46, 10, 13, 1, 4),
           (12, 12, 64, 20, 13, 1, 4), (16, 16, 64, 40, 3, 1, 2)],
    "HLG": [(32, 32, 30, 50, 11, 1, 4), (32, 32, 30, 30, 11, 1, 4), (16, 16, 20, 50, 5, 1, 2)],
}
SHAPE = {"HG": "THGShape", "HLG": "TLHGShape"}       # the kernel's shape type of a line
IN_PLACE = {"THGShape": "GShape", "TLHGShape": "LGShape"}
FLOAT32 = {"THGShape": "TGShape", "TLHGShape": "TLGShape"}


_mangled = lambda kind, cap: isa.group_kernel(kind, cap, inject=True)


KERNELS = [(SHAPE[kind], cap) for kind in ("HG", "HLG") for cap in REQUIRED[kind]]
_id = lambda v: v if isinstance(v, str) else "%dv%d" % (v[2], v[3])


# ------------------------------------------------------------------ the list
def test_committed_half_lines_stand_on_their_fast_lines():
    half = isa.def_lines(DEF)
    assert set(half) == {"HG", "HLG"}, sorted(half)
    for kind, shapes in REQUIRED.items():
        for s in shapes:
            assert s in half[kind], (kind, s)
    fixed = isa.def_lines("pursuit_specializations.def", ("XG",))["XG"]
    live = isa.def_lines("pursuit_live_specializations.def", ("XLG",))["XLG"]
    for s in half["HG"] + half["HLG"]:
        assert s in fixed, s          # (the same NW: the tuple holds it)
    for s in half["HLG"]:
        assert s in live, s
    # BASELINE configs[4] is not listed: tests/test_step_to_f16_gpu.py (XG_runs_generic) pins its half step to the generic kernel;
    # listing it goes together with that test
    assert not any(s[:6] == (32, 32, 16, 60, 7, 1) for s in half["HG"] + half["HLG"])
    # the two-buffer list keeps its six kinds: the half lines have a file of their own
    assert not any(k.startswith("H") for k in isa.def_lines("pursuit_to_specializations.def"))


def test_every_includer_defines_both_kinds():
    for name in ("pursuit_to_group_f16.hip", "pursuit_to_group_f16_live.hip", "pursuit.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "%s"' % DEF in text and '__has_include("%s")' % DEF.replace(".def", ".local.def") in text, name
        head = text[:text.rindex('#include "%s"' % DEF)]
        for kind in ("HG", "HLG"):
            assert re.search(r"^#define %s\(" % kind, head, re.M), (name, kind)


# ------------------------------------------------------------------ the built library
@pytest.fixture(scope="module")
def lib_kernels():
    return isa.built_kernels()


@pytest.mark.parametrize("kind,cap", KERNELS, ids=_id)
def test_built_library_holds_the_half_group_kernel(lib_kernels, kind, cap):
    k = lib_kernels.get(_mangled(kind, cap))
    assert k is not None, "the library has no %s kernel of %s" % (kind, cap)
    assert k["scratch"] == 0 and k["vgpr_spills"] == 0, k
    # the arguments are exactly the float32 group kernels': WaveDev / WaveIO did not grow
    assert k["args"] == lib_kernels[_mangled(IN_PLACE[kind], cap)]["args"]
    f32 = lib_kernels.get(_mangled(FLOAT32[kind], cap))   # (a half line does not need a float32 two-buffer line)
    if f32 is not None:
        assert k["vgprs"] <= f32["vgprs"], (k["vgprs"], f32["vgprs"])


def test_the_lines_with_a_float32_two_buffer_kernel_are_compared(lib_kernels):
    """(the register comparison above is not skipped everywhere: the authors' shapes have both forms)"""
    both = [(kind, cap) for kind, cap in KERNELS if _mangled(FLOAT32[kind], cap) in lib_kernels]
    assert len(both) >= 7, both


# ------------------------------------------------------------------ emitted code
TU = isa.group_tu([(k, cap) for kind, cap in KERNELS for k in (kind, IN_PLACE[kind])], inject=True)


@pytest.fixture(scope="module")
def asm():
    return isa.compile_asm(TU)


@pytest.mark.parametrize("kind,cap", KERNELS, ids=_id)
def test_half_group_kernel_no_scratch(asm, kind, cap):
    meta = isa.kernel_meta(asm, _mangled(kind, cap))
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta


def test_half_group_kernels_have_no_masked_spills(asm):
    assert isa.masked_spills(asm, "THGShape") + isa.masked_spills(asm, "TLHGShape") == []


@pytest.mark.parametrize("kind,cap", KERNELS, ids=_id)
def test_half_group_kernel_adds_no_barrier_and_moves_whole_8_byte_slots(asm, kind, cap):
    inst, ip = isa.kernel_insts(asm, _mangled(kind, cap)), isa.kernel_insts(asm, _mangled(IN_PLACE[kind], cap))
    barriers = lambda insts: sum(1 for i in insts if i.startswith("s_barrier"))
    assert barriers(inst) == barriers(ip) and barriers(ip) > 0, (barriers(inst), barriers(ip))
    # a slot is 8 bytes: it is loaded and stored as one word, the two-buffer pass's stores non-temporal; nothing float4-sized is left
    assert any(re.match(r"global_load_dwordx2\s", i) for i in inst)
    assert any(re.match(r"global_store_dwordx2\s", i) and i.endswith(" nt") for i in inst)
    assert any(re.match(r"global_store_dwordx4\s", i) and i.endswith(" nt") for i in ip)
    assert not any(re.match(r"global_store_dwordx4\s", i) for i in inst), "a float4 store in a kernel over binary16 buffers"


# ------------------------------------------------------------------ the build tool
def test_pursuit_to_group_f16_lines():
    from madrl_amd import build as B
    assert B.pursuit_to_group_f16_lines(32, 32, 30, 50, 11, 1) == ("HG(32, 32, 30, 50, 11, 1, 4)", "XG(32, 32, 30, 50, 11, 1, 4)")
    assert B.pursuit_to_group_f16_lines(32, 32, 30, 50, 11, 1, live=True) == ("HLG(32, 32, 30, 50, 11, 1, 4)", "XG(32, 32, 30, 50, 11, 1, 4)")
    assert B.pursuit_to_group_f16_lines(16, 16, 20, 50, 5, 1, live=True) == ("HLG(16, 16, 20, 50, 5, 1, 2)", "XG(16, 16, 20, 50, 5, 1, 2)")
    assert B.pursuit_to_group_f16_lines(32, 32, 16, 60, 7, 1) == ("HG(32, 32, 16, 60, 7, 1, 2)", "XG(32, 32, 16, 60, 7, 1, 2)")
    line, why = B.pursuit_to_group_f16_lines(16, 16, 8, 30, 7, 1)          # one wavefront per env
    assert line is None and "--pursuit-to-shape" in why
    line, why = B.pursuit_to_group_f16_lines(24, 24, 20, 300, 9, 1)        # the crowd kernel
    assert line is None and "crowd kernel" in why and "no half form" in why
    line, why = B.pursuit_to_group_f16_lines(16, 16, 8, 30, 6, 1)          # no fast path at all
    assert line is None and "even obs_range" in why
    line, why = B.pursuit_to_group_f16_lines(32, 32, 30, 50, 11, 1, include_id=False)
    assert line is None and "flatten without the id" in why
    # the float32 tools are as they were
    assert B.pursuit_to_group_lines(32, 32, 30, 50, 11, 1, live=True) == ("XLG(32, 32, 30, 50, 11, 1, 4)", "XG(32, 32, 30, 50, 11, 1, 4)")
    assert B.pursuit_to_lines(16, 16, 8, 30, 7, 1) == ("X(16, 16, 8, 30, 7, 1)", "X(16, 16, 8, 30, 7, 1)")


@pytest.mark.parametrize("shape,reason", [((16, 16, 8, 30, 7, 1), "--pursuit-to-shape"), ((24, 24, 20, 300, 9, 1), "no half form"),
                                          ((16, 16, 8, 30, 6, 1), "even obs_range"), ((16, 16, 8, 30, 6, 1, 1), "even obs_range")])
def test_build_refuses_a_shape_without_a_half_group_kernel(shape, reason):
    """python -m madrl_amd.build --pursuit-to-group-f16-shape: a one-wavefront shape, a crowd shape and a shape without a fast path are
    refused with the reason, before anything is written or compiled"""
    local = [os.path.join(CSRC, n) for n in (DEF.replace(".def", ".local.def"), "pursuit_to_specializations.local.def",
                                             "pursuit_specializations.local.def", "pursuit_live_specializations.local.def")]
    had = [os.path.exists(f) and open(f).read() for f in local]
    r = subprocess.run([sys.executable, "-m", "madrl_amd.build", "--pursuit-to-group-f16-shape"] + [str(v) for v in shape], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode != 0
    assert "no half-precision multi-wavefront kernel" in r.stdout and reason in r.stdout
    assert [os.path.exists(f) and open(f).read() for f in local] == had
