"""CPU test (-m "not gpu"): the half-precision two-buffer step of the multi-wavefront family (pursuit_group_kernel over a THGShape /
TLHGShape, the HG / HLG lines of pursuit_to_f16_group_specializations.def) -- the list, the kernels of the built library, the emitted code
of the instantiations compiled for gfx950 with the build's own flags beside their in-place counterparts, and the build tool's lines and
refusals."""
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

import test_kernel_metadata as built          # noqa: E402  (_kernels)
import test_live_counts_group_isa as group_isa   # noqa: E402  (_body, _meta)

CSRC = os.path.join(ROOT, "madrl_amd", "csrc")
DEF = "pursuit_to_f16_group_specializations.def"
REQUIRED = {
    "HG": [(32, 32, 30, 50, 11, 1, 4), (32, 32, 30, 30, 11, 1, 4), (10, 10, 36, 12, 11, 1, 4), (12, 12, 46, 10, 13, 1, 4),
           (12, 12, 64, 20, 13, 1, 4), (16, 16, 64, 40, 3, 1, 2)],
    "HLG": [(32, 32, 30, 50, 11, 1, 4), (32, 32, 30, 30, 11, 1, 4), (16, 16, 20, 50, 5, 1, 2)],
}
SHAPE = {"HG": "THGShape", "HLG": "TLHGShape"}       # the kernel's shape type of a line
IN_PLACE = {"THGShape": "GShape", "TLHGShape": "LGShape"}
FLOAT32 = {"THGShape": "TGShape", "TLHGShape": "TLGShape"}


def _lines(name):
    out = {}
    for m in re.finditer(r"^\s*([XH][A-Z]*)\(([^)]*)\)", open(os.path.join(CSRC, name)).read(), re.M):
        out.setdefault(m.group(1), []).append(tuple(int(v) for v in m.group(2).split(",")))
    return out


def _mangled(kind, cap):
    return "_ZN5madrl2pw20pursuit_group_kernelINS0_%d%sI%sEELi1ELb1EEEvNS0_7WaveDevENS0_6WaveIOE" % (
        len(kind), kind, "".join("Li%dE" % v for v in cap))


KERNELS = [(SHAPE[kind], cap) for kind in ("HG", "HLG") for cap in REQUIRED[kind]]
_id = lambda v: v if isinstance(v, str) else "%dv%d" % (v[2], v[3])


# ------------------------------------------------------------------ the list
def test_committed_half_lines_stand_on_their_fast_lines():
    half = _lines(DEF)
    assert set(half) == {"HG", "HLG"}, sorted(half)
    for kind, shapes in REQUIRED.items():
        for s in shapes:
            assert s in half[kind], (kind, s)
    fixed = _lines("pursuit_specializations.def").get("XG", [])
    live = _lines("pursuit_live_specializations.def").get("XLG", [])
    for s in half["HG"] + half["HLG"]:
        assert s in fixed, s          # (the same NW: the tuple holds it)
    for s in half["HLG"]:
        assert s in live, s
    # BASELINE configs[4] is not listed: tests/test_step_to_f16_gpu.py (XG_runs_generic) pins its half step to the generic kernel;
    # listing it goes together with that test
    assert not any(s[:6] == (32, 32, 16, 60, 7, 1) for s in half["HG"] + half["HLG"])
    # the two-buffer list keeps its six kinds: the half lines have a file of their own
    assert not any(k.startswith("H") for k in _lines("pursuit_to_specializations.def"))


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
    return built._kernels()


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
def _compile():
    from madrl_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    tu = '#include "common.hpp"\n#include "pursuit_group.hpp"\nnamespace madrl { namespace pw {\n'
    for kind, cap in KERNELS:
        for k in (kind, IN_PLACE[kind]):
            tu += "template __global__ void pursuit_group_kernel<%s<%d, %d, %d, %d, %d, %d, %d>, 1, true>(const WaveDev, const WaveIO);\n" % ((k,) + cap)
    tu += "} }\n"
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "group_to_f16.hip"), os.path.join(tmp, "group_to_f16.s")
        with open(src, "w") as f:
            f.write(tu)
        subprocess.run([B.HIPCC] + [f for f in B.FLAGS if f != "-Wall"] + ["-I", CSRC, "--cuda-device-only", "-S", src, "-o", out],
                       check=True, capture_output=True)
        import find_masked_spills
        masked = find_masked_spills.scan(out, "THGShape") + find_masked_spills.scan(out, "TLHGShape")
        text = open(out).read()
    return text, masked


@pytest.fixture(scope="module")
def asm():
    return _compile()


@pytest.mark.parametrize("kind,cap", KERNELS, ids=_id)
def test_half_group_kernel_no_scratch(asm, kind, cap):
    meta = group_isa._meta(asm[0], _mangled(kind, cap))
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta
    assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), meta


def test_half_group_kernels_have_no_masked_spills(asm):
    assert asm[1] == []


@pytest.mark.parametrize("kind,cap", KERNELS, ids=_id)
def test_half_group_kernel_adds_no_barrier_and_moves_whole_8_byte_slots(asm, kind, cap):
    to = group_isa._body(asm[0], _mangled(kind, cap))
    ip = group_isa._body(asm[0], _mangled(IN_PLACE[kind], cap))
    barriers = lambda body: sum(1 for l in body if l.strip().startswith("s_barrier"))
    assert barriers(to) == barriers(ip) and barriers(ip) > 0, (barriers(to), barriers(ip))
    inst = [l.strip().split(";")[0].strip() for l in to]
    # a slot is 8 bytes: it is loaded and stored as one word, the two-buffer pass's stores non-temporal; nothing float4-sized is left
    assert any(re.match(r"global_load_dwordx2\s", i) for i in inst)
    assert any(re.match(r"global_store_dwordx2\s", i) and i.endswith(" nt") for i in inst)
    assert any(re.match(r"global_store_dwordx4\s", i) and i.endswith(" nt") for i in (l.strip().split(";")[0].strip() for l in ip))
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
