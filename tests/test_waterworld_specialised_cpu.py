"""CPU tests (-m "not gpu") around the specialised Waterworld kernels and their list, csrc/waterworld_specializations.def:
  * build.waterworld_wave_lds_bytes restates the kernels' static LDS, and the built code objects agree with it, line by line;
  * every line has its six kernels (reset and step: float32, float32 with the fused StandardizedEnv, half), none with scratch or VGPR spills;
  * `python -m madrl_amd.build --waterworld-shape` refuses a shape that cannot be built or would never run before it writes anything, and a
    hand-edited list fails to compile with a line that names the option;
  * the host's dispatch key, restated, finds exactly one line for each test configuration of tests/test_waterworld_specialised_gpu.py;
  * madrl_waterworld_last_launch_kernel is declared, bound and exported (ABI 8)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import isa
from waterworld_parity import SPEC_SHAPES

LIST = "waterworld_specializations.def"
TEST_LINES = [(3, 9, 4, 12, 50), (2, 3, 2, 64, 450), (3, 3, 3, 1, 10), (2, 2, 2, 256, 1795), (8, 30, 16, 8, 59), (10, 30, 16, 6, 45),
              (2, 40, 3, 8, 59), (32, 16, 14, 4, 31), (1, 1, 1, 30, 213)]
F32_NAME = "waterworld_kernelILi%dELi%dELi%dELi%dELi%dELb%dELi%dEEE"       # <MODE, TNp, TNe, TNpo, TK, FUSED, TD>
F16_NAME = "waterworld_kernel_f16ILi%dELi%dELi%dELi%dELi%dELb0ELi%dEEE"    # <MODE, TNp, TNe, TNpo, TK, FUSED = false, TD>


def _lines():
    return isa.def_lines(LIST, ("X",))["X"]


def _six_kernels(line):
    """the six kernels of a line in the built library: name fragment -> notes"""
    ks = isa.built_kernels()
    frags = [F32_NAME % ((mode,) + line[:4] + (fused, line[4])) for mode in (0, 1) for fused in (0, 1)]
    frags += [F16_NAME % ((mode,) + line) for mode in (0, 1)]
    out = {}
    for frag in frags:
        hit = [n for n in ks if frag in n]
        assert len(hit) == 1, (line, frag, hit)
        out[frag] = ks[hit[0]]
    return out


def test_the_list_holds_the_test_lines_once_each():
    lines = _lines()
    assert len(lines) == len(set(lines)), "a line is listed twice"
    assert lines[:4] == [(5, 10, 10, 30, 213), (8, 10, 10, 30, 213), (3, 10, 5, 30, 213), (3, 5, 10, 30, 213)]
    assert lines[4:] == TEST_LINES == [SPEC_SHAPES[n][0] for n in SPEC_SHAPES]
    assert (4, 7, 10, 30, 213) not in lines       # tests/test_edge_cases_gpu.py runs it as a shape without a line


def test_lds_formula_is_the_static_lds_of_every_listed_kernel():
    from madrl_amd import build as B
    assert B.waterworld_wave_lds_bytes(5, 10, 10, 30, 213) == 5952
    assert B.waterworld_wave_lds_bytes(2, 2, 2, 256, 1795) == 23744
    assert B.waterworld_wave_lds_bytes(32, 15, 15, 256, 1795) == 241264
    for line in _lines():
        want = B.waterworld_wave_lds_bytes(*line)
        for frag, k in _six_kernels(line).items():
            assert k["lds"] == want, (line, frag, k["lds"], want)


def test_every_line_has_its_six_kernels_without_scratch_or_vgpr_spills():
    """a specialised kernel's registers are allocated for its occupancy, and a spill store reaches HBM"""
    for line in _lines():
        for frag, k in _six_kernels(line).items():
            assert k["scratch"] == 0 and k["vgpr_spills"] == 0, (line, frag, k)
            assert len(k["args"]) == 2, (line, frag, k["args"])


@pytest.fixture
def scratch_lists(tmp_path, monkeypatch):
    """build.py pointed at a copy of the list that holds the four lines of the shapes people run, so that nothing is written to the tree"""
    from madrl_amd import build as B
    text = open(os.path.join(B.CSRC, LIST)).read()
    (tmp_path / LIST).write_text(text[:text.index("// Test shapes")])
    monkeypatch.setattr(B, "CSRC", str(tmp_path))
    return tmp_path


def test_add_waterworld_shape_refuses_what_cannot_be_built_before_it_writes(scratch_lists):
    from madrl_amd import build as B
    local = scratch_lists / LIST.replace(".def", ".local.def")
    for bad, why in (((32, 15, 15, 256), "LDS"), ((32, 15, 15, 256, 1795), "LDS"), ((12, 25, 25, 256), "LDS"), ((12, 25, 25, 256, 1795), "LDS"),
                     ((5, 10, 10, 30, 214), "OBS_DIM"), ((5, 10, 10, 30, 211), "OBS_DIM"), ((5, 10, 10, 30, 0), "OBS_DIM"), ((3, 9, 4, 12, 52), "OBS_DIM"), ((3, 9, 4, 12, 7 * 12), "OBS_DIM"),
                     ((33, 10, 10, 30), "refuses"), ((13, 25, 25, 30), "refuses"), ((5, 10, 10, 257), "refuses"), ((5, 10, 10, 0), "refuses"),
                     ((5, 0, 10, 30), "refuses")):
        with pytest.raises(ValueError, match=why):
            B.add_waterworld_shape(*bad)
        assert not local.exists(), bad
    # the bound is the handle's 64 KiB: 62 particles at the sensor limit fit with seven pursuers and not with eight
    assert B.waterworld_wave_lds_bytes(7, 27, 28, 256, 1795) <= 64 * 1024 < B.waterworld_wave_lds_bytes(8, 27, 27, 256, 1795)
    assert B.waterworld_shape_refusal(7, 27, 28, 256, 1795) is None
    with pytest.raises(ValueError, match="LDS"):
        B.add_waterworld_shape(8, 27, 27, 256)
    assert not local.exists()
    for line in TEST_LINES:
        assert B.waterworld_shape_refusal(*line) is None, line
        assert B.add_waterworld_shape(*line) is True, line
        assert B.add_waterworld_shape(*line) is False, line      # listed now
    assert B.add_waterworld_shape(5, 10, 10, 30) is False          # the committed list has it (OBS_DIM defaults to 7 K + 3)
    assert isa.def_lines(os.path.join(str(scratch_lists), local.name), ("X",))["X"] == TEST_LINES
    for width in (4 * 12 + 2, 4 * 12 + 3, 7 * 12 + 2, 7 * 12 + 3):
        assert B.waterworld_shape_refusal(4, 4, 4, 12, width) is None


def test_a_hand_edited_line_beyond_the_lds_fails_with_a_line_that_names_the_option():
    """the static_assert of waterworld_wave_body.inc, reached through an entry like waterworld_kernel's: host and device pass both see it,
    the device pass alone is compiled here"""
    tu = """#include "waterworld_wave.hpp"
namespace {
using namespace madrl;
template <int MODE, int TNp, int TNe, int TNpo, int TK, bool FUSED = false, int TD = 0>
__global__ __launch_bounds__(64) void probe_kernel(const WwDev d, const WwIO io) {
#define MADRL_WW_BODY_LIVE 0
#define MADRL_WW_BODY_RANGES 0
#define MADRL_WW_BODY_HALF 0
#include "waterworld_wave_body.inc"
}
template __global__ void probe_kernel<1, %d, %d, %d, %d, false, %d>(const WwDev, const WwIO);
}
"""
    with pytest.raises(subprocess.CalledProcessError) as e:
        isa.compile_asm(tu % (12, 25, 25, 256, 1795), ("-fsyntax-only",))
    err = e.value.stderr.decode()
    assert "static assertion failed" in err and "--waterworld-shape" in err and "64 KiB" in err, err[-2000:]


def test_the_dispatch_key_finds_one_line_per_test_configuration():
    """ww_launch compares (Np, Ne, Npo, K, ww_obs_dim_of(cfg)) with every line: restated in build.waterworld_line_of"""
    from madrl_amd import build as B
    src = open(os.path.join(isa.CSRC, "waterworld.hip")).read()
    assert "d.Np == w.Np && d.Ne == w.Ne && d.Npo == w.Npo && d.K == w.K && d.D == w.D" in src
    assert "c->n_sensors * (c->speed_features ? 7 : 4) + 2 + (c->addid ? 1 : 0)" in src
    for name, (line, kw) in SPEC_SHAPES.items():
        key = {k: kw[k] for k in ("n_pursuers", "n_evaders", "n_poison", "n_sensors", "speed_features", "addid") if k in kw}
        assert B.waterworld_line_of(**key) == [line], name
        assert B.waterworld_is_specialised(*line)
    assert B.waterworld_line_of(5, 10) == [(5, 10, 10, 30, 213)]
    assert B.waterworld_line_of(4, 7) == [] and B.waterworld_line_of(3, 9, 4, 12) == [] and B.waterworld_line_of(3, 10, 5, 12, False, False) == []


def test_last_launch_kernel_is_declared_bound_and_exported():
    from madrl_amd import _lib
    from madrl_amd.waterworld import BatchedMAWaterWorld
    header = open(os.path.join(isa.ROOT, "include", "madrl_hip.h")).read()
    m = re.search(r"\bint\s+madrl_waterworld_last_launch_kernel\s*\(([^;]*)\)\s*;", header)
    assert m and len(m.group(1).split(",")) == 2 == len(_lib.SIGNATURES["madrl_waterworld_last_launch_kernel"][1])
    values = dict(re.findall(r"#define MADRL_WW_LAUNCH_(\w+) (\d+)", header))
    assert [values[n.upper()] for n in BatchedMAWaterWorld._LAUNCH_KERNELS] == [str(i) for i in range(6)]
    assert re.search(r"#define MADRL_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    L = _lib.lib()
    assert L.madrl_abi_version() == 8
    out = C.c_int32(-1)
    assert L.madrl_waterworld_last_launch_kernel(None, C.byref(out)) != 0 and out.value == -1     # a NULL handle is refused, host only
    assert b"last_launch_kernel" in L.madrl_last_error()
