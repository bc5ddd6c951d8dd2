"""CPU tests (-m "not gpu") of per-env agent counts on the PursuitEvade crowd kernel (pursuit_live_crowd_kernel over an LCShape, the XLC
lines of pursuit_live_specializations.def):
  * the lists are consistent -- every XLC line is an XC line, NW included -- and the build tool forms, refuses and appends the right lines;
  * the BUILT library holds one live kernel per XLC line and mode, without a private segment, inside the register budget of its workgroup
    and with exactly the LDS of the fixed-shape kernel;
  * the emitted live step and reset kernels have as many non-temporal float4 stores and as many s_barrier instructions as the fixed-shape
    kernels of the same line: counting the live slots and reading the pending counts fit behind the barriers that were there."""
import os
import re
import subprocess

import pytest

import isa
from isa import CSRC
from madrl_amd.build import pursuit_live_crowd_lines, add_pursuit_live_crowd_shape

CAPS = [(128, 128, 100, 300, 21, 0, 16), (48, 48, 100, 300, 21, 0, 8), (24, 24, 20, 300, 9, 1, 1), (20, 20, 260, 40, 5, 1, 2)]


def test_def_lists_are_consistent():
    from madrl_amd import build as B
    live = isa.def_lines("pursuit_live_specializations.def", ("XL", "XLG", "XLC"))
    crowd = isa.def_lines("pursuit_crowd_specializations.def", ("XC",))["XC"]
    assert set(live["XLC"]) == set(CAPS)
    for line in live["XLC"]:
        assert line in crowd, line   # same shape, same NW
        assert B.pursuit_fast_path(*line[:6])[0] is None, line   # no X / XG path: that shape keeps its kernel and its XL / XLG line
        assert B.pursuit_crowd_path(*line[:6]) == ("XC", line[6]), line
    # tests/test_pursuit_crowd_gpu.py pins per-env counts at this capacity to the generic kernel
    assert not any(line[:6] == (24, 24, 70, 90, 9, 1) for line in live["XLC"])
    # every translation unit that includes the live list defines all three macros
    for src in ("pursuit.hip", "pursuit_live_group.hip", "pursuit_live_crowd.hip"):
        text = open(os.path.join(CSRC, src)).read()
        assert "pursuit_live_specializations.local.def" in text, src
        for macro in ("XL(", "XLG(", "XLC("):
            assert "#define " + macro in text, (src, macro)


def test_build_tool_forms_refuses_and_appends_the_live_crowd_lines(tmp_path, monkeypatch):
    from madrl_amd import build as B
    assert pursuit_live_crowd_lines(128, 128, 100, 300, 21, 0) == ("XLC(128, 128, 100, 300, 21, 0, 16)", "XC(128, 128, 100, 300, 21, 0, 16)")
    assert pursuit_live_crowd_lines(24, 24, 20, 300, 9, 1) == ("XLC(24, 24, 20, 300, 9, 1, 1)", "XC(24, 24, 20, 300, 9, 1, 1)")
    for cap in CAPS:
        assert pursuit_live_crowd_lines(*cap[:6]) == ("XLC(%s)" % ", ".join(map(str, cap)), "XC(%s)" % ", ".join(map(str, cap)))
    # what pursuit_crowd_path refuses, the live form refuses too -- and add_pursuit_live_crowd_shape raises with the same reason
    for bad, kw, why in (((128, 128, 100, 300, 20, 0), {}, "even obs_range"),
                         ((24, 24, 20, 300, 9, 1), dict(include_id=False), "flatten without the id")):
        assert pursuit_live_crowd_lines(*bad, **kw) is None
        assert why in B.pursuit_crowd_path(*bad, **kw)[1]
    with pytest.raises(ValueError, match="even obs_range"):
        add_pursuit_live_crowd_shape(128, 128, 100, 300, 20, 0)
    # a capacity with an X / XG path keeps it (pursuit_live_lines forms its lines)
    assert pursuit_live_crowd_lines(16, 16, 8, 30, 7, 1) is None and B.pursuit_live_lines(16, 16, 8, 30, 7, 1) is not None
    assert pursuit_live_crowd_lines(32, 32, 30, 50, 11, 1) is None
    with pytest.raises(ValueError, match="--pursuit-live-shape"):
        add_pursuit_live_crowd_shape(16, 16, 8, 30, 7, 1)
    # the one-wavefront / group tool keeps refusing crowd capacities
    assert B.pursuit_live_lines(128, 128, 100, 300, 21, 0) is None
    # appending: both lines of a new capacity land in the local files once, a committed capacity adds nothing
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    for name in ("pursuit_crowd_specializations.def", "pursuit_live_specializations.def"):
        (csrc / name).write_text(open(os.path.join(CSRC, name)).read())
    monkeypatch.setattr(B, "CSRC", str(csrc))
    assert add_pursuit_live_crowd_shape(64, 64, 80, 200, 11, 1) is True and add_pursuit_live_crowd_shape(64, 64, 80, 200, 11, 1) is False
    assert add_pursuit_live_crowd_shape(128, 128, 100, 300, 21, 0) is False
    assert (csrc / "pursuit_live_specializations.local.def").read_text().startswith("XLC(64, 64, 80, 200, 11, 1, 2)")
    assert (csrc / "pursuit_crowd_specializations.local.def").read_text().startswith("XC(64, 64, 80, 200, 11, 1, 2)")
    assert len((csrc / "pursuit_live_specializations.local.def").read_text().splitlines()) == 1
    assert len((csrc / "pursuit_crowd_specializations.local.def").read_text().splitlines()) == 1
    # the XC line exists already (the pinned 70 v 90 shape): only the XLC line is appended
    assert add_pursuit_live_crowd_shape(24, 24, 70, 90, 9, 1) is True
    assert len((csrc / "pursuit_crowd_specializations.local.def").read_text().splitlines()) == 1
    assert (csrc / "pursuit_live_specializations.local.def").read_text().splitlines()[1].startswith("XLC(24, 24, 70, 90, 9, 1, 2)")


def test_live_hint_names_the_crowd_line():
    """the per-env-counts hint of a batch on the generic kernel names the XLC line and the build command for a capacity above 64 of a kind"""
    import types
    import warnings
    from madrl_amd.pursuit import BatchedPursuitEvade
    fake = types.SimpleNamespace(xs=64, ys=64, n_pursuers=80, n_evaders=200, obs_range=11, flatten=True, include_id=True, train_pursuit=True,
                                 per_env_counts=True, kernel_kind="generic")
    BatchedPursuitEvade._hinted.discard((64, 64, 80, 200, 11, 1))
    with warnings.catch_warnings(record=True) as got:
        warnings.simplefilter("always")
        BatchedPursuitEvade._hint_fast_path(fake)
        BatchedPursuitEvade._hint_fast_path(fake)   # once per shape
    assert len(got) == 1
    msg = str(got[0].message)
    assert "XLC(64,64,80,200,11,1,2)" in msg and "--pursuit-live-crowd-shape 64 64 80 200 11 1" in msg, msg


def test_built_live_crowd_kernels():
    from madrl_amd import build as B
    built = isa.built_kernels()
    ks = {n: k for n, k in built.items() if "pursuit_live_crowd_kernel" in n}
    assert len(ks) >= 2 * len(CAPS)
    for cap in CAPS:
        for mode in (0, 1):   # reset launch, step launch
            name = isa.crowd_kernel(cap, mode, live=True)
            assert name in ks, name
            k = ks[name]
            assert k["scratch"] == 0 and k["vgpr_spills"] == 0, (name, k)
            assert k["vgprs"] <= 512 // max(64 * cap[6] // 256, 1), (name, k)
            assert k["lds"] == B.pursuit_crowd_lds_bytes(*cap[:6]) == built[isa.crowd_kernel(cap, mode)]["lds"], (name, k["lds"])   # the live form adds no LDS
            (o0, s0), (o1, _s1) = k["args"][:2]   # CrowdDev and CrowdIO by value where the fixed kernel has them; the pending counts behind
            assert o0 == 0 and o1 == (s0 + 7) // 8 * 8, (name, k["args"])


TU = '#include "common.hpp"\n#include "pursuit_crowd.hpp"\nnamespace madrl { namespace pc {\n'
for _cap in CAPS:
    for _mode in (0, 1):
        TU += "template __global__ void pursuit_crowd_kernel<CShape<%d, %d, %d, %d, %d, %d, %d>, %d>(const CrowdDev, const CrowdIO);\n" % (_cap + (_mode,))
        TU += ("template __global__ void pursuit_live_crowd_kernel<LCShape<%d, %d, %d, %d, %d, %d, %d>, %d>(const CrowdDev, const CrowdIO, "
               "const int32_t *);\n" % (_cap + (_mode,)))
TU += "} }\n"


@pytest.fixture(scope="module")
def asm():
    return isa.compile_asm(TU)


@pytest.mark.parametrize("mode", [0, 1], ids=["reset", "step"])
@pytest.mark.parametrize("cap", CAPS, ids=lambda c: "%dx%d_%dv%d" % c[:4])
def test_live_crowd_kernel_keeps_the_fixed_kernels_stores_and_barriers(asm, cap, mode):
    live, fix = isa.kernel_insts(asm, isa.crowd_kernel(cap, mode, live=True)), isa.kernel_insts(asm, isa.crowd_kernel(cap, mode))
    nt4 = lambda k: sum(1 for i in k if i.startswith("global_store_dwordx4") and re.search(r"\bnt\b", i))
    bar = lambda k: sum(1 for i in k if i.startswith("s_barrier"))
    print(cap, mode, "non-temporal float4 stores", nt4(live), nt4(fix), "barriers", bar(live), bar(fix))
    assert nt4(fix) > 0 and nt4(live) == nt4(fix), (nt4(live), nt4(fix))
    assert bar(fix) > 0 and bar(live) == bar(fix), (bar(live), bar(fix))
    # the live slots are counted with one LDS minimum where the record is loaded; the pending counts are scalar loads, nothing is spilled
    assert sum(1 for i in live if i.startswith("ds_min_u32")) == 1
    assert not any(i.startswith("scratch_") for i in live)


def test_run_time_pairwise_sum_is_numpys_for_every_count(tmp_path):
    """np_sum_n (the global reward's mean over a run-time pursuer count) is the kernel's own text, np_base included, compiled for the host:
    equal to numpy's float64 add.reduce for every count a capacity can hold, 1 .. 1 023, and 1 024.  The GPU tests reach it at four counts."""
    import ctypes as C
    import shutil
    import numpy as np
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    text = open(os.path.join(CSRC, "pursuit_crowd.hpp")).read()
    funcs = [re.search(r"^__device__ __forceinline__ double %s\(.*?^}\n" % name, text, re.M | re.S).group(0) for name in ("np_base", "np_sum_n")]
    src = tmp_path / "np_sum_n.cpp"
    src.write_text("#include <cstdint>\n#define __device__\n#define __forceinline__ static inline\n" + "".join(funcs) +
                   'extern "C" double crowd_np_sum_n(const double *a, int n) { return np_sum_n(a, n); }\n')
    so = tmp_path / "np_sum_n.so"
    # (no contraction, no reassociation: the order of the additions is what is under test)
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True, capture_output=True)
    L = C.CDLL(str(so))
    L.crowd_np_sum_n.restype = C.c_double
    L.crowd_np_sum_n.argtypes = [C.c_void_p, C.c_int]
    rng = np.random.RandomState(3)
    for n in range(1, 1025):
        a = np.ascontiguousarray(rng.uniform(-5, 5, n) * 10.0 ** rng.randint(-6, 6, n))
        assert L.crowd_np_sum_n(a.ctypes.data_as(C.c_void_p), n) == float(np.add.reduce(a)), n
