"""CPU tests (-m "not gpu") of the StandardizedEnv epilogue fused into the hostage-world kernels: the C ABI symbol, and the metadata of
the four gfx950 instantiations hostage_kernel<MODE, ..., FUSED = true> of the BUILT library (read as tests/test_pursuit_crowd_build.py
reads its kernels')."""
import os
import re

from isa import built_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hostage_kernel<MODE, TNr, TNh, TNc, TK, TD, FUSED> in the unnamed namespace of hostage.hip
NAME = "_ZN12_GLOBAL__N_114hostage_kernelILi%dELi%dELi%dELi%dELi%dELi%dELb%dEEEvNS_5HwDevENS_4HwIOE"
SPEC, GENERIC = (3, 10, 5, 30, 156), (0, 0, 0, 0, 0)
HIP = os.path.join(ROOT, "madrl_amd", "csrc", "hostage.hip")


def _define(name):
    """the default of an `#ifndef NAME / #define NAME <integer>` pair in hostage.hip: what the build uses"""
    m = re.search(r"^#define %s (\d+)\b" % name, open(HIP).read(), re.M)
    assert m, "hostage.hip defines no integer %s" % name
    return int(m.group(1))


def _fused_waves():
    """amdgpu_waves_per_eu the fused instantiations declare, read from hostage.hip: the specialised reset and step have a constant each;
    the generic ones declare 1..8 and the compiler chooses (the budget of one resident wavefront says nothing there: scratch and spills do)"""
    assert _define("MADRL_HW_WAVES") == 7
    step, reset = _define("MADRL_HW_FUSED_STEP_WAVES"), _define("MADRL_HW_FUSED_RESET_WAVES")
    assert 1 <= step <= 7 and 1 <= reset <= 7
    return {(0,) + SPEC: reset, (1,) + SPEC: step, (0,) + GENERIC: 1, (1,) + GENERIC: 1}


def _vgpr_budget(waves):
    """VGPRs a wavefront may hold for `waves` of them to be resident on a SIMD: 512 per lane, allocated in blocks of 8 (gfx90a and later)"""
    return 512 // waves // 8 * 8


def test_header_declares_and_library_exports_the_symbol():
    from madrl_amd import _lib
    header = open(os.path.join(ROOT, "include", "madrl_hip.h")).read()
    assert re.search(r"int\s+madrl_hostage_set_standardize\s*\(\s*madrl_hostage\s*\*\s*\w+\s*,\s*const\s+madrl_standardize_args\s*\*\s*\w+\s*\)\s*;", header)
    assert len(_lib.SIGNATURES["madrl_hostage_set_standardize"][1]) == 2
    assert hasattr(_lib.lib(), "madrl_hostage_set_standardize")
    assert _lib.lib().madrl_abi_version() == _lib.ABI_VERSION == 8   # (the symbol was added at 7; 8: madrl_waterworld_last_launch_kernel)


def test_fused_instantiations_exist_and_fit_their_occupancy():
    ks = built_kernels()
    hostage = [n for n in ks if "hostage_kernelILi" in n]
    assert len(hostage) == 8, sorted(hostage)   # reset and step x specialised and generic x plain and fused
    for (mode, *shape), waves in _fused_waves().items():
        fused, plain = NAME % ((mode,) + tuple(shape) + (1,)), NAME % ((mode,) + tuple(shape) + (0,))
        assert fused in ks and plain in ks, (fused, plain)
        k = ks[fused]
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0, (fused, k)   # a spill store would reach HBM
        assert k["vgprs"] <= _vgpr_budget(waves), (fused, k, waves)
        assert k["args"] == ks[plain]["args"], (fused, k["args"])        # the same two by-value arguments: HwDev, HwIO
    # the plain specialised kernels keep the occupancy they were tuned to (7 wavefronts per SIMD)
    for mode in (0, 1):
        k = ks[NAME % ((mode,) + SPEC + (0,))]
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["vgprs"] <= _vgpr_budget(7), (mode, k)
