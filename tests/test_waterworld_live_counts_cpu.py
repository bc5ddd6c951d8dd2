"""CPU tests (-m "not gpu") of per-env particle counts on the Waterworld crowd kernel (madrl_waterworld_set_particle_counts,
csrc/waterworld_crowd.hip): the built library holds the live-count kernels for reset and step, none with a private segment, beside the
fixed-shape ones; the C function is declared in the header, exported and known to the ctypes layer."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_built_library_has_the_live_count_kernels_without_a_private_segment():
    from isa import built_kernels
    ks = built_kernels()
    live = {n: k for n, k in ks.items() if "ww_crowd_kernel_live" in n}
    assert len(live) >= 2 and any("ILi0E" in n for n in live) and any("ILi1E" in n for n in live), sorted(live)   # reset and step
    for n, k in live.items():
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0, (n, k)
        assert len(k["args"]) == 3 and k["args"][2][1] == 16, (n, k["args"])   # (WwDev, WwIO, the two count arrays)
    fixed = {n: k for n, k in ks.items() if "ww_crowd_kernel" in n and n not in live}
    assert len(fixed) >= 2 and all(len(k["args"]) == 2 for k in fixed.values()), sorted(fixed)   # the fixed-shape entries keep their arguments


def test_set_particle_counts_is_declared_and_exported():
    from madrl_amd import _lib
    header = open(os.path.join(ROOT, "include", "madrl_hip.h")).read()
    assert re.search(r"int madrl_waterworld_set_particle_counts\(madrl_waterworld \*h, const int32_t \*pending_dev, int32_t \*live_dev\);", header)
    fn = _lib.lib().madrl_waterworld_set_particle_counts
    assert len(fn.argtypes) == 3
    assert fn(None, None, None) == -1 and b"NULL" in _lib.lib().madrl_last_error()   # no handle: refused before anything is touched
