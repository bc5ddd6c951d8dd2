"""CPU tests (-m "not gpu") of per-env particle counts on the hostage-world crowd kernel (madrl_hostage_set_particle_counts,
csrc/hostage_crowd.hip): the built library holds the live-count kernels for reset and step, none with a private segment, beside the
fixed-shape ones; the C function is declared in the header, exported and known to the ctypes layer."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_built_library_has_the_live_count_kernels_without_a_private_segment():
    from isa import built_kernels
    ks = built_kernels()
    live = {n: k for n, k in ks.items() if "hw_crowd_kernel_live" in n}
    assert len(live) >= 2 and any("ILi0E" in n for n in live) and any("ILi1E" in n for n in live), sorted(live)   # reset and step
    for n, k in live.items():
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0, (n, k)
        assert len(k["args"]) == 3 and k["args"][2][1] == 16, (n, k["args"])   # (HwDev, HwIO, the two count arrays)
    fixed = {n: k for n, k in ks.items() if "hw_crowd_kernel" in n and n not in live}
    assert len(fixed) >= 2 and all(len(k["args"]) == 2 for k in fixed.values()), sorted(fixed)   # the fixed-shape entries keep their arguments


def test_set_particle_counts_is_declared_and_exported():
    from madrl_amd import _lib
    header = open(os.path.join(ROOT, "include", "madrl_hip.h")).read()
    assert re.search(r"int madrl_hostage_set_particle_counts\(madrl_hostage \*h, const int32_t \*pending_dev, int32_t \*live_dev\);", header)
    assert "madrl_hostage_set_particle_counts" in _lib.SIGNATURES
    fn = _lib.lib().madrl_hostage_set_particle_counts
    assert len(fn.argtypes) == 3
    assert fn(None, None, None) == -1 and b"NULL" in _lib.lib().madrl_last_error()   # no handle: refused before anything is touched


def test_the_count_code_of_the_two_particle_worlds_is_one():
    """set_particle_counts keeps each world's keyword names; everything else about the counts is BatchedParticleWorld's"""
    import inspect
    from madrl_amd.hostage import BatchedContinuousHostageWorld as H
    from madrl_amd.particle import BatchedParticleWorld as P
    from madrl_amd.waterworld import BatchedMAWaterWorld as W
    for name in ("_require_counts", "_checked_counts", "_set_pending", "particle_counts", "live_agents", "_slot_exists", "setup", "get_state"):
        assert getattr(H, name) is getattr(P, name) and getattr(W, name) is getattr(P, name), name
    assert list(inspect.signature(H.set_particle_counts).parameters)[1:] == ["n_good", "n_hostages", "n_bad", "mask"]
    assert list(inspect.signature(W.set_particle_counts).parameters)[1:] == ["n_pursuers", "n_evaders", "n_poison", "mask"]
    assert inspect.signature(H.__init__).parameters["per_env_counts"].default is False
