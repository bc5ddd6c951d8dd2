"""CPU tests (-m "not gpu") of per-env particle counts on the one-wavefront Waterworld kernel (`per_env_counts="wave"`:
waterworld_kernel_live, csrc/waterworld.hip): the built library holds the live entry for reset and step, with the count arrays as a third
argument and without a private segment, beside the fixed-shape instantiations, which keep their two arguments; the constructor takes the
one-wavefront form by value and refuses every other combination before it touches a device."""
import inspect

import pytest


def test_built_library_has_the_one_wavefront_live_kernels():
    from isa import built_kernels
    ks = built_kernels()
    live = {n: k for n, k in ks.items() if "waterworld_kernel_live" in n}
    assert len(live) == 2 and any("liveILi0E" in n for n in live) and any("liveILi1E" in n for n in live), sorted(live)   # reset and step
    for n, k in live.items():
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0, (n, k)
        assert len(k["args"]) == 3 and k["args"][2][1] == 16, (n, k["args"])   # (WwDev, WwIO, the two count arrays)
        (o0, s0), (o1, s1), (o2, _s2) = k["args"]
        assert o1 == (s0 + 7) // 8 * 8 and o2 == (o1 + s1 + 7) // 8 * 8, (n, k["args"])   # struct {Dev d; IO io; ParticleCounts cn;}
    fixed = {n: k for n, k in ks.items() if "waterworld_kernelILi" in n}
    assert len(fixed) >= 20 and not set(fixed) & set(live), sorted(fixed)
    assert all(len(k["args"]) == 2 for k in fixed.values()), sorted(fixed)   # the fixed-shape entries keep their arguments


def test_constructor_values_are_checked_before_a_device_is_touched():
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    from madrl_amd.waterworld import BatchedMAWaterWorld, MAWaterWorld
    nodev = "cuda:99"   # never reached: the flags are checked first
    with pytest.raises(ValueError, match="crowd=True"):       # True keeps meaning the crowd kernel's form
        BatchedMAWaterWorld(3, 4, n_envs=2, device=nodev, per_env_counts=True)
    with pytest.raises(ValueError, match="without crowd=True"):
        BatchedMAWaterWorld(3, 4, n_envs=2, device=nodev, crowd=True, per_env_counts="wave")
    for other in ("crowd", "Wave", 2, 0.5):
        with pytest.raises(ValueError, match="per_env_counts must be"):
            BatchedMAWaterWorld(3, 4, n_envs=2, device=nodev, per_env_counts=other)
    with pytest.raises(ValueError, match="no live counts"):
        BatchedContinuousHostageWorld(3, 4, 2, 2, 2, n_envs=2, device=nodev, per_env_counts="wave")
    with pytest.raises(ValueError, match="crowd=True"):
        BatchedContinuousHostageWorld(3, 4, 2, 2, 2, n_envs=2, device=nodev, per_env_counts=True)
    with pytest.raises(ValueError, match="without crowd=True"):   # the drop-in passes the flag through
        MAWaterWorld(3, 4, device=nodev, crowd=True, per_env_counts="wave")


def test_set_particle_counts_signatures_are_unchanged():
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    from madrl_amd.waterworld import BatchedMAWaterWorld
    assert list(inspect.signature(BatchedMAWaterWorld.set_particle_counts).parameters) == ["self", "n_pursuers", "n_evaders", "n_poison", "mask"]
    assert list(inspect.signature(BatchedContinuousHostageWorld.set_particle_counts).parameters) == ["self", "n_good", "n_hostages", "n_bad", "mask"]
    assert inspect.signature(BatchedMAWaterWorld.__init__).parameters["per_env_counts"].default is False
    fn = __import__("madrl_amd._lib", fromlist=["lib"]).lib().madrl_waterworld_set_particle_counts
    assert len(fn.argtypes) == 3
