"""CPU tests (-m "not gpu") of the half-precision observation rows of the particle worlds (BatchedMAWaterWorld / BatchedContinuousHostageWorld
with obs_dtype=torch.float16): the C ABI symbols, the gfx950 kernels of the BUILT library, and every refusal that is raised before a
device is touched (device="cuda:99" is never reached)."""
import inspect
import os
import pickle
import re

import pytest
import torch

import isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOWHERE = "cuda:99"
SYMBOLS = {"madrl_waterworld_reset_f16": 4, "madrl_waterworld_step_f16": 8, "madrl_hostage_reset_f16": 4, "madrl_hostage_step_f16": 8,
           "madrl_heuristic_waterworld_f16": 6}
F16, F32 = torch.float16, torch.float32


def _ww(**kw):
    from madrl_amd.waterworld import BatchedMAWaterWorld
    return BatchedMAWaterWorld(5, 10, n_envs=4, device=NOWHERE, **kw)


def _hw(**kw):
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    return BatchedContinuousHostageWorld(3, 10, 5, 2, 2, n_envs=4, device=NOWHERE, **kw)


@pytest.fixture
def no_device(monkeypatch):
    """constructors that stop before setup(): everything a constructor decides without a device can then be looked at"""
    from madrl_amd.particle import BatchedParticleWorld
    monkeypatch.setattr(BatchedParticleWorld, "setup", lambda self: None)


def test_header_signatures_and_library_hold_the_five_symbols():
    from madrl_amd import _lib
    header = open(os.path.join(ROOT, "include", "madrl_hip.h")).read()
    L = _lib.lib()
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name), name
    for name in ("madrl_waterworld_reset_f16", "madrl_waterworld_step_f16", "madrl_hostage_reset_f16", "madrl_hostage_step_f16"):
        assert "uint16_t *obs_dev" in re.search(r"\bint\s+%s\s*\(([^;]*)\)" % name, header).group(1), name
    assert "const uint16_t *obs" in re.search(r"\bint\s+madrl_heuristic_waterworld_f16\s*\(([^;]*)\)", header).group(1)
    assert L.madrl_abi_version() == _lib.ABI_VERSION == 8   # (the symbols were appended at 7; 8: madrl_waterworld_last_launch_kernel)


def _kernarg_view(k):
    (o0, s0), (o1, _s1) = k["args"]
    return o0 == 0 and o1 == (s0 + 7) // 8 * 8   # struct {Dev d; IO io;}: io follows d, 8-byte aligned


def test_built_library_holds_the_half_waterworld_kernels():
    from madrl_amd import build as B
    ks = {n: k for n, k in isa.built_kernels().items() if "waterworld_kernel_f16" in n}
    shapes = sorted(B.specialised_shapes("waterworld_specializations.def"))
    assert len(shapes) >= 4
    name = "waterworld_kernel_f16ILi%dELi%dELi%dELi%dELi%dELb0ELi%dEEE"   # <MODE, TNp, TNe, TNpo, TK, FUSED = false, TD>
    want = {name % (mode, 0, 0, 0, 0, 0): False for mode in (0, 1)}
    want.update({name % ((mode,) + s[:4] + (s[4],)): True for mode in (0, 1) for s in shapes})
    assert len(ks) == len(want), sorted(ks)
    for frag, spec in want.items():
        hit = [n for n in ks if frag in n]
        assert len(hit) == 1, (frag, sorted(ks))
        k = ks[hit[0]]
        assert len(k["args"]) == 2 and _kernarg_view(k), (hit[0], k["args"])
        if spec:
            assert k["scratch"] == 0 and k["vgpr_spills"] == 0, (hit[0], k)
    # none of them is taken for a float32 kernel by the tests that select those by name
    assert not any(t in n for n in ks for t in ("waterworld_kernelILi", "waterworld_kernel_live", "hostage_kernelILi"))


def test_built_library_holds_the_half_hostage_kernels():
    ks = {n: k for n, k in isa.built_kernels().items() if "hostage_kernel_f16" in n}
    name = "hostage_kernel_f16ILi%dELi%dELi%dELi%dELi%dELi%dELb0EEE"   # <MODE, TNr, TNh, TNc, TK, TD, FUSED = false>
    want = {name % (mode, 0, 0, 0, 0, 0): False for mode in (0, 1)}
    want.update({name % (mode, 3, 10, 5, 30, 156): True for mode in (0, 1)})
    assert len(ks) == 4, sorted(ks)
    for frag, spec in want.items():
        hit = [n for n in ks if frag in n]
        assert len(hit) == 1, (frag, sorted(ks))
        k = ks[hit[0]]
        assert len(k["args"]) == 2 and _kernarg_view(k), (hit[0], k["args"])
        if spec:
            assert k["scratch"] == 0 and k["vgpr_spills"] == 0, (hit[0], k)
    assert not any(t in n for n in ks for t in ("waterworld_kernelILi", "waterworld_kernel_live", "hostage_kernelILi"))


def test_specialised_half_kernels_keep_the_float32_kernels_register_budget():
    """the half entries declare the occupancy of their float32 counterparts: their VGPRs fit the same number of resident wavefronts"""
    ks = isa.built_kernels()
    waves = lambda k: min(8, 512 // max(8, (k["vgprs"] + 7) // 8 * 8))
    n = 0
    for name, k in ks.items():
        if ("waterworld_kernel_f16ILi" in name or "hostage_kernel_f16ILi" in name) and "ELi0ELi0ELi0ELi0E" not in name:
            twin = ks[name.replace("20waterworld_kernel_f16", "17waterworld_kernel").replace("21waterworld_kernel_f16", "17waterworld_kernel")
                      .replace("18hostage_kernel_f16", "14hostage_kernel")]
            assert waves(k) >= waves(twin) and k["lds"] == twin["lds"], (name, k, twin)
            n += 1
    assert n >= 10


def test_constructor_refusals_come_before_a_device():
    for mk in (_ww, _hw):
        for bad in (torch.bfloat16, torch.float64, torch.int16, "float16", None):
            with pytest.raises(ValueError, match="obs_dtype"):
                mk(obs_dtype=bad)
        with pytest.raises(ValueError, match="crowd"):
            mk(obs_dtype=F16, crowd=True)
        with pytest.raises(ValueError, match="crowd|per_env_counts"):
            mk(obs_dtype=F16, crowd=True, per_env_counts=True)
    with pytest.raises(ValueError, match="per_env_counts"):
        _ww(obs_dtype=F16, per_env_counts="wave")
    with pytest.raises(ValueError, match="sensor_range"):
        _ww(obs_dtype=F16, sensor_range=[0.2, 0.2, 0.3, 0.2, 0.2])


def test_dropins_refuse_a_half_dtype():
    from madrl_amd.hostage import ContinuousHostageWorld
    from madrl_amd.waterworld import MAWaterWorld
    for bad in (F16, torch.bfloat16):
        with pytest.raises(ValueError, match="obs_dtype"):
            MAWaterWorld(5, 10, device=NOWHERE, obs_dtype=bad)
        with pytest.raises(ValueError, match="obs_dtype"):
            ContinuousHostageWorld(3, 10, 5, 2, 2, device=NOWHERE, obs_dtype=bad)


def test_flag_travels_only_when_set(no_device):
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    from madrl_amd.waterworld import BatchedMAWaterWorld
    for cls, mk in ((BatchedMAWaterWorld, _ww), (BatchedContinuousHostageWorld, _hw)):
        params = [p for p in inspect.signature(cls.__init__).parameters if p not in ("self", "kwargs")]
        assert "obs_dtype" in params
        plain, half = mk(), mk(obs_dtype=F16)
        # a pickle of an env built without the flag: the constructor arguments that existed before it, and nothing of it on the instance
        assert list(plain.__getstate__()) == [p for p in params if p not in ("crowd", "per_env_counts", "obs_dtype")]
        assert "obs_dtype" not in vars(plain) and plain.obs_dtype is F32
        assert list(mk(obs_dtype=F32).__getstate__()) == list(plain.__getstate__())   # naming the default is building without the flag
        assert half.__getstate__()["obs_dtype"] is F16 and half.obs_dtype is F16
        copy = pickle.loads(pickle.dumps(half))
        assert type(copy) is cls and copy.obs_dtype is F16 and copy.__getstate__()["obs_dtype"] is F16
        assert pickle.loads(pickle.dumps(plain)).obs_dtype is F32


def test_half_env_has_no_fused_standardize(no_device):
    from madrl_amd import _lib
    for mk in (_ww, _hw):
        assert mk().fused_standardize is True
        half = mk(obs_dtype=F16)
        assert half.fused_standardize is False
        with pytest.raises(_lib.MadrlError, match="half-precision"):
            half.bind_standardize()


def test_float32_readers_refuse_half_rows_and_say_why():
    from madrl_amd import _lib
    rows = torch.zeros((2, 5, 213), dtype=F16)
    with pytest.raises(TypeError, match="float32") as e:
        _lib.require_float32(rows, "StandardizedEnv")
    assert "obs_dtype=torch.float16" in str(e.value) and "PursuitEvade" not in str(e.value)   # no longer one env's message
    assert _lib.require_float32(rows.float(), "StandardizedEnv").dtype is F32


def test_policies_read_their_own_element_type():
    from madrl_amd.heuristics import MultiWalkerHeuristicPolicy, WaterworldHeuristicPolicy
    with pytest.raises(ValueError, match="obs_dtype"):
        WaterworldHeuristicPolicy(obs_dtype=torch.bfloat16)
    assert WaterworldHeuristicPolicy().obs_dtype is F32 and WaterworldHeuristicPolicy(obs_dtype=F16).obs_dtype is F16
    half, full = torch.zeros((2, 5, 213), dtype=F16), torch.zeros((2, 5, 213), dtype=F32)
    with pytest.raises(TypeError, match="float32"):   # the float32 kernel would read past the end of a half tensor
        WaterworldHeuristicPolicy()(half)
    with pytest.raises(TypeError, match="float16"):
        WaterworldHeuristicPolicy(obs_dtype=F16)(full)
    with pytest.raises(TypeError, match="float16"):
        WaterworldHeuristicPolicy(obs_dtype=F16)(full.double())
    with pytest.raises(TypeError, match="float32"):
        MultiWalkerHeuristicPolicy()(torch.zeros((2, 3, 32), dtype=F16))


def test_obs_destination_takes_the_envs_dtype():
    from madrl_amd import _lib
    like32, like16 = torch.zeros((3, 1, 11), dtype=F32), torch.zeros((3, 1, 11), dtype=F16)
    assert _lib.obs_destination(torch.zeros(33, dtype=F16), like16).shape == like16.shape
    assert _lib.obs_destination(torch.zeros(33, dtype=F32), like32).shape == like32.shape
    odd = torch.zeros(40, dtype=F16)[3:36]   # a slot at an odd element of a larger tensor
    assert _lib.obs_destination(odd, like16).data_ptr() == odd.data_ptr()
    with pytest.raises(ValueError, match="contiguous float32 tensor of 33 elements"):   # the float32 env's message as it was
        _lib.obs_destination(torch.zeros(33, dtype=F16), like32)
    with pytest.raises(ValueError, match="contiguous float16 tensor of 33 elements"):
        _lib.obs_destination(torch.zeros(33, dtype=F32), like16)
    with pytest.raises(ValueError, match="float16"):
        _lib.obs_destination(torch.zeros(34, dtype=F16), like16)
