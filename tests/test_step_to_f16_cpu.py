"""Half-precision observation slots (madrl_pursuit_step_to_f16), the parts that need no GPU: the exported symbols, the metadata of the half
two-buffer kernels beside the float32 ones, and the obs_dtype argument of BatchedPursuitEvade."""
import ctypes as C
import inspect
import os

import pytest
import torch

import isa
from isa import SO

HERE = os.path.dirname(os.path.abspath(__file__))


def _to_lines():
    """the X / XL lines of pursuit_to_specializations.def: (live, (xs, ys, p, e, r, flatten))"""
    lines = isa.def_lines("pursuit_to_specializations.def", ("X", "XL"))
    out = [(False, v) for v in lines["X"]] + [(True, v) for v in lines["XL"]]
    assert len(out) >= 5 and any(live for live, _ in out), "the list has X and XL lines"
    return out


def _wave_name(shape_type, args):
    """the mangled name of pursuit_wave_kernel<pw::SHAPE<args>, 1, true, false>"""
    return isa.wave_kernel(shape_type, args, inject=True)


def test_the_library_exports_both_symbols():
    if not os.path.exists(SO):
        pytest.skip("library not built")
    L = C.CDLL(SO)
    for name in ("madrl_pursuit_step_to_f16", "madrl_pursuit_step_to_f16_kernel_kind"):
        assert hasattr(L, name), name
    from madrl_amd import _lib
    assert _lib.SIGNATURES["madrl_pursuit_step_to_f16"] == (C.c_int, [C.c_void_p] * 9)
    assert _lib.SIGNATURES["madrl_pursuit_step_to_f16_kernel_kind"] == (C.c_int, [C.c_void_p] * 2)
    assert L.madrl_abi_version() == 8 == _lib.ABI_VERSION
    header = open(os.path.join(HERE, "..", "include", "madrl_hip.h")).read()
    assert header.index("int madrl_pursuit_step_to(") < header.index("int madrl_pursuit_step_to_f16(") < header.index("int madrl_pursuit_step_sharded(")


@pytest.mark.parametrize("live,args", _to_lines(), ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else ("XL" if v else "X"))
def test_every_one_wavefront_line_has_its_half_kernel(live, args):
    """(The XL kernels are compiled in a translation unit of their own, pursuit_to_f16_live.hip, with the basic scalar register allocator:
    the default one leaves them a 20-byte private segment that no instruction touches.)"""
    ks = isa.built_kernels()
    half = ks.get(_wave_name("TLHShape" if live else "THShape", args))
    f32 = ks.get(_wave_name("TLShape" if live else "TShape", args))
    assert f32 is not None, ("the float32 two-buffer kernel is gone", live, args)
    assert half is not None, ("no half two-buffer kernel", live, args)
    # WaveDev and WaveIO did not grow: the half pointers travel in the float fields
    assert half["args"] == f32["args"] == [(0, 176), (176, 88)], (live, args, half["args"], f32["args"])
    assert half["vgprs"] <= f32["vgprs"], (live, args, half["vgprs"], f32["vgprs"])
    assert half["scratch"] == 0 and half["vgpr_spills"] == 0, (live, args, half)


def test_the_generic_half_kernels_take_the_float32_kernels_arguments():
    ks = isa.built_kernels()
    half = {n: k for n, k in ks.items() if "pursuit_to_f16_kernel" in n}
    f32 = {n: k for n, k in ks.items() if "pursuit_to_kernel" in n}
    assert len(half) == 16 and len(f32) == 16   # NT 1..8, with and without per-env agent counts
    assert {tuple(k["args"]) for k in half.values()} == {tuple(k["args"]) for k in f32.values()} and len({tuple(k["args"]) for k in f32.values()}) == 1


def test_obs_dtype_values_are_checked_before_a_device_is_touched():
    from madrl_amd import _lib
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    nodev = "cuda:99"   # never reached
    kw = dict(n_envs=4, device=nodev, n_pursuers=8, n_evaders=30, obs_range=7)
    for bad in (torch.bfloat16, torch.float64, torch.int16, "float16", None):
        with pytest.raises(ValueError, match="obs_dtype"):
            BatchedPursuitEvade([rectangle_map(16, 16)], obs_dtype=bad, **kw)
    assert inspect.signature(BatchedPursuitEvade.__init__).parameters["obs_dtype"].default is torch.float32
    for good in (torch.float16, torch.float32):   # accepted: the constructor goes on to the device (or to the missing library) and fails there
        with pytest.raises(Exception) as ei:
            BatchedPursuitEvade([rectangle_map(16, 16)], obs_dtype=good, **kw)
        assert not isinstance(ei.value, (ValueError, TypeError)), ei.value


def test_step_to_keeps_its_signature_and_docstring():
    from madrl_amd.pursuit import BatchedPursuitEvade
    assert str(inspect.signature(BatchedPursuitEvade.step_to)) == "(self, actions, obs_out, rew_out=None, done_out=None, evader_actions=None)"
    doc = BatchedPursuitEvade.step_to.__doc__
    assert doc.startswith("step() with the observations written to `obs_out` (float32, contiguous, on the env's device, N * P * obs_dim elements: e.g.")
    assert doc.rstrip().endswith("kernel (step_to_kernel_kind).") and len(doc) == 1037


def test_native_consumers_of_observation_rows_refuse_half_rows():
    """The device chase policy and the wrappers' epilogue kernels read (and StandardizedEnv writes) float32 through the raw pointer with
    element counts taken from the tensor: float16 rows would be read, or written, past the end of their buffer.  Each entry point raises
    before it takes a pointer (no library, no device needed); the N == 1 drop-in is not offered the dtype."""
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import PursuitEvade
    from madrl_amd.wrappers import ObservationBuffer, StandardizedEnv
    half = torch.zeros((4, 8, 148), dtype=torch.float16)
    with pytest.raises(TypeError, match="float32"):
        PursuitHeuristicPolicy(7)(half)
    with pytest.raises(TypeError, match="float32"):
        PursuitHeuristicPolicy(7).sample_actions(half)
    buf = object.__new__(ObservationBuffer)
    buf._buf, buf._buffer_size = None, 2
    with pytest.raises(TypeError, match="float32"):
        buf._push(half, None)
    assert buf._buf is None
    std = object.__new__(StandardizedEnv)
    std._enable_obsnorm, std._fused, std._own = True, False, dict(obs_mean=None, obs_var=None, rew_mean=None, rew_var=None)
    with pytest.raises(TypeError, match="float32"):
        std._norm_obs(half)
    assert std._own["obs_mean"] is None
    with pytest.raises(TypeError, match="obs_dtype"):
        PursuitEvade([rectangle_map(16, 16)], device="cuda:99", obs_dtype=torch.float16, n_pursuers=8, n_evaders=30, obs_range=7)
