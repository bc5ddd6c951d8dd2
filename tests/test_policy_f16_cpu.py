"""The chase policy over half-precision observation rows (madrl_heuristic_pursuit_f16, PursuitHeuristicPolicy(obs_dtype=torch.float16)), the
parts that need no GPU: the symbol in the header, the library and the binding, the metadata of the two half kernels beside the float32
ones, and the obs_dtype argument of the policy class."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import isa
from isa import SO

HERE = os.path.dirname(os.path.abspath(__file__))
_ARGS = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p,
         C.c_void_p]


def test_the_header_declares_the_half_call_next_to_the_float32_one():
    header = open(os.path.join(HERE, "..", "include", "madrl_hip.h")).read()
    assert header.index("int madrl_heuristic_pursuit(") < header.index("int madrl_heuristic_pursuit_f16(") < header.index("int madrl_heuristic_waterworld(")
    decl = re.search(r"int madrl_heuristic_pursuit_f16\(([^;]*)\);", header).group(1)
    assert [" ".join(a.split()) for a in decl.split(",")] == [
        "const void *obs_f16", "int64_t n_rows", "int32_t obs_range", "int64_t row_stride", "int32_t cell_stride", "int32_t ch_offset",
        "const uint8_t *table_dev", "uint64_t seed", "int64_t row_id_base", "uint32_t tick", "uint32_t *tick_dev", "int32_t *actions", "void *stream"]
    assert re.search(r"#define MADRL_ABI_VERSION\s+8\b", header)


def test_the_library_exports_it_and_the_binding_knows_13_arguments():
    from madrl_amd import _lib
    L = C.CDLL(SO)
    assert hasattr(L, "madrl_heuristic_pursuit_f16")
    res, args = _lib.SIGNATURES["madrl_heuristic_pursuit_f16"]
    assert res is C.c_int and len(args) == 13 and args == _ARGS == _lib.SIGNATURES["madrl_heuristic_pursuit"][1]
    assert L.madrl_abi_version() == 8 == _lib.ABI_VERSION


def test_argument_checks_are_those_of_the_float32_call():
    """refused before anything is launched (no device needed), with the float32 call's message under the new name"""
    from madrl_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(16)   # never dereferenced: every call below is refused first
    good = dict(obs=one, n_rows=1, obs_range=7, table=one, actions=one)
    for bad in (dict(obs=None), dict(table=None), dict(actions=None), dict(n_rows=0), dict(obs_range=0), dict(obs_range=256)):
        a = dict(good, **bad)
        for name, what in (("madrl_heuristic_pursuit_f16", "heuristic_pursuit_f16"), ("madrl_heuristic_pursuit", "heuristic_pursuit")):
            rc = getattr(L, name)(a["obs"], a["n_rows"], a["obs_range"], 148, 1, 98, a["table"], 0, 0, 0, None, a["actions"], None)
            assert rc != 0, (name, bad)
            assert L.madrl_last_error().decode() == what + ": bad argument", (name, bad, L.madrl_last_error())


def test_the_half_kernels_have_no_private_segment_and_no_spill():
    ks = isa.built_kernels()
    pick = lambda part: [k for n, k in ks.items() if part in n]
    generic, rows = pick("pursuit_policy_f16_kernel"), pick("pursuit_policy_rows_f16_kernel")
    assert len(generic) == 1 and len(rows) == 1, (len(generic), len(rows))
    for half, f32 in ((generic[0], pick("21pursuit_policy_kernel")), (rows[0], pick("26pursuit_policy_rows_kernel"))):
        assert len(f32) == 1
        assert half["scratch"] == 0 and half["vgpr_spills"] == 0 and half["sgpr_spills"] == 0, half
        assert half["lds"] == 0 and half["args"] == f32[0]["args"], (half, f32[0])
        assert half["vgprs"] <= 64, half   # eight wavefronts per SIMD, as the float32 kernels


def test_obs_dtype_is_checked_before_a_device_is_touched():
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    sig = inspect.signature(PursuitHeuristicPolicy.__init__)
    assert list(sig.parameters) == ["self", "obs_range", "flatten", "seed", "row_id_base", "obs_dtype"]
    assert sig.parameters["obs_dtype"].default is torch.float32
    for bad in (torch.bfloat16, torch.float64, torch.int16, "float16", None):
        with pytest.raises(ValueError, match="obs_dtype"):
            PursuitHeuristicPolicy(7, obs_dtype=bad)
    for good in (torch.float16, torch.float32):
        pol = PursuitHeuristicPolicy(7, obs_dtype=good)
        assert pol.obs_dtype is good and pol._tick is None and pol._table is None   # nothing on a device yet


def test_a_policy_reads_exactly_its_own_element_type():
    """each refusal is raised before a pointer is taken: CPU tensors, no library call"""
    from madrl_amd.heuristics import PursuitHeuristicPolicy
    half_pol = PursuitHeuristicPolicy(7, obs_dtype=torch.float16)
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.int16):
        rows = torch.zeros((4, 8, 148), dtype=dtype)
        with pytest.raises(TypeError, match="obs_dtype"):
            half_pol(rows)
        with pytest.raises(TypeError, match="obs_dtype"):
            half_pol.sample_actions(rows, out=torch.zeros((4, 8), dtype=torch.int32))
    assert half_pol._tick is None and half_pol._table is None and half_pol._act is None
    with pytest.raises(TypeError, match="float32"):   # as before: the float32 policy on half rows
        PursuitHeuristicPolicy(7, obs_dtype=torch.float32)(torch.zeros((4, 8, 148), dtype=torch.float16))
