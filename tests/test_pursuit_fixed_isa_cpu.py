"""CPU test (-m "not gpu"): the emitted code of the Pursuit step kernel with its launch constants folded in (pw::FShape, pursuit_wave.hpp;
the XF lines of csrc/pursuit_fixed_specializations.def), against the plain kernel of the same shape from the SAME compile.

The headline instantiation of both is compiled for gfx950 with the build's own flags, once.  The fixed kernel must keep the store protocol
of the plain one (5 NS + 6 stores per env, NS of them non-temporal float4, the one exact wait vmcnt(5 NS + 6) that tests/test_wave_isa_budget.py finds in the plain kernel, no scratch, at most 96
VGPRs) and must have shed what its contract makes constant:
  * no scalar parked in a VGPR lane (sgpr_spill_count 0: the plain kernel has 6 and reads them back in every env);
  * no scalar load on the non-reset path of the env loop (the plain kernel loads the grid stride at the top of every iteration, the
    urgency reward in every reward block, the flag plane's pointer in every epilogue, the map pointer at every load_map);
  * fewer static scalar-ALU and vector-ALU instructions in the env loop, by a committed margin;
  * none of the reset draws' lane-uniform Philox rounds (v_mul_hi_u32 / v_mul_lo_u32) between the evader draw and the pass loop.
And the list and the library agree: every XF line has its kernel, nothing else is an FShape kernel."""
import re

import pytest

import isa
from isa import NS, VM_PER_ENV, SHAPE, HEADLINE, HEADLINE_VGPRS

FIXED = isa.wave_kernel("FShape", SHAPE)
TU = isa.HEADLINE_TU.replace("} }\n", "template __global__ void pursuit_wave_kernel<FShape<%d, %d, %d, %d, %d, %d>, 1, false, false>"
                                      "(const WaveDev, const WaveIO);\n} }\n" % SHAPE)

# Static instructions of the env loop, plain -> fixed, as this compile gives them (hipcc 7.2): SALU 267 -> 227, VALU 686 -> 554.
# The margins are those differences minus 5.
SALU_MARGIN = 35
VALU_MARGIN = 127
SLOAD_MARGIN = 5


@pytest.fixture(scope="module")
def asm():
    return isa.compile_asm(TU)


def _valu(insts):
    return [i for i in insts if i.startswith("v_")]


def _sloads(insts):
    return [i for i in insts if i.startswith("s_load")]


def test_store_protocol_and_registers(asm):
    loop = isa.wave_env_loop(asm, FIXED, VM_PER_ENV)   # (asserts the one exact wait)
    stores = [i for i in loop if re.match(r"global_store_\w+", i)]
    assert len(stores) == VM_PER_ENV, stores
    assert sum(1 for i in stores if i.startswith("global_store_dwordx4") and i.endswith(" nt")) == NS, stores
    meta = isa.kernel_meta(asm, FIXED)
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
    assert meta["vgpr_count"] <= HEADLINE_VGPRS, meta
    assert meta["sgpr_spill_count"] == 0, meta
    assert not isa.masked_spills(asm, "FShape")


def test_fewer_scalar_and_vector_instructions_than_the_plain_kernel(asm):
    plain, fixed = isa.wave_env_loop(asm, HEADLINE, VM_PER_ENV), isa.wave_env_loop(asm, FIXED, VM_PER_ENV)
    ps, fs, pv, fv = len(isa.salu(plain)), len(isa.salu(fixed)), len(_valu(plain)), len(_valu(fixed))
    print("env loop, plain -> fixed: SALU %d -> %d, VALU %d -> %d, s_load %d -> %d" % (ps, fs, pv, fv, len(_sloads(plain)), len(_sloads(fixed))))
    assert fs <= ps - SALU_MARGIN, (ps, fs)
    assert fv <= pv - VALU_MARGIN, (pv, fv)
    assert len(_sloads(fixed)) <= len(_sloads(plain)) - SLOAD_MARGIN


def _loop_layout(asm, name):
    """-> (blocks of the env loop in layout order, those of them inside the pass loop): the pass loop is the one loop directly inside
    the env loop (Depth=2) that holds the observation stores (LLVM may lay its latch out ahead of its header: the first of its blocks
    in layout is where the straight-line code of an env ends)"""
    blks = isa.blocks(isa.kernel_body(asm, name))
    home = [b for b in blks if isa.exact_wait(VM_PER_ENV)(b)]
    assert len(home) == 1
    env = (isa._parents(home[0]) or [isa._header(home[0])])[0]
    inside = isa.loop_blocks(blks, env)
    passes = [b["name"] for b in inside if "Loop Header: Depth=2" in b["notes"] and
              any(isa.nt_float4_store(x) for x in isa.loop_blocks(blks, b["name"]))]
    assert len(passes) == 1, passes
    in_pass = isa.loop_blocks(blks, passes[0])
    return [b for b in blks if any(b is x for x in inside)], in_pass


def test_no_scalar_load_on_the_non_reset_path(asm):
    """Outside the pass loop the env loop holds no scalar load at all.  Inside it the reset block comes first in layout -- from the pass
    loop's header to the end of the reset's rejection loop (the one Depth=3 loop: `att < 1024`) -- and may read its cold arguments; the
    observation pass behind it may not."""
    blks, in_pass = _loop_layout(asm, FIXED)
    for b in blks:
        if not any(b is x for x in in_pass):
            assert not _sloads(b["insts"]), (b["name"], b["notes"][:80], _sloads(b["insts"]))
    depth3 = [i for i, b in enumerate(in_pass) if "Depth=3" in b["notes"]]
    assert depth3, "the reset's rejection loop was not found inside the pass loop"
    for b in in_pass[depth3[-1] + 1:]:
        assert not _sloads(b["insts"]), (b["name"], _sloads(b["insts"]))
    # the plain kernel from the same compile does load on that path: the check can see what it is about
    pblks, p_in_pass = _loop_layout(asm, HEADLINE)
    assert sum(len(_sloads(b["insts"])) for b in pblks if not any(b is x for x in p_in_pass)) >= 3


def _muls_between_evader_draw_and_pass_loop(asm, name):
    blks, in_pass = _loop_layout(asm, name)
    flat = []
    for b in blks:
        if b is in_pass[0]:
            break
        flat += b["insts"]
    else:
        raise AssertionError("pass loop not laid out inside the env loop")
    # the evader draw ends with RandomPolicy.act: __umulhi(r.x, 5u)
    last = max(i for i, x in enumerate(flat) if re.match(r"v_mul_hi_u32 v\d+, v\d+, 5$", x) or re.match(r"v_mul_hi_u32 v\d+, 5, v\d+$", x))
    return [x for x in flat[last + 1:] if x.startswith(("v_mul_hi_u32", "v_mul_lo_u32"))]


def test_reset_draws_stay_inside_the_reset_branch(asm):
    assert _muls_between_evader_draw_and_pass_loop(asm, FIXED) == []
    assert len(_muls_between_evader_draw_and_pass_loop(asm, HEADLINE)) >= 4   # (the plain kernel carries them: the check can see them)


def test_every_xf_line_has_its_kernel_and_nothing_else_is_fixed():
    lines = isa.def_lines("pursuit_fixed_specializations.def", ("XF",))["XF"]
    assert len(lines) == 5 and lines[0] == SHAPE and SHAPE[:5] + (0,) in lines
    x_lines = isa.def_lines("pursuit_specializations.def", ("X",))["X"]
    assert all(l in x_lines for l in lines)
    built = {n for n in isa.built_kernels() if "FShape" in n}
    assert built == {isa.wave_kernel("FShape", l) for l in lines}, sorted(built)
    for n in built:
        k = isa.built_kernels()[n]
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["sgpr_spills"] == 0, (n, k)
