"""CPU test (-m "not gpu") of tests/isa.py itself, on a short assembly text written for this test (no compiler): two kernels; in the first
an env loop (Depth=1) with an inner loop and a rare-path block laid out after the loop but annotated with its header, and a second
top-level loop without stores."""
import pytest

import isa

ASM = """\t.globl\tkern_a
kern_a:
; %bb.0:
\ts_load_dwordx4 s[0:3], s[4:5], 0x0
\tglobal_load_dword v1, v0, s[0:1]
\ts_waitcnt vmcnt(0)
\ts_cbranch_scc1 .LBB0_7
.LBB0_1:                                ; %table
                                        ; =>This Inner Loop Header: Depth=1
\tds_write_b32 v2, v1
\ts_add_u32 s6, s6, 1                    ; a comment behind an instruction
\ts_cbranch_scc0 .LBB0_1
; %bb.2:
\ts_mov_b32 s7, 0
.LBB0_3:                                ; %env
                                        ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB0_4 Depth 2
\ts_waitcnt vmcnt(3)
\ts_and_b32 s8, s8, s9
\t.p2align\t3
.LBB0_4:                                ; %row
                                        ;   Parent Loop BB0_3 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
\tglobal_store_dwordx4 v[4:7], v[2:3], off nt
\ts_sub_u32 s10, s10, 1
\ts_cbranch_scc1 .LBB0_4
; %bb.5:                                ;   in Loop: Header=BB0_3 Depth=1
\tglobal_store_dword v[2:3], v8, off
\ts_cbranch_vccnz .LBB0_8
.LBB0_6:                                ;   in Loop: Header=BB0_3 Depth=1
\ts_barrier
\ts_cbranch_scc0 .LBB0_3
.LBB0_7:
\ts_endpgm
.LBB0_8:                                ; %rare
                                        ;   in Loop: Header=BB0_3 Depth=1
\ts_or_b32 s11, s11, 1
\ts_branch .LBB0_6
.Lfunc_end0:
\t.size\tkern_a, .Lfunc_end0-kern_a

\t.globl\tkern_b
kern_b:
; %bb.0:
\ts_waitcnt vmcnt(3)
\ts_endpgm
.Lfunc_end1:

\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           176
        .value_kind:     by_value
      - .offset:         176
        .size:           88
        .value_kind:     by_value
    .group_segment_fixed_size: 4096
    .name:           kern_a
    .private_segment_fixed_size: 0
    .sgpr_count:     40
    .sgpr_spill_count: 0
    .symbol:         kern_a.kd
    .uses_dynamic_stack: false
    .vgpr_count:     96
    .vgpr_spill_count: 0
  - .agpr_count:     4
    .args:           []
    .group_segment_fixed_size: 0
    .name:           kern_b
    .private_segment_fixed_size: 24
    .sgpr_count:     8
    .sgpr_spill_count: 0
    .vgpr_count:     3
    .vgpr_spill_count: 2
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
"""
ENV = ["s_waitcnt vmcnt(3)", "s_and_b32 s8, s8, s9", "global_store_dwordx4 v[4:7], v[2:3], off nt", "s_sub_u32 s10, s10, 1",
       "s_cbranch_scc1 .LBB0_4", "global_store_dword v[2:3], v8, off", "s_cbranch_vccnz .LBB0_8", "s_barrier", "s_cbranch_scc0 .LBB0_3",
       "s_or_b32 s11, s11, 1", "s_branch .LBB0_6"]


def _blocks(name="kern_a"):
    return isa.blocks(isa.kernel_body(ASM, name))


def test_body_insts_and_blocks():
    assert isa.kernel_body(ASM, "kern_b") == ["kern_b:", "; %bb.0:", "\ts_waitcnt vmcnt(3)", "\ts_endpgm"]
    assert isa.kernel_insts(ASM, "kern_b") == ["s_waitcnt vmcnt(3)", "s_endpgm"]
    blks = _blocks()
    assert [b["name"] for b in blks] == [None, "BB0_1", None, "BB0_3", "BB0_4", None, "BB0_6", "BB0_7", "BB0_8"]
    assert blks[1]["insts"] == ["ds_write_b32 v2, v1", "s_add_u32 s6, s6, 1", "s_cbranch_scc0 .LBB0_1"]   # comments and directives dropped
    assert "Child Loop BB0_4" in blks[3]["notes"] and "Parent Loop BB0_3 Depth=1" in blks[4]["notes"] and "Header=BB0_3" in blks[8]["notes"]
    assert [i for b in blks for i in b["insts"]] == isa.kernel_insts(ASM, "kern_a")
    for missing in ("kern_c", "kern"):   # (a prefix of a name is not the name)
        with pytest.raises(LookupError):
            isa.kernel_body(ASM, missing)


def test_env_loop_by_both_rules():
    blks = _blocks()
    assert isa.env_loop(blks, isa.exact_wait(3), once="once") == ENV          # home in the outer loop's header
    assert isa.env_loop(blks, isa.nt_float4_store) == ENV                     # home in the inner loop: climbs to the Depth=1 loop
    assert isa.wave_env_loop(ASM, "kern_a", 3) == ENV and isa.store_env_loop(ASM, "kern_a") == ENV
    with pytest.raises(AssertionError, match=r"exact wait vmcnt\(5\) must appear once"):
        isa.wave_env_loop(ASM, "kern_a", 5)                                   # no such wait
    twice = isa.blocks(isa.kernel_body(ASM.replace("s_and_b32 s8, s8, s9", "s_and_b32 s8, s8, s9\n.LBB0_9:   ;   in Loop: Header=BB0_3 Depth=1\n\ts_waitcnt vmcnt(3)"), "kern_a"))
    assert len([b for b in twice if isa.exact_wait(3)(b)]) == 2
    with pytest.raises(AssertionError, match="must appear once"):
        isa.env_loop(twice, isa.exact_wait(3), once="the exact wait must appear once")
    assert len(isa.env_loop(twice, isa.exact_wait(3))) == len(ENV) + 1        # without once: the first home block's loop
    # the table loop is a loop of its own
    assert isa.env_loop(blks, lambda b: "ds_write_b32 v2, v1" in b["insts"]) == blks[1]["insts"]


def test_before_env_loop():
    blks = _blocks()
    pre, loops = isa.before_env_loop(blks)
    assert [b["name"] for b in pre] == [None, "BB0_1", None] and loops == ["BB0_1"]
    with pytest.raises(AssertionError, match="expected one top-level loop with global stores"):
        isa.before_env_loop(isa.blocks(isa.kernel_body(ASM.replace("ds_write_b32 v2, v1", "global_store_dword v[2:3], v1, off"), "kern_a")))
    with pytest.raises(AssertionError, match="expected one top-level loop with global stores"):
        isa.before_env_loop(_blocks("kern_b"))


def test_salu():
    assert isa.salu(ENV) == ["s_and_b32 s8, s8, s9", "s_sub_u32 s10, s10, 1", "s_or_b32 s11, s11, 1"]
    assert isa.salu(isa.kernel_insts(ASM, "kern_a")[:4]) == []   # scalar loads, waits and branches are not issued on the scalar ALU
    assert "s_waitcnt" in isa.NOT_SALU and "s_barrier" in isa.NOT_SALU


def test_kernel_meta_reads_its_own_entry():
    a, b = isa.kernel_meta(ASM, "kern_a"), isa.kernel_meta(ASM, "kern_b")
    assert a == dict(agpr_count=0, group_segment_fixed_size=4096, private_segment_fixed_size=0, sgpr_count=40, sgpr_spill_count=0,
                     vgpr_count=96, vgpr_spill_count=0)   # (the arguments' offsets and sizes are not the kernel's fields)
    assert (b["private_segment_fixed_size"], b["vgpr_spill_count"], b["vgpr_count"], b["agpr_count"]) == (24, 2, 3, 4)
    with pytest.raises(LookupError, match="0 entries named kern_c"):
        isa.kernel_meta(ASM, "kern_c")
    with pytest.raises(LookupError, match="0 entries named kern "):
        isa.kernel_meta(ASM, "kern")
    with pytest.raises(LookupError, match="2 entries named kern_a"):
        isa.kernel_meta(ASM.replace(".name:           kern_b", ".name:           kern_a"), "kern_a")


def test_mangled_names():
    assert isa.HEADLINE == isa.wave_kernel("Shape", (16, 16, 8, 30, 7, 1)) == \
        "_ZN5madrl2pw19pursuit_wave_kernelINS0_5ShapeILi16ELi16ELi8ELi30ELi7ELi1EEELi1ELb0ELb0EEEvNS0_7WaveDevENS0_6WaveIOE"
    group = {
        ("LGShape", (16, 16, 20, 50, 5, 1, 2)):
            "_ZN5madrl2pw20pursuit_group_kernelINS0_7LGShapeILi16ELi16ELi20ELi50ELi5ELi1ELi2EEELi1ELb0EEEvNS0_7WaveDevENS0_6WaveIOE",
        ("LGShape", (32, 32, 30, 50, 11, 1, 4)):
            "_ZN5madrl2pw20pursuit_group_kernelINS0_7LGShapeILi32ELi32ELi30ELi50ELi11ELi1ELi4EEELi1ELb0EEEvNS0_7WaveDevENS0_6WaveIOE",
        ("GShape", (32, 32, 16, 60, 7, 1, 2)):
            "_ZN5madrl2pw20pursuit_group_kernelINS0_6GShapeILi32ELi32ELi16ELi60ELi7ELi1ELi2EEELi1ELb0EEEvNS0_7WaveDevENS0_6WaveIOE",
        ("GShape", (32, 32, 30, 50, 11, 1, 4)):
            "_ZN5madrl2pw20pursuit_group_kernelINS0_6GShapeILi32ELi32ELi30ELi50ELi11ELi1ELi4EEELi1ELb0EEEvNS0_7WaveDevENS0_6WaveIOE",
    }
    for (shape, ints), name in group.items():
        assert isa.group_kernel(shape, ints) == isa.mangled("pw", "pursuit_group_kernel", shape, ints, (1, False), isa.WAVE_ARGS) == name
    assert isa.group_kernel("TGShape", (32, 32, 16, 60, 7, 1, 2), inject=True) == \
        "_ZN5madrl2pw20pursuit_group_kernelINS0_7TGShapeILi32ELi32ELi16ELi60ELi7ELi1ELi2EEELi1ELb1EEEvNS0_7WaveDevENS0_6WaveIOE"
    assert isa.crowd_kernel((24, 24, 20, 300, 9, 1, 1), 0) == \
        "_ZN5madrl2pc20pursuit_crowd_kernelINS0_6CShapeILi24ELi24ELi20ELi300ELi9ELi1ELi1EEELi0EEEvNS0_8CrowdDevENS0_7CrowdIOE"
    assert isa.crowd_kernel((128, 128, 100, 300, 21, 0, 16), 1, live=True) == \
        "_ZN5madrl2pc25pursuit_live_crowd_kernelINS0_7LCShapeILi128ELi128ELi100ELi300ELi21ELi0ELi16EEELi1EEEvNS0_8CrowdDevENS0_7CrowdIOEPKi"
