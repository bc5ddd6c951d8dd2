"""CPU test (-m "not gpu"): the emitted start-up code of the Pursuit fast kernels.

Before its first env a workgroup copies its tables from global memory to LDS.  Written as bounds-checked strided loops this compiled to
one global_load -> s_waitcnt vmcnt(0) -> ds_write chain per 64 (or NT) elements, each next load behind a branch: about twenty dependent
round trips to L2 per workgroup, made by all workgroups of a launch at once.  The kernels now stage everything in batches of
unconditional loads with one wait per batch ("table staging", pursuit_wave.hpp).  This test compiles the headline one-wavefront
instantiation and two multi-wavefront ones for gfx950 with the build's own flags and checks, in the code BEFORE the env loop:
  * headline: every global_load precedes the first s_waitcnt vmcnt (one batch);
  * multi-wavefront: no loop contains a global_load, and a global_load follows a vmcnt wait at most once (two batches) -- also in the
    per-env-counts instantiations (LGShape), whose second batch is the first env's record, action and masks;
  * all three: no scratch, no VGPR spills, and not more VGPRs than the kernels had with the serial fills.
"""
import re

import pytest

import isa

# kernel -> (instantiation, VGPRs of the build before the staged start-up; the headline's 96 is also its budget at five wavefronts per SIMD)
KERNELS = {
    "wave": ("pursuit_wave_kernel<Shape<16, 16, 8, 30, 7, 1>, 1, false, false>", isa.HEADLINE_VGPRS),
    "group_c5": ("pursuit_group_kernel<GShape<32, 32, 16, 60, 7, 1, 2>, 1, false>", 115),
    "group_authors": ("pursuit_group_kernel<GShape<32, 32, 30, 50, 11, 1, 4>, 1, false>", 113),
}
# per-env agent counts: the start-up's shape is checked, the register contracts are those of tests/test_live_counts_group_isa.py
LIVE_KERNELS = {
    "live_20v50": "pursuit_group_kernel<LGShape<16, 16, 20, 50, 5, 1, 2>, 1, false>",
    "live_authors": "pursuit_group_kernel<LGShape<32, 32, 30, 50, 11, 1, 4>, 1, false>",
}
MANGLED = {
    "live_20v50": isa.group_kernel("LGShape", (16, 16, 20, 50, 5, 1, 2)),
    "live_authors": isa.group_kernel("LGShape", (32, 32, 30, 50, 11, 1, 4)),
    "wave": isa.HEADLINE,
    "group_c5": isa.group_kernel("GShape", (32, 32, 16, 60, 7, 1, 2)),
    "group_authors": isa.group_kernel("GShape", (32, 32, 30, 50, 11, 1, 4)),
}

TU = """#include "common.hpp"
#include "pursuit_wave.hpp"
#include "pursuit_group.hpp"
namespace madrl { namespace pw {
%s
} }
""" % "\n".join("template __global__ void %s(const WaveDev, const WaveIO);" % k for k in [k for k, _ in KERNELS.values()] + list(LIVE_KERNELS.values()))


@pytest.fixture(scope="module")
def asm_text():
    return isa.compile_asm(TU)


def _before_env_loop(text, name):
    return isa.before_env_loop(isa.blocks(isa.kernel_body(text, MANGLED[name])))


def _events(pre):
    """'L' per global_load, 'W' per s_waitcnt that names vmcnt, in layout order"""
    ev = []
    for b in pre:
        for i in b["insts"]:
            if i.startswith("global_load"):
                ev.append("L")
            elif i.startswith("s_waitcnt") and "vmcnt" in i:
                ev.append("W")
    return "".join(ev)


def test_headline_startup_is_one_batch(asm_text):
    pre, _ = _before_env_loop(asm_text, "wave")
    ev = _events(pre)
    assert ev.count("L") >= 52, ev   # 19 table trips, 30 slot constants, the first env's record, action and mask
    assert "W" in ev and "L" not in ev[ev.index("W"):], "a global_load after the first vmcnt wait: " + ev


@pytest.mark.parametrize("name", ["group_c5", "group_authors", "live_20v50", "live_authors"])
def test_group_startup_is_at_most_two_batches(asm_text, name):
    pre, loops = _before_env_loop(asm_text, name)
    for b in pre:
        looped = b["name"] in loops or any(("Header=%s " % h) in b["notes"] + " " for h in loops)
        assert not (looped and any(i.startswith("global_load") for i in b["insts"])), "a global_load in a loop before the env loop (%s)" % b["name"]
    ev = _events(pre)
    assert "L" in ev
    assert len(re.findall(r"WL", ev)) <= 1, "more than two batches of loads: " + ev


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_startup_register_budget(asm_text, name):
    meta = isa.kernel_meta(asm_text, MANGLED[name])
    assert meta["private_segment_fixed_size"] == 0
    assert meta["vgpr_spill_count"] == 0
    assert meta["vgpr_count"] <= KERNELS[name][1], "%d VGPRs, %d before" % (meta["vgpr_count"], KERNELS[name][1])
