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
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# kernel -> VGPRs of the build before the staged start-up (the headline's 96 is also its budget at five wavefronts per SIMD)
KERNELS = {
    "wave": ("pursuit_wave_kernel<Shape<16, 16, 8, 30, 7, 1>, 1, false, false>", 96),
    "group_c5": ("pursuit_group_kernel<GShape<32, 32, 16, 60, 7, 1, 2>, 1, false>", 115),
    "group_authors": ("pursuit_group_kernel<GShape<32, 32, 30, 50, 11, 1, 4>, 1, false>", 113),
}
# per-env agent counts: the start-up's shape is checked, the register contracts are those of tests/test_live_counts_group_isa.py
LIVE_KERNELS = {
    "live_20v50": "pursuit_group_kernel<LGShape<16, 16, 20, 50, 5, 1, 2>, 1, false>",
    "live_authors": "pursuit_group_kernel<LGShape<32, 32, 30, 50, 11, 1, 4>, 1, false>",
}
MANGLED = {
    "live_20v50": "_ZN5madrl2pw20pursuit_group_kernelINS0_7LGShapeILi16ELi16ELi20ELi50ELi5ELi1ELi2EEELi1ELb0EEEvNS0_7WaveDevENS0_6WaveIOE",
    "live_authors": "_ZN5madrl2pw20pursuit_group_kernelINS0_7LGShapeILi32ELi32ELi30ELi50ELi11ELi1ELi4EEELi1ELb0EEEvNS0_7WaveDevENS0_6WaveIOE",
    "wave": "_ZN5madrl2pw19pursuit_wave_kernelINS0_5ShapeILi16ELi16ELi8ELi30ELi7ELi1EEELi1ELb0ELb0EEEvNS0_7WaveDevENS0_6WaveIOE",
    "group_c5": "_ZN5madrl2pw20pursuit_group_kernelINS0_6GShapeILi32ELi32ELi16ELi60ELi7ELi1ELi2EEELi1ELb0EEEvNS0_7WaveDevENS0_6WaveIOE",
    "group_authors": "_ZN5madrl2pw20pursuit_group_kernelINS0_6GShapeILi32ELi32ELi30ELi50ELi11ELi1ELi4EEELi1ELb0EEEvNS0_7WaveDevENS0_6WaveIOE",
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
    from madrl_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "startup.hip"), os.path.join(tmp, "startup.s")
        with open(src, "w") as f:
            f.write(TU)
        subprocess.run([B.HIPCC] + [f for f in B.FLAGS if f != "-Wall"] + ["-I", B.CSRC, "--cuda-device-only", "-S", src, "-o", out],
                       check=True, capture_output=True)
        return open(out).read()


def _blocks(text, name):
    """the basic blocks of a kernel in layout order: (label, annotation text, instructions)"""
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(MANGLED[name] + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur = [], None
    for l in lines[start + 1:end]:
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)", l)
        if m:
            cur = dict(name=m.group(1), notes=l, insts=[], open=True)
            blocks.append(cur)
        elif cur is not None:
            t = l.strip()
            if t.startswith(";") and cur["open"]:
                cur["notes"] += " " + t
            elif t and not t.startswith((";", ".")):
                cur["open"] = False
                cur["insts"].append(t.split(";")[0].strip())
    return blocks


def _before_env_loop(text, name):
    """-> (blocks before the env loop, names of the loop headers among them).  The env loop is the outermost loop (Depth=1 header) that
    holds global stores; every block of it is annotated with its header, so 'before' = not in that loop and laid out before its header."""
    blocks = _blocks(text, name)
    in_loop = lambda b, h: b["name"] == h or ("Header=%s " % h) in b["notes"] + " " or ("Parent Loop %s " % h) in b["notes"] + " "
    heads = [b["name"] for b in blocks if "Loop Header: Depth=1" in b["notes"]]
    env = [h for h in heads if any(i.startswith("global_store") for b in blocks if in_loop(b, h) for i in b["insts"])]
    assert len(env) == 1, "expected one top-level loop with global stores (the env loop), found %r" % env
    at = next(i for i, b in enumerate(blocks) if b["name"] == env[0])
    pre = [b for b in blocks[:at] if not in_loop(b, env[0])]
    assert pre, "no code before the env loop?"
    return pre, [b["name"] for b in pre if "Loop Header" in b["notes"]]


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
    meta = asm_text[asm_text.index("amdhsa.kernels:"):]
    entries = [e for e in re.split(r"\n  - (?=\.)", meta) if re.search(r"\.name:\s+%s\n" % re.escape(MANGLED[name]), e)]   # one list item per kernel
    assert len(entries) == 1
    entry = entries[0]
    get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, entry).group(1))
    assert get("private_segment_fixed_size") == 0
    assert get("vgpr_spill_count") == 0
    assert get("vgpr_count") <= KERNELS[name][1], "%d VGPRs, %d before" % (get("vgpr_count"), KERNELS[name][1])
