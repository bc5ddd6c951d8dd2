"""CPU test (-m "not gpu"): the scalar-instruction budget of the headline kernel's env loop.

The one-wavefront Pursuit step kernel (pursuit_wave.hpp) is issue-bound, and its scalar instructions share ONE scalar pipe per CU
among four SIMDs: 20 extra dependent SALU per observation slot (100 per env, MADRL_ABLATE=128) cost 7.3 us of a 71.8 us launch
(profiles/r07_wave).  The observation pass therefore builds its store masks with one vector compare each and sets exec with one s_mov
per store.  This test compiles the headline instantiation (BASELINE configs[1]) for gfx950 with the build's own flags and checks, in
the emitted code of the env loop (every block LLVM annotates as inside it, rare paths included):
  * the static SALU count stays within a committed budget;
  * the loop issues exactly VM_PER_ENV = 5 * NS + 6 stores, NS of them non-temporal float4, and waits for the record prefetch with
    exactly s_waitcnt vmcnt(VM_PER_ENV) (results would be silently wrong otherwise);
  * no scratch and no VGPR spills.
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

SHAPE = (16, 16, 8, 30, 7, 1)   # XS, YS, P, E, obs_range, flatten
NS = 5                           # float4 slots per lane: 8 pursuers x 37 float4 = 296 slots over 64 lanes
VM_PER_ENV = 5 * NS + 6
SALU_BUDGET = 320                # 309 since the observation pass builds its store masks on the vector unit (407 before)
# not issued on the scalar ALU: waits, nops, branches, scalar memory, barriers
NOT_SALU = ("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_load", "s_buffer", "s_barrier", "s_setprio", "s_sleep", "s_endpgm")

TU = """#include "common.hpp"
#include "pursuit_wave.hpp"
namespace madrl { namespace pw {
template __global__ void pursuit_wave_kernel<Shape<%d, %d, %d, %d, %d, %d>, 1, false, false>(const WaveDev, const WaveIO);
} }
""" % SHAPE


@pytest.fixture(scope="module")
def kernel_asm():
    from madrl_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "wave_headline.hip"), os.path.join(tmp, "wave_headline.s")
        with open(src, "w") as f:
            f.write(TU)
        subprocess.run([B.HIPCC] + [f for f in B.FLAGS if f != "-Wall"] + ["-I", B.CSRC, "--cuda-device-only", "-S", src, "-o", out],
                       check=True, capture_output=True)
        text = open(out).read()
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN5madrl2pw19pursuit_wave_kernel\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return text, lines[start:end]


def _env_loop(body):
    """instructions of every basic block of the loop whose body holds the record prefetch's exact wait, inner loops included
    (LLVM annotates each block with its innermost loop header, and each inner loop header with its parent loops)"""
    blocks, cur = [], None
    for l in body:
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)", l)
        if m:
            cur = dict(name=m.group(1), notes=l, insts=[], open=True)
            blocks.append(cur)
        elif cur is not None:
            t = l.strip()
            if t.startswith(";") and cur["open"]:
                cur["notes"] += " " + t   # the annotation lines right after the label
            elif t and not t.startswith((";", ".")):
                cur["open"] = False
                cur["insts"].append(t.split(";")[0].strip())
    wait = "s_waitcnt vmcnt(%d)" % VM_PER_ENV
    home = [b for b in blocks if wait in b["insts"]]
    assert len(home) == 1, "the record prefetch's exact wait vmcnt(%d) must appear once" % VM_PER_ENV
    hm = re.search(r"Header=(BB\d+_\d+)", home[0]["notes"])
    headers = {hm.group(1) if hm else home[0]["name"]}
    grown = True
    while grown:   # inner loops: headers whose parent loops include one of ours
        grown = False
        for b in blocks:
            if b["name"] and b["name"] not in headers and any(p in headers for p in re.findall(r"Parent Loop (BB\d+_\d+)", b["notes"])):
                headers.add(b["name"])
                grown = True
    own = lambda b: b["name"] in headers or any(h in headers for h in re.findall(r"Header=(BB\d+_\d+)", b["notes"]))
    return [i for b in blocks if own(b) for i in b["insts"]]


def test_env_loop_salu_budget(kernel_asm):
    loop = _env_loop(kernel_asm[1])
    salu = [i for i in loop if i.startswith("s_") and not i.startswith(NOT_SALU)]
    assert len(salu) <= SALU_BUDGET, "env loop: %d static SALU instructions, budget %d" % (len(salu), SALU_BUDGET)


def test_env_loop_store_count(kernel_asm):
    loop = _env_loop(kernel_asm[1])
    stores = [i for i in loop if re.match(r"global_store_\w+", i)]
    assert len(stores) == VM_PER_ENV, stores
    assert sum(1 for i in stores if i.startswith("global_store_dwordx4") and i.endswith(" nt")) == NS, stores


def test_no_scratch(kernel_asm):
    text = kernel_asm[0]
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", text)
    assert re.search(r"\.vgpr_spill_count:\s+0\b", text)
