"""CPU test (-m "not gpu"): the live-count instantiation of the headline shape (per-env agent counts, LShape in pursuit_wave.hpp) keeps the
contracts of the fixed-shape step kernel (tests/test_wave_isa_budget.py): no scratch, no VGPR spills, exactly VM_PER_ENV stores in the env
loop -- the stores of observation rows past an env's live pursuer count stay issued with an empty exec mask -- and one exact
s_waitcnt vmcnt(VM_PER_ENV) for the record prefetch."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_wave_isa_budget as fixed   # noqa: E402  (_env_loop and the budgets of the fixed-shape kernel)

SHAPE = fixed.SHAPE   # the headline capacity, 8 v 30 (BASELINE configs[1]): NS and VM_PER_ENV as for the fixed-shape kernel
# static SALU of the env loop, rare paths included: 358 at flatten=1 (the fixed-shape kernel: 309).  The additions are the two ballot
# popcounts of the live counts, the global reward's sum over a run-time count, and the reset's pending-count loads and id-cell refresh.
SALU_BUDGET = 370


def _asm(shape):
    from madrl_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    tu = ('#include "common.hpp"\n#include "pursuit_wave.hpp"\nnamespace madrl { namespace pw {\n'
          "template __global__ void pursuit_wave_kernel<LShape<%d, %d, %d, %d, %d, %d>, 1, false, false>(const WaveDev, const WaveIO);\n"
          "} }\n" % shape)
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "wave_live.hip"), os.path.join(tmp, "wave_live.s")
        with open(src, "w") as f:
            f.write(tu)
        subprocess.run([B.HIPCC] + [f for f in B.FLAGS if f != "-Wall"] + ["-I", B.CSRC, "--cuda-device-only", "-S", src, "-o", out],
                       check=True, capture_output=True)
        text = open(out).read()
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN5madrl2pw19pursuit_wave_kernelINS0_6LShape\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return text, lines[start:end]


@pytest.fixture(scope="module")
def live_asm():
    return _asm(SHAPE)


def test_live_kernel_is_listed_for_the_headline_capacity():
    text = open(os.path.join(ROOT, "madrl_amd", "csrc", "pursuit_live_specializations.def")).read()
    listed = {tuple(int(v) for v in m.group(1).split(",")) for m in re.finditer(r"^\s*XL\(([^)]*)\)", text, re.M)}
    assert SHAPE in listed and (16, 16, 8, 30, 7, 0) in listed


def test_live_env_loop_store_count(live_asm):
    loop = fixed._env_loop(live_asm[1])
    stores = [i for i in loop if re.match(r"global_store_\w+", i)]
    assert len(stores) == fixed.VM_PER_ENV, stores
    assert sum(1 for i in stores if i.startswith("global_store_dwordx4") and i.endswith(" nt")) == fixed.NS, stores


def test_live_env_loop_salu_budget(live_asm):
    loop = fixed._env_loop(live_asm[1])
    salu = [i for i in loop if i.startswith("s_") and not i.startswith(fixed.NOT_SALU)]
    assert len(salu) <= SALU_BUDGET, len(salu)


def test_live_no_scratch(live_asm):
    text = live_asm[0]
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", text)
    assert re.search(r"\.vgpr_spill_count:\s+0\b", text)
