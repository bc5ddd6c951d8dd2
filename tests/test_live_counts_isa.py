"""CPU test (-m "not gpu"): the live-count instantiation of the headline shape (per-env agent counts, LShape in pursuit_wave.hpp) keeps the
contracts of the fixed-shape step kernel (tests/test_wave_isa_budget.py): no scratch, no VGPR spills, exactly VM_PER_ENV stores in the env
loop -- the stores of observation rows past an env's live pursuer count stay issued with an empty exec mask -- and one exact
s_waitcnt vmcnt(VM_PER_ENV) for the record prefetch."""
import re

import pytest

import isa
from isa import NS, SHAPE, VM_PER_ENV   # the headline capacity, 8 v 30 (BASELINE configs[1]): NS and VM_PER_ENV as for the fixed-shape kernel

# static SALU of the env loop, rare paths included: 358 at flatten=1 (the fixed-shape kernel: 309).  The additions are the two ballot
# popcounts of the live counts, the global reward's sum over a run-time count, and the reset's pending-count loads and id-cell refresh.
SALU_BUDGET = 370
LIVE = isa.wave_kernel("LShape", SHAPE)
TU = ('#include "common.hpp"\n#include "pursuit_wave.hpp"\nnamespace madrl { namespace pw {\n'
      "template __global__ void pursuit_wave_kernel<LShape<%d, %d, %d, %d, %d, %d>, 1, false, false>(const WaveDev, const WaveIO);\n"
      "} }\n" % SHAPE)


@pytest.fixture(scope="module")
def live_asm():
    return isa.compile_asm(TU)


def test_live_kernel_is_listed_for_the_headline_capacity():
    listed = isa.def_lines("pursuit_live_specializations.def", ("XL",))["XL"]
    assert SHAPE in listed and (16, 16, 8, 30, 7, 0) in listed


def test_live_env_loop_store_count(live_asm):
    loop = isa.wave_env_loop(live_asm, LIVE, VM_PER_ENV)
    stores = [i for i in loop if re.match(r"global_store_\w+", i)]
    assert len(stores) == VM_PER_ENV, stores
    assert sum(1 for i in stores if i.startswith("global_store_dwordx4") and i.endswith(" nt")) == NS, stores


def test_live_env_loop_salu_budget(live_asm):
    salu = isa.salu(isa.wave_env_loop(live_asm, LIVE, VM_PER_ENV))
    assert len(salu) <= SALU_BUDGET, len(salu)


def test_live_no_scratch(live_asm):
    meta = isa.kernel_meta(live_asm, LIVE)
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
