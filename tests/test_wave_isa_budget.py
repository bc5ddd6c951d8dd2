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
import re

import pytest

import isa
from isa import NS, VM_PER_ENV

SALU_BUDGET = 320                # 309 since the observation pass builds its store masks on the vector unit (407 before)


@pytest.fixture(scope="module")
def kernel_asm():
    return isa.compile_asm(isa.HEADLINE_TU)


def test_env_loop_salu_budget(kernel_asm):
    salu = isa.salu(isa.wave_env_loop(kernel_asm, isa.HEADLINE, VM_PER_ENV))
    assert len(salu) <= SALU_BUDGET, "env loop: %d static SALU instructions, budget %d" % (len(salu), SALU_BUDGET)


def test_env_loop_store_count(kernel_asm):
    loop = isa.wave_env_loop(kernel_asm, isa.HEADLINE, VM_PER_ENV)
    stores = [i for i in loop if re.match(r"global_store_\w+", i)]
    assert len(stores) == VM_PER_ENV, stores
    assert sum(1 for i in stores if i.startswith("global_store_dwordx4") and i.endswith(" nt")) == NS, stores


def test_no_scratch(kernel_asm):
    meta = isa.kernel_meta(kernel_asm, isa.HEADLINE)
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
