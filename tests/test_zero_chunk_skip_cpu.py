"""CPU test (-m "not gpu"): the headline instantiation of the one-wavefront Pursuit step kernel with the "zeros over known zeros" rule
(pursuit_wave.hpp, Shape::ZSKIP) still fits the 96 vector registers of five wavefronts per SIMD, and the pricing build of the rule
(MADRL_ABLATE bit 1024) compiles.  What the env loop issues is tests/test_wave_isa_budget.py's business; this file reads the kernel's
metadata only."""
import isa
from isa import HEADLINE, HEADLINE_TU, HEADLINE_VGPRS   # the same translation unit as tests/test_wave_isa_budget.py: the headline instantiation alone


def test_headline_kernel_keeps_96_vgprs_and_no_scratch():
    meta = isa.kernel_meta(isa.compile_asm(HEADLINE_TU), HEADLINE)
    assert meta["vgpr_count"] <= HEADLINE_VGPRS
    assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0


def test_pricing_build_compiles():
    meta = isa.kernel_meta(isa.compile_asm(HEADLINE_TU, ["-DMADRL_ABLATE=1024"]), HEADLINE)
    assert meta["vgpr_count"] <= HEADLINE_VGPRS   # (five wavefronts per SIMD: the build is timed against the shipped kernel)
