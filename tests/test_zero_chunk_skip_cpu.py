"""CPU test (-m "not gpu"): the headline instantiation of the one-wavefront Pursuit step kernel with the "zeros over known zeros" rule
(pursuit_wave.hpp, Shape::ZSKIP) still fits the 96 vector registers of five wavefronts per SIMD, and the pricing build of the rule
(MADRL_ABLATE bit 1024) compiles.  What the env loop issues is tests/test_wave_isa_budget.py's business; this file reads the kernel's
metadata only."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_wave_isa_budget import TU   # the same translation unit: the headline instantiation alone


def _compile(extra):
    from madrl_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "wave_headline.hip"), os.path.join(tmp, "wave_headline.s")
        with open(src, "w") as f:
            f.write(TU)
        subprocess.run([B.HIPCC] + [f for f in B.FLAGS if f != "-Wall"] + extra + ["-I", B.CSRC, "--cuda-device-only", "-S", src, "-o", out],
                       check=True, capture_output=True)
        return open(out).read()


def _meta(text, key):
    vals = re.findall(r"\.%s:\s+(\d+)" % key, text)
    assert len(vals) == 1, (key, vals)
    return int(vals[0])


def test_headline_kernel_keeps_96_vgprs_and_no_scratch():
    text = _compile([])
    assert _meta(text, "vgpr_count") <= 96
    assert _meta(text, "vgpr_spill_count") == 0 and _meta(text, "private_segment_fixed_size") == 0


def test_pricing_build_compiles():
    text = _compile(["-DMADRL_ABLATE=1024"])
    assert _meta(text, "vgpr_count") <= 96   # (five wavefronts per SIMD: the build is timed against the shipped kernel)
