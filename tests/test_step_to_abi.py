"""madrl_pursuit_step_to: the ABI entries and the list of two-buffer specialisations (no GPU needed)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madrl_amd", "csrc")

REQUIRED = {
    "X": [(16, 16, 8, 30, 7, 1), (16, 16, 8, 30, 7, 0), (10, 10, 2, 2, 3, 1), (6, 6, 3, 5, 11, 0)],
    "XC": [(24, 24, 20, 300, 9, 1, 1), (48, 48, 100, 300, 21, 0, 8), (128, 128, 100, 300, 21, 0, 16)],
    "XL": [(16, 16, 8, 30, 7, 1)],
    "XLC": [(24, 24, 20, 300, 9, 1, 1)],
}


def _lines(name):
    out = {}
    for m in re.finditer(r"^\s*(X[A-Z]*)\(([^)]*)\)", open(os.path.join(CSRC, name)).read(), re.M):
        out.setdefault(m.group(1), []).append(tuple(int(v) for v in m.group(2).split(",")))
    return out


def test_signatures_and_abi_version():
    from madrl_amd import _lib
    assert "madrl_pursuit_step_to" in _lib.SIGNATURES and len(_lib.SIGNATURES["madrl_pursuit_step_to"][1]) == 9
    assert "madrl_pursuit_step_to_kernel_kind" in _lib.SIGNATURES and len(_lib.SIGNATURES["madrl_pursuit_step_to_kernel_kind"][1]) == 2
    assert _lib.ABI_VERSION == 8
    if os.path.exists(_lib.SO_PATH):
        assert _lib.lib().madrl_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "madrl_hip.h")).read()
    assert re.search(r"int\s+madrl_pursuit_step_to\s*\(", header) and re.search(r"int\s+madrl_pursuit_step_to_kernel_kind\s*\(", header)


def test_committed_two_buffer_lines_stand_on_fast_lines():
    to = _lines("pursuit_to_specializations.def")
    for kind, shapes in REQUIRED.items():
        for s in shapes:
            assert s in to.get(kind, []), (kind, s)
    fixed = _lines("pursuit_specializations.def").get("X", [])
    crowd = _lines("pursuit_crowd_specializations.def").get("XC", [])
    live = _lines("pursuit_live_specializations.def")
    for s in to.get("X", []) + to.get("XL", []):
        assert s in fixed, s
    for s in to.get("XC", []) + to.get("XLC", []):
        assert s in crowd, s   # (the same NW: the tuple holds it)
    for s in to.get("XL", []):
        assert s in live.get("XL", []), s
    for s in to.get("XLC", []):
        assert s in live.get("XLC", []), s


def test_pursuit_to_lines():
    from madrl_amd import build
    assert build.pursuit_to_lines(16, 16, 8, 30, 7, 1) == ("X(16, 16, 8, 30, 7, 1)", "X(16, 16, 8, 30, 7, 1)")
    assert build.pursuit_to_lines(128, 128, 100, 300, 21, 0) == ("XC(128, 128, 100, 300, 21, 0, 16)", "XC(128, 128, 100, 300, 21, 0, 16)")
    line, why = build.pursuit_to_lines(32, 32, 16, 60, 7, 1)        # BASELINE C5: the multi-wavefront kernel
    assert line is None and "multi-wavefront" in why
    line, why = build.pursuit_to_lines(16, 16, 8, 30, 6, 1)         # even obs_range: no fast path at all
    assert line is None and "even obs_range" in why


@pytest.mark.parametrize("shape,reason", [((32, 32, 16, 60, 7, 1), "multi-wavefront"), ((16, 16, 8, 30, 6, 1), "even obs_range")])
def test_build_refuses_a_shape_without_an_x_or_xc_fast_path(shape, reason):
    """python -m madrl_amd.build --pursuit-to-shape: refused with the reason, before anything is written or compiled"""
    local = os.path.join(CSRC, "pursuit_to_specializations.local.def")
    had = os.path.exists(local)
    r = subprocess.run([sys.executable, "-m", "madrl_amd.build", "--pursuit-to-shape"] + [str(v) for v in shape], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode != 0
    assert "no two-buffer fast kernel" in r.stdout and reason in r.stdout
    assert os.path.exists(local) == had
