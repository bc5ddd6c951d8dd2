"""The Pursuit kernels' host-built tables (madrl_amd/csrc/pursuit_tables.hpp) on a CPU, under the sanitizers.

tests/host/pursuit_tables_check.cpp runs both builders (the generic kernel's byte image, the wave / group kernels' dword image) and the
eligibility rules over a fixed list of configurations: every committed X / XG line with its line's geometry, even obs_range, no id, obs_range 1,
three maps, two configurations that are not eligible and a map with a bad cell.  Its output -- sizes, offsets, fstride, the verdict, a hash of
each image -- must equal tests/fixtures/pursuit_tables_expected.txt, which was recorded from the table code as it stood inside
madrl_pursuit_create (moved into the two functions verbatim) before it was simplified.  A new line in pursuit_specializations.def adds a line
to the output: run the program and append that line to the fixture.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "pursuit_tables_check.cpp")
EXPECTED = os.path.join(ROOT, "tests", "fixtures", "pursuit_tables_expected.txt")


def test_tables_are_the_recorded_ones_and_sanitizer_clean(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pursuit_tables_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe]
    # the sanitizer runtimes linked statically where the compiler has the option (gcc links them dynamically by default, and a dynamic
    # runtime refuses to start behind any other preloaded library)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True, cwd=ROOT)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)   # directly: nothing is preloaded for it
    assert r.returncode == 0, r.stderr
    got, want = r.stdout.splitlines(), open(EXPECTED).read().splitlines()
    assert len(want) >= 25
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
    # what the issue's list asks of the output itself
    lines = [l for l in got if l.startswith(("X ", "XG "))]
    assert len(lines) >= 17 and all("eligible=1" in l for l in lines)
    assert sum("eligible=0" in l for l in got) == 2
    assert got[-1].endswith("bad cell map=1 x=1 y=2 value=1")
