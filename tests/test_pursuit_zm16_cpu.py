"""The 16-bit-per-lane stale-zero mask format of the one-wavefront Pursuit kernel (madrl_amd/csrc/pursuit_zm16.hpp) on a CPU, under the sanitizers.

tests/host/pursuit_zm16_check.cpp evaluates the format's predicate for every committed X line and, for every line that has the format and
every lane, round-trips pack / unpack over the lane's useful bits (every subset, single bits, all ones, all zeros, 4 096 seeded random
words), checks pack(all ones) == 0xFFFF, pack(0) == 0 and the premises (at most four useful slots, the dropped slot is not useful).  The
predicate column must equal tests/fixtures/pursuit_zm16_shapes.txt: true for every flattened line except 13 v 51 (8 slots per lane, six useful).
A new X line adds a line to the output: decide its verdict by hand (flatten, at most 5 slots per lane, at most 4 of them with a channel-1 / 2
cell) and append it to the fixture.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "pursuit_zm16_check.cpp")
EXPECTED = os.path.join(ROOT, "tests", "fixtures", "pursuit_zm16_shapes.txt")


def test_zm16_round_trip_and_predicate_sanitizer_clean(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pursuit_zm16_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe]
    # the sanitizer runtimes linked statically where the compiler has the option (as tests/test_pursuit_tables_cpu.py does)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True, cwd=ROOT)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)   # its own executable: nothing is preloaded
    assert r.returncode == 0, r.stderr
    got, want = r.stdout.splitlines(), open(EXPECTED).read().splitlines()
    assert len(want) >= 14
    verdicts = ["%s %s" % (l.split()[0], [f for f in l.split() if f.startswith("zm16=")][0]) for l in got]
    assert verdicts == want
    # every line that has the format went through the round trips: every subset (at most 2^16) + single bits + 4 096 random words, per lane
    checked = [l for l in got if "zm16=1" in l]
    assert len(checked) == sum("zm16=1" in w for w in want) >= 8
    for l in checked:
        assert int(l.split("words=")[1]) >= 64 * 4096
    # the headline shape drops a slot (5 slots per lane, 4 useful)
    assert got[0].startswith("X(16,16,8,30,7,1) slots=5 useful=4 zm16=1")
