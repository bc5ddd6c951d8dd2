"""The 32-bit edges of the RNG counter words without a GPU (the GPU side: tests/test_wide_counters_gpu.py, which trusts the oracles there).

  * PursuitEvade: tests/host/pursuit_wide_check.cpp holds the kernels' shared rules (madrl_amd/csrc/pursuit_rules.hpp) against the C
    oracle's independent statement of them -- as tests/test_pursuit_rules_cpu.py does at small values -- for global env indices on both
    sides of 2^31 and up to 2^32 - 2 and ticks that cross 2^31 and wrap at 2^32, under the sanitizers (a signed overflow in either
    statement is an error there, not a wrap).
  * MultiWalker: the CPU build of the product's source against the independent restatement oracle/multiwalker_ref.c at
    env_id_base = 2^32 - 1 - N, the largest the library accepts, and across 2^31; the base must reach the terrain draws."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "pursuit_wide_check.cpp")
ORACLE = os.path.join(ROOT, "oracle", "pursuit_oracle.c")
FLOAT_FLAGS = ["-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile: every double operation rounds on its own, as NumPy's do
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_pursuit_rules_equal_the_oracle_at_wide_env_ids_and_ticks(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    cc = next((c for c in (os.environ.get("CC"), "gcc", "cc", "clang") if c and shutil.which(c)), None)
    if cxx is None or cc is None:
        pytest.skip("no host C / C++ compiler")
    assert "pursuit_rules" not in open(ORACLE).read()   # the oracle stays the independent statement
    obj, exe = str(tmp_path / "pursuit_oracle.o"), str(tmp_path / "pursuit_wide_check")
    subprocess.run([cc, "-std=gnu11", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unknown-pragmas"] + SAN + FLOAT_FLAGS + ["-c", ORACLE, "-o", obj],
                   check=True, cwd=ROOT)
    cmd = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas"] + SAN + FLOAT_FLAGS + [SRC, obj, "-o", exe, "-lm"]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True, cwd=ROOT)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)   # directly: nothing is preloaded for it
    assert r.returncode == 0, r.stderr
    got = dict(l.split(" ", 1) for l in r.stdout.splitlines())
    assert set(got) == {"f", "g", "h"}, r.stdout
    assert "ticks=4294967295,0 " in got["g"] and "base=4294967231 " in got["g"], got["g"]


@pytest.mark.parametrize("n_walkers", [3, 7, 10])   # the three capacity classes (4, 8 and 16 lanes per env)
@pytest.mark.parametrize("which", ["largest", "straddles_2^31"])
def test_multiwalker_cpu_build_equals_the_independent_restatement_at_wide_env_ids(n_walkers, which):
    from oracle import multiwalker as mwo
    from oracle import multiwalker_ref as mwr
    W, N, T = n_walkers, 16, 60
    base = 2**32 - 1 - N if which == "largest" else 2**31 - N // 2
    kw = dict(n_walkers=W, n_envs=N, seed=8, position_noise=0, angle_noise=0)
    ref, core = mwr.MultiWalkerRef(env_id_base=base, poly=True, **kw), mwo.MultiWalkerOracle(env_id_base=base, lanes_descending=True, **kw)
    ref.reset(); core.reset()
    assert np.array_equal(ref.terrain(), core.terrain())
    low = mwo.MultiWalkerOracle(env_id_base=base - 2**31, **kw)   # the same indices without bit 31
    low.reset()
    assert not np.array_equal(low.terrain(), core.terrain()), "bit 31 of the global env index does not reach the terrain draws"
    assert len({core.terrain()[n].tobytes() for n in range(N)}) == N, "two envs drew the same terrain"
    rng = np.random.RandomState(4)
    n_done = 0
    for t in range(T):
        a = rng.uniform(-1, 1, (N, W, 4)).astype(np.float32)
        if t % 30 > 14:   # limp walkers collapse: episodes end, and reset(mask=) draws the next terrain at these env ids
            a[:] = 0
        _ro, _rr, rd = ref.step(a)
        _co, _cr, cd = core.step(a)
        assert np.array_equal(ref.bodies(), core.bodies()[0]) and np.array_equal(rd, cd), t
        if rd.any():
            ref.reset(mask=rd); core.reset(mask=rd)
            assert np.array_equal(ref.terrain(), core.terrain()), t
            n_done += int(rd.sum())
    assert n_done > 0, "no episode ended: reset(mask=) was never compared"
    assert not core.overflow().any()
