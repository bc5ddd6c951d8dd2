"""The state-buffer layout of a MultiWalker handle (madrl_amd/csrc/multiwalker_layout.hpp: mw_layout) on a CPU, under the sanitizers.

tests/host/multiwalker_layout_check.cpp, compiled once per capacity class, checks for every n_walkers the class holds, one_hot 0 and 1 and
n_envs in {1, 15, 16, 17, 16 384} that the regions of the buffer lie in order and disjoint, start aligned (records, spare records and spare
observations to 16 bytes, the dword arrays to 4), that step_count is the third of the four trailing dwords and that the last region ends
exactly at `total`; it prints every total.  Those totals, and what madrl_multiwalker_state_bytes answers for the same grid (no device is
needed for that call), must be the sizes in BYTES below: recorded from the library as it stood when state_bytes summed the regions in one
expression and create() carved them with a running pointer.  They are what callers allocate and checkpoints hold.
"""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "multiwalker_layout_check.cpp")
CLASSES = {4: 4, 8: 8, 10: 16}            # walkers a class has room for -> lanes per env (multiwalker_c4 / _c8 / _c10.hip)
N_ENVS = (1, 15, 16, 17, 16384)
BYTES = {   # (n_walkers, one_hot) -> madrl_multiwalker_state_bytes at each of N_ENVS
    (1, 0): (31500, 472052, 503520, 535004, 515588112),
    (1, 1): (31660, 474404, 506016, 537660, 518144016),
    (2, 0): (33868, 507572, 541408, 575260, 554385424),
    (2, 1): (34188, 512260, 546400, 580572, 559497232),
    (3, 0): (36236, 543092, 579296, 615516, 593182736),
    (3, 1): (36716, 550116, 586784, 623484, 600850448),
    (4, 0): (37484, 561812, 599264, 636732, 613629968),
    (4, 1): (38108, 571172, 609248, 647340, 623853584),
    (5, 0): (65068, 975572, 1040608, 1105660, 1065566224),
    (5, 1): (65852, 987284, 1053088, 1118924, 1078345744),
    (6, 0): (66860, 1002452, 1069280, 1136124, 1094926352),
    (6, 1): (67804, 1016500, 1084256, 1152044, 1110261776),
    (7, 0): (68684, 1029812, 1098464, 1167132, 1124810768),
    (7, 1): (69788, 1046196, 1115936, 1185708, 1142702096),
    (8, 0): (70476, 1056692, 1127136, 1197596, 1154170896),
    (8, 1): (71724, 1075412, 1147104, 1218812, 1174618128),
    (9, 0): (86604, 1298612, 1385184, 1471772, 1418412048),
    (9, 1): (88012, 1319684, 1407648, 1495644, 1441415184),
    (10, 0): (88396, 1325492, 1413856, 1502236, 1447772176),
    (10, 1): (89964, 1348900, 1438816, 1528764, 1473331216),
}


def _class_of(n_walkers):
    """the smallest class that holds n_walkers: the one madrl_multiwalker_state_bytes answers for"""
    return min(c for c in CLASSES if n_walkers <= c)


@pytest.mark.parametrize("cap", sorted(CLASSES))
def test_layout_is_ordered_aligned_and_the_recorded_size(cap, tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / ("multiwalker_layout_check_c%d" % cap))
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-DMW_CAPW=%d" % cap, "-DMW_NLANES=%d" % CLASSES[cap], SRC, "-o", exe]
    # the sanitizer runtimes linked statically where the compiler has the option (gcc links them dynamically by default, and a dynamic
    # runtime refuses to start behind any other preloaded library)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True, cwd=ROOT)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)   # directly: nothing is preloaded for it
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(v) for v in l.split()) for l in r.stdout.splitlines()]
    assert [row[:3] for row in rows] == [(w, oh, n) for w in range(1, cap + 1) for oh in (0, 1) for n in N_ENVS], "the whole grid, once"
    mine = [row for row in rows if _class_of(row[0]) == cap]   # (a walker count below the class's own range: checked above, never dispatched here)
    assert len(mine) == 10 * sum(_class_of(w) == cap for w in range(1, 11))
    for w, oh, n, total, world_dw in mine:
        assert total == BYTES[w, oh][N_ENVS.index(n)], "n_walkers %d one_hot %d n_envs %d" % (w, oh, n)
        assert world_dw % 4 == 0   # record_stride, whole 16-byte words


def test_state_bytes_answers_the_recorded_sizes():
    from madrl_amd import _lib
    L = _lib.lib()
    for (w, oh), want in sorted(BYTES.items()):
        cfg = _lib.MultiWalkerConfig()
        cfg.struct_size = C.sizeof(_lib.MultiWalkerConfig)
        cfg.n_walkers, cfg.one_hot = w, oh
        for n, bytes_ in zip(N_ENVS, want):
            total = C.c_uint64()
            _lib.check(L.madrl_multiwalker_state_bytes(C.byref(cfg), n, C.byref(total)))
            assert total.value == bytes_, "n_walkers %d one_hot %d n_envs %d" % (w, oh, n)
    # the anchors at n_envs = 17
    at17 = lambda w, oh: BYTES[w, oh][N_ENVS.index(17)]
    assert (at17(3, 0), at17(4, 1), at17(5, 0), at17(8, 1), at17(10, 0), at17(10, 1)) == (615516, 647340, 1105660, 1218812, 1502236, 1528764)
