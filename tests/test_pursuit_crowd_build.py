"""CPU tests (-m "not gpu") of the PursuitEvade crowd kernel's build side: which shapes madrl_amd.build.pursuit_crowd_path accepts and how a
shape is added, and invariants of the BUILT gfx950 kernels (one per XC line and mode, no private segment, LDS inside a workgroup's 160 KiB)."""
import os

import pytest

import isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEF = os.path.join(ROOT, "madrl_amd", "csrc", "pursuit_crowd_specializations.def")
COMMITTED = {(128, 128, 100, 300, 21, 0): 16,   # the authors' CNN launch line (runners/old/rllab/pursuit_cnn.sh:1)
             (24, 24, 20, 300, 9, 1): 1, (20, 20, 260, 40, 5, 1): 2, (24, 24, 70, 90, 9, 1): 2,   # the recorded goldens above 64 of a kind
             (48, 48, 100, 300, 21, 0): 8}


def _lines():
    return isa.def_lines("pursuit_crowd_specializations.def", ("XC",))["XC"]


def test_which_shapes_can_have_a_crowd_kernel_and_how_they_are_added(tmp_path, monkeypatch):
    from madrl_amd import build as b
    lines = _lines()
    for shape, nw in COMMITTED.items():
        assert b.pursuit_crowd_path(*shape) == ("XC", nw), shape
        assert shape + (nw,) in lines, shape
    for v in lines:   # every committed line passes its own check
        assert b.pursuit_crowd_path(*v[:6]) == ("XC", v[6]), v
    for shape, kw, why in (((24, 24, 70, 90, 8, 1), {}, "even"), ((24, 24, 70, 90, 9, 1), dict(include_id=False), "flatten without the id"),
                           ((250, 250, 100, 300, 21, 0), {}, "LDS"), ((256, 20, 100, 300, 5, 1), {}, "255"),
                           ((20, 256, 100, 300, 5, 1), {}, "255"), ((64, 64, 1024, 30, 5, 1), {}, "1 023")):
        kind, reason = b.pursuit_crowd_path(*shape, **kw)
        assert kind is None and why in reason, (shape, reason)
    # the one-wavefront / group fast paths keep refusing what they refused
    kind, reason = b.pursuit_fast_path(128, 128, 100, 300, 21, 0)
    assert kind is None and "more than 64" in reason
    assert b.pursuit_live_lines(128, 128, 100, 300, 21, 0) is None
    # the LDS the build tool computes is the LDS the kernel declares (CShape::LDS_DWORDS): 21 904 cells and 400 agents
    assert b.pursuit_crowd_lds_bytes(128, 128, 100, 300, 21, 0) == 91232
    # appending: a new shape lands in the local file once, a committed one not at all
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    (csrc / "pursuit_crowd_specializations.def").write_text(open(DEF).read())
    monkeypatch.setattr(b, "CSRC", str(csrc))
    assert b.add_pursuit_crowd_shape(64, 64, 80, 200, 11, 1) is True and b.add_pursuit_crowd_shape(64, 64, 80, 200, 11, 1) is False
    assert b.add_pursuit_crowd_shape(128, 128, 100, 300, 21, 0) is False
    assert (csrc / "pursuit_crowd_specializations.local.def").read_text().startswith("XC(64, 64, 80, 200, 11, 1, 2)")
    assert len((csrc / "pursuit_crowd_specializations.local.def").read_text().splitlines()) == 1
    with pytest.raises(ValueError):
        b.add_pursuit_crowd_shape(24, 24, 70, 90, 8, 1)
    for src in ("pursuit.hip", "pursuit_crowd.hip"):
        assert "pursuit_crowd_specializations.local.def" in open(os.path.join(ROOT, "madrl_amd", "csrc", src)).read()


def test_built_crowd_kernels():
    from madrl_amd import build as b
    ks = {n: k for n, k in isa.built_kernels().items() if "pursuit_crowd_kernel" in n}
    lines = _lines()
    assert len(lines) >= 5 and len(ks) >= 2 * len(lines)
    for v in lines:
        for mode in (0, 1):   # reset launch, step launch
            name = isa.crowd_kernel(v, mode)
            assert name in ks, name
            k = ks[name]
            assert k["scratch"] == 0, (name, k)   # no private segment: a spill store of these store-bound kernels would reach HBM
            assert k["vgprs"] <= 512 // max(64 * v[6] // 256, 1), (name, k)   # the workgroup's wavefronts fit the SIMDs' register files
            assert k["lds"] <= 163840 and k["lds"] == b.pursuit_crowd_lds_bytes(*v[:6]), (name, k["lds"])
            (o0, s0), (o1, _s1) = k["args"][:2]   # two by-value arguments: CrowdDev, then CrowdIO
            assert o0 == 0 and o1 == (s0 + 7) // 8 * 8, (name, k["args"])
