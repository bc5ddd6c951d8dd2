#!/usr/bin/env python
"""Check that every file under tests/golden/ is what its generator writes TODAY when it runs the unmodified reference -- byte
for byte.  (The goldens are the anchor of every parity claim; this is the check that they are the reference's output and not
something edited afterwards.)  Needs a checkout of the reference, named by MADRL_REFERENCE_ROOT (oracle/ref_loader.py), so it is a
maintainer's script and not part of the test suite, which runs from the repository alone.  The one family left out is
multiwalker_box2d_*: it needs pybox2d (PARITY UNPINNED, tests/test_oracle_multiwalker_golden.py).

    MADRL_REFERENCE_ROOT=/path/to/MADRL python oracle/check_goldens.py
"""
import glob
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
GENERATORS = [("make_golden_reset_hist.py", []), ("make_golden_multiwalker.py", ["--envlayer"]), ("make_golden_pursuit.py", []), ("make_golden_pursuit_fuzz.py", []),
              ("make_golden_waterworld.py", []), ("make_golden_waterworld_fuzz.py", []), ("make_golden_hostage.py", []), ("make_golden_hostage_fuzz.py", []),
              ("make_golden_pursuit_evader.py", []), ("make_golden_callers.py", []), ("make_golden_wrappers.py", []), ("make_golden_heuristics.py", []),
              ("make_golden_curriculum.py", [])]


def main():
    if not ref_loader.reference_available():
        raise SystemExit("no reference tree at %s (set MADRL_REFERENCE_ROOT)" % ref_loader.REFERENCE_ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, MADRL_GOLDEN_OUT=tmp)

        def run(g):
            return g, subprocess.run([sys.executable, os.path.join(HERE, g[0])] + g[1], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)

        with ThreadPoolExecutor(4) as ex:
            for g, r in ex.map(run, GENERATORS):
                assert r.returncode == 0, "%s failed:\n%s" % (g[0], r.stderr[-2000:])
        made = sorted(os.path.basename(p) for p in glob.glob(os.path.join(tmp, "*")))
        have = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "*")))
        assert made == have, "generated but not committed: %s; committed but not generated: %s" % (sorted(set(made) - set(have)), sorted(set(have) - set(made)))
        differ = [n for n in made if open(os.path.join(tmp, n), "rb").read() != open(os.path.join(GOLDEN, n), "rb").read()]
        assert not differ, "regenerated files differ from the committed ones: %s" % differ
    print("%d golden files regenerate byte for byte" % len(made))


if __name__ == "__main__":
    main()
