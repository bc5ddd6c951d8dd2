#!/usr/bin/env python
"""Record tests/golden/wwcrowd_*.npz: the UNMODIFIED reference MAWaterWorld at shapes beyond one wavefront's worth of particles (more
than 62 particles or 32 pursuers), which only the crowd kernel (madrl_amd/csrc/waterworld_crowd.hip, `crowd=True`) runs.

The recorder is oracle/make_golden_waterworld.run_scenario, as it is (teacher-forcing protocol, see its docstring); this script only
chooses the scenarios and the file names.  The files are named wwcrowd_*, not waterworld_*: the older Waterworld tests glob
waterworld_*.npz and build their envs without `crowd=True`.

    MADRL_REFERENCE_ROOT=/path/to/MADRL python scripts/record_wwcrowd_goldens.py [--check]

--check regenerates into a temporary directory and compares with the committed files byte for byte.

The seeds were chosen so that the float32 oracle alone replays every recorded step within 1e-5 (a `<=` decided differently in float32
than in float64 shows as an error far above that: seed 13 of the third scenario has one such step and is not used).
"""
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# name, constructor arguments, keyword arguments, steps, seed
SCENARIOS = [
    ("20_60_40", (20, 60, 2, 40), dict(), 40, 11),
    ("40_30_20", (40, 30, 3, 20), dict(obstacle_loc=None, reward_mech="global", n_sensors=12), 40, 12),
    ("33_100_100", (33, 100, 1, 100), dict(n_sensors=20, ev_speed=0.05, radius=0.02), 30, 21),
]


def record(out_dir):
    """-> the files written into out_dir"""
    with tempfile.TemporaryDirectory() as tmp:
        os.environ["MADRL_GOLDEN_OUT"] = tmp   # read by make_golden_waterworld when it is imported
        sys.path.insert(0, ROOT)
        from oracle import ref_loader
        from oracle import make_golden_waterworld as mg
        assert mg.OUT == tmp, "oracle.make_golden_waterworld was imported before MADRL_GOLDEN_OUT was set"
        R = ref_loader.load()
        made = []
        for name, args, kw, steps, seed in SCENARIOS:
            mg.run_scenario(R, name, args, kw, episodes=1, steps=steps, seed=seed, action_kind="uniform", cluster=True)
            dst = os.path.join(out_dir, "wwcrowd_%s.npz" % name)
            shutil.move(os.path.join(tmp, "waterworld_%s.npz" % name), dst)
            made.append(dst)
    return made


def main():
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as chk:
            differ = []
            for p in record(chk):
                committed = os.path.join(GOLDEN, os.path.basename(p))
                if not os.path.exists(committed) or open(p, "rb").read() != open(committed, "rb").read():
                    differ.append(os.path.basename(p))
            if differ:
                raise SystemExit("regenerated files differ from the committed ones: %s" % differ)
            print("%d wwcrowd golden files regenerate byte for byte" % len(SCENARIOS))
    else:
        for p in record(GOLDEN):
            print("%s  %.1f KB" % (os.path.relpath(p, ROOT), os.path.getsize(p) / 1024.0))


if __name__ == "__main__":
    main()
