#!/usr/bin/env python
"""Record tests/golden/hwcrowd_*.npz: the UNMODIFIED reference ContinuousHostageWorld at shapes beyond one wavefront's worth of particles
(more than 61 particles or 32 rescuers), which only the crowd kernel (madrl_amd/csrc/hostage_crowd.hip, `crowd=True`) runs.

The recorder is oracle/make_golden_hostage.run, as it is (teacher-forcing protocol and the herding that drives a scenario through key, gate,
hostages and bomb: see its docstring); this script only chooses the scenarios and the file names.  The files are named hwcrowd_*, not
hostage_*: the older hostage tests glob hostage_*.npz and build their envs without `crowd=True`.

    MADRL_REFERENCE_ROOT=/path/to/MADRL python scripts/record_hwcrowd_goldens.py [--check]

--check regenerates into a temporary directory and compares with the committed files byte for byte.

The recordings are used under one condition: the float32 oracle alone replays every recorded step within 1e-5 (a `<=` decided differently
in float32 than in float64 shows as an error far above that).  The seeds below meet it -- worst steps 2.8e-6, 9.6e-7 and 8.2e-6 -- and
tests/test_hostage_crowd_cpu.py asserts it; a scenario whose regenerated file does not gets another seed, named here.
"""
import importlib
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# name, constructor arguments, keyword arguments, episodes, steps, seed
SCENARIOS = [
    ("20_30_40", (20, 30, 40, 2, 1), dict(), 2, 45, 31),
    ("33_10_20_local", (33, 10, 20, 3, 1), dict(reward_mech="local", n_sensors=12, sensor_range=0.3, bad_speed=0.03), 2, 45, 32),
    ("8_64_100", (8, 64, 100, 1, 1), dict(n_sensors=20, action_scale=0.03, addid=False), 1, 60, 33),
]


def record(out_dir):
    """-> the files written into out_dir"""
    with tempfile.TemporaryDirectory() as tmp:
        os.environ["MADRL_GOLDEN_OUT"] = tmp   # read by make_golden_hostage when it is imported
        sys.path.insert(0, ROOT)
        from oracle import ref_loader
        from oracle import make_golden_hostage as mg
        assert mg.OUT == tmp, "oracle.make_golden_hostage was imported before MADRL_GOLDEN_OUT was set"
        ref_loader.load()
        H = importlib.import_module("madrl_environments.hostage")
        made = []
        for name, args, kw, episodes, steps, seed in SCENARIOS:
            mg.run(H, name, args, kw, episodes, steps, seed)
            dst = os.path.join(out_dir, "hwcrowd_%s.npz" % name)
            shutil.move(os.path.join(tmp, "hostage_%s.npz" % name), dst)
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
            print("%d hwcrowd golden files regenerate byte for byte" % len(SCENARIOS))
    else:
        for p in record(GOLDEN):
            print("%s  %.1f KB" % (os.path.relpath(p, ROOT), os.path.getsize(p) / 1024.0))


if __name__ == "__main__":
    main()
