#!/usr/bin/env python
"""Generate tests/golden/wwrange_*.npz: the UNMODIFIED reference MAWaterWorld run with one sensor range per pursuer (the array form of
`sensor_range`, waterworld.py:96, :109), recorded with the teacher-forcing protocol of oracle/make_golden_waterworld.py.

TEST INFRASTRUCTURE ONLY (needs the reference tree; the outputs are committed).  `run_scenario` records into a scratch directory -- its
files are named waterworld_*.npz and carry only the scalar cfg_sensor_range (element 0) -- and every file is saved again under
tests/golden/ as wwrange_<name>.npz with one added key, cfg_sensor_ranges (float64 [n_pursuers]).  The prefix matters: the tests of the
uniform kernels replay every waterworld_*.npz / wwcrowd_*.npz with the scalar range.

    python scripts/make_golden_waterworld_ranges.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden_waterworld as mg  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

# name -> (constructor args, constructor keywords without sensor_range, the ranges, run_scenario keywords)
SCENARIOS = {
    # one-wavefront shape (also run on the crowd kernel): four pursuers, four ranges
    "4_8_6_k12": ((4, 8, 2, 6), dict(n_sensors=12), (0.1, 0.35, 0.2, 0.5), dict(episodes=2, steps=60, seed=7, cluster=True)),
    # crowd-only shape (33 pursuers): the ranges cycle over three values
    "33_12_8_k8": ((33, 12, 2, 8), dict(n_sensors=8), tuple((0.15, 0.45, 0.3)[i % 3] for i in range(33)),
                   dict(episodes=1, steps=40, seed=11, cluster=True)),
}


def main():
    R = ref_loader.load()
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        mg.OUT = tmp
        for name, (args, kw, ranges, run) in SCENARIOS.items():
            ranges = np.asarray(ranges, dtype=np.float64)
            mg.run_scenario(R, name, args, dict(kw, sensor_range=ranges), **run)
            g = dict(np.load(os.path.join(tmp, "waterworld_%s.npz" % name)))
            assert ranges.shape == (int(g["cfg_n_pursuers"]),) and float(g["cfg_sensor_range"]) == ranges[0]
            g["cfg_sensor_ranges"] = ranges
            path = os.path.join(OUT, "wwrange_%s.npz" % name)
            np.savez_compressed(path, **g)
            print("%s  %.1f KB" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
