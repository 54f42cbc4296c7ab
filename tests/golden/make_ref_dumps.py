"""Fixture generator: the reference binary's dumps for the tests that compare against it (tests/util.py reference_case), as DATA.

Run where the reference sources are present (build() then compiles oracle/_ref/ref_driver):   python tests/golden/make_ref_dumps.py
Writes tests/golden/ref_dumps/<side>_<name>.npz: the input positions / velocities (to catch a drifting generator) and, for every dumped
step, the 16 energy fields and x, y, z, vx, vy, vz, fx, fy, fz.  No reference source code is stored.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import casefile, oracle     # noqa: E402
from util import REF_CPU, REF_GPU, reference_case, reference_fixture_path     # noqa: E402


def main():
    oracle.build()
    assert oracle.ref_available(), "oracle/_ref/ref_driver is missing: the reference sources are needed to regenerate these fixtures"
    for side, names in (("cpu", REF_CPU), ("gpu", REF_GPU)):
        for name in names:
            case = reference_case(side, name)
            ref = oracle.run_ref(case)
            out = {"in_" + k: np.asarray(case[k], dtype=np.float64) for k in ("x", "y", "z", "vx", "vy", "vz")}
            steps = sorted(ref["dumps"])
            out["steps"] = np.array(steps, dtype=np.int64)
            for st in steps:
                d = ref["dumps"][st]
                out["e_%d" % st] = np.array([d[k] for k in casefile.ENERGY_FIELDS], dtype=np.float64)
                for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
                    out["%s_%d" % (k, st)] = d[k]
            path = reference_fixture_path(side, name)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.savez_compressed(path, **out)
            print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
