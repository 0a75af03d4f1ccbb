"""Generates tests/golden/otg3_core_vectors.npz: seeded cases of the jerk-limited OTG core (brake pre-trajectory, step 1, step 2 at three
durations) and the REFERENCE's answers on them -- its vendored Ruckig 0.10.1 classes, through `oracle/_ref/otg3_compare --record N` (built by
`make -C oracle ref`).  tests/test_otg_reference.py runs the product's core (tests/cpp/otg3_vectors.cpp) on the stored cases and compares.

    python tests/golden/make_otg3_golden.py            # rewrites tests/golden/otg3_core_vectors.npz (needs the reference build)"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
N_CASES = 800          # 100 of each of the 8 kinds of start / goal state
CASE, RECORD = 12, 173
PATH = os.path.join(HERE, "otg3_core_vectors.npz")


def main():
    import otg_ref
    if otg_ref.build() is None or not os.path.exists(otg_ref.COMPARE):
        raise SystemExit("the reference build oracle/_ref/otg3_compare is not available")
    raw = subprocess.run([otg_ref.COMPARE, "--record", str(N_CASES)], capture_output=True, check=True, timeout=300).stdout
    a = np.frombuffer(raw, np.float64).reshape(N_CASES, CASE + RECORD)
    np.savez_compressed(PATH, cases=a[:, :CASE], records=a[:, CASE:])
    print(PATH, a.shape)


if __name__ == "__main__":
    main()
