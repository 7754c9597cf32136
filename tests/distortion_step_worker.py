"""Child process of tests/test_gpu_marker_distortion.py: one step case of its table with whatever RSBA_* switches the environment
carries (they are read when a solver is created), the device's outputs saved for the parent's numpy side.
usage: distortion_step_worker.py CASE OUT.npz"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import marker_step_accuracy as msa  # noqa: E402
import test_gpu_marker_distortion as t  # noqa: E402


def main():
    case = {c.name: c for c in msa.CASES}[sys.argv[1]]
    dev = t.step_pair(case)
    np.savez(sys.argv[2], start=dev["start"], x1=dev["x1"], log=dev["log"], elim=dev["elim"], stats=json.dumps(dev["stats"]), x1_again=dev["x1_again"],
             log_again=dev["log_again"])


if __name__ == "__main__":
    main()
