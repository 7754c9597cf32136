"""Child process of tests/test_gpu_marker_intrinsics_elim.py: the RSBA_MT_* switches are read from the environment when a solver is
created, so every setting gets a process of its own.  Solves one case of tests/marker_intrinsics_ref.py with free intrinsics under
schur_impl = 3 and writes what the parent compares into an .npz file.

usage: marker_intr_elim_worker.py CASE OUT.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import marker_intrinsics_ref as iref   # noqa: E402
import test_gpu_marker_intrinsics as dense   # noqa: E402


def main():
    name, path = sys.argv[1], sys.argv[2]
    cs = iref.case(name)
    out = dense._solve(cs, 3, profile=True)
    s = out["summary"]
    np.savez(path, params=out["params"], intr=out["intr"], dist=out["dist"], log=out["log"], rms=out["rms"], rms_solver=out["rms_solver"], elim=out["elim"],
             summary=np.array([s.termination_type, s.stop_reason, s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps], np.int64),
             costs=np.array([s.initial_cost, s.final_cost]), kernels=np.array(sorted(out["stats"])))


if __name__ == "__main__":
    main()
