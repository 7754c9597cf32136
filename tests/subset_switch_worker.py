"""Child process of tests/test_gpu_marker_subset.py::test_switches: solves case S1 of tests/marker_subset_ref.py (masks set) on the
time-eliminating path with whatever RSBA_* switches the environment carries (they are read at solver create) and saves what the
parent compares with the reference: the iteration log, the downloaded parameters, the RMS and which path ran (not profiled: the product
kernels run side by side on their streams unless a switch says otherwise).

    python tests/subset_switch_worker.py OUT.npz
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import marker_subset_ref as sref  # noqa: E402
from realsensecalibration_amd import capi  # noqa: E402


def main():
    cs = sref.case("S1")
    pr = capi.Problem.marker_chain(cs["prob"])
    for b, m in cs["masks"].items():
        pr.set_parameter_subset_constant(6 * b, m)
    s = capi.Solver(pr, capi.default_options(schur_impl=2))
    try:
        elim = s.eliminates_times()
        summ = s.run()
        s.download()
        _, rms = pr.reprojection_error()
        np.savez(sys.argv[1], log=s.iterations(), params=pr.params.copy(), rms=rms, elim=elim,
                 summary=np.array([summ.termination_type, summ.stop_reason, summ.num_iterations]), final_cost=summ.final_cost)
    finally:
        s.close()
        pr.close()


if __name__ == "__main__":
    main()
