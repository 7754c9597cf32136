"""Child process of tests/test_gpu_marker_prior.py::test_switches: solves case P1 of tests/marker_prior_ref.py (priors set) on the
time-eliminating path with whatever RSBA_* switches the environment carries (they are read at solver create) and saves what the
parent compares with the reference: the iteration log, the downloaded parameters, the RMS and which path ran (not profiled: the product
kernels run side by side on their streams unless a switch says otherwise) — and then, from one more run of a single profiled iteration
on the same solver, the names of the kernels it launched.

    python tests/prior_switch_worker.py OUT.npz
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import marker_prior_ref as pref  # noqa: E402
from realsensecalibration_amd import capi  # noqa: E402


def main():
    cs = pref.case("P1")
    pr = capi.Problem.marker_chain(cs["prob"])
    for b, (A, v) in cs["priors"].items():
        pr.set_block_prior(6 * b, A, v)
    s = capi.Solver(pr, capi.default_options(schur_impl=2))
    try:
        elim = s.eliminates_times()
        summ = s.run()
        s.download()
        _, rms = pr.reprojection_error()
        log, params = s.iterations(), pr.params.copy()
        s.configure_run(1, 1)
        s.run()
        np.savez(sys.argv[1], log=log, params=params, rms=rms, elim=elim, kernels=np.array(sorted(s.kernel_stats(64))),
                 summary=np.array([summ.termination_type, summ.stop_reason, summ.num_iterations]), final_cost=summ.final_cost)
    finally:
        s.close()
        pr.close()


if __name__ == "__main__":
    main()
