"""Time rsba_solver_evaluate and rsba_solver_set_parameters + rsba_solver_run at cfg3's shape (64 cameras x 100k points x 2M observations).

  python tools/evaluate_timing.py [--reps 5] [--steps 5]

After one warm-up call of each kind (the first evaluate builds its index tables and its arena), wall-clock times of
  evaluate, residuals only      (the call includes the 32 MB device-to-host copy of the residuals)
  evaluate, cost only           (the same kernels, no residual copy)
  evaluate with the gradient
  set_parameters + run          (--steps LM iterations) against create + run of a new solver on the same values
                                (setup_s: the host planning set_parameters does not repeat)
Kernel times are not taken here: run the tool once under `rocprofv3 --kernel-trace --stats -- python tools/evaluate_timing.py
--reps 1` and read k_eval_* from the statistics.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from realsensecalibration_amd import capi, synthetic  # noqa: E402


def _best(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--config", default="cfg3")
    a = ap.parse_args()
    capi.load()
    prob = synthetic.make_config(a.config)
    o = capi.default_options(huber_delta=prob.get("huber_delta", 0.0), max_num_iterations=a.steps)
    pr = capi.Problem.points(prob)
    t0 = time.perf_counter()
    s = capi.Solver(pr, o)
    create_s = time.perf_counter() - t0
    x1 = prob["params"] + 1e-4 * np.random.default_rng(1).standard_normal(len(prob["params"]))
    # warm-up: tables, arena, one run
    s.evaluate()
    s.run()
    lib, cost = capi.load(), capi.C.c_double()
    res = {"config": a.config, "C": prob["C"], "P": prob["P"], "N": prob["N"], "steps": a.steps, "create_s": create_s,
           "evaluate_residuals_s": _best(lambda: s.evaluate(gradient=False), a.reps),
           "evaluate_cost_only_s": _best(lambda: lib.rsba_solver_evaluate(s.h, None, capi.C.byref(cost), None, None), a.reps),
           "evaluate_gradient_s": _best(lambda: s.evaluate(), a.reps)}

    def reset_and_run():
        s.set_parameters(x1)
        s.run()

    res["set_parameters_and_run_s"] = _best(reset_and_run, a.reps)
    res["set_parameters_s"] = _best(lambda: s.set_parameters(x1), a.reps)

    def create_and_run():
        p2 = capi.Problem.points(dict(prob, params=x1))
        s2 = capi.Solver(p2, o)
        s2.run()
        s2.close()
        p2.close()

    res["create_and_run_s"] = _best(create_and_run, max(1, min(a.reps, 2)))
    # algorithmic bytes of a residual-only call: every observation record (u, v, camera: 20 B) in, its two residuals (16 B) out
    res["algorithmic_bytes_residuals"] = 36 * prob["N"]
    print(json.dumps(res), flush=True)
    s.close()
    pr.close()


if __name__ == "__main__":
    main()
