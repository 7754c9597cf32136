"""Child process of tests/test_gpu_point_step.py: runs cases of tests/point_step_accuracy.py through the public API (capi.Problem.points,
capi.Solver) with whatever RSBA_* switches the environment carries (they are read once per process) and prints one JSON line per
case: the expected back-substitution form, the backward errors and bars of both steps (camera and point rows apart), the scalars'
figures, and every check that failed.  Usage: point_step_worker.py <schur_impl> <case name>...
Test infrastructure: the numpy reference of point_step_accuracy.py is the reference."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import point_step_accuracy as psa  # noqa: E402
from realsensecalibration_amd import capi  # noqa: E402

SWITCHES = ("RSBA_BACKSUB_PROJ", "RSBA_FUSED_LIN", "RSBA_DECIDED_DAMP", "RSBA_FIRST_STAGED", "RSBA_PIPELINE", "RSBA_FORCE_COMM")


def solve(case, prob, consts, impl, iterations):
    """A fresh solver taking `iterations` accepted steps -> (all parameters, log rows, schedule_info)."""
    pr = capi.Problem.points(prob)
    try:
        for c in consts[0]:
            pr.set_camera_constant(c)
        for j in consts[1]:
            pr.set_point_constant(j)
        s = capi.Solver(pr, capi.default_options(schur_impl=impl, huber_delta=case.huber, initial_trust_region_radius=case.radius,
                                                 max_num_iterations=iterations, function_tolerance=-1.0, gradient_tolerance=-1.0,
                                                 parameter_tolerance=-1.0, min_relative_decrease=-1e300))
        try:
            s.run()
            s.download()
            return pr.params.copy(), s.iterations(), s.schedule_info()
        finally:
            s.close()
    finally:
        pr.close()


def _blocks_moved(mdl, a, b):
    moved = np.concatenate([np.any(a[:mdl.nc].reshape(-1, 6) != b[:mdl.nc].reshape(-1, 6), axis=1),
                            np.any(a[mdl.nc:].reshape(-1, 3) != b[mdl.nc:].reshape(-1, 3), axis=1)])
    free = np.concatenate([mdl.cam_free, mdl.pt_free])
    return bool(np.all(moved[free])), int(np.sum(~moved[free]))


def _step_report(r):
    return {k: {f: r[k][f] for f in ("eta", "bar", "ratio", "recovery", "row")} for k in ("cam", "pt")}


def run_case(name, impl, env):
    t0 = time.time()
    case = psa.BY_NAME[name]
    mdl = psa.model(case)
    prob, x0 = mdl.prob, mdl.x0
    consts = psa.constants(case, prob)
    sys1 = psa.System(mdl, x0, case.radius)
    t_ref = time.time() - t0
    x1, log1, info1 = solve(case, prob, consts, impl, 1)
    out = dict(name=name, impl=impl, form=psa.expected_form(case, env, impl), n=mdl.n_free, m=mdl.m, N=mdl.N, slices=psa.slices(mdl.P),
               kappa_s=sys1.kappa_s, kappa_p=sys1.kappa_pmax)
    fixed = ~mdl.free
    checks = [("one accepted step", log1.shape[0] == 2 and int(log1[1, 7]) == 3, log1.tolist()),
              ("no stall or fallback", info1["stalls"] == 0 and info1["fallbacks"] == 0, info1)]
    if not checks[0][1]:
        out["failures"] = ["%s: %s" % (w, d) for w, ok, d in checks if not ok]
        return out
    # ---- step 1
    r1 = sys1.check(x1)
    out["step1"] = _step_report(r1)
    checks += [("step 1 backward error, camera rows", r1["cam"]["eta"] <= r1["cam"]["bar"], r1["cam"]),
               ("step 1 backward error, point rows", r1["pt"]["eta"] <= r1["pt"]["bar"], r1["pt"]),
               ("radius", log1[0, 6] == case.radius, log1[0, 6])]
    sc, out["scalars1"] = psa.scalar_checks(sys1, x1, log1[0, 1], log1[0, 3], log1[1, 2], log1[1, 4], log1[1, 5], "step 1")
    checks += sc
    cost_x1 = mdl.cost(x1)
    checks.append(("cost re-evaluated at x1", abs(log1[1, 1] - cost_x1) <= 1e-12 * cost_x1, (log1[1, 1], cost_x1)))
    moved, stuck = _blocks_moved(mdl, x1, x0)
    checks += [("step 1: constant and unreferenced blocks keep their bits", np.array_equal(x1[fixed], x0[fixed]), None),
               ("step 1: every free block moved", moved, stuck)]
    if impl != 0:
        # ---- a second one-step solver: the same bits
        x1b, log1b, _ = solve(case, prob, consts, impl, 1)
        checks += [("second solver: x1", np.array_equal(x1b, x1), float(np.abs(x1b - x1).max())),
                   ("second solver: log", np.array_equal(log1b, log1), (log1b.tolist(), log1.tolist()))]
        # ---- step 2: the two-step run's rows 0 and 1 are the one-step run's, so it went through x1
        x2, log2, info2 = solve(case, prob, consts, impl, 2)
        same = log2.shape[0] == 3 and np.array_equal(log2[:2], log1) and int(log2[2, 7]) == 3
        checks += [("two-step run: rows 0 and 1 equal the one-step run's bit for bit", same, (log2.tolist(), log1.tolist())),
                   ("two-step run: no stall or fallback", info2["stalls"] == 0 and info2["fallbacks"] == 0, info2)]
        if same:
            sys2 = psa.System(mdl, x1, log1[1, 6], scale=sys1.s)
            r2 = sys2.check(x2)
            out["step2"] = _step_report(r2)
            out["radius2"] = float(log1[1, 6])
            checks += [("step 2 backward error, camera rows", r2["cam"]["eta"] <= r2["cam"]["bar"], r2["cam"]),
                       ("step 2 backward error, point rows", r2["pt"]["eta"] <= r2["pt"]["bar"], r2["pt"])]
            sc, out["scalars2"] = psa.scalar_checks(sys2, x2, log2[1, 1], log2[1, 3], log2[2, 2], log2[2, 4], log2[2, 5], "step 2")
            checks += sc
            moved, stuck = _blocks_moved(mdl, x2, x1)
            checks += [("step 2: constant and unreferenced blocks keep their bits", np.array_equal(x2[fixed], x0[fixed]), None),
                       ("step 2: every free block moved", moved, stuck)]
    if case.huber:
        past = int(np.sum(sys1.sumsq > case.huber ** 2))
        checks.append(("blocks on both sides of the loss's threshold", 0 < past < mdl.N, past))
    out["failures"] = ["%s: %s" % (w, d) for w, ok, d in checks if not ok]
    out["seconds"] = dict(total=time.time() - t0, reference=t_ref)
    return out


def main():
    impl = int(sys.argv[1])
    env = {k: os.environ[k] for k in SWITCHES if k in os.environ}
    for name in sys.argv[2:]:
        print(json.dumps(run_case(name, impl, env)), flush=True)


if __name__ == "__main__":
    main()
