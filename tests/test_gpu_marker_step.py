"""One LM step of the marker-chain model on the GPU, held as a linear solve (tests/marker_step_accuracy.py has the measure, the bar's
derivation and the case list; tests/test_marker_step_accuracy_cpu.py shows the bar is neither vacuous nor false).

Whole solves hide an inexact step: Levenberg-Marquardt corrects it, and the fixed point depends on the gradient alone.  Here every
case runs ONE step through the public API (max_num_iterations = 1, the tolerances at -1, the step accepted) and is held to:
  (a) the path it ran is the path the case names: eliminates_times() and the kernel statistics' names; where two variants share a
      name (the accumulation on the matrix cores with three or eight tiles or on the VALU with its sums in LDS or memory; the
      reduced solve with the triangle in LDS or the panel solver; the three back-substitutions) the expected one is computed from
      the thresholds of PlanMarkerChain (csrc/ba_marker_plan.hpp; marker_step_accuracy.expected_path) and printed (full_report() names no path: its
      linear solver line reads DENSE_SCHUR on every one);
  (b) delta = x1 - x0 solves the full damped normal equations of the numpy reference within the derived componentwise
      backward-error bar, row by row;
  (c) the log's scalars: cost, gradient_max_norm, step_norm, the model cost change (cost_change / relative_decrease) at the
      device's own delta, the candidate cost at the downloaded x1;
  (d) constant, base and unreferenced blocks keep their bits; a second solver (not profiled, so with the product kernels side by
      side on their streams) returns the same x1 and log rows, bit for bit.
The second-state cases reach their start with set_parameters on the same solver.  Every case prints eta, bar, kappa, m, the path and
eta / bar; profiles/marker_chain_step_backward_error.txt is that table from an MI355X."""
import numpy as np
import pytest

import marker_step_accuracy as msa
from realsensecalibration_amd import capi

pytestmark = pytest.mark.gpu
U = msa.U


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


_SYSTEMS = {}


def _system(case, mc):
    """The numpy side of a case, once per shape: the switch variants share it (a second state starts from the device's own solution)."""
    if case.state == "second":
        return msa.System(mc, mc.x0(), case.radius, dense=case.impl == 0)
    key = (msa.shape_key(case), case.impl == 0)
    if key not in _SYSTEMS:
        _SYSTEMS[key] = msa.System(mc, mc.x0(), case.radius, dense=case.impl == 0)
    return _SYSTEMS[key]


def _model(case):
    return capi.MODEL_MARKER_CHAIN_TEST2 if case.variant == 1 else capi.MODEL_MARKER_CHAIN


def _options(case, **kw):
    if case.force:
        kw["min_relative_decrease"] = -1e300
    return capi.default_options(schur_impl=case.impl, huber_delta=msa.LOSS_A if case.loss != "none" else 0.0, loss_type=1 if case.loss == "cauchy" else 0,
                                initial_trust_region_radius=case.radius, **kw)


def _one_step(case, prob, start, profile):
    """One step from `start` (all parameters; None: the problem's own) -> (x1 (all parameters), log rows, eliminates_times, kernel names)."""
    pr = capi.Problem.marker_chain(prob, _model(case))
    try:
        for b in msa.constant_blocks(case, prob):
            pr.set_parameter_block_constant(6 * b)
        s = capi.Solver(pr, _options(case, max_num_iterations=1, function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0))
        try:
            elim = s.eliminates_times()
            if start is not None:
                s.set_parameters(start)
            if profile:
                s.configure_run(1, 1)
            s.run()
            s.download()
            log = s.iterations()
            stats = s.kernel_stats(64) if profile else {}
        finally:
            s.close()
        return pr.params.copy(), log, elim, stats
    finally:
        pr.close()


def _converged(case, prob):
    pr = capi.Problem.marker_chain(prob, _model(case))
    try:
        summ = pr.solve(_options(case))
        assert summ.termination_type == capi.CONVERGENCE
        return pr.params.copy()
    finally:
        pr.close()


@pytest.mark.parametrize("case", msa.CASES, ids=[c.name for c in msa.CASES])
def test_one_step_within_its_backward_error_bar(case, monkeypatch):
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    base = msa.problem(case.prob)
    start = None
    prob = base
    if case.state == "second":
        prob = msa.start_problem(case, _converged(case, base))
        start = np.asarray(prob["params"], float)
    mc = msa.chain_at(case, prob)
    path = msa.expected_path(case, mc)
    x1_full, log, elim, stats = _one_step(case, base, start, profile=True)
    x1_again, log_again, _, _ = _one_step(case, base, start, profile=False)
    sysm = _system(case, mc)
    failures = msa.path_failures(path, elim, stats)
    assert log.shape[0] == 2 and int(log[1, 7]) == 3, "the step was not accepted: %s" % (log,)
    x1 = x1_full.reshape(-1, 6)[mc.free_blocks].ravel()
    r = sysm.check(x1)
    print("\nMCSTEP %-52s n %4d m %6d kappa %8.2f eta %.2e bar %.2e (recovery %.1e) eta/bar %.2e  %s" % (
        case.name, sysm.n, sysm.m, sysm.kappa, r["eta"], r["bar"], r["recovery"], r["ratio"], msa.path_text(path)))
    checks = [("backward error", r["eta"] <= r["bar"], r)]
    # ---- the scalars
    cost0, gmax0, radius0 = log[0, 1], log[0, 3], log[0, 6]
    cost_change, step_norm, rel = log[1, 2], log[1, 4], log[1, 5]
    nd, tol = sysm.step_norm_tolerance(x1)
    mcc, mcc_tol = sysm.model_cost_change(x1)
    cand_ref = mc.cost(x1)[0]
    cand = cost0 - cost_change
    print("       cost %.1e  gmax %.1e  step_norm %.1e (tol %.1e)  mcc %.1e (tol %.1e)  candidate %.1e  cost(x1) %.1e" % (
        abs(cost0 - sysm.cost) / sysm.cost, abs(gmax0 - sysm.gmax) / sysm.gmax, abs(step_norm - nd) / nd, tol / nd,
        abs(cost_change / rel - mcc) / abs(mcc), mcc_tol / abs(mcc), abs(cand - cand_ref) / cand_ref, abs(log[1, 1] - cand_ref) / cand_ref))
    checks += [
        ("radius", radius0 == case.radius, radius0),
        ("cost", abs(cost0 - sysm.cost) <= 1e-12 * sysm.cost, (cost0, sysm.cost)),
        ("gradient_max_norm", abs(gmax0 - sysm.gmax) <= 1e-11 * sysm.gmax, (gmax0, sysm.gmax)),
        ("step_norm", abs(step_norm - nd) <= tol, (step_norm, nd, tol)),
        ("model cost change", abs(cost_change / rel - mcc) <= mcc_tol + 2 * U * abs(mcc), (cost_change / rel, mcc, mcc_tol)),
        ("candidate cost", abs(cand - cand_ref) <= 1e-12 * cand_ref + U * (abs(cost_change) + cand_ref), (cand, cand_ref)),
        ("cost re-evaluated at x1", abs(log[1, 1] - cand_ref) <= 1e-12 * cand_ref, (log[1, 1], cand_ref)),
    ]
    # ---- the exact parts
    x0_full = np.asarray(prob["params"], float).reshape(-1, 6)
    fixed = np.setdiff1d(np.arange(x0_full.shape[0]), mc.free_blocks)
    assert 0 in fixed and (case.variant == 1 or mc.C + mc.T in fixed)
    checks += [
        ("constant, base and unreferenced blocks", np.array_equal(x1_full.reshape(-1, 6)[fixed], x0_full[fixed]), None),
        ("a free block moved", bool(np.all(np.any(x1_full.reshape(-1, 6)[mc.free_blocks] != x0_full[mc.free_blocks], axis=1))), None),
        ("second solver: x1", np.array_equal(x1_again, x1_full), float(np.abs(x1_again - x1_full).max())),
        ("second solver: log", np.array_equal(log_again, log), (log_again, log)),
    ]
    if case.loss != "none":
        res = mc.residuals(mc.full(mc.x0()))
        past = int(np.sum(np.sum(res * res, axis=1) > msa.LOSS_A ** 2))
        checks.append(("blocks past the loss's threshold", 0 < past < mc.N, past))
    failures += ["%s: %s" % (what, detail) for what, ok, detail in checks if not ok]
    assert not failures, "\n".join(failures)
