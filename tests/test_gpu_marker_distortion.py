"""Lens distortion (OpenCV's k1 k2 p1 p2 k3, rsba_problem_set_distortion) on the marker-chain models, on the GPU, against the numpy
reference tests/marker_distortion_ref.py (MarkerChainDist: marker_loss_ref.MarkerChain with residuals() replaced; every Jacobian
by complex step).  Problems are redetected — the truth projected through the distorted model plus 0.3 px noise — with
coefficients(C, seed) unless a test says otherwise.

1. Whole solves at the project's parity bar (README, "Parity is tested at"): the same accept / reject sequence and termination,
   every iterate's cost to 1e-9 relative, every free block to 1e-6 relative, the RMS to 1e-4 px; tests/test_marker_distortion_ref_cpu.py
   pins every case's trajectory as robust.
2. One LM step as a linear solve, tests/marker_step_accuracy.py's measure and bar with MarkerChainDist in place of MarkerChain and
   the rounding count of a Jacobian entry recounted (below).
3. Evaluate, the CRS Jacobian and covariance blocks on 3 x 70 x 5 (Huber, a constant time and marker) and hongo, both paths.
4. Nothing changes without coefficients: an all-zero array and none give identical bits.
5. It matters: with zero noise the distorted solve reaches the truth, the pinhole solve of the same detections does not.
6. Two runs of a distortion solver from set_parameters(x0) return identical bits.

The recount (u = 2^-53; a rounding is counted as a relative perturbation of what it feeds, as marker_step_accuracy does).
marker_step_accuracy.C_JAC = 37 is the longest chain of roundings into one entry of the pinhole rows (test_gpu_jacobian.py's table):
pose constants 10, three rigid transforms 12, [iz, al, ga] 4, Q_t 2, Q_m 3, w x Q_m 2, the product with Jl 3, the corrector 1.
With distortion (ProjectCorner<true> and CarryQ, csrc/ba_math.hpp) the bracket and Q_t change; the rest stands:
    pose constants                                                                                     10
    three rigid transforms                                                                             12
    iz = 1 / Z                                                                                          1
    x = X iz                                                                                            1
    xx = x x,  r2 = xx + yy                                                                             2
    drad = k1 + r2 (2 k2 + (3 k3) r2)        3 k3, times r2, the sum, times r2, the sum                 5   (rad's chain is 6, but 2 xx drad
    2 xx drad                                (2 xx is exact)                                            1    leads: 4 + 5 + 1 against 4 + 6)
    rad + 2 xx drad, + the tangential terms                                                             2
    d00 x, + d01 y, times -al                                                                           3   -> Q: 15 in place of 4
    Q_t = Q_0 R + Q_1 R + Q_2 R              product, two sums (the middle-row term)                    3   in place of 2
    Q_m = Q_t R_t                                                                                       3
    a = w x Q_m                                                                                         2
    J = a K                                                                                             3
    the corrector's product                                                                             1
                                                                                                 total 49
so term 1 of the step bar is gamma_{m + 2 x 49} / (1 - gamma_{m + 2 x 49}), and a CRS value is held to 16 x 49 u of its block's largest
entry (test_gpu_jacobian.py's 16 x FLOOR u; there is no second build of this reference to take a d_J from, the floor is the bar).
A residual: iz 1, x 1, xx 1, r2 1, rad 6, x rad 1, + the tangential terms 1, fx xd 1, + ppx 1, - u 1 = 15 roundings of numbers no
larger than a pixel coordinate, so rbar = 16 x 15 ulp(max |observation coordinate|) where test_gpu_evaluate.py has 16 x 4 ulp for the
pinhole form; the gradient and cost bars are that file's formulas on this rbar.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import evaluate_ref as er
import jacobian_ref as jr
import marker_distortion_ref as dref
import marker_loss_ref as ref
import marker_step_accuracy as msa
import solve_accuracy as sa
from realsensecalibration_amd import capi
from realsensecalibration_amd import synthetic as syn

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
C_JAC_DIST = 49      # the recount above
R_FLOOR = 15
REASON = {"gradient": 1, "parameter": 2, "function": 3, "max_iterations": 4, "min_radius": 5, "invalid_steps": 6}
TERM = {"CONVERGENCE": 0, "NO_CONVERGENCE": 1, "FAILURE": 2}
PINHOLE_RMS = 5.013298e-02   # tests/test_marker_distortion_ref_cpu.py: the pinhole reference on the zero-noise distorted detections
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


def _model(variant):
    return capi.MODEL_MARKER_CHAIN_TEST2 if variant == 1 else capi.MODEL_MARKER_CHAIN


def _options(schur_impl, loss="none", a=0.0, **kw):
    return capi.default_options(schur_impl=schur_impl, huber_delta=a if loss != "none" else 0.0, loss_type=1 if loss == "cauchy" else 0, **kw)


def _problem(cs, dist="case"):
    prob = dict(cs["prob"])
    prob.pop("dist", None)
    pr = capi.Problem.marker_chain(prob, _model(cs["variant"]))
    for b in cs["constant_blocks"]:
        pr.set_parameter_block_constant(6 * b)
    if cs.get("weights") is not None:
        pr.set_observation_weights(cs["weights"])
    if isinstance(dist, str):
        dist = cs["dist"]
    if dist is not None:
        pr.set_distortion(dist)
    return pr


def _solve(cs, schur_impl, dist="case"):
    pr = _problem(cs, dist)
    try:
        s = capi.Solver(pr, _options(schur_impl, cs["loss"], cs["a"]))
        try:
            elim = s.eliminates_times()
            summ = s.run()
            s.download()
            log, params = s.iterations(), pr.params.copy()
        finally:
            s.close()
        _, rms = pr.reprojection_error()
    finally:
        pr.close()
    return summ, log, params, rms, elim


# ------------------------------------------------------------------------------------------------ 1. whole solves
@pytest.mark.parametrize("schur_impl", [0, 2])
@pytest.mark.parametrize("name", dref.SOLVE_CASES)
def test_solve_matches_the_distorted_reference(name, schur_impl):
    cs, mc, summary, rows, final = dref.reference_run(name)
    summ, log, params, rms, elim = _solve(cs, schur_impl)
    assert elim == (1 if schur_impl == 2 else 0)
    assert (summ.termination_type, summ.stop_reason, summ.num_iterations) == (TERM[summary["termination"]], REASON[summary["reason"]], len(rows) - 1)
    assert [int(v) for v in log[:, 7]] == [rw["valid"] + 2 * rw["successful"] for rw in rows]
    worst = max(abs(log[j, 1] - rw["cost"]) / rw["cost"] for j, rw in enumerate(rows))
    got = params.reshape(-1, 6)
    free = mc.free_blocks
    err = np.abs(got[free] - final[free]).max(axis=1) / np.maximum(np.abs(final[free]).max(axis=1), 1e-12)
    rms_ref = np.sqrt(summary["final_sumsq"] / (8.0 * cs["prob"]["N"]))
    print("%s schur_impl %d: %d iterations, cost error %.2e (bar 1e-9), block error %.2e (bar 1e-6), rms %.6f against %.6f"
          % (name, schur_impl, len(rows) - 1, worst, err.max(), rms, rms_ref))
    for j, rw in enumerate(rows):
        assert abs(log[j, 1] - rw["cost"]) <= 1e-9 * rw["cost"], "iterate %d: cost %.15e, reference %.15e" % (j, log[j, 1], rw["cost"])
    assert abs(summ.final_cost - summary["final_cost"]) <= 1e-9 * summary["final_cost"]
    assert err.max() < 1e-6, "final parameters differ from the reference's by %.2e relative per block" % err.max()
    start = np.asarray(cs["prob"]["params"]).reshape(-1, 6)
    fixed = np.setdiff1d(np.arange(got.shape[0]), free)
    np.testing.assert_array_equal(got[fixed], start[fixed])
    assert abs(rms - rms_ref) <= 1e-4, (rms, rms_ref)
    # and the coefficients are in the result: the pinhole solve of the same problem ends elsewhere
    _, _, params_pin, _, _ = _solve(cs, schur_impl, dist=None)
    assert np.abs(params_pin - params).max() > 1e-5


# ------------------------------------------------------------------------------------------------ 2. one LM step
STEP_CASES = ["minimal_2x3x2", "minimal_2x3x2_test2", "rows_per_shot_6x8x6", "width_13x8x14", "width_33x6x34", "wide_62x3x62", "wide_8x6x12",
              "wide_8x6x12_backsub_wg", "dense_4x40x6", "loss_6x8x6_huber", "const_6x8x6_none", "second_8x24x12"]
_BY_NAME = {c.name: c for c in msa.CASES}


def step_problem(case):
    """The case's problem of marker_step_accuracy, redetected through coefficients(C, seed) (a displaced case: redetected, then displaced)."""
    key = case.prob
    base = msa.problem(key[1] if key[0] == "disp" else key)
    C, T, M = base["C"], base["T"], base["M"]
    dist = dref.coefficients(C, C + T + M)
    p = dref.redetect(base, dist, 0.3, C + T + M)
    if key[0] == "disp":
        p = dict(ref.displace_corners(p, 0.05, 40.0, C * T * M), dist=dist)
    return p, dist


def step_chain(case, prob, dist):
    return dref.MarkerChainDist(prob, dist, case.variant, case.loss, msa.LOSS_A if case.loss != "none" else 0.0, msa.constant_blocks(case, prob))


def _step_options(case, **kw):
    return capi.default_options(schur_impl=case.impl, huber_delta=msa.LOSS_A if case.loss != "none" else 0.0, loss_type=1 if case.loss == "cauchy" else 0,
                                initial_trust_region_radius=case.radius, **kw)


def one_step(case, prob, dist, start, profile):
    """One forced step from `start` (all parameters; None: the problem's own) -> (x1 (all parameters), log rows, eliminates_times, kernel names)."""
    p = dict(prob)
    p.pop("dist", None)
    pr = capi.Problem.marker_chain(p, _model(case.variant))
    try:
        for b in msa.constant_blocks(case, prob):
            pr.set_parameter_block_constant(6 * b)
        pr.set_distortion(dist)
        s = capi.Solver(pr, _step_options(case, max_num_iterations=1, function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0))
        try:
            elim = s.eliminates_times()
            if start is not None:
                s.set_parameters(start)
            if profile:
                s.configure_run(1, 1)
            s.run()
            s.download()
            log = s.iterations()
            stats = sorted(s.kernel_stats(64)) if profile else []
        finally:
            s.close()
        return pr.params.copy(), log, elim, stats
    finally:
        pr.close()


def step_pair(case):
    """What the device contributes to a step case: the start (all parameters), the profiled and the unprofiled step."""
    prob, dist = step_problem(case)
    start = None
    if case.state == "second":
        p = dict(prob)
        p.pop("dist", None)
        pr = capi.Problem.marker_chain(p, _model(case.variant))
        try:
            pr.set_distortion(dist)
            assert pr.solve(_step_options(case)).termination_type == capi.CONVERGENCE
            full = pr.params.reshape(-1, 6).copy()
        finally:
            pr.close()
        fb = step_chain(case, prob, dist).free_blocks
        full[fb] = msa.perturbed(full[fb].ravel()).reshape(-1, 6)
        start = full.ravel()
    x1, log, elim, stats = one_step(case, prob, dist, start, True)
    x1b, logb, _, _ = one_step(case, prob, dist, start, False)
    return dict(start=np.asarray(prob["params"], float) if start is None else start, x1=x1, log=log, elim=elim, stats=stats, x1_again=x1b, log_again=logb)


@pytest.mark.parametrize("name", STEP_CASES)
def test_one_step_within_its_backward_error_bar(name, tmp_path):
    case = _BY_NAME[name]
    if case.env:
        # the switches are read at create: a child process with them in its environment, as tests/switch_worker.py is run
        out = str(tmp_path / "step.npz")
        r = subprocess.run([sys.executable, os.path.join(HERE, "distortion_step_worker.py"), name, out], env=dict(os.environ, **dict(case.env)),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        z = np.load(out)
        dev = dict(start=z["start"], x1=z["x1"], log=z["log"], elim=int(z["elim"]), stats=json.loads(str(z["stats"])), x1_again=z["x1_again"], log_again=z["log_again"])
    else:
        dev = step_pair(case)
    prob, dist = step_problem(case)
    prob = dict(prob, params=dev["start"])
    mc = step_chain(case, prob, dist)
    path = msa.expected_path(case, mc)
    pin = ref.MarkerChain(prob, case.variant, case.loss, msa.LOSS_A if case.loss != "none" else 0.0, msa.constant_blocks(case, prob))
    assert msa.expected_path(case, pin) == path   # the path is a matter of the index arrays: the same with and without coefficients
    failures = msa.path_failures(path, dev["elim"], set(dev["stats"]))
    log, x1_full = dev["log"], dev["x1"]
    assert log.shape[0] == 2 and int(log[1, 7]) == 3, "the step was not accepted: %s" % (log,)
    sysm = msa.System(mc, mc.x0(), case.radius, dense=case.impl == 0)
    gf = sa.gamma(sysm.m + 2 * C_JAC_DIST)
    sysm.forming = gf / (1.0 - gf)
    x1 = x1_full.reshape(-1, 6)[mc.free_blocks].ravel()
    r = sysm.check(x1)
    print("\nMCSTEP-DIST %-28s n %4d m %6d kappa %8.2f eta %.2e bar %.2e (recovery %.1e) eta/bar %.2e  %s" % (
        name, sysm.n, sysm.m, sysm.kappa, r["eta"], r["bar"], r["recovery"], r["ratio"], msa.path_text(path)))
    checks = [("backward error", r["eta"] <= r["bar"], r)]
    cost0, gmax0, radius0 = log[0, 1], log[0, 3], log[0, 6]
    cost_change, step_norm, rel = log[1, 2], log[1, 4], log[1, 5]
    nd, tol = sysm.step_norm_tolerance(x1)
    mcc, mcc_tol = sysm.model_cost_change(x1)
    cand_ref = mc.cost(x1)[0]
    cand = cost0 - cost_change
    checks += [
        ("radius", radius0 == case.radius, radius0),
        ("cost", abs(cost0 - sysm.cost) <= 1e-12 * sysm.cost, (cost0, sysm.cost)),
        ("gradient_max_norm", abs(gmax0 - sysm.gmax) <= 1e-11 * sysm.gmax, (gmax0, sysm.gmax)),
        ("step_norm", abs(step_norm - nd) <= tol, (step_norm, nd, tol)),
        ("model cost change", abs(cost_change / rel - mcc) <= mcc_tol + 2 * U * abs(mcc), (cost_change / rel, mcc, mcc_tol)),
        ("candidate cost", abs(cand - cand_ref) <= 1e-12 * cand_ref + U * (abs(cost_change) + cand_ref), (cand, cand_ref)),
        ("cost re-evaluated at x1", abs(log[1, 1] - cand_ref) <= 1e-12 * cand_ref, (log[1, 1], cand_ref)),
    ]
    x0_full = np.asarray(prob["params"], float).reshape(-1, 6)
    fixed = np.setdiff1d(np.arange(x0_full.shape[0]), mc.free_blocks)
    checks += [
        ("constant, base and unreferenced blocks", np.array_equal(x1_full.reshape(-1, 6)[fixed], x0_full[fixed]), None),
        ("a free block moved", bool(np.all(np.any(x1_full.reshape(-1, 6)[mc.free_blocks] != x0_full[mc.free_blocks], axis=1))), None),
        ("second solver: x1", np.array_equal(dev["x1_again"], x1_full), None),
        ("second solver: log", np.array_equal(dev["log_again"], log), None),
    ]
    # the pinhole system at the same point is another system: the device's step does not solve it
    pin_sys = msa.System(pin, pin.x0(), case.radius, dense=case.impl == 0)
    rp = pin_sys.check(x1)
    checks.append(("the step belongs to the distorted model", rp["eta"] > 100 * rp["bar"], rp))
    if case.loss != "none":
        res = mc.residuals(mc.full(mc.x0()))
        past = int(np.sum(np.sum(res * res, axis=1) > msa.LOSS_A ** 2))
        checks.append(("blocks past the loss's threshold", 0 < past < mc.N, past))
    failures += ["%s: %s" % (what, detail) for what, ok, detail in checks if not ok]
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 3. evaluate, Jacobian, covariance
def _eval_case(name):
    if name == "hongo":
        return dref.case("hongo")
    base = syn.make_marker_chain(3, 70, 5, seed=35)
    dist = dref.coefficients(3, 35)
    prob = dref.redetect(base, dist, 0.3, 35)
    prob = dict(ref.displace_corners(prob, 0.05, 40.0, 3 * 70 * 5), dist=dist)
    return dict(prob=prob, dist=dist, variant=0, loss="huber", a=2.0, weights=None, constant_blocks=(3 + 4, 3 + 70 + 2))


def _rows(mc, full):
    """evaluate_ref's row format from the chain's raw residuals and complex-step Jacobians."""
    r, J = mc.residuals(full), mc.jacobians(full)
    C, T = mc.C, mc.T
    rows = []
    for i in range(mc.N):
        blocks = [(6 * (C + int(mc.t[i])), J[i][:, 6:12])]
        if mc.has_cam[i]:
            blocks.append((6 * int(mc.c[i]), J[i][:, 0:6]))
        if mc.has_mar[i]:
            blocks.append((6 * (C + T + int(mc.m[i])), J[i][:, 12:18]))
        rows.append((r[i], blocks))
    return rows


def _check_queries(cs, s, x, label):
    """cost, residuals, gradient and CRS values at x (all parameters) against the reference; J'r against the gradient.  -> outputs."""
    mc = dref.MarkerChainDist(dict(cs["prob"], params=x), cs["dist"], cs["variant"], "none", 0.0, ())   # (raw rows; the loss is applied by finish)
    rows = _rows(mc, mc.full0)
    const = [(6 * b, 6) for b in cs["constant_blocks"]]
    rbar = 16 * R_FLOOR * float(np.spacing(np.abs(np.asarray(cs["prob"]["obs"])).max()))
    out = {}
    for apply_loss in ((True, False) if cs["loss"] != "none" else (True,)):
        want = er.finish(rows, x.size, const, cs["loss"], cs["a"], apply_loss)
        gbar = want.abs_J * rbar + (64 + want.n_terms) * U * want.abs_Jr
        cbar = rbar * np.abs(want.residuals).sum() + mc.N * U * want.cost
        cost, r, g = s.evaluate(apply_loss_function=apply_loss)
        live = want.live
        q_r = np.abs(r - want.residuals).max() / rbar
        q_g = (np.abs(g - want.gradient)[live] / gbar[live]).max()
        q_c = abs(cost - want.cost) / cbar
        jref = jr.assemble(rows, x.size, const, cs["loss"], cs["a"], apply_loss)
        shape, indptr, indices = s.jacobian_structure()
        vals = s.evaluate_jacobian(apply_loss_function=apply_loss)
        assert shape == jref.shape and np.array_equal(indptr, jref.indptr) and np.array_equal(indices, jref.indices)
        q_j = (np.abs(vals - jref.values) / (16 * C_JAC_DIST * U * jref.scale)).max()
        jtr = jr.transpose_times(shape, indptr, indices, vals, r)
        q_t = (np.abs(jtr - g)[live] / gbar[live]).max()
        print("%s%s apply_loss=%d: error / bar  residual %.3f  gradient %.3f  cost %.3f  jacobian %.3f  J'r %.3f" % (label, "", apply_loss, q_r, q_g, q_c, q_j, q_t))
        assert q_r <= 1.0 and q_g <= 1.0 and q_c <= 1.0 and q_j <= 1.0 and q_t <= 1.0, (q_r, q_g, q_c, q_j, q_t)
        assert np.all(g[~live] == 0.0) and np.all(jtr[~live] == 0.0)
        out[apply_loss] = (cost, r, g, vals)
    return out


@pytest.mark.parametrize("name", ["3x70x5_huber_const", "hongo"])
def test_evaluate_jacobian_and_covariance(name):
    cs = _eval_case(name)
    C, T, M = cs["prob"]["C"], cs["prob"]["T"], cs["prob"]["M"]
    at_start = {}
    for impl in (0, 2):
        pr = _problem(cs)
        s = capi.Solver(pr, _options(impl, cs["loss"], cs["a"], max_num_iterations=4))
        try:
            assert s.eliminates_times() == (1 if impl == 2 else 0)
            x0 = np.asarray(cs["prob"]["params"], float)
            at_start[impl] = _check_queries(cs, s, x0, "%s schur_impl %d, before any run" % (name, impl))
            s.run()
            s.download()
            x = pr.params.copy()
            _check_queries(cs, s, x, "%s schur_impl %d, after a run" % (name, impl))
            # covariance at x: camera, time, marker and cross blocks against the reference's dense inverse
            mc = dref.MarkerChainDist(dict(cs["prob"], params=x), cs["dist"], cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])
            Sinv, fb = ref.covariance(mc, mc.x0())
            pos = {int(b): 6 * k for k, b in enumerate(fb)}
            s.covariance_compute(apply_loss_function=1)
            cams = [b for b in fb if b < C][:3]
            times = [b for b in fb if C <= b < C + T][:4]
            marks = [b for b in fb if b >= C + T][:3]
            pairs = [(a, a) for a in cams + times + marks] + [(cams[0], t) for t in times] + [(cams[-1], m) for m in marks] + [(times[0], times[1]), (times[1], marks[0])]
            got = s.covariance_blocks([(6 * a, 6 * b) for a, b in pairs])
            worst = 0.0
            for (a, b), blk in zip(pairs, got):
                want = Sinv[pos[a]:pos[a] + 6, pos[b]:pos[b] + 6]
                worst = max(worst, float(np.abs(blk - want).max() / np.abs(want).max()))
            tc = s.time_covariances()
            for t in times:
                want = Sinv[pos[t]:pos[t] + 6, pos[t]:pos[t] + 6]
                worst = max(worst, float(np.abs(tc[t - C] - want).max() / np.abs(want).max()))
            for b in cs["constant_blocks"]:
                if C <= b < C + T:
                    assert not tc[b - C].any()
            print("%s schur_impl %d: covariance, %d pairs, worst error / bar %.3e (bar 1e-8)" % (name, impl, len(pairs), worst / 1e-8))
            assert worst <= 1e-8
        finally:
            s.close()
            pr.close()
    # the two paths share the evaluation kernels: identical bits before any run (M1's property)
    for apply_loss, (cost, r, g, vals) in at_start[0].items():
        cost2, r2, g2, vals2 = at_start[2][apply_loss]
        assert cost == cost2
        for a, b in ((r, r2), (g, g2), (vals, vals2)):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 4. nothing changes without coefficients
def _everything(cs, schur_impl, dist):
    pr = _problem(cs, dist)
    try:
        s = capi.Solver(pr, _options(schur_impl, cs["loss"], cs["a"]))
        try:
            ev0 = s.evaluate()
            jac0 = s.evaluate_jacobian()
            s.run()
            s.download()
            return dict(log=s.iterations(), params=pr.params.copy(), cost=ev0[0], r=ev0[1], g=ev0[2], jac=jac0, ev1=s.evaluate(), jac1=s.evaluate_jacobian(),
                        rms=pr.reprojection_error())
        finally:
            s.close()
    finally:
        pr.close()


@pytest.mark.parametrize("schur_impl", [0, 2])
@pytest.mark.parametrize("name", ["4x40x6", "hongo"])
def test_zero_coefficients_are_no_coefficients(name, schur_impl):
    cs = dict(dref.case(name))
    zeros = np.zeros((cs["prob"]["C"], 5))
    a, b = _everything(cs, schur_impl, None), _everything(cs, schur_impl, zeros)
    assert a["log"].shape[0] > 2
    np.testing.assert_array_equal(a["log"][:, [0, 1, 2, 3, 4, 5, 6, 7]], b["log"][:, [0, 1, 2, 3, 4, 5, 6, 7]])
    np.testing.assert_array_equal(a["params"], b["params"])
    assert a["cost"] == b["cost"] and a["rms"] == b["rms"]
    for k in ("r", "g", "jac", "jac1"):
        np.testing.assert_array_equal(a[k], b[k])
    for u, v in zip(a["ev1"], b["ev1"]):
        np.testing.assert_array_equal(u, v)
    c = _everything(cs, schur_impl, cs["dist"])
    assert not np.array_equal(c["params"], a["params"])   # (and a non-zero set is something else)
    pr = _problem(cs, zeros)
    try:
        np.testing.assert_array_equal(pr.distortion, zeros)
        pr.set_distortion(None)
        assert pr.distortion is None
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 5. it matters
@pytest.mark.parametrize("schur_impl", [0, 2])
def test_distortion_reaches_the_truth_and_pinhole_does_not(schur_impl):
    """A deviation from the issue, which asks for the comparison with the truth to be gauge-aligned with tests/gauge.py: that module
    aligns the point model (cameras and points under a similarity).  This problem has Main_Calibration's wiring (variant 0), where camera
    0 and marker 0 are not in the chain and the marker side fixes the scale: there is no gauge orbit to align along, and raw parameters
    are compared.  The RMS at the distorted solve's end is 2e-9 px, a sum of residuals that are differences of pixel-sized numbers: it is
    held to the reference's at the same point within test 3's residual bar rbar (an error of rbar in every residual moves the RMS by
    at most rbar), 1.5 % of it here, not within a bar both values are below."""
    prob, dist, truth = dref.zero_noise_problem()
    cs = dict(prob=prob, dist=dist, variant=0, loss="none", a=0.0, weights=None, constant_blocks=())
    summ, log, params, rms, _ = _solve(cs, schur_impl)
    mc = dref.MarkerChainDist(prob, dist)
    err = np.abs(params.reshape(-1, 6) - truth).max()   # (the wiring fixes the gauge: camera 0 and marker 0 are not in the chain)
    rms_ref = dref.rms(mc, params.reshape(-1, 6)[mc.free_blocks].ravel())
    print("schur_impl %d with coefficients: %.3e off the truth, rms %.3e px (reference at the same point %.3e)" % (schur_impl, err, rms, rms_ref))
    rbar = 16 * R_FLOOR * float(np.spacing(np.abs(np.asarray(prob["obs"])).max()))
    assert summ.termination_type == capi.CONVERGENCE and err < 1e-6 and rms < 1e-6
    assert rms_ref > 10 * rbar and abs(rms - rms_ref) <= rbar, (rms, rms_ref, rbar)
    summ_p, _, params_p, rms_p, _ = _solve(cs, schur_impl, dist=None)
    pin = ref.MarkerChain(prob, 0)
    rms_p_ref = dref.rms(pin, params_p.reshape(-1, 6)[pin.free_blocks].ravel())
    err_p = np.abs(params_p.reshape(-1, 6) - truth).max()
    print("schur_impl %d without: %.3e off the truth, rms %.6e px (pinhole reference's minimum %.6e)" % (schur_impl, err_p, rms_p, PINHOLE_RMS))
    assert abs(rms_p - PINHOLE_RMS) <= 1e-4 and abs(rms_p - rms_p_ref) <= 1e-9 and err_p > 1e-3


# ------------------------------------------------------------------------------------------------ 6. repetition
@pytest.mark.parametrize("schur_impl", [0, 2])
def test_two_runs_return_identical_bits(schur_impl):
    cs = dref.case("4x40x6_huber")
    pr = _problem(cs)
    s = capi.Solver(pr, _options(schur_impl, cs["loss"], cs["a"]))
    try:
        x0 = np.asarray(cs["prob"]["params"], float)
        res = []
        for _ in range(2):
            s.set_parameters(x0)
            s.run()
            s.download()
            res.append((s.iterations().copy(), pr.params.copy(), s.evaluate()))
        np.testing.assert_array_equal(res[0][0][:, :8], res[1][0][:, :8])
        np.testing.assert_array_equal(res[0][1], res[1][1])
        for u, v in zip(res[0][2], res[1][2]):
            np.testing.assert_array_equal(u, v)
        assert res[0][0].shape[0] > 3
    finally:
        s.close()
        pr.close()
