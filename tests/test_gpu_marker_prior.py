"""Gaussian priors on camera and marker blocks (ceres::NormalPrior, rsba_problem_set_block_prior) on the marker-chain models, through
the C ABI, against tests/marker_prior_ref.py — a numpy reference that shares no code with the product; its cases and the condition
that their priors ACT (every solution moves by at least 1e-3) are pinned without a device by tests/test_marker_prior_ref_cpu.py.

Bars (BASELINE's, as tests/test_gpu_marker_subset.py::_compare holds them): the same accept / reject sequence, iteration count,
termination and reason, every iterate's cost to 1e-9 relative, every block of the raw parameters to 1e-6 relative, the final RMS to
1e-4 px; every block that is not free and every masked component keeps the bits of its start value.

One LM step: tests/marker_step_accuracy.py's backward-error bar on marker_prior_ref.PriorSystem — the reference's rows with the prior
rows appended, the bar's longest sum counting the six extra rows of a prior block.  Nothing in the bar is fitted.

Queries: tests/test_gpu_marker_subset.py's bars for the observations' part, unchanged.  A prior's residual A (x - b) is six products
and five additions on top of one subtraction: |error| <= 8 u (|A| |x - b|) per entry; its Jacobian entries are copies of A (exact).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import evaluate_ref as er
import jacobian_ref as jr
import marker_prior_ref as pref
import marker_subset_ref as sref
import marker_weight_ref as wref
import oracle_lib
from realsensecalibration_amd import capi
from test_gpu_marker_weights import SWITCHES

pytestmark = pytest.mark.gpu

REASON = {"gradient": 1, "parameter": 2, "function": 3, "max_iterations": 4, "min_radius": 5, "invalid_steps": 6}
TERM = {"CONVERGENCE": 0, "NO_CONVERGENCE": 1, "FAILURE": 2}
U = 2.0 ** -53
HERE = os.path.dirname(os.path.abspath(__file__))
C_JAC = 37
DENSE_KERNELS = {"k_marker_eval", "k_marker_system", "k_marker_candidate"}
ELIM_KERNELS = {"k_pose_constants", "k_mc_slot_products", "k_mc_time_products", "k_mc_cross", "k_mc_accumulate", "k_marker_reduce",
                "k_marker_reduced_solve", "k_time_backsub_terms", "k_marker_schur_finish"}
PRIOR_KERNELS = {"k_marker_prior_rows", "k_mc_prior_system", "k_mc_prior_candidate"}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


def _options(cs, schur_impl, **kw):
    return capi.default_options(schur_impl=schur_impl, huber_delta=cs["a"] if cs["loss"] != "none" else 0.0, loss_type=1 if cs["loss"] == "cauchy" else 0, **kw)


def _problem(cs, priors="case"):
    prob = cs["prob"]
    if cs.get("dist") is not None:
        prob = dict(prob, dist=cs["dist"])
    pr = capi.Problem.marker_chain(prob, capi.MODEL_MARKER_CHAIN_TEST2 if cs["variant"] == 1 else capi.MODEL_MARKER_CHAIN)
    for b in cs["constant_blocks"]:
        pr.set_parameter_block_constant(6 * b)
    if cs.get("weights") is not None:
        pr.set_observation_weights(cs["weights"])
    for b, m in cs["masks"].items():
        pr.set_parameter_subset_constant(6 * b, m)
    for b, (A, v) in (cs["priors"] if isinstance(priors, str) else (priors or {})).items():
        pr.set_block_prior(6 * b, A, v)
    return pr


def _run(s, pr):
    summ = s.run()
    s.download()
    return summ, s.iterations(), pr.params.copy()


def _solve(cs, schur_impl, priors="case", **kw):
    """-> (summary, log, parameters, rms, eliminates_times) of a fresh problem and solver."""
    pr = _problem(cs, priors)
    try:
        s = capi.Solver(pr, _options(cs, schur_impl, **kw))
        try:
            elim = s.eliminates_times()
            summ, log, params = _run(s, pr)
        finally:
            s.close()
        _, rms = pr.reprojection_error()
    finally:
        pr.close()
    return summ, log, params, rms, elim


def _compare_run(run, label, summary3, final_cost, log, params, rms):
    """A device solve against a reference run (case, chain, summary, rows, final) at the parity bar."""
    cs, mc, summary, rows, final = run
    assert tuple(summary3) == (TERM[summary["termination"]], REASON[summary["reason"]], len(rows) - 1), (summary3, summary)
    assert [int(v) for v in log[:, 7]] == [rw["valid"] + 2 * rw["successful"] for rw in rows]
    worst = max(abs(log[j, 1] - rw["cost"]) / rw["cost"] for j, rw in enumerate(rows))
    got = params.reshape(-1, 6)
    free = mc.free_blocks
    err = np.abs(got[free] - final[free]).max(axis=1) / np.maximum(np.abs(final[free]).max(axis=1), 1e-12)
    rms_ref = np.sqrt(summary["final_sumsq"] / (8.0 * cs["prob"]["N"]))
    print("%s: %d iterations, cost error %.2e (bar 1e-9), block error %.2e (bar 1e-6), rms %.6f against %.6f"
          % (label, len(rows) - 1, worst, err.max(), rms, rms_ref))
    for j, rw in enumerate(rows):
        assert abs(log[j, 1] - rw["cost"]) <= 1e-9 * rw["cost"], "iterate %d: cost %.15e, reference %.15e" % (j, log[j, 1], rw["cost"])
    assert abs(final_cost - summary["final_cost"]) <= 1e-9 * summary["final_cost"]
    assert err.max() < 1e-6, "final parameters differ from the reference's by %.2e relative per block" % err.max()
    start = np.asarray(cs["prob"]["params"], float)
    fixed = np.setdiff1d(np.arange(got.shape[0]), free)
    np.testing.assert_array_equal(got[fixed], start.reshape(-1, 6)[fixed])
    np.testing.assert_array_equal(params[mc.masked_slots], start[mc.masked_slots])
    assert abs(rms - rms_ref) <= 1e-4, (rms, rms_ref)   # the raw reprojection metric: no prior in it


def _compare(pid, label, summary3, final_cost, log, params, rms):
    _compare_run(pref.reference_run(pid), "%s %s" % (pid, label), summary3, final_cost, log, params, rms)


def _check(pid, schur_impl, expect_elim=None):
    cs = pref.case(pid)
    summ, log, params, rms, elim = _solve(cs, schur_impl)
    assert elim == (expect_elim if expect_elim is not None else (1 if schur_impl == 2 else 0))
    _compare(pid, "schur_impl %d" % schur_impl, (summ.termination_type, summ.stop_reason, summ.num_iterations), summ.final_cost, log, params, rms)
    return params


# ------------------------------------------------------------------------------------------------ 1. whole solves
@pytest.mark.parametrize("schur_impl", [0, 2])
@pytest.mark.parametrize("pid", ["P1", "P2", "P3", "P4", "P1w", "D1"])
def test_solve_matches_the_prior_reference(pid, schur_impl):
    """The issue's table on the dense path and with the time blocks eliminated."""
    _check(pid, schur_impl)


def test_default_path_above_384_unknowns():
    """(12, 40, 20), 432 unknowns, priors on a third of the camera / marker blocks: schur_impl 1 picks the elimination whatever the
    priors say, 186 reduced columns go through the matrix-core accumulation."""
    _check("X12", 1, expect_elim=1)


def test_rsba_solve_honours_the_priors():
    cs, mc, summary, rows, final = pref.reference_run("P1")
    pr = _problem(cs)
    try:
        summ = pr.solve(_options(cs, 2))
        assert summ.num_iterations == len(rows) - 1 and abs(summ.final_cost - summary["final_cost"]) <= 1e-9 * summary["final_cost"]
        assert abs(summ.initial_cost - summary["initial_cost"]) <= 1e-9 * summary["initial_cost"]
        assert np.abs(pr.params.reshape(-1, 6) - final).max() < 1e-6
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 2. one step as a linear solve
def _one_step(cs, schur_impl, radius, min_lm, profile):
    pr = _problem(cs)
    try:
        s = capi.Solver(pr, _options(cs, schur_impl, max_num_iterations=1, function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0,
                                     initial_trust_region_radius=radius, min_lm_diagonal=min_lm))
        try:
            if profile:
                s.configure_run(1, 1)
            s.run()
            s.download()
            return pr.params.copy(), s.iterations(), s.eliminates_times(), (s.kernel_stats(64) if profile else {})
        finally:
            s.close()
    finally:
        pr.close()


_SYSTEMS = {}

STEPS = [(pid, impl, radius, min_lm) for pid in ("P1", "P3") for impl in (0, 2) for radius in (1e4, 1e-2) for min_lm in (1e-6, 0.0)]


@pytest.mark.parametrize("pid,schur_impl,radius,min_lm", STEPS)
def test_one_step_within_its_backward_error_bar(pid, schur_impl, radius, min_lm):
    """The step solves the reference's damped normal equations WITH the prior rows within marker_step_accuracy's bar; the log's
    scalars; a second solver returns the same bits."""
    cs, mc, _, _, _ = pref.reference_run(pid)
    key = (pid, schur_impl == 0, radius, min_lm)
    if key not in _SYSTEMS:
        _SYSTEMS[key] = pref.PriorSystem(mc, mc.x0(), radius, dense=schur_impl == 0, min_lm=min_lm)
    sysm = _SYSTEMS[key]
    x1_full, log, elim, stats = _one_step(cs, schur_impl, radius, min_lm, profile=True)
    x1_again, log_again, _, _ = _one_step(cs, schur_impl, radius, min_lm, profile=False)
    assert elim == (1 if schur_impl == 2 else 0)
    assert log.shape[0] == 2 and int(log[1, 7]) == 3, "the step was not accepted: %s" % (log,)
    want_kernels = {"k_marker_prior_rows", "k_marker_system"} if schur_impl == 0 else {"k_mc_prior_system", "k_mc_prior_candidate", "k_marker_reduce"}
    assert want_kernels <= set(stats), sorted(stats)
    x1 = mc.compact(x1_full)
    r = sysm.check(x1)
    print("\nPRIORSTEP %s schur_impl %d radius %g min_lm %g: n %d m %d kappa %.2f eta %.2e bar %.2e (recovery %.1e) eta/bar %.2e" % (
        pid, schur_impl, radius, min_lm, sysm.n, sysm.m, sysm.kappa, r["eta"], r["bar"], r["recovery"], r["ratio"]))
    checks = [("backward error", r["eta"] <= r["bar"], r)]
    cost0, gmax0, radius0 = log[0, 1], log[0, 3], log[0, 6]
    cost_change, step_norm, rel = log[1, 2], log[1, 4], log[1, 5]
    nd, tol = sysm.step_norm_tolerance(x1)
    mcc, mcc_tol = sysm.model_cost_change(x1)
    cand_ref = mc.cost(x1)[0]
    cand = cost0 - cost_change
    print("       cost %.1e  gmax %.1e  step_norm %.1e (tol %.1e)  mcc %.1e (tol %.1e)  candidate %.1e  cost(x1) %.1e" % (
        abs(cost0 - sysm.cost) / sysm.cost, abs(gmax0 - sysm.gmax) / sysm.gmax, abs(step_norm - nd) / nd, tol / nd,
        abs(cost_change / rel - mcc) / abs(mcc), mcc_tol / abs(mcc), abs(cand - cand_ref) / cand_ref, abs(log[1, 1] - cand_ref) / cand_ref))
    start = np.asarray(cs["prob"]["params"], float)
    fixed = np.setdiff1d(np.arange(start.size // 6), mc.free_blocks)
    checks += [
        ("radius", radius0 == radius, radius0),
        ("cost", abs(cost0 - sysm.cost) <= 1e-12 * sysm.cost, (cost0, sysm.cost)),
        ("gradient_max_norm", abs(gmax0 - sysm.gmax) <= 1e-11 * sysm.gmax, (gmax0, sysm.gmax)),
        ("step_norm", abs(step_norm - nd) <= tol, (step_norm, nd, tol)),
        ("model cost change", abs(cost_change / rel - mcc) <= mcc_tol + 2 * U * abs(mcc), (cost_change / rel, mcc, mcc_tol)),
        ("candidate cost", abs(cand - cand_ref) <= 1e-12 * cand_ref + U * (abs(cost_change) + cand_ref), (cand, cand_ref)),
        ("cost re-evaluated at x1", abs(log[1, 1] - cand_ref) <= 1e-12 * cand_ref, (log[1, 1], cand_ref)),
        ("masked components: an exact zero step", np.array_equal(x1_full[mc.masked_slots], start[mc.masked_slots]), None),
        ("constant, base and unreferenced blocks", np.array_equal(x1_full.reshape(-1, 6)[fixed], start.reshape(-1, 6)[fixed]), None),
        ("second solver: x1", np.array_equal(x1_again, x1_full), float(np.abs(x1_again - x1_full).max())),
        ("second solver: log", np.array_equal(log_again, log), (log_again, log)),
    ]
    failures = ["%s: %s" % (what, detail) for what, ok, detail in checks if not ok]
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 3. path switches
_DEFAULT_RUN = {}


@pytest.mark.parametrize("env", SWITCHES + [{"RSBA_MT_SPLIT": "0"}, {"RSBA_MT_SPLIT_BACKSUB": "1"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_switches(env, tmp_path):
    """Every switch tests/test_gpu_marker_subset.py::test_switches walks, each in a child process with the switch in its environment,
    on P1 at the parity bar: the split back-substitution (the default, and asked for by name) and the wavefront-per-time one
    (RSBA_MT_SPLIT_BACKSUB=0).  What ran: the child's kernel names hold the two prior kernels and the split elimination's — never
    k_time_eliminate: a solver with priors runs the loss instances, which keep the split elimination under RSBA_MT_SPLIT=0 (rsba.h), so
    that case returns the default path's bits.  The back-substitutions share one timer name; that RSBA_MT_SPLIT_BACKSUB=0 took the
    other one (k_time_backsub_terms, with the extra bp_time entry) shows in the bits, which differ from the default's."""
    out = str(tmp_path / "switch.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "prior_switch_worker.py"), out], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    assert int(z["elim"]) == 1
    names = set(str(k) for k in z["kernels"])
    assert {"k_mc_prior_system", "k_mc_prior_candidate", "k_mc_slot_products", "k_mc_time_products", "k_mc_accumulate", "k_marker_reduce",
            "k_time_backsub_terms", "k_marker_schur_finish"} <= names and "k_time_eliminate" not in names, sorted(names)
    if "default" not in _DEFAULT_RUN:
        _DEFAULT_RUN["default"] = _solve(pref.case("P1"), 2)
    _, log_d, x_d, _, _ = _DEFAULT_RUN["default"]
    same = np.array_equal(z["params"], x_d) and np.array_equal(z["log"][:, 1:8], log_d[:, 1:8])
    if env in ({"RSBA_MT_SPLIT": "0"}, {"RSBA_MT_SPLIT_BACKSUB": "1"}):
        assert same, "the switch is documented as not taken / as the default: the default path's bits"
    if env.get("RSBA_MT_SPLIT_BACKSUB") == "0":
        assert not same, "another back-substitution sums in another order: the default's bits mean the switch was not taken"
    _compare("P1", ",".join("%s=%s" % kv for kv in env.items()), [int(v) for v in z["summary"]], float(z["final_cost"]), z["log"], z["params"], float(z["rms"]))


# ------------------------------------------------------------------------------------------------ 4. the two paths
@pytest.mark.parametrize("pid", ["P1", "P3"])
def test_dense_and_eliminating_agree(pid):
    cs = pref.case(pid)
    s0, log0, x0, rms0, e0 = _solve(cs, 0)
    s2, log2, x2, rms2, e2 = _solve(cs, 2)
    assert (e0, e2) == (0, 1) and log0.shape == log2.shape and np.array_equal(log0[:, 7], log2[:, 7])
    assert np.abs(log0[:, 1] - log2[:, 1]).max() <= 1e-9 * log0[:, 1].max()
    a, b = x0.reshape(-1, 6), x2.reshape(-1, 6)
    err = np.abs(a - b).max(axis=1) / np.maximum(np.abs(a).max(axis=1), 1e-12)
    print("%s: dense against eliminating, block difference %.2e (bar 1e-6)" % (pid, err.max()))
    assert err.max() < 1e-6 and abs(rms0 - rms2) <= 1e-4


# ------------------------------------------------------------------------------------------------ 5. identities
def _stats(cs, schur_impl, priors, clear=False):
    pr = _problem(cs, priors)
    if clear:
        for b in priors:
            pr.set_block_prior(6 * b, None)
        assert pr.num_block_priors == 0
    s = capi.Solver(pr, _options(cs, schur_impl, profile_kernels=1))
    try:
        nres = s.num_residuals
        summ, log, x = _run(s, pr)
        costs = s.final_costs()
        return {k: n for k, (n, _) in s.kernel_stats(64).items()}, log, x, costs, nres
    finally:
        s.close()
        pr.close()


@pytest.mark.parametrize("schur_impl,pid", [(0, "P1"), (2, "P1"), (1, "X12")], ids=["dense", "eliminated", "default_12x40x20"])
def test_no_priors_are_no_priors(schur_impl, pid):
    """Priors set and then removed give the bits of a problem that never had any — parameters, log and costs — and the solver launches
    the same kernels the same number of times: none of the prior kernels.  With priors they join."""
    cs = pref.case(pid)
    plain, log0, x0, costs0, n0 = _stats(cs, schur_impl, None)
    cleared, log1, x1, costs1, n1 = _stats(cs, schur_impl, cs["priors"], clear=True)
    assert log0.shape[0] > 3 and plain == cleared and not (PRIOR_KERNELS & set(plain))
    np.testing.assert_array_equal(log1, log0)
    np.testing.assert_array_equal(x1, x0)
    assert costs1 == costs0 and n1 == n0 == 8 * cs["prob"]["N"]
    assert set(plain) == (DENSE_KERNELS if schur_impl == 0 else ELIM_KERNELS)
    with_p, log2, x2, _, n2 = _stats(cs, schur_impl, cs["priors"])
    added = {"k_marker_prior_rows"} if schur_impl == 0 else {"k_mc_prior_system", "k_mc_prior_candidate"}
    assert added <= set(with_p) and n2 == 8 * cs["prob"]["N"] + 6 * len(cs["priors"])
    assert not np.array_equal(x2, x0)


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_repeated_runs_and_a_rerun_from_the_start_are_bit_identical(schur_impl):
    cs = pref.case("P3")
    start = np.asarray(cs["prob"]["params"], float)
    pr = _problem(cs)
    s = capi.Solver(pr, _options(cs, schur_impl))
    try:
        _, log0, x0 = _run(s, pr)
        _, log1, x1 = _run(s, pr)
        s.set_parameters(start)
        _, log2, x2 = _run(s, pr)
    finally:
        s.close()
        pr.close()
    _, log, x, _, _ = _solve(cs, schur_impl)
    assert log.shape[0] > 3
    for lg, xx in ((log0, x0), (log1, x1), (log2, x2)):
        np.testing.assert_array_equal(lg, log)
        np.testing.assert_array_equal(xx, x)


# ------------------------------------------------------------------------------------------------ 6. queries
def _masked_rows(rows, mc):
    bits = {6 * int(b): [q for q in range(6) if (m >> q) & 1] for b, m in mc.masks.items() if b in set(int(v) for v in mc.free_blocks)}
    out = []
    for r, blocks in rows:
        nb = []
        for off, J in blocks:
            if off in bits:
                J = np.array(J, float)
                J[:, bits[off]] = 0.0
            nb.append((off, J))
        out.append((r, nb))
    return out


def _prior_terms(cs, mc, x):
    """The priors at x (all parameters), ambient layout: per prior (offset, live, r (6), A~ (6 x 6, zero columns where masked),
    the bound on an entry of r)."""
    full = np.asarray(x, float).reshape(-1, 6)
    free = set(int(b) for b in mc.free_blocks)
    out = []
    for b, (A, v) in sorted(cs["priors"].items()):
        d = full[b] - v
        At = A.copy()
        m = mc.masks.get(b, 0) if b in free else 0
        At[:, [q for q in range(6) if (m >> q) & 1]] = 0.0
        out.append((6 * b, b in free, A @ d, At, 8 * U * (np.abs(A) @ np.abs(d))))
    return out


def _check_queries(cs, mc, s, x, label):
    """cost, residuals, gradient and the CRS matrix at x: the observations' part under test_gpu_marker_subset's bars, the priors'
    rows behind it."""
    raw = [_masked_rows(er.marker_rows(o, cs["prob"], x, cs["variant"]), mc) for o in (oracle_lib.load(), oracle_lib.load_nocontract())]
    const = [(6 * b, 6) for b in cs["constant_blocks"]]
    slots = mc.masked_slots
    N, K = mc.N, len(cs["priors"])
    terms = _prior_terms(cs, mc, x)
    assert s.num_residuals == 8 * N + 6 * K
    out = {}
    for apply_loss in (True, False):   # (both values on every case: a prior is in the cost and the gradient for either)
        want, alt = (er.finish(rw, x.size, const, cs["loss"], cs["a"], apply_loss) for rw in raw)
        rbar = 16.0 * max(np.abs(want.residuals - alt.residuals).max(), 4.0 * np.spacing(np.abs(cs["prob"]["obs"]).max()))
        gbar = want.abs_J * rbar + (64 + want.n_terms) * U * want.abs_Jr
        cbar = rbar * np.abs(want.residuals).sum() + N * U * want.cost
        # the priors on top: no loss for either value of apply_loss
        want_g, want_cost = want.gradient.copy(), want.cost
        for off, live, r, At, rb in terms:
            want_cost += 0.5 * float(r @ r)
            cbar += float(np.abs(r) @ rb) + 16 * U * 0.5 * float(r @ r)
            if live:
                want_g[off:off + 6] += At.T @ r
                gbar[off:off + 6] += np.abs(At).T @ rb + 8 * U * (np.abs(At).T @ np.abs(r))
        cbar += U * want_cost
        cost, r, g = s.evaluate(apply_loss_function=apply_loss)
        assert r.size == 8 * N + 6 * K
        live = want.live.copy()
        live[slots] = False
        q_r = np.abs(r[:8 * N] - want.residuals).max() / rbar
        for k, (off, _, rp, _, rb) in enumerate(terms):   # residual order: ascending parameter offset behind the observations'
            got = r[8 * N + 6 * k:8 * N + 6 * k + 6]
            assert np.all(np.abs(got - rp) <= rb), (off, got, rp, rb)
        q_g = (np.abs(g - want_g)[live] / gbar[live]).max()
        q_c = abs(cost - want_cost) / cbar
        jref, jalt = (jr.assemble(rw, x.size, const, cs["loss"], cs["a"], apply_loss) for rw in raw)
        jbar = 16.0 * max((np.abs(jref.values - jalt.values) / jref.scale).max(), C_JAC * U)
        shape, indptr, indices = s.jacobian_structure()
        vals = s.evaluate_jacobian(apply_loss_function=apply_loss)
        nnz = jref.indptr[-1]
        assert shape == (8 * N + 6 * K, x.size)
        assert np.array_equal(indptr[:8 * N + 1], jref.indptr) and np.array_equal(indices[:nnz], jref.indices)
        q_j = (np.abs(vals[:nnz] - jref.values) / jref.scale).max() / jbar
        at = nnz
        for k, (off, is_live, _, At, _) in enumerate(terms):   # six rows per prior: the block's six columns, A's values, zeros stored
            for i in range(6):
                row = 8 * N + 6 * k + i
                assert indptr[row] == at
                if is_live:
                    assert np.array_equal(indices[at:at + 6], off + np.arange(6)) and np.array_equal(vals[at:at + 6], At[i]), (off, i)
                    at += 6
                assert indptr[row + 1] == at      # (empty for a prior on a constant block)
        assert at == indices.size == vals.size
        jtr = jr.transpose_times(shape, indptr, indices, vals, r)
        q_t = (np.abs(jtr - g)[live] / gbar[live]).max()
        print("%s apply_loss=%d: error / bar  residual %.3f  gradient %.3f  cost %.3f  jacobian %.3f  J'r %.3f" % (label, apply_loss, q_r, q_g, q_c, q_j, q_t))
        assert q_r <= 1.0 and q_g <= 1.0 and q_c <= 1.0 and q_j <= 1.0 and q_t <= 1.0, (q_r, q_g, q_c, q_j, q_t)
        if slots.size:
            in_masked = np.isin(indices, slots)
            assert in_masked.any() and np.all(vals[in_masked] == 0.0)
            assert np.isin(indices[nnz:], slots).any()      # a mask on a prior block: exact zeros in the prior's rows too
        assert np.all(g[slots] == 0.0) and np.all(jtr[slots] == 0.0)
        assert np.all(g[~want.live] == 0.0) and np.all(jtr[~want.live] == 0.0)
        out[apply_loss] = (cost, r, g, vals)
    return out


def _check_covariance(cs, mc, s, x, label):
    """Blocks of inv(H_ref), H_ref = J'J + sum A'A at x: prior blocks, blocks without one, times, camera x marker, time x time and
    time x camera pairs, to 1e-8 of the block's largest entry (test_gpu_marker_subset's bar); zeros where the lift has them."""
    prob = cs["prob"]
    C, T = prob["C"], prob["T"]
    cov, fb = sref.covariance(mc, mc.compact(x))
    pos = {int(b): 6 * k for k, b in enumerate(fb)}
    s.covariance_compute()
    cam_p, cam, mk1, mk2 = (2 if 2 in pos else 3), 1, C + T + 1, C + T + 2
    times = [int(b) for b in fb if C <= b < C + T]
    tim, other_t = times[3], times[0]
    pairs = [(cam_p, cam_p), (cam, cam), (mk1, mk1), (mk2, mk2), (tim, tim), (cam, mk1), (mk2, cam_p), (cam_p, tim), (tim, mk2), (tim, other_t), (other_t, tim), (mk1, mk2)]
    got = s.covariance_blocks([(6 * a, 6 * b) for a, b in pairs])
    worst = 0.0
    for (a, b), blk in zip(pairs, got):
        want = cov[pos[a]:pos[a] + 6, pos[b]:pos[b] + 6]
        worst = max(worst, float(np.abs(blk - want).max() / np.abs(want).max()))
        assert np.array_equal(blk == 0.0, want == 0.0), (a, b)
    for a, b in ((mk1, mk1), (mk2, cam)):
        want = cov[pos[a]:pos[a] + 6, pos[b]:pos[b] + 6]
        worst = max(worst, float(np.abs(s.covariance_block(6 * a, 6 * b) - want).max() / np.abs(want).max()))
    tc = s.time_covariances()
    for t in (tim, other_t):
        want = cov[pos[t]:pos[t] + 6, pos[t]:pos[t] + 6]
        worst = max(worst, float(np.abs(tc[t - C] - want).max() / np.abs(want).max()))
    print("%s: covariance, worst block error %.2e (bar 1e-8)" % (label, worst))
    assert worst <= 1e-8


@pytest.mark.parametrize("pid", ["P1", "P3"])
def test_evaluate_jacobian_and_covariance(pid):
    cs, mc, _, _, _ = pref.reference_run(pid)
    if pid == "P3":
        # off centre: at b = the start values a prior on a constant block has a zero residual for ever
        cs = dict(cs, priors={b: (A, v + (0.01 if b in cs["constant_blocks"] else 0.0)) for b, (A, v) in cs["priors"].items()})
        mc = pref.chain_of(cs)
    at_start = {}
    for impl in (0, 2):
        pr = _problem(cs)
        s = capi.Solver(pr, _options(cs, impl))
        try:
            assert s.eliminates_times() == (1 if impl == 2 else 0)
            x0 = np.asarray(cs["prob"]["params"], float)
            at_start[impl] = _check_queries(cs, mc, s, x0, "%s schur_impl %d, before any run" % (pid, impl))
            _check_covariance(cs, mc, s, x0, "%s schur_impl %d, before any run" % (pid, impl))
            s.run()
            s.download()
            x = pr.params.copy()
            _check_queries(cs, mc, s, x, "%s schur_impl %d, after a run" % (pid, impl))
            _check_covariance(cs, mc, s, x, "%s schur_impl %d, after a run" % (pid, impl))
        finally:
            s.close()
            pr.close()
    for apply_loss, (cost, r, g, vals) in at_start[0].items():   # the two paths share the query kernels: identical bits before any run
        cost2, r2, g2, vals2 = at_start[2][apply_loss]
        assert cost == cost2
        for a, b in ((r, r2), (g, g2), (vals, vals2)):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. a prior cures a rank deficiency
@pytest.mark.parametrize("schur_impl", [0, 2])
def test_a_prior_cures_a_rank_deficiency(schur_impl):
    """4x40x6 with every observation of marker 3 at weight 0: covariance_compute reports the rank deficiency; with A = diag(a_q) on
    marker 3 it returns, the block is diag(1 / a_q^2), its cross blocks with every other block are zero and the solve matches the
    reference.  A cross block has no entry to be relative to: it is held to 1e-8 of sqrt(max |C_aa| max |C_bb|), the size the
    Cauchy-Schwarz inequality allows it."""
    base = pref.case("P1")
    prob = base["prob"]
    C, T = prob["C"], prob["T"]
    mk3 = C + T + 3
    w = np.where(np.asarray(prob["m"]) == 3, 0.0, 1.0)
    a_q = np.array([50.0, 40.0, 30.0, 20.0, 10.0, 5.0])
    cs = dict(base, weights=w, priors={})
    pr = _problem(cs)
    s = capi.Solver(pr, _options(cs, schur_impl))
    try:
        with pytest.raises(capi.RsbaError) as e:
            s.covariance_compute()
        assert e.value.code == capi.ERR_RANK_DEFICIENT
    finally:
        s.close()
        pr.close()
    start = np.asarray(prob["params"], float).reshape(-1, 6)
    cs = dict(cs, priors={mk3: (np.diag(a_q), start[mk3].copy())})
    mc = pref.chain_of(cs)
    x, summary, rows = pref.minimise(mc)
    pr = _problem(cs)
    s = capi.Solver(pr, _options(cs, schur_impl))
    try:
        summ, log, params = _run(s, pr)
        _, rms = pr.reprojection_error()
        s.covariance_compute()
        blk = s.covariance_block(6 * mk3, 6 * mk3)
        want = np.diag(1.0 / a_q ** 2)
        assert np.abs(blk - want).max() <= 1e-8 * want.max(), blk
        others = [int(b) for b in mc.free_blocks if b != mk3]
        diag = s.covariance_blocks([(6 * b, 6 * b) for b in others])
        cross = s.covariance_blocks([(6 * mk3, 6 * b) for b in others])
        for b, d, c in zip(others, diag, cross):
            assert np.abs(c).max() <= 1e-8 * np.sqrt(want.max() * np.abs(d).max()), (b, c)
    finally:
        s.close()
        pr.close()
    _compare_run((cs, mc, summary, rows, mc.full(x)), "rank cure schur_impl %d" % schur_impl, (summ.termination_type, summ.stop_reason, summ.num_iterations), summ.final_cost, log, params, rms)
    np.testing.assert_array_equal(params.reshape(-1, 6)[mk3], start[mk3])   # nothing pulls marker 3 away from the prior's centre


# ------------------------------------------------------------------------------------------------ 8. the solver-level setter
@pytest.mark.parametrize("schur_impl", [0, 2])
def test_solver_level_setter(schur_impl):
    cs = pref.case("P1")
    prob = cs["prob"]
    C, T = prob["C"], prob["T"]
    start = np.asarray(prob["params"], float)
    tight = {b: (A * 4.0, v) for b, (A, v) in cs["priors"].items() if b in (2, C + T + 1)}   # sigma 0.02 -> 0.005 on two blocks
    second = {**cs["priors"], **tight}
    _, log_a, x_a, _, _ = _solve(cs, schur_impl)
    _, log_b, x_b, _, _ = _solve(cs, schur_impl, priors=second)
    assert not np.array_equal(x_a, x_b)
    pr = _problem(cs)
    s = capi.Solver(pr, _options(cs, schur_impl))
    try:
        _, log0, x0 = _run(s, pr)
        np.testing.assert_array_equal(x0, x_a)
        s.covariance_compute()
        before = s.covariance_block(12, 12)
        for b, (A, v) in tight.items():
            s.set_block_prior(6 * b, A, v)
        with pytest.raises(capi.RsbaError):      # the covariance result was dropped by the setter
            s.covariance_block(12, 12)
        s.set_parameters(start)
        _, log1, x1 = _run(s, pr)
        np.testing.assert_array_equal(log1, log_b)
        np.testing.assert_array_equal(x1, x_b)
        s.covariance_compute()
        assert not np.array_equal(s.covariance_block(12, 12), before)
        # a block without a prior at create, a time block, NULL and non-finite values: refused, and the next run has the old bits
        lib = capi.load()
        A, v = np.eye(6), np.zeros(6)
        vp = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)   # noqa: E731
        assert lib.rsba_solver_set_block_prior(s.h, 6 * 1, vp(A), vp(v)) == capi.ERR_UNSUPPORTED
        assert lib.rsba_solver_set_block_prior(s.h, 6 * (C + 1), vp(A), vp(v)) == capi.ERR_UNSUPPORTED
        assert lib.rsba_solver_set_block_prior(s.h, 12, None, vp(v)) == capi.ERR_ARG
        assert lib.rsba_solver_set_block_prior(s.h, 12, vp(A), None) == capi.ERR_ARG
        assert lib.rsba_solver_set_block_prior(s.h, 12, vp(np.full((6, 6), np.nan)), vp(v)) == capi.ERR_ARG
        s.set_parameters(start)
        _, log2, x2 = _run(s, pr)
        np.testing.assert_array_equal(log2, log_b)
        np.testing.assert_array_equal(x2, x_b)
        assert pr.block_prior(12)[0][0, 0] == cs["priors"][2][0][0, 0]   # the problem's own copy is not touched
    finally:
        s.close()
        pr.close()
    # a solver without priors takes none
    pr = _problem(cs, priors=None)
    s = capi.Solver(pr, _options(cs, schur_impl))
    try:
        with pytest.raises(capi.RsbaError) as e:
            s.set_block_prior(12, np.eye(6), np.zeros(6))
        assert e.value.code == capi.ERR_UNSUPPORTED
    finally:
        s.close()
        pr.close()


# ------------------------------------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("schur_impl", [0, 2])
def test_a_prior_on_an_unreferenced_block_is_refused(schur_impl):
    """P1 without the observations of marker 2: a prior on marker 2 names a block outside the program — RSBA_ERR_UNSUPPORTED from
    rsba_solver_create and from rsba_solve; without that prior the problem solves."""
    cs = pref.case("P1")
    prob = cs["prob"]
    C, T = prob["C"], prob["T"]
    cut = wref.select_rows(prob, np.flatnonzero(np.asarray(prob["m"]) != 2))
    cs = dict(cs, prob=cut)
    pr = _problem(cs)
    try:
        with pytest.raises(capi.RsbaError) as e:
            capi.Solver(pr, _options(cs, schur_impl))
        assert e.value.code == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.RsbaError) as e:
            pr.solve(_options(cs, schur_impl))
        assert e.value.code == capi.ERR_UNSUPPORTED
        np.testing.assert_array_equal(pr.params, np.asarray(cut["params"], float))
        pr.set_block_prior(6 * (C + T + 2), None)
        assert pr.solve(_options(cs, schur_impl)).num_iterations > 3
    finally:
        pr.close()
