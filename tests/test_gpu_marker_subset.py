"""Constant components of a pose block (ceres::SubsetParameterization, rsba_problem_set_parameter_subset_constant) on the marker-chain
models, through the C ABI, against tests/marker_subset_ref.py — a numpy reference that REMOVES the masked columns, so it does not
share the device's formulation (zero columns, a unit diagonal; tests/test_marker_subset_ref_cpu.py shows the two agree).

Bars (BASELINE's, as tests/test_gpu_marker_weights.py holds them): the same accept / reject sequence, iteration count and termination,
every iterate's cost to 1e-9 relative, every block of the raw parameters to 1e-6 relative (no gauge fit), the final RMS to 1e-4 px;
every masked component and every block that is not free keeps the bits of its start value.  The cases and their decision margins
are pinned without a device by tests/test_marker_subset_ref_cpu.py.

One LM step (test_one_step_*): tests/marker_step_accuracy.py's backward-error bar with n the number of FREE components.  A mask adds no
arithmetic to row formation on either path: the dense path stores the rows as without masks and then overwrites the masked columns
with 0.0; the time-eliminating path forms the small products as without masks and overwrites the masked entries with 0.0 (1.0 on a
masked diagonal).  An overwritten entry carries no rounding at all, the others are the parent's bits, so the bar's rounding count
(m + 2 x 37 per entry of A) stays the parent's.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import evaluate_ref as er
import jacobian_ref as jr
import marker_loss_ref as ref
import marker_subset_ref as sref
import marker_weight_ref as wref
import oracle_lib
from realsensecalibration_amd import capi
from realsensecalibration_amd import synthetic as syn
from test_gpu_marker_weights import SWITCHES

pytestmark = pytest.mark.gpu

REASON = {"gradient": 1, "parameter": 2, "function": 3, "max_iterations": 4, "min_radius": 5, "invalid_steps": 6}
TERM = {"CONVERGENCE": 0, "NO_CONVERGENCE": 1, "FAILURE": 2}
U = 2.0 ** -53
HERE = os.path.dirname(os.path.abspath(__file__))
C_JAC = 37   # tests/test_gpu_jacobian.py's count for the marker chain


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


def _options(cs, schur_impl, **kw):
    return capi.default_options(schur_impl=schur_impl, huber_delta=cs["a"] if cs["loss"] != "none" else 0.0, loss_type=1 if cs["loss"] == "cauchy" else 0, **kw)


def _problem(cs, masks="case", prob=None):
    prob = cs["prob"] if prob is None else prob
    if cs.get("dist") is not None:
        prob = dict(prob, dist=cs["dist"])
    pr = capi.Problem.marker_chain(prob, capi.MODEL_MARKER_CHAIN_TEST2 if cs["variant"] == 1 else capi.MODEL_MARKER_CHAIN)
    for b in cs["constant_blocks"]:
        pr.set_parameter_block_constant(6 * b)
    if cs.get("weights") is not None:
        pr.set_observation_weights(cs["weights"])
    for b, m in (cs["masks"] if isinstance(masks, str) else (masks or {})).items():
        pr.set_parameter_subset_constant(6 * b, m)
    return pr


def _run(s, pr):
    summ = s.run()
    s.download()
    return summ, s.iterations(), pr.params.copy()


def _solve(cs, schur_impl, masks="case", prob=None, **kw):
    """-> (summary, log, parameters, rms, eliminates_times) of a fresh problem and solver."""
    pr = _problem(cs, masks, prob)
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


def _compare(sid, label, summary3, final_cost, log, params, rms):
    """A device solve of case sid against the reference's at the parity bar."""
    cs, mc, summary, rows, final = sref.reference_run(sid)
    assert tuple(summary3) == (TERM[summary["termination"]], REASON[summary["reason"]], len(rows) - 1), (summary3, summary)
    assert [int(v) for v in log[:, 7]] == [rw["valid"] + 2 * rw["successful"] for rw in rows]
    worst = max(abs(log[j, 1] - rw["cost"]) / rw["cost"] for j, rw in enumerate(rows))
    got = params.reshape(-1, 6)
    free = mc.free_blocks
    err = np.abs(got[free] - final[free]).max(axis=1) / np.maximum(np.abs(final[free]).max(axis=1), 1e-12)
    rms_ref = np.sqrt(summary["final_sumsq"] / (8.0 * cs["prob"]["N"]))
    print("%s %s: %d iterations, cost error %.2e (bar 1e-9), block error %.2e (bar 1e-6), rms %.6f against %.6f"
          % (sid, label, len(rows) - 1, worst, err.max(), rms, rms_ref))
    for j, rw in enumerate(rows):
        assert abs(log[j, 1] - rw["cost"]) <= 1e-9 * rw["cost"], "iterate %d: cost %.15e, reference %.15e" % (j, log[j, 1], rw["cost"])
    assert abs(final_cost - summary["final_cost"]) <= 1e-9 * summary["final_cost"]
    assert err.max() < 1e-6, "final parameters differ from the reference's by %.2e relative per block" % err.max()
    start = np.asarray(cs["prob"]["params"], float)
    fixed = np.setdiff1d(np.arange(got.shape[0]), free)
    np.testing.assert_array_equal(got[fixed], start.reshape(-1, 6)[fixed])
    assert mc.masked_slots.size > 0
    np.testing.assert_array_equal(params[mc.masked_slots], start[mc.masked_slots])   # every masked component: its start value's bits
    assert abs(rms - rms_ref) <= 1e-4, (rms, rms_ref)


def _check(sid, schur_impl, expect_elim=None):
    cs = sref.case(sid)
    summ, log, params, rms, elim = _solve(cs, schur_impl)
    assert elim == (expect_elim if expect_elim is not None else (1 if schur_impl == 2 else 0))
    _compare(sid, "schur_impl %d" % schur_impl, (summ.termination_type, summ.stop_reason, summ.num_iterations), summ.final_cost, log, params, rms)
    return params


# ------------------------------------------------------------------------------------------------ 1. whole solves
@pytest.mark.parametrize("schur_impl", [0, 2])
@pytest.mark.parametrize("sid", ["S1", "S2", "S3"])
def test_solve_matches_the_subset_reference(sid, schur_impl):
    """The issue's table on the dense path and with the time blocks eliminated."""
    _check(sid, schur_impl)


def test_default_path_above_384_unknowns():
    """(12, 40, 20), 420 ambient unknowns, masks on 9 of 72 blocks (cameras, times and markers): schur_impl 1 picks the elimination
    whatever the masks say, 180 reduced columns go through the matrix-core accumulation."""
    _check("X12", 1, expect_elim=1)


def test_dense_path_above_384_unknowns():
    """The same problem on the dense path: 420 columns, the 1024-thread instance of the one-workgroup system."""
    _check("X12", 0, expect_elim=0)


def test_rsba_solve_honours_the_masks():
    cs, mc, summary, rows, final = sref.reference_run("S2")
    pr = _problem(cs)
    try:
        summ = pr.solve(_options(cs, 2))
        assert summ.num_iterations == len(rows) - 1 and abs(summ.final_cost - summary["final_cost"]) <= 1e-9 * summary["final_cost"]
        start = np.asarray(cs["prob"]["params"], float)
        np.testing.assert_array_equal(pr.params[mc.masked_slots], start[mc.masked_slots])
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

STEPS = [(sid, impl, radius, 1e-6) for sid in ("S1", "S3") for impl in (0, 2) for radius in (1e4, 1e-2)] + [("S1", 0, 1e4, 0.0), ("S3", 2, 1e4, 0.0)]


@pytest.mark.parametrize("sid,schur_impl,radius,min_lm", STEPS)
def test_one_step_within_its_backward_error_bar(sid, schur_impl, radius, min_lm):
    """The step on the free components solves the reference's damped normal equations WITHOUT the masked columns within
    marker_step_accuracy's bar; the log's scalars; exact zeros on the masked components; a second solver returns the same bits.
    min_lm_diagonal = 0 once per path: nothing but the unit diagonal keeps a masked pivot positive."""
    cs, mc, _, _, _ = sref.reference_run(sid)
    key = (sid, schur_impl == 0, radius, min_lm)
    if key not in _SYSTEMS:
        _SYSTEMS[key] = sref.SubsetSystem(mc, mc.x0(), radius, dense=schur_impl == 0, min_lm=min_lm)
    sysm = _SYSTEMS[key]
    x1_full, log, elim, stats = _one_step(cs, schur_impl, radius, min_lm, profile=True)
    x1_again, log_again, _, _ = _one_step(cs, schur_impl, radius, min_lm, profile=False)
    assert elim == (1 if schur_impl == 2 else 0)
    assert log.shape[0] == 2 and int(log[1, 7]) == 3, "the step was not accepted: %s" % (log,)
    want_kernels = {"k_marker_subset_rows", "k_marker_system"} if schur_impl == 0 else {"k_mc_subset_slots", "k_mc_subset_cross", "k_mc_time_products", "k_mc_accumulate"}
    assert want_kernels <= set(stats), sorted(stats)
    x1 = mc.compact(x1_full)
    r = sysm.check(x1)
    print("\nSUBSTEP %s schur_impl %d radius %g min_lm %g: n %d (ambient %d) m %d kappa %.2f eta %.2e bar %.2e (recovery %.1e) eta/bar %.2e" % (
        sid, schur_impl, radius, min_lm, sysm.n, mc.ambient_n, sysm.m, sysm.kappa, r["eta"], r["bar"], r["recovery"], r["ratio"]))
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
    free_slots = np.setdiff1d((6 * mc.free_blocks[:, None] + np.arange(6)).ravel(), mc.masked_slots)
    checks += [
        ("radius", radius0 == radius, radius0),
        ("cost", abs(cost0 - sysm.cost) <= 1e-12 * sysm.cost, (cost0, sysm.cost)),
        ("gradient_max_norm (over the free components)", abs(gmax0 - sysm.gmax) <= 1e-11 * sysm.gmax, (gmax0, sysm.gmax)),
        ("step_norm", abs(step_norm - nd) <= tol, (step_norm, nd, tol)),
        ("model cost change", abs(cost_change / rel - mcc) <= mcc_tol + 2 * U * abs(mcc), (cost_change / rel, mcc, mcc_tol)),
        ("candidate cost", abs(cand - cand_ref) <= 1e-12 * cand_ref + U * (abs(cost_change) + cand_ref), (cand, cand_ref)),
        ("cost re-evaluated at x1", abs(log[1, 1] - cand_ref) <= 1e-12 * cand_ref, (log[1, 1], cand_ref)),
        ("masked components: an exact zero step", np.array_equal(x1_full[mc.masked_slots], start[mc.masked_slots]), None),
        ("constant, base and unreferenced blocks", np.array_equal(x1_full.reshape(-1, 6)[fixed], start.reshape(-1, 6)[fixed]), None),
        ("every free component moved", bool(np.all(x1_full[free_slots] != start[free_slots])), None),
        ("second solver: x1", np.array_equal(x1_again, x1_full), float(np.abs(x1_again - x1_full).max())),
        ("second solver: log", np.array_equal(log_again, log), (log_again, log)),
    ]
    failures = ["%s: %s" % (what, detail) for what, ok, detail in checks if not ok]
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 3. path switches
@pytest.mark.parametrize("env", SWITCHES + [{"RSBA_MT_SPLIT": "0"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_switches(env, tmp_path):
    """Every switch tests/test_gpu_marker_weights.py::test_switches walks (and RSBA_MT_SPLIT=0), each in a child process with the
    switch in its environment, on S1 with masks at the parity bar.  (A masked solver keeps the split elimination and the split
    back-substitution under RSBA_MT_SPLIT=0 / RSBA_MT_SPLIT_BACKSUB=0: the masks are applied to their products.)"""
    out = str(tmp_path / "switch.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "subset_switch_worker.py"), out], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    assert int(z["elim"]) == 1
    _compare("S1", ",".join("%s=%s" % kv for kv in env.items()), [int(v) for v in z["summary"]], float(z["final_cost"]), z["log"], z["params"], float(z["rms"]))


# ------------------------------------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("schur_impl", [0, 2])
@pytest.mark.parametrize("sid", ["S1w", "D1"])
def test_masks_compose_with_weights_loss_and_distortion(sid, schur_impl):
    """S1w: S1's data and masks under 4x40x6_frac_huber's weights and Huber 2 (the kLoss instances); D1: tests/marker_distortion_ref.py's
    4x40x6 rig, detections made through its coefficients (the kDist instances)."""
    _check(sid, schur_impl)


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_the_block_call_wins_over_a_mask(schur_impl):
    """S3 plus a mask on each of its constant blocks (a camera, a time, a marker): the bits of S3 without those masks."""
    cs = sref.case("S3")
    more = dict(cs["masks"])
    more.update({b: 0b010110 for b in cs["constant_blocks"]})
    _, log0, x0, rms0, _ = _solve(cs, schur_impl)
    _, log1, x1, rms1, _ = _solve(cs, schur_impl, masks=more)
    assert log0.shape[0] > 3
    np.testing.assert_array_equal(log0, log1)
    np.testing.assert_array_equal(x0, x1)
    assert rms0 == rms1


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_masks_on_base_and_unreferenced_blocks_are_ignored(schur_impl):
    """S1 without the observations of time 5 (an unreferenced block), masks on it and on the base blocks camera 0 / marker 0."""
    cs = sref.case("S1")
    prob = cs["prob"]
    C, T = prob["C"], prob["T"]
    prob = wref.select_rows(prob, np.flatnonzero(np.asarray(prob["t"]) != 5))
    more = dict(cs["masks"])
    more.update({0: 0b000111, C + T: 0b101010, C + 5: 0b000001})
    _, log0, x0, rms0, _ = _solve(cs, schur_impl, prob=prob)
    _, log1, x1, rms1, _ = _solve(cs, schur_impl, masks=more, prob=prob)
    assert log0.shape[0] > 3
    np.testing.assert_array_equal(log0, log1)
    np.testing.assert_array_equal(x0, x1)
    assert rms0 == rms1
    start = np.asarray(prob["params"], float).reshape(-1, 6)
    np.testing.assert_array_equal(x1.reshape(-1, 6)[[0, C + T, C + 5]], start[[0, C + T, C + 5]])


# ------------------------------------------------------------------------------------------------ 5. identities
def _stats(cs, schur_impl, masks, clear=False):
    pr = _problem(cs, masks)
    if clear:
        for b in masks:
            pr.set_parameter_subset_constant(6 * b, 0)
    s = capi.Solver(pr, _options(cs, schur_impl, profile_kernels=1))
    try:
        summ, log, x = _run(s, pr)
        return {k: n for k, (n, _) in s.kernel_stats(64).items()}, log, x
    finally:
        s.close()
        pr.close()


@pytest.mark.parametrize("schur_impl,sid", [(0, "S1"), (2, "S1"), (1, "X12")], ids=["dense", "eliminated", "default_12x40x20"])
def test_zero_masks_are_no_masks(schur_impl, sid):
    """Masks all zero, and masks set then cleared, give the bits of a problem that never had any, and the solver launches the same
    kernels the same number of times; with masks the subset kernels join them."""
    cs = sref.case(sid)
    plain, log0, x0 = _stats(cs, schur_impl, None)
    zeros, log1, x1 = _stats(cs, schur_impl, {b: 0 for b in cs["masks"]})
    cleared, log2, x2 = _stats(cs, schur_impl, cs["masks"], clear=True)
    assert log0.shape[0] > 3 and plain == zeros == cleared
    for log, x in ((log1, x1), (log2, x2)):
        np.testing.assert_array_equal(log, log0)
        np.testing.assert_array_equal(x, x0)
    masked, log3, x3 = _stats(cs, schur_impl, cs["masks"])
    added = {"k_marker_subset_rows"} if schur_impl == 0 else {"k_mc_subset_slots", "k_mc_subset_cross"}
    assert set(masked) == set(plain) | added and not (added & set(plain))
    assert not np.array_equal(x3, x0)
    if schur_impl == 0:
        assert set(plain) == {"k_marker_eval", "k_marker_system", "k_marker_candidate"}
    else:
        assert set(plain) == {"k_pose_constants", "k_mc_slot_products", "k_mc_time_products", "k_mc_cross", "k_mc_accumulate", "k_marker_reduce",
                              "k_marker_reduced_solve", "k_time_backsub_terms", "k_marker_schur_finish"}


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_repeated_runs_and_a_rerun_from_the_start_are_bit_identical(schur_impl):
    cs = sref.case("S3")
    start = np.asarray(cs["prob"]["params"], float)
    pr = _problem(cs)
    s = capi.Solver(pr, _options(cs, schur_impl))
    try:
        _, log0, x0 = _run(s, pr)
        _, log1, x1 = _run(s, pr)          # from the solution: the start of every run is the uploaded / set state
        s.set_parameters(start)
        _, log2, x2 = _run(s, pr)
        # new values for masked components are taken, and held
        moved = start.copy()
        slots = sref.reference_run("S3")[1].masked_slots
        moved[slots] += 1e-3
        s.set_parameters(moved)
        _, _, x3 = _run(s, pr)
    finally:
        s.close()
        pr.close()
    _, log, x, _, _ = _solve(cs, schur_impl)
    assert log.shape[0] > 3
    for lg, xx in ((log0, x0), (log1, x1), (log2, x2)):
        np.testing.assert_array_equal(lg, log)
        np.testing.assert_array_equal(xx, x)
    np.testing.assert_array_equal(x3[slots], moved[slots])
    assert np.all(x3[slots] != x[slots])


@pytest.mark.parametrize("sid", ["S1", "S3"])
def test_dense_and_eliminating_agree(sid):
    cs = sref.case(sid)
    s0, log0, x0, rms0, e0 = _solve(cs, 0)
    s2, log2, x2, rms2, e2 = _solve(cs, 2)
    assert (e0, e2) == (0, 1) and log0.shape == log2.shape and np.array_equal(log0[:, 7], log2[:, 7])
    assert np.abs(log0[:, 1] - log2[:, 1]).max() <= 1e-9 * log0[:, 1].max()
    a, b = x0.reshape(-1, 6), x2.reshape(-1, 6)
    err = np.abs(a - b).max(axis=1) / np.maximum(np.abs(a).max(axis=1), 1e-12)
    print("%s: dense against eliminating, block difference %.2e (bar 1e-6)" % (sid, err.max()))
    assert err.max() < 1e-6 and abs(rms0 - rms2) <= 1e-4


# ------------------------------------------------------------------------------------------------ 6. queries
def _masked_rows(rows, mc):
    """evaluate_ref rows with the masked components' columns set to zero: what Ceres' local Jacobian leaves of them, in the ambient
    layout the device keeps."""
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


def _check_queries(cs, mc, s, x, label):
    """cost, residuals, gradient and the CRS values at x (all parameters) under test_gpu_evaluate's / test_gpu_jacobian's bars (the
    reference rows are the oracle's, both builds, their masked columns zeroed); exact zeros in the masked slots; J'r = gradient."""
    raw = [_masked_rows(er.marker_rows(o, cs["prob"], x, cs["variant"]), mc) for o in (oracle_lib.load(), oracle_lib.load_nocontract())]
    const = [(6 * b, 6) for b in cs["constant_blocks"]]
    slots = mc.masked_slots
    out = {}
    for apply_loss in ((True, False) if cs["loss"] != "none" else (True,)):
        want, alt = (er.finish(rw, x.size, const, cs["loss"], cs["a"], apply_loss) for rw in raw)
        rbar = 16.0 * max(np.abs(want.residuals - alt.residuals).max(), 4.0 * np.spacing(np.abs(cs["prob"]["obs"]).max()))
        gbar = want.abs_J * rbar + (64 + want.n_terms) * U * want.abs_Jr
        cbar = rbar * np.abs(want.residuals).sum() + mc.N * U * want.cost
        cost, r, g = s.evaluate(apply_loss_function=apply_loss)
        live = want.live.copy()
        assert np.all(live[slots]) and np.all(want.gradient[slots] == 0.0)
        live[slots] = False   # (their bar is 0: held exactly below)
        q_r = np.abs(r - want.residuals).max() / rbar
        q_g = (np.abs(g - want.gradient)[live] / gbar[live]).max()
        q_c = abs(cost - want.cost) / cbar
        jref, jalt = (jr.assemble(rw, x.size, const, cs["loss"], cs["a"], apply_loss) for rw in raw)
        jbar = 16.0 * max((np.abs(jref.values - jalt.values) / jref.scale).max(), C_JAC * U)
        shape, indptr, indices = s.jacobian_structure()
        vals = s.evaluate_jacobian(apply_loss_function=apply_loss)
        assert shape == jref.shape and np.array_equal(indptr, jref.indptr) and np.array_equal(indices, jref.indices)   # the structure keeps the six columns
        q_j = (np.abs(vals - jref.values) / jref.scale).max() / jbar
        jtr = jr.transpose_times(shape, indptr, indices, vals, r)
        q_t = (np.abs(jtr - g)[live] / gbar[live]).max()
        print("%s apply_loss=%d: error / bar  residual %.3f  gradient %.3f  cost %.3f  jacobian %.3f  J'r %.3f" % (label, apply_loss, q_r, q_g, q_c, q_j, q_t))
        assert q_r <= 1.0 and q_g <= 1.0 and q_c <= 1.0 and q_j <= 1.0 and q_t <= 1.0, (q_r, q_g, q_c, q_j, q_t)
        in_masked = np.isin(indices, slots)
        assert in_masked.any() and np.all(vals[in_masked] == 0.0) and np.all(jref.values[in_masked] == 0.0)
        assert np.all(g[slots] == 0.0) and np.all(jtr[slots] == 0.0)
        assert np.all(g[~want.live] == 0.0) and np.all(jtr[~want.live] == 0.0)
        out[apply_loss] = (cost, r, g, vals)
    return out


def _check_covariance(cs, s, x, label):
    """A masked camera, a masked marker (and the one with a single free component), a masked time, cross pairs and the time marginals
    against the lifted reference, to 1e-8 of the block's largest entry (test_gpu_marker_weights.py::test_covariance's bar); zeros exact."""
    prob = cs["prob"]
    C, T = prob["C"], prob["T"]
    mc = sref.chain_of(cs, prob=dict(prob, params=x))
    cov, fb = sref.covariance(mc, mc.x0())
    pos = {int(b): 6 * k for k, b in enumerate(fb)}
    s.covariance_compute()   # (RSBA_ERR_RANK_DEFICIENT would raise)
    cam, tim, mk2, mk1 = 1, C + 3, C + T + 2, C + T + 1
    other_t = [int(b) for b in fb if C <= b < C + T and b != tim][0]
    pairs = [(cam, cam), (mk2, mk2), (mk1, mk1), (tim, tim), (cam, tim), (tim, mk2), (mk1, cam), (tim, other_t), (other_t, tim), (mk2, other_t), (cam, mk1)]
    got = s.covariance_blocks([(6 * a, 6 * b) for a, b in pairs])
    worst = 0.0
    for (a, b), blk in zip(pairs, got):
        want = cov[pos[a]:pos[a] + 6, pos[b]:pos[b] + 6]
        worst = max(worst, float(np.abs(blk - want).max() / np.abs(want).max()))
        assert np.array_equal(blk == 0.0, want == 0.0) and (want == 0.0).any(), (a, b)   # zeros where the lift has them, exactly, and nowhere else
    for a, b in ((cam, cam), (mk2, cam), (cam, mk1)):   # the single-block query
        want = cov[pos[a]:pos[a] + 6, pos[b]:pos[b] + 6]
        blk = s.covariance_block(6 * a, 6 * b)
        worst = max(worst, float(np.abs(blk - want).max() / np.abs(want).max()))
        assert np.array_equal(blk == 0.0, want == 0.0)
    tc = s.time_covariances()
    for t in (tim, other_t):
        want = cov[pos[t]:pos[t] + 6, pos[t]:pos[t] + 6]
        worst = max(worst, float(np.abs(tc[t - C] - want).max() / np.abs(want).max()))
        assert np.array_equal(tc[t - C] == 0.0, want == 0.0)
    print("%s: covariance, worst block error %.2e (bar 1e-8)" % (label, worst))
    assert worst <= 1e-8


@pytest.mark.parametrize("sid", ["S1", "S3"])
def test_evaluate_jacobian_and_covariance(sid):
    cs, mc, _, _, _ = sref.reference_run(sid)
    at_start = {}
    for impl in (0, 2):
        pr = _problem(cs)
        s = capi.Solver(pr, _options(cs, impl))
        try:
            assert s.eliminates_times() == (1 if impl == 2 else 0)
            x0 = np.asarray(cs["prob"]["params"], float)
            at_start[impl] = _check_queries(cs, mc, s, x0, "%s schur_impl %d, before any run" % (sid, impl))
            _check_covariance(cs, s, x0, "%s schur_impl %d, before any run" % (sid, impl))
            s.run()
            s.download()
            x = pr.params.copy()
            _check_queries(cs, mc, s, x, "%s schur_impl %d, after a run" % (sid, impl))
            _check_covariance(cs, s, x, "%s schur_impl %d, after a run" % (sid, impl))
        finally:
            s.close()
            pr.close()
    # the two paths share the query kernels: identical bits before any run
    for apply_loss, (cost, r, g, vals) in at_start[0].items():
        cost2, r2, g2, vals2 = at_start[2][apply_loss]
        assert cost == cost2
        for a, b in ((r, r2), (g, g2), (vals, vals2)):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals():
    lib = capi.load()
    pr = capi.Problem.points(syn.make_problem(2, 40, 2, seed=3))
    try:
        assert lib.rsba_problem_set_parameter_subset_constant(pr.h, 6, 0b000111) == capi.ERR_UNSUPPORTED
        s = capi.Solver(pr, capi.default_options())   # and the point model solves as before
        try:
            assert s.run().termination_type == capi.CONVERGENCE
        finally:
            s.close()
    finally:
        pr.close()
    pr = capi.Problem.marker_chain(ref.hongo())
    try:
        assert lib.rsba_problem_set_parameter_subset_constant(pr.h, 6, 63) == capi.ERR_ARG
        assert lib.rsba_problem_set_parameter_subset_constant(pr.h, 6, 64) == capi.ERR_ARG
        assert pr.parameter_subset_constant(6) == 0
    finally:
        pr.close()
