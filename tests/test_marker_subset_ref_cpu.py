"""tests/marker_subset_ref.py (the numpy reference with constant components of a pose block, ceres::SubsetParameterization) pinned by
properties that need no product code, and the decision margins of the cases tests/test_gpu_marker_subset.py compares accept / reject
sequences on.  No GPU.
"""
import numpy as np
import pytest

import marker_loss_ref as ref
import marker_step_accuracy as msa
import marker_subset_ref as sref
import solve_accuracy as sa

SIDS = ["S1", "S2", "S3"]


def test_the_table():
    """The issue's table: unknowns before and after the masks, rows, termination."""
    want = {"S1": (288, 275, 11), "S2": (114, 101, 17), "S3": (210, 197, 29)}
    for sid in SIDS:
        cs, mc, summary, rows, final = sref.reference_run(sid)
        assert (mc.ambient_n, mc.n, len(rows)) == want[sid]
        assert (summary["termination"], summary["reason"]) == ("CONVERGENCE", "function")
        assert [rw["successful"] for rw in rows[1:-1]] == [1] * (len(rows) - 2) and rows[-1]["successful"] == 0


@pytest.mark.parametrize("min_lm", [1e-6, 0.0])
@pytest.mark.parametrize("radius", [1e4, 1e-2])
@pytest.mark.parametrize("sid", SIDS)
def test_removed_columns_equal_zero_columns_with_a_unit_diagonal(sid, radius, min_lm):
    """(i) The step of the program without the masked columns equals, on the free components, the step of the ambient system whose
    masked columns are zero with a unit diagonal and a zero gradient, and that system's step is exactly 0 on the masked components —
    the equivalence a device may use, for any damping options (min_lm_diagonal = 0 included: the unit diagonal is the pivot).

    Both are fp64 Cholesky solves of one SPD system (the masked components are decoupled), so each is held to that system — the
    damped normal equations over the free components, summed in np.longdouble — under marker_step_accuracy's bar without its
    recovery term: forming (the fp64 sums that built H and g here) + solve (Higham Thm 10.3 / 10.4, plain substitutions: no explicit
    inverse, kappa = 0) + 4 u.  Their difference is then bounded by twice that in the same metric."""
    cs, mc, _, _, _ = sref.reference_run(sid)
    x = mc.x0()
    _, _, _, H, g, _ = mc.linearise(x)
    d_removed = sref.lm_step(H, g, radius, min_lm)
    Ha, ga = sref.zero_column_system(mc, H, g)
    d_zero = sref.lm_step(Ha, ga, radius, min_lm)
    assert np.all(d_zero[~mc.keep] == 0.0) and (~mc.keep).sum() == mc.ambient_n - mc.n == 13
    sysm = sref.SubsetSystem(mc, x, radius, dense=True, min_lm=min_lm)
    bar = sysm.forming + sa.gamma(3 * mc.n + 1) / (1.0 - sa.gamma(mc.n + 1)) + 4 * msa.U
    eta_removed = sa.backward_errors(sysm.A, sysm.b, d_removed).max()
    eta_zero = sa.backward_errors(sysm.A, sysm.b, d_zero[mc.keep]).max()
    # the two steps against each other, in the metric of the system's diagonal (the denominator of eta, row-independent part)
    d = np.sqrt(np.diagonal(sysm.A).astype(float))
    diff = np.abs(d * (d_removed - d_zero[mc.keep])).max() / np.sum(d * np.abs(d_removed))
    print("%s radius %g min_lm %g: eta %.2e (removed) %.2e (zero columns), bar %.2e; scaled difference %.2e" % (sid, radius, min_lm, eta_removed, eta_zero, bar, diff))
    assert eta_removed <= bar and eta_zero <= bar
    assert np.abs(d_removed).max() > 0.0


def test_the_masks_bind():
    """(ii) The masked run differs from the unmasked one: a higher final cost, and the masked components bitwise at their start."""
    for sid in SIDS:
        cs, mc, summary, rows, final = sref.reference_run(sid)
        mc0 = ref.MarkerChain(cs["prob"], cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])
        x0, summary0, _ = ref.minimise(mc0)
        assert summary["final_cost"] > summary0["final_cost"] * (1.0 + 1e-6), sid
        start = np.asarray(cs["prob"]["params"], float)
        assert mc.masked_slots.size == 13
        np.testing.assert_array_equal(final.ravel()[mc.masked_slots], start[mc.masked_slots])
        moved = np.abs(mc0.full(x0).ravel()[mc.masked_slots] - start[mc.masked_slots])
        assert moved.min() > 0.0 and moved.max() > 1e-5, sid   # (left free, the noise does move them)
        # every free component of a masked block moved
        free_slots = np.setdiff1d((6 * mc.free_blocks[:, None] + np.arange(6)).ravel(), mc.masked_slots)
        assert np.all(final.ravel()[free_slots] != start[free_slots])


@pytest.mark.parametrize("sid", SIDS + ["X12", "S1w", "D1"])
def test_decision_margins(sid):
    """(iii) No decision of the reference's run within 10 % of its threshold: the relative decrease against min_relative_decrease =
    1e-3, |cost change| against function_tolerance x cost, the step norm against parameter_tolerance (|x| + parameter_tolerance)
    with the ambient |x|, max |g| against gradient_tolerance.  Comparing accept / reject sequences with the device then never rests
    on a coin flip."""
    cs, mc, summary, rows, final = sref.reference_run(sid)
    m_rel = m_fun = m_par = m_grad = np.inf
    for j, rw in enumerate(rows[1:], 1):
        m_grad = min(m_grad, abs(rw["gradient_max_norm"] / 1e-10 - 1.0))
        if not rw["valid"]:
            continue
        last = j == len(rows) - 1
        m_par = min(m_par, abs(rw["step_norm"] / (1e-8 * (rw["x_norm"] + 1e-8)) - 1.0))
        before = rw["cost"] + rw["cost_change"] if rw["successful"] else rw["cost"]
        m_fun = min(m_fun, abs(abs(rw["cost_change"]) / (1e-6 * before) - 1.0))
        if last and summary["reason"] == "function":
            continue   # (ended before the relative decrease was formed)
        m_rel = min(m_rel, abs(rw["relative_decrease"] / 1e-3 - 1.0))
    print("%s: %d rows, margins %.3g (relative decrease) %.3g (function) %.3g (parameter) %.3g (gradient)" % (sid, len(rows), m_rel, m_fun, m_par, m_grad))
    assert min(m_rel, m_fun, m_par, m_grad) > 0.1
    assert summary["termination"] == "CONVERGENCE" and len(rows) > 3
    if sid not in SIDS:
        return   # (the device test's further cases: X12 nine masked blocks of 72, S1w weights and Huber, D1 lens distortion)
    # the issue's figures: the deciding |cost change| / cost and the one before it
    want = {"S1": (5.3e-7, 3.2e-6), "S2": (8.1e-7, 1.8e-6), "S3": (5.7e-7, 1.2e-6)}[sid]
    got = (abs(rows[-1]["cost_change"]) / rows[-1]["cost"], abs(rows[-2]["cost_change"]) / (rows[-2]["cost"] + rows[-2]["cost_change"]))
    assert abs(got[0] / want[0] - 1.0) < 0.05 and abs(got[1] / want[1] - 1.0) < 0.05, got
    assert min(rw["relative_decrease"] for rw in rows[1:-1]) > 0.01


def test_the_loop_uses_the_ambient_norm():
    """(iv) A hand-sized case (2 cameras, 3 times, 2 markers) whose held components carry most of |x|: with parameter_tolerance placed
    between step / |x|_local and step / |x|_ambient of one iteration, the ambient rule stops there on the parameter tolerance and
    the local rule goes on."""
    prob = msa.problem(("syn", 2, 3, 2, 1.0))
    C, T = prob["C"], prob["T"]
    masks = {1: 0b111000, C + 1: 0b111000, C + T + 1: 0b111000}   # the translations of a camera, a time and a marker
    mc = sref.SubsetMarkerChain(prob, masks)
    _, _, rows = sref.minimise(mc, function_tolerance=-1.0, max_num_iterations=6, ambient=False)
    _, _, rows_a = sref.minimise(mc, function_tolerance=-1.0, max_num_iterations=6, ambient=True)
    j = 3
    local, ambient, step = rows[j]["x_norm"], rows_a[j]["x_norm"], rows[j]["step_norm"]
    assert rows[j]["valid"] and ambient > 1.05 * local and step == rows_a[j]["step_norm"]
    tol = step / np.sqrt(local * ambient)
    assert all(rw["step_norm"] > tol * (rw["x_norm"] + tol) for rw in rows_a[1:j])
    _, s_amb, r_amb = sref.minimise(mc, function_tolerance=-1.0, parameter_tolerance=tol, max_num_iterations=6, ambient=True)
    _, s_loc, r_loc = sref.minimise(mc, function_tolerance=-1.0, parameter_tolerance=tol, max_num_iterations=6, ambient=False)
    assert (s_amb["reason"], len(r_amb)) == ("parameter", j + 1)
    assert len(r_loc) > j + 1
    # and the ambient norm is that of all six components of the blocks in the program, no more: a wholly constant block stays out
    mcc = sref.SubsetMarkerChain(prob, masks, constant_blocks=(C + 2,))
    full = mcc.full(mcc.x0())
    assert mcc.ambient_norm(mcc.x0()) == float(np.linalg.norm(full[mcc.free_blocks])) and C + 2 not in mcc.free_blocks


def test_masks_on_blocks_outside_the_program_are_ignored():
    cs = sref.case("S3")
    C, T = cs["prob"]["C"], cs["prob"]["T"]
    base = sref.chain_of(cs)
    more = dict(cs["masks"])
    more.update({0: 0b000001, C + T: 0b010101, cs["constant_blocks"][0]: 0b001100})   # the base blocks and a constant block
    mc = sref.chain_of(cs, masks=more)
    assert mc.n == base.n and np.array_equal(mc.cols, base.cols) and np.array_equal(mc.masked_slots, base.masked_slots)


@pytest.mark.parametrize("sid", ["S1", "S3"])
def test_covariance_lift(sid):
    """(v) Zeros in the masked rows and columns, and the free part is the inverse of the compacted J'J."""
    cs, mc, summary, rows, final = sref.reference_run(sid)
    x = mc.compact(final)
    cov, free = sref.covariance(mc, x)
    assert cov.shape == (mc.ambient_n, mc.ambient_n) and np.array_equal(free, mc.free_blocks)
    assert np.all(cov[~mc.keep] == 0.0) and np.all(cov[:, ~mc.keep] == 0.0)
    H = mc.linearise(x)[3]
    part = cov[np.ix_(mc.keep, mc.keep)]
    assert np.abs(part @ H - np.eye(mc.n)).max() < 1e-8
    # it is not the free part of the unmasked inverse: holding components changes the others' covariance
    mc0 = ref.MarkerChain(dict(cs["prob"], params=final.ravel()), cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])
    cov0, _ = ref.covariance(mc0, mc0.x0())
    assert np.abs(cov0[np.ix_(mc.keep, mc.keep)] - part).max() > 1e-3 * np.abs(part).max()
