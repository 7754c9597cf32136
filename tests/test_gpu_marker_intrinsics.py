"""Free intrinsics (rsba_problem_set_intrinsics_free: the solve refines a camera's fx fy cx cy k1 k2) on the marker-chain models, through
the C ABI, against tests/marker_intrinsics_ref.py — a numpy reference that shares no code with the product; its cases are pinned
without a device by tests/test_marker_intrinsics_ref_cpu.py.

Bars (BASELINE's): the same valid / successful sequence, iteration count, termination and reason; every iterate's cost and the final
cost to 1e-9 relative; every pose block and every intrinsics block to 1e-6, both as the largest absolute difference and relative to
the block's largest entry; the final RMS to 1e-4 px.  Every block that is not in the program, every held component and every camera
without a block keeps the bits of its start value.  schur_impl 0 and 2 return the same bits: such a solver is on the dense path.

One LM step: the componentwise backward-error bar of tests/marker_step_accuracy.py applies to a dense system with extra columns —
nothing in it knows what a column means.  It is taken through marker_subset_ref.SubsetSystem (System for a chain whose held
components are removed, which is how the reference's compact view states this program) on the damped normal equations over all free
components, intrinsics included, with dense = True.  The six intrinsics columns are shorter products than the pose columns'
(at most 4 roundings against the 37 the bar counts per entry), so the bar's forming term covers them.  Nothing in the bar is fitted.
"""
import re

import numpy as np
import pytest

import marker_intrinsics_ref as iref
import marker_loss_ref as ref
import marker_subset_ref as sref
from realsensecalibration_amd import capi, synthetic

pytestmark = pytest.mark.gpu

REASON = {"gradient": 1, "parameter": 2, "function": 3, "max_iterations": 4, "min_radius": 5, "invalid_steps": 6}
TERM = {"CONVERGENCE": 0, "NO_CONVERGENCE": 1, "FAILURE": 2}
INTR_KERNELS = {"k_marker_intr_eval", "k_marker_intr_subset_rows", "k_marker_intr_system", "k_marker_intr_candidate"}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


def _options(cs, schur_impl, **kw):
    return capi.default_options(schur_impl=schur_impl, huber_delta=cs["a"] if cs["loss"] != "none" else 0.0, loss_type=1 if cs["loss"] == "cauchy" else 0, **kw)


def _problem(cs, masks="case"):
    pr = capi.Problem.marker_chain(cs["prob"], capi.MODEL_MARKER_CHAIN_TEST2 if cs["variant"] == 1 else capi.MODEL_MARKER_CHAIN)
    for b in cs["constant_blocks"]:
        pr.set_parameter_block_constant(6 * b)
    if cs["weights"] is not None:
        pr.set_observation_weights(cs["weights"])
    for b, m in cs["pose_masks"].items():
        pr.set_parameter_subset_constant(6 * b, m)
    for b, (A, v) in cs["priors"].items():
        pr.set_block_prior(6 * b, A, v)
    for k, m in enumerate(cs["masks"] if isinstance(masks, str) else masks):
        if m:
            pr.set_intrinsics_free(k, m)
    return pr


def _state(pr):
    d = pr.distortion
    return pr.params.copy(), pr.intrinsics, (np.zeros((pr.num_cameras, 5)) if d is None else d)


def _solve(cs, schur_impl, masks="case", profile=False, **kw):
    """-> dict(summary, log, params, intr, dist, rms, rms_solver, elim, stats, report) of a fresh problem and solver."""
    pr = _problem(cs, masks)
    try:
        s = capi.Solver(pr, _options(cs, schur_impl, **kw))
        try:
            if profile:
                s.configure_run(kw.get("max_num_iterations", 50), 1)
            summ = s.run()
            s.download()
            params, intr, dist = _state(pr)
            out = dict(summary=summ, log=s.iterations(), params=params, intr=intr, dist=dist, elim=s.eliminates_times(),
                       stats=s.kernel_stats(64) if profile else {}, report=s.full_report(),
                       rms_solver=float(np.sqrt(s.final_costs()[1] / (8.0 * cs["prob"]["N"]))))
        finally:
            s.close()
        out["rms"] = pr.reprojection_error()[1]
    finally:
        pr.close()
    return out


def _bits(out):
    s = out["summary"]
    return (out["params"].tobytes(), out["intr"].tobytes(), out["dist"].tobytes(), out["log"].tobytes(),
            (s.termination_type, s.stop_reason, s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps, s.initial_cost, s.final_cost))


def _compare(name, out, run):
    cs, mc, x, summary, rows = run
    s, log = out["summary"], out["log"]
    assert (s.termination_type, s.stop_reason, s.num_iterations) == (TERM[summary["termination"]], REASON[summary["reason"]], len(rows) - 1), summary
    assert [int(v) for v in log[:, 7]] == [rw["valid"] + 2 * rw["successful"] for rw in rows]
    worst = max(abs(log[j, 1] - rw["cost"]) / rw["cost"] for j, rw in enumerate(rows))
    final = mc.full(x)
    got = out["params"].reshape(-1, 6)
    free = mc.free_blocks
    perr = np.abs(got[free] - final[free]).max(axis=1)
    prel = perr / np.maximum(np.abs(final[free]).max(axis=1), 1e-12)
    six_ref = mc.six(x)
    six = np.concatenate([out["intr"], out["dist"][:, :2]], axis=1)
    ierr = np.abs(six - six_ref).max(axis=1)
    irel = ierr / np.abs(six_ref).max(axis=1)
    rms_ref = np.sqrt(summary["final_sumsq"] / (8.0 * cs["prob"]["N"]))
    print("%s: %d iterations, n %d, cost error %.2e (bar 1e-9), pose blocks %.2e abs %.2e rel, intrinsics blocks %.2e abs %.2e rel (bar 1e-6), rms %.6f against %.6f"
          % (name, len(rows) - 1, mc.n, worst, perr.max(), prel.max(), ierr.max(), irel.max(), out["rms"], rms_ref))
    for j, rw in enumerate(rows):
        assert abs(log[j, 1] - rw["cost"]) <= 1e-9 * rw["cost"], "iterate %d: cost %.15e, reference %.15e" % (j, log[j, 1], rw["cost"])
    assert abs(s.final_cost - summary["final_cost"]) <= 1e-9 * summary["final_cost"]
    assert perr.max() < 1e-6 and prel.max() < 1e-6, (perr.max(), prel.max())
    assert ierr.max() < 1e-6 and irel.max() < 1e-6, (ierr.max(), irel.max())
    assert abs(out["rms"] - rms_ref) <= 1e-4, (out["rms"], rms_ref)
    assert abs(out["rms"] - out["rms_solver"]) <= 1e-9, (out["rms"], out["rms_solver"])   # the problem now holds what the solver ended at
    # what is not solved for keeps its bits
    start = np.asarray(cs["prob"]["params"], float).reshape(-1, 6)
    fixed = np.setdiff1d(np.arange(got.shape[0]), free)
    assert got[fixed].tobytes() == start[fixed].tobytes()
    for b, m in mc.pose_masks.items():
        q = [k for k in range(6) if (m >> k) & 1]
        assert got[b, q].tobytes() == start[b, q].tobytes(), b
    six0 = np.concatenate([np.asarray(cs["prob"]["intr"], float), np.asarray(cs["dist"], float)[:, :2]], axis=1)
    for k, m in enumerate(cs["masks"]):
        q = [c for c in range(6) if not (m >> c) & 1]
        assert six[k, q].tobytes() == six0[k, q].tobytes(), "camera %d: a held component moved" % k
        if m:
            assert (six[k, [c for c in range(6) if (m >> c) & 1]] != six0[k, [c for c in range(6) if (m >> c) & 1]]).all(), k
    assert out["dist"][:, 2:].tobytes() == np.asarray(cs["dist"], float)[:, 2:].tobytes()     # p1 p2 k3 are constants


# ------------------------------------------------------------------------------------------------ 1. whole solves
@pytest.mark.parametrize("name", iref.SOLVE_CASES)
def test_solve_matches_the_reference(name):
    """The issue's cases; schur_impl 0 and 2 both run the dense path and return the same bits."""
    run = iref.reference_run(name)
    cs = run[0]
    a = _solve(cs, 0, profile=True)
    b = _solve(cs, 2)
    assert a["elim"] == 0 and b["elim"] == 0
    assert INTR_KERNELS <= set(a["stats"]) and "k_marker_system" not in a["stats"] and "k_marker_eval" not in a["stats"], sorted(a["stats"])
    assert ("k_marker_intr_prior_rows" in a["stats"]) == bool(cs["priors"])
    _compare(name, a, run)
    assert _bits(a) == _bits(b)
    m = re.search(r"Parameters\s+(\d+)\s+(\d+)", a["report"])
    nconst = sum(1 for c in cs["constant_blocks"])
    assert m and int(m.group(2)) == run[1].n and int(m.group(1)) == run[1].n + 6 * nconst, a["report"]


def test_rsba_solve_writes_the_refined_values_back():
    """rsba_solve on a problem WITHOUT a distortion array, k1 k2 of one camera free: the array appears, zeros elsewhere."""
    base = synthetic.make_marker_chain(3, 12, 4, seed=iref.RIG_SEED)
    prob = dict(base, intr=iref.displaced_intrinsics(base["intr"]))
    cs = dict(prob=dict(prob, dist=np.zeros((3, 5))), dist=np.zeros((3, 5)), masks=[0, 0x3F, 0], variant=0, loss="none", a=0.0, weights=None,
              constant_blocks=(), pose_masks={}, priors={})
    mc = iref.chain_of(cs)
    x, summary, rows = ref.minimise(mc)
    pr = capi.Problem.marker_chain(prob)
    try:
        assert pr.distortion is None
        pr.set_intrinsics_free(1, ("fx", "fy", "cx", "cy", "k1", "k2"))
        summ = pr.solve(capi.default_options())
        assert summ.num_iterations == len(rows) - 1 and abs(summ.final_cost - summary["final_cost"]) <= 1e-9 * summary["final_cost"]
        d = pr.distortion
        assert d is not None and not d[[0, 2]].any() and not d[1, 2:].any() and d[1, :2].all()
        six = np.concatenate([pr.intrinsics, d[:, :2]], axis=1)
        assert np.abs(six - mc.six(x)).max() < 1e-6 and np.abs(pr.params.reshape(-1, 6) - mc.full(x)).max() < 1e-6
        assert six[[0, 2]].tobytes() == mc.six(mc.x0())[[0, 2]].tobytes()
        # a later solver starts from the refined values: its first cost is this one's last
        again = pr.solve(capi.default_options())
        assert abs(again.initial_cost - summ.final_cost) <= 1e-9 * summ.final_cost
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 2. one step as a linear solve
@pytest.mark.parametrize("name", ["3x12x4_3f", "3x70x5_mixed"])
def test_one_step_within_its_backward_error_bar(name):
    """x1 - x0 over every free component, intrinsics columns included, solves the reference's damped normal equations within
    marker_step_accuracy's componentwise backward-error bar (module docstring); n <= 384 and n > 384: both factorisations."""
    cs, mc, _, _, _ = iref.reference_run(name)
    cv = mc.compact_view()
    sysm = sref.SubsetSystem(cv, cv.x0(), 1e4, dense=True)
    out = _solve(cs, 0, profile=True, max_num_iterations=1, function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0)
    log = out["log"]
    assert log.shape[0] == 2 and int(log[1, 7]) == 3, "the step was not accepted: %s" % (log,)
    assert (mc.n <= 384) == (name == "3x12x4_3f")
    x1 = np.concatenate([out["params"].reshape(-1, 6)[mc.free_blocks].ravel(), np.concatenate([out["intr"], out["dist"][:, :2]], axis=1)[mc.cams].ravel()])
    assert x1[mc.held].tobytes() == mc.x0()[mc.held].tobytes()      # a held component's step is an exact zero
    r = sysm.check(x1[cv.keep])
    print("\nINTRSTEP %s: n %d (%d kept) m %d kappa %.2f eta %.2e bar %.2e (recovery %.1e) eta/bar %.2e" % (
        name, mc.n, cv.n, sysm.m, sysm.kappa, r["eta"], r["bar"], r["recovery"], r["ratio"]))
    assert r["eta"] <= r["bar"], r
    # the log's scalars, at marker_step_accuracy's tolerances
    assert abs(log[0, 1] - sysm.cost) <= 1e-12 * sysm.cost and abs(log[0, 3] - sysm.gmax) <= 1e-11 * sysm.gmax
    nd, tol = sysm.step_norm_tolerance(x1[cv.keep])
    assert abs(log[1, 4] - nd) <= tol, (log[1, 4], nd, tol)
    mcc, mcc_tol = sysm.model_cost_change(x1[cv.keep])
    assert abs(log[1, 2] / log[1, 5] - mcc) <= mcc_tol + 2 * 2.0 ** -53 * abs(mcc), (log[1, 2] / log[1, 5], mcc, mcc_tol)


# ------------------------------------------------------------------------------------------------ 3. mask 0: today's bits
@pytest.mark.parametrize("which", ["4x40x6", "hongo"])
def test_mask_zero_everywhere_returns_the_bits_of_a_problem_never_touched(which):
    if which == "hongo":
        prob, C = ref.hongo(), 4
    else:
        prob, C = synthetic.make_marker_chain(4, 40, 6, seed=iref.RIG_SEED), 4
    cs = dict(prob=prob, dist=None, masks=[0] * C, variant=0, loss="none", a=0.0, weights=None, constant_blocks=(), pose_masks={}, priors={})
    for impl in (0, 2):
        outs = []
        for touch in (False, True):
            pr = capi.Problem.marker_chain(prob)
            try:
                if touch:
                    for k in range(C):
                        pr.set_intrinsics_free(k, 0x3F)
                    for k in range(C):
                        pr.set_intrinsics_free(k, 0)
                s = capi.Solver(pr, _options(cs, impl))
                try:
                    s.configure_run(50, 1)
                    summ = s.run()
                    s.download()
                    assert s.eliminates_times() == (1 if impl == 2 else 0)
                    assert not any(k.startswith("k_marker_intr") for k in s.kernel_stats(64))
                    outs.append(_bits(dict(summary=summ, log=s.iterations(), params=pr.params.copy(), intr=pr.intrinsics, dist=np.zeros(1))))
                    assert pr.distortion is None and pr.intrinsics.tobytes() == np.ascontiguousarray(prob["intr"], np.float64).tobytes()
                finally:
                    s.close()
            finally:
                pr.close()
        assert outs[0] == outs[1], impl


# ------------------------------------------------------------------------------------------------ 4. zero noise: the truth
def test_zero_noise_reaches_the_truth_and_fixed_intrinsics_cannot():
    cs = iref.case("3x12x4_3f", noise=0.0)
    out = _solve(cs, 1)
    err = np.abs(np.concatenate([out["intr"], out["dist"][:, :2]], axis=1) - cs["truth_six"])
    fixed = _solve(cs, 0, masks=[0, 0, 0])
    print("zero noise: cost %.2e, intrinsics %.2e px off the truth, k1 k2 %.2e; intrinsics fixed: cost %.3f" % (
        out["summary"].final_cost, err[:, :4].max(), err[:, 4:].max(), fixed["summary"].final_cost))
    assert err[:, :4].max() < 1e-4 and err[:, 4:].max() < 1e-6
    assert fixed["summary"].final_cost > 1.0
    assert fixed["intr"].tobytes() == np.asarray(cs["prob"]["intr"], float).tobytes()


# ------------------------------------------------------------------------------------------------ 5. reproducible, resident
def test_two_runs_and_two_solvers_return_identical_bits():
    """run() restarts from the uploaded state, intrinsics included; the setters of weights and priors keep working on such a solver."""
    cs = iref.case("3x70x5_mixed_all")
    first = _solve(cs, 1)
    pr = _problem(cs)
    try:
        s = capi.Solver(pr, _options(cs, 1))
        try:
            got = []
            for turn in range(2):
                summ = s.run()
                s.download()
                params, intr, dist = _state(pr)
                got.append(_bits(dict(summary=summ, log=s.iterations(), params=params, intr=intr, dist=dist)))
                if turn == 0:   # the same values through the solver-level setters: nothing changes
                    s.set_observation_weights(cs["weights"])
                    for b, (A, v) in cs["priors"].items():
                        s.set_block_prior(6 * b, A, v)
            assert got[0] == got[1] == _bits(first)
            # other weights: another solve
            s.set_observation_weights(np.ones(cs["prob"]["N"]))
            other = s.run()
            assert other.final_cost != first["summary"].final_cost
        finally:
            s.close()
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_a_mask_on_a_camera_no_observation_names_is_refused():
    cs = iref.case("3x12x4_3f")
    prob = cs["prob"]
    keep = np.asarray(prob["c"]) != 2
    prob = dict(prob, N=int(keep.sum()), t=prob["t"][keep], c=prob["c"][keep], m=prob["m"][keep], obs=np.asarray(prob["obs"])[keep])
    pr = capi.Problem.marker_chain(prob)
    try:
        pr.set_intrinsics_free(0, 0x0F)
        pr.set_intrinsics_free(2, 0x01)
        before = _state(pr)
        for impl in (0, 1, 2):
            with pytest.raises(capi.RsbaError) as e:
                capi.Solver(pr, capi.default_options(schur_impl=impl))
            assert e.value.code == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.RsbaError) as e:
            pr.solve()
        assert e.value.code == capi.ERR_UNSUPPORTED
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, _state(pr)))
        pr.set_intrinsics_free(2, 0)      # without it the problem solves
        assert pr.solve().termination_type == 0
    finally:
        pr.close()


def test_more_than_8192_columns_is_refused_before_anything_is_allocated():
    """2 x 1400 x 2: about 1400 time blocks in the program, some 8400 columns with the intrinsics block, more than 8192: refused by the host's plan (the dense matrix
    would be 0.5 GB), at once."""
    prob = synthetic.make_marker_chain(2, 1400, 2, seed=3)
    pr = capi.Problem.marker_chain(prob)
    try:
        pr.set_intrinsics_free(1, 0x03)
        for impl in (0, 1, 2):
            with pytest.raises(capi.RsbaError) as e:
                capi.Solver(pr, capi.default_options(schur_impl=impl))
            assert e.value.code == capi.ERR_UNSUPPORTED
    finally:
        pr.close()


def test_queries_without_a_place_for_the_block_are_refused():
    cs = iref.case("3x12x4_0f")
    pr = _problem(cs)
    try:
        s = capi.Solver(pr, _options(cs, 1))
        try:
            s.run()
            for call in (lambda: s.evaluate(), lambda: s.evaluate(residuals=False, gradient=False), lambda: s.evaluate_jacobian(),
                         lambda: s.jacobian_structure(), lambda: s.covariance_compute(), lambda: s.set_parameters(pr.params.copy())):
                with pytest.raises(capi.RsbaError) as e:
                    call()
                assert e.value.code == capi.ERR_UNSUPPORTED
            s.download()     # and the solver is as it was
            assert s.eliminates_times() == 0 and len(s.iterations()) > 2
        finally:
            s.close()
    finally:
        pr.close()
