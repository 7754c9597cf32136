"""Per-observation weights (ceres::ScaledLoss) on the marker-chain models, through the C ABI, against tests/marker_weight_ref.py.

Block i contributes 1/2 a_i rho(s_i); its rows are scaled by sqrt(a_i rho'(s_i)); the raw sum of squares is not weighted.  Bars
(BASELINE's, as tests/test_gpu_marker_loss.py holds them): the same accept / reject sequence and termination, every iterate's cost to
1e-9 relative, every free block to 1e-6 relative, blocks that are not free keep their bits, the final RMS to 1e-4 px.  The cases and
their decision margins are pinned without a device by tests/test_marker_weight_ref_cpu.py.
"""
import numpy as np
import pytest

import evaluate_ref as er
import marker_loss_ref as ref
import marker_weight_ref as wref
import oracle_lib
from realsensecalibration_amd import capi
from realsensecalibration_amd import synthetic as syn

pytestmark = pytest.mark.gpu

REASON = {"gradient": 1, "parameter": 2, "function": 3, "max_iterations": 4, "min_radius": 5, "invalid_steps": 6}
TERM = {"CONVERGENCE": 0, "NO_CONVERGENCE": 1, "FAILURE": 2}
EPS = np.finfo(float).eps


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


def _options(schur_impl, loss, a, **kw):
    return capi.default_options(schur_impl=schur_impl, huber_delta=a if loss != "none" else 0.0, loss_type=1 if loss == "cauchy" else 0, **kw)


def _model(cs):
    return capi.MODEL_MARKER_CHAIN_TEST2 if cs["variant"] == 1 else capi.MODEL_MARKER_CHAIN


def _problem(cs, weights="case", params=None):
    prob = cs["prob"] if params is None else dict(cs["prob"], params=params)
    pr = capi.Problem.marker_chain(prob, _model(cs))
    for b in cs["constant_blocks"]:
        pr.set_parameter_block_constant(6 * b)
    if isinstance(weights, str):
        weights = cs["weights"]
    if weights is not None:
        pr.set_observation_weights(weights)
    return pr


def _run(s, pr):
    summ = s.run()
    s.download()
    return summ, s.iterations(), pr.params.copy()


def _solve(cs, schur_impl, weights="case", expect_elim=None):
    """-> (summary, log, parameters, rms, eliminates_times) of a fresh problem and solver."""
    pr = _problem(cs, weights)
    try:
        s = capi.Solver(pr, _options(schur_impl, cs["loss"], cs["a"]))
        try:
            elim = s.eliminates_times()
            if expect_elim is not None:
                assert elim == expect_elim
            summ, log, params = _run(s, pr)
        finally:
            s.close()
        _, rms = pr.reprojection_error()
    finally:
        pr.close()
    return summ, log, params, rms, elim


def _check(name, schur_impl, expect_elim=None):
    cs, mc, summary, rows, final = wref.reference_run(name)
    summ, log, params, rms, _ = _solve(cs, schur_impl, expect_elim=expect_elim)
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
    return cs, got, start


# ------------------------------------------------------------------------------------------------ 1. solve parity
@pytest.mark.parametrize("schur_impl", [0, 2])
@pytest.mark.parametrize("name", wref.TABLE)
def test_solve_matches_the_weighted_reference(name, schur_impl):
    """The issue's table on the dense path and with the time blocks eliminated (test2_*: RSBA_MODEL_MARKER_CHAIN_TEST2)."""
    cs, got, start = _check(name, schur_impl)
    if name == "4x40x6_time7_huber":
        # a free block all of whose observations have weight 0: in the program, a zero step, its bits unchanged
        b = cs["prob"]["C"] + 7
        np.testing.assert_array_equal(got[b], start[b])


def test_default_path_eliminates_at_432_unknowns():
    """(12, 40, 20): the smallest shape where schur_impl 1 picks the elimination; weights alone (no loss) keep that choice."""
    _check("12x40x20_mask_none", 1, expect_elim=1)


def test_many_workgroups():
    """(8, 400, 16), Huber 2 and the mask: several workgroups in the weight, product and candidate passes."""
    _check("8x400x16_mask_huber", 2, expect_elim=1)


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_constant_blocks(schur_impl):
    """A constant camera, time and marker block plus the mask: the kConst instances."""
    _check("const_mask_huber", schur_impl)


# ------------------------------------------------------------------------------------------------ 2. switches
SWITCHES = [{"RSBA_MT_ACC_MFMA": "0"}, {"RSBA_MT_FORK": "0"}, {"RSBA_MT_SOLVE_LDS": "0"}, {"RSBA_MT_SPLIT_BACKSUB": "0"},
            {"RSBA_MT_SPLIT_BACKSUB": "0", "RSBA_MT_BACKSUB_WG": "0"}]


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_switches(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check("4x40x6_mask_huber", 2, expect_elim=1)


# ------------------------------------------------------------------------------------------------ 3. resident update
@pytest.mark.parametrize("schur_impl", [0, 2])
def test_resident_update_equals_a_solver_created_with_the_weights(schur_impl):
    """The intended loop: all ones and Huber 2, run, evaluate raw residuals, zero the offenders' weights, run again on the same solver."""
    cs = wref.case("4x40x6_mask_huber")
    N = cs["prob"]["N"]
    start = np.asarray(cs["prob"]["params"], float)
    pr = _problem(cs, np.ones(N))
    s = capi.Solver(pr, _options(schur_impl, "huber", 2.0))
    try:
        summ0, log0, x0 = _run(s, pr)
        _, r, _ = s.evaluate(gradient=False, apply_loss_function=False)
        worst = np.sort(np.sum(r.reshape(N, 8) ** 2, axis=1))[-int(cs["hit"].sum())]
        assert np.all(np.sum(r.reshape(N, 8) ** 2, axis=1)[cs["hit"]] >= worst)   # the raw residuals name the displaced rows
        s.covariance_compute()
        s.set_observation_weights(cs["weights"])
        with pytest.raises(capi.RsbaError):
            s.covariance_block(6, 6)   # the covariance was that of the old weights
        np.testing.assert_array_equal(s.iterations(), log0)   # log and parameters stay
        s.download()
        np.testing.assert_array_equal(pr.params, x0)
        s.set_parameters(start)
        summ1, log1, x1 = _run(s, pr)
        # validation on the solver: nothing changes
        bad = cs["weights"].copy()
        bad[3] = -1.0
        assert capi.load().rsba_solver_set_observation_weights(s.h, bad.ctypes.data_as(capi.C.c_void_p)) == capi.ERR_ARG
        bad[3] = np.nan
        assert capi.load().rsba_solver_set_observation_weights(s.h, bad.ctypes.data_as(capi.C.c_void_p)) == capi.ERR_ARG
        assert capi.load().rsba_solver_set_observation_weights(s.h, None) == capi.ERR_ARG
        summ2, log2, x2 = _run(s, pr)
    finally:
        s.close()
        pr.close()
    _, log, x, _, _ = _solve(cs, schur_impl)
    assert log.shape[0] > 2 and not np.array_equal(log0, log)
    np.testing.assert_array_equal(log1, log)
    np.testing.assert_array_equal(x1, x)
    np.testing.assert_array_equal(log2, log)
    np.testing.assert_array_equal(x2, x)


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_a_solver_without_weights_and_loss_refuses(schur_impl):
    cs = wref.case("4x40x6_mask_none")
    pr = _problem(cs, None)
    s = capi.Solver(pr, _options(schur_impl, "none", 0.0))
    try:
        _, log0, x0 = _run(s, pr)
        with pytest.raises(capi.RsbaError) as e:
            s.set_observation_weights(cs["weights"])
        assert e.value.code == capi.ERR_UNSUPPORTED
        s.set_parameters(np.asarray(cs["prob"]["params"], float))
        _, log1, x1 = _run(s, pr)
        np.testing.assert_array_equal(log0, log1)
        np.testing.assert_array_equal(x0, x1)
    finally:
        s.close()
        pr.close()


def test_point_model_solver_refuses():
    pr = capi.Problem.points(syn.make_problem(2, 40, 2, seed=3))
    s = capi.Solver(pr, capi.default_options(huber_delta=1.0))
    try:
        with pytest.raises(capi.RsbaError) as e:
            s.set_observation_weights(np.ones(pr.num_observations))
        assert e.value.code == capi.ERR_UNSUPPORTED
    finally:
        s.close()
        pr.close()


def test_rsba_solve_honours_the_problems_weights():
    cs, mc, summary, rows, final = wref.reference_run("4x40x6_mask_none")
    pr = _problem(cs)
    try:
        summ = pr.solve(_options(2, "none", 0.0))
        assert summ.num_iterations == len(rows) - 1 and abs(summ.final_cost - summary["final_cost"]) <= 1e-9 * summary["final_cost"]
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 4. bit identities
@pytest.mark.parametrize("schur_impl", [0, 2])
def test_all_ones_with_huber_equals_unweighted_huber(schur_impl):
    cs = wref.case("4x40x6_mask_huber")
    _, log0, x0, rms0, _ = _solve(cs, schur_impl, weights=None)
    _, log1, x1, rms1, _ = _solve(cs, schur_impl, weights=np.ones(cs["prob"]["N"]))
    assert log0.shape[0] > 2
    np.testing.assert_array_equal(log0, log1)
    np.testing.assert_array_equal(x0, x1)
    assert rms0 == rms1


@pytest.mark.parametrize("schur_impl,shape", [(0, (6, 40, 9)), (2, (12, 40, 20))], ids=["dense", "eliminated"])
def test_all_ones_without_a_loss_equals_the_loss_free_run(schur_impl, shape):
    """The weights-only solver runs the loss instances with rho(s) = s: 1 * s and sqrt(1) * 1 change no bit."""
    cs = dict(prob=syn.make_marker_chain(*shape, seed=34), variant=0, loss="none", a=0.0, constant_blocks=())
    _, log0, x0, rms0, e0 = _solve(cs, schur_impl, weights=None)
    _, log1, x1, rms1, e1 = _solve(cs, schur_impl, weights=np.ones(cs["prob"]["N"]))
    assert log0.shape[0] > 2 and e0 == e1 == (1 if schur_impl else 0)
    np.testing.assert_array_equal(log0, log1)
    np.testing.assert_array_equal(x0, x1)
    assert rms0 == rms1


def _kernel_names(cs, schur_impl, weights):
    pr = _problem(cs, weights)
    s = capi.Solver(pr, _options(schur_impl, "none", 0.0, profile_kernels=1))
    try:
        s.run()
        return set(s.kernel_stats())
    finally:
        s.close()
        pr.close()


def test_an_unweighted_loss_free_solver_launches_what_it_launched():
    cs = dict(prob=syn.make_marker_chain(12, 40, 20, seed=34), variant=0, loss="none", a=0.0, constant_blocks=())
    plain = _kernel_names(cs, 2, None)
    assert plain == {"k_pose_constants", "k_mc_slot_products", "k_mc_time_products", "k_mc_cross", "k_mc_accumulate", "k_marker_reduce",
                     "k_marker_reduced_solve", "k_time_backsub_terms", "k_marker_schur_finish"}
    assert _kernel_names(cs, 2, np.ones(cs["prob"]["N"])) == plain | {"k_mc_block_weight"}


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_repeated_weighted_runs_are_bit_identical(schur_impl):
    cs = wref.case("4x40x6_fracmask_cauchy")
    pr = _problem(cs)
    s = capi.Solver(pr, _options(schur_impl, cs["loss"], cs["a"]))
    try:
        runs = [_run(s, pr) for _ in range(2)]
        np.testing.assert_array_equal(runs[0][1], runs[1][1])
        np.testing.assert_array_equal(runs[0][2], runs[1][2])
    finally:
        s.close()
        pr.close()


# ------------------------------------------------------------------------------------------------ 5. evaluate and Jacobian
def _perturbed(cs, seed=77):
    x = np.asarray(cs["prob"]["params"], float).copy()
    return x + 1e-3 * np.random.default_rng(seed).standard_normal(x.shape)


@pytest.mark.parametrize("schur_impl", [0, 2])
@pytest.mark.parametrize("name", ["4x40x6_fracmask_cauchy", "hongo_mask_huber"])
def test_evaluate_and_jacobian(name, schur_impl):
    cs = wref.case(name)
    prob, w, N = cs["prob"], cs["weights"], cs["prob"]["N"]
    x = _perturbed(cs)
    prw, pru = _problem(cs), _problem(cs, None)
    sw, su = (capi.Solver(p, _options(schur_impl, cs["loss"], cs["a"])) for p in (prw, pru))
    try:
        sw.set_parameters(x)
        su.set_parameters(x)
        # the structure does not depend on weights
        shape_w, indptr, indices = sw.jacobian_structure()
        shape_u, indptr_u, indices_u = su.jacobian_structure()
        assert shape_w == shape_u
        np.testing.assert_array_equal(indptr, indptr_u)
        np.testing.assert_array_equal(indices, indices_u)
        # apply_loss_function = 0 ignores the weights with the loss: the unweighted solver's bits
        c0, r0, g0 = sw.evaluate(apply_loss_function=False)
        cu, ru, gu = su.evaluate(apply_loss_function=False)
        j0, ju = sw.evaluate_jacobian(apply_loss_function=False), su.evaluate_jacobian(apply_loss_function=False)
        assert c0 == cu
        np.testing.assert_array_equal(r0, ru)
        np.testing.assert_array_equal(g0, gu)
        np.testing.assert_array_equal(j0, ju)
        # apply_loss_function = 1: block i's raw output times sqrt(a_i rho'(s_i)), formed here.  16 eps relative per entry: s is a sum
        # of 8 squares (at most 8 eps), rho' and its root halve the relative error and add a rounding each, then one product
        c1, r1, g1 = sw.evaluate()
        j1 = sw.evaluate_jacobian()
        s = np.sum(r0.reshape(N, 8) ** 2, axis=1)
        rho, rho1 = ref.rho_and_rho1(s, cs["loss"], cs["a"])
        f = np.sqrt(w * rho1)
        want_r = r0.reshape(N, 8) * f[:, None]
        err_r = np.abs(r1.reshape(N, 8) - want_r)
        assert np.all(err_r <= 16 * EPS * np.abs(want_r)), (err_r / np.maximum(np.abs(want_r), 1e-300)).max() / EPS
        rows_of = np.repeat(np.arange(8 * N), np.diff(indptr))   # the CRS row of every value; block = row // 8
        want_j = j0 * f[rows_of // 8]
        err_j = np.abs(j1 - want_j)
        assert np.all(err_j <= 16 * EPS * np.abs(want_j)), (err_j / np.maximum(np.abs(want_j), 1e-300)).max() / EPS
        zero = w == 0.0
        assert zero.any() and np.all(r1.reshape(N, 8)[zero] == 0.0) and np.all(j1[zero[rows_of // 8]] == 0.0)
        assert np.all(r1.reshape(N, 8)[~zero] != 0.0)
        # cost = 1/2 sum a_i rho(s_i): all terms are non-negative
        want_c = 0.5 * float(np.sum(w * rho))
        print("%s schur_impl %d: residual %.1f eps, Jacobian %.1f eps, cost %.2e relative"
              % (name, schur_impl, (err_r / np.maximum(np.abs(want_r), 1e-300)).max() / EPS, (err_j / np.maximum(np.abs(want_j), 1e-300)).max() / EPS,
                 abs(c1 - want_c) / want_c))
        assert abs(c1 - want_c) <= (N + 16) * EPS * want_c
        # the gradient against the weighted reference's, with test_gpu_evaluate's rounding bound on the corrected rows: the residual bar
        # from the oracle's own spread (contracted against uncontracted arithmetic)
        mc = wref.WeightedMarkerChain(dict(prob, params=x), w, cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])
        _, rt, Jt, _, g_ref, _ = mc.linearise(mc.x0())
        raw = [np.array([r for r, _ in er.marker_rows(o, prob, x, cs["variant"])]) for o in (oracle_lib.load(), oracle_lib.load_nocontract())]
        rbar = 16.0 * max(np.abs(raw[0] - raw[1]).max(), 4.0 * np.spacing(np.abs(prob["obs"]).max()))
        n = mc.n
        cl = np.where(mc.cols >= 0, mc.cols, n)
        abs_J, abs_Jr, n_terms = np.zeros(n + 1), np.zeros(n + 1), np.zeros(n + 1)
        np.add.at(abs_J, cl, np.abs(Jt).sum(axis=1))
        np.add.at(abs_Jr, cl, np.einsum("krq,kr->kq", np.abs(Jt), np.abs(rt)))
        np.add.at(n_terms, cl, 8.0)
        gbar = abs_J[:n] * rbar + (64 + n_terms[:n]) * (EPS / 2) * abs_Jr[:n]
        got = g1.reshape(-1, 6)[mc.free_blocks].ravel()
        q = np.abs(got - g_ref) / gbar
        print("   gradient error / bar %.3f" % q.max())
        assert q.max() <= 1.0
        fixed = np.setdiff1d(np.arange(g1.size // 6), mc.free_blocks)
        assert np.all(g1.reshape(-1, 6)[fixed] == 0.0)
    finally:
        sw.close()
        su.close()
        prw.close()
        pru.close()


# ------------------------------------------------------------------------------------------------ 6. covariance
def _covariance_case(name):
    if name != "5x40x8_frac_cauchy":
        return wref.case(name)
    clean = syn.make_marker_chain(5, 40, 8, seed=35)
    prob = ref.displace_corners(clean, 0.05, 40.0, 35)
    return dict(prob=prob, variant=0, weights=np.random.default_rng(6).choice([0.25, 1.0, 4.0], prob["N"]), loss="cauchy", a=2.0, constant_blocks=(),
                hit=wref.hit_rows(clean, prob))


@pytest.mark.parametrize("schur_impl", [0, 2])
@pytest.mark.parametrize("name", ["hongo_mask_huber", "5x40x8_frac_cauchy"])
def test_covariance(name, schur_impl):
    """After a weighted solve every camera / marker x camera / marker block against the reference's (J~'J~)^-1, to 1e-8 of the block's
    largest entry; apply_loss_function = 0 against an unweighted solver at the same parameters to 1e-10 (test_gpu_marker_loss's bars)."""
    cs = _covariance_case(name)
    prob = cs["prob"]
    C, T, M = prob["C"], prob["T"], prob["M"]
    pr = _problem(cs)
    s = capi.Solver(pr, _options(schur_impl, cs["loss"], cs["a"], max_num_iterations=20))
    try:
        s.run()
        s.download()
        s.covariance_compute()
        x = pr.params.copy()
        mc = wref.WeightedMarkerChain(dict(prob, params=x), cs["weights"], cs["variant"], cs["loss"], cs["a"])
        cov, free = ref.covariance(mc, mc.x0())
        at = {b: 6 * i for i, b in enumerate(free)}
        blocks = [b for b in free if b < C or b >= C + T]
        assert len(blocks) == (C - 1) + (M - 1)
        worst = 0.0
        for p in blocks:
            for q in blocks:
                got = s.covariance_block(6 * p, 6 * q)
                want = cov[at[p]:at[p] + 6, at[q]:at[q] + 6]
                worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
        print("%s schur_impl %d: covariance block error %.2e (bar 1e-8)" % (name, schur_impl, worst))
        assert worst <= 1e-8
        s.covariance_compute(apply_loss_function=0)
        plain = [s.covariance_block(6 * p, 6 * q) for p in blocks for q in blocks]
    finally:
        s.close()
        pr.close()
    pr0 = _problem(cs, None, params=x)
    s0 = capi.Solver(pr0, _options(schur_impl, "none", 0.0))
    try:
        s0.covariance_compute()
        for k, (p, q) in enumerate((p, q) for p in blocks for q in blocks):
            want = s0.covariance_block(6 * p, 6 * q)
            assert np.abs(plain[k] - want).max() <= 1e-10 * np.abs(want).max(), (p, q)
    finally:
        s0.close()
        pr0.close()


@pytest.mark.parametrize("schur_impl", [0, 2])
def test_covariance_of_a_time_with_zero_weights_is_rank_deficient(schur_impl):
    cs = wref.case("4x40x6_time7_huber")
    pr = _problem(cs)
    s = capi.Solver(pr, _options(schur_impl, cs["loss"], cs["a"]))
    try:
        s.run()
        with pytest.raises(capi.RsbaError) as e:
            s.covariance_compute()
        assert e.value.code == capi.ERR_RANK_DEFICIENT
        s.covariance_compute(apply_loss_function=0)   # without the loss the weights are ignored too: the system is regular
    finally:
        s.close()
        pr.close()
