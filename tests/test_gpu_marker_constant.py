"""Constant parameter blocks (ceres::Problem::SetParameterBlockConstant) on the marker chain's time-eliminating path.

A constant camera or marker has no reduced column but its transform is applied in every residual that names it; a constant time is
eliminated with E = 0 (no step); with every camera and marker constant only the times are solved.  The path is asserted before
anything is solved, so a regression can never start a large dense solve.  Bars (BASELINE's, as in test_gpu_marker_loss): the same
accept / reject sequence and termination, every iterate's cost to 1e-9 relative, every free block to 1e-6 relative, the final RMS to
1e-4 px, and the constant blocks bit-identical to their input.

Coverage of the switches: 4 x 40 x 6 and 12 x 40 x 20 run every constant set under every elimination switch and back-substitution
selection, with no loss, Huber and Cauchy.  8 x 400 x 16 (the eliminating numpy reference, about five seconds a linearisation) runs three
constant sets under the default and RSBA_MT_SPLIT=0; 8 x 5000 x 16 runs one LM iteration of two sets.
"""
import numpy as np
import pytest

import marker_loss_ref as ref
import marker_sparse_ref as sref
from realsensecalibration_amd import capi
from realsensecalibration_amd import synthetic as syn

pytestmark = pytest.mark.gpu

REASON = {"gradient": 1, "parameter": 2, "function": 3, "max_iterations": 4, "min_radius": 5, "invalid_steps": 6}
TERM = {"CONVERGENCE": 0, "NO_CONVERGENCE": 1, "FAILURE": 2}
LOSS_A = {"none": 0.0, "huber": 2.0, "cauchy": 2.0}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


def _options(schur_impl, loss, **kw):
    a = LOSS_A[loss]
    return capi.default_options(schur_impl=schur_impl, huber_delta=a, loss_type=1 if loss == "cauchy" else 0, **kw)


def _solve(prob, model, schur_impl, loss, constant_blocks=(), expect_elim=True, profile=False, **kw):
    pr = capi.Problem.marker_chain(prob, model)
    try:
        for b in constant_blocks:
            pr.set_parameter_block_constant(6 * b)
        s = capi.Solver(pr, _options(schur_impl, loss, **kw))
        try:
            if expect_elim is not None:
                assert s.eliminates_times() == (1 if expect_elim else 0)
            if profile:
                s.configure_run(kw.get("max_num_iterations", 50), 1)
            summ = s.run()
            s.download()
            log = s.iterations()
            stats = s.kernel_stats(64) if profile else None
        finally:
            s.close()
        params = pr.params.copy()
        _, rms = pr.reprojection_error()
    finally:
        pr.close()
    return summ, log, params, rms, stats


def _assert_matches(prob, got, summary, rows, final, free):
    summ, log, params, rms, _ = got
    assert (summ.termination_type, summ.stop_reason, summ.num_iterations) == (TERM[summary["termination"]], REASON[summary["reason"]], len(rows) - 1)
    assert [int(v) for v in log[:, 7]] == [rw["valid"] + 2 * rw["successful"] for rw in rows]
    for j, rw in enumerate(rows):
        assert abs(log[j, 1] - rw["cost"]) <= 1e-9 * rw["cost"], "iterate %d: cost %.15e, reference %.15e" % (j, log[j, 1], rw["cost"])
    assert abs(summ.final_cost - summary["final_cost"]) <= 1e-9 * summary["final_cost"]
    p = params.reshape(-1, 6)
    if free.size:
        err = np.abs(p[free] - final[free]).max(axis=1) / np.maximum(np.abs(final[free]).max(axis=1), 1e-12)
        assert err.max() < 1e-6, "final parameters differ from the reference's by %.2e relative per block" % err.max()
    fixed = np.setdiff1d(np.arange(p.shape[0]), free)
    np.testing.assert_array_equal(p[fixed], np.asarray(prob["params"]).reshape(-1, 6)[fixed])
    rms_ref = np.sqrt(summary["final_sumsq"] / (8.0 * prob["N"]))
    assert abs(rms - rms_ref) <= 1e-4, (rms, rms_ref)


_REF = {}


def _reference(key, prob, model, loss, const, sparse=False):
    if key not in _REF:
        variant = 1 if model == capi.MODEL_MARKER_CHAIN_TEST2 else 0
        if sparse:
            smc = sref.SparseMarkerChain(prob, variant, loss, LOSS_A[loss], const)
            x, summary, rows = sref.minimise(smc)
            mc = smc.mc
        else:
            mc = ref.MarkerChain(prob, variant, loss, LOSS_A[loss], const)
            x, summary, rows = ref.minimise(mc)
        _REF[key] = (summary, rows, mc.full(x), mc.free_blocks)
    return _REF[key]


def _check(prob, model, schur_impl, loss, const, key, sparse=False):
    summary, rows, final, free = _reference(key, prob, model, loss, const, sparse)
    got = _solve(prob, model, schur_impl, loss, const)
    _assert_matches(prob, got, summary, rows, final, free)
    return got


def _rig(shape):
    C, T, M = shape
    return ref.displace_corners(syn.make_marker_chain(C, T, M, seed=50 + C + T + M), 0.05, 40.0, C * T * M)


def _const_set(prob, kind):
    C, T, M = prob["C"], prob["T"], prob["M"]
    if kind == "one_each":
        return (2, C + 5, C + T + 3)
    if kind == "markers":
        return tuple(C + T + m for m in range(1, M))
    if kind == "cameras":
        return tuple(range(1, min(C, 4)))
    if kind == "times":
        # several times; the first one's cameras and markers constant too: residual blocks with no free block (fixed cost only)
        t0 = int(prob["t"][0])
        sel = np.asarray(prob["t"]) == t0
        cams = sorted({int(c) for c in np.asarray(prob["c"])[sel] if c != 0})
        mars = sorted({C + T + int(m) for m in np.asarray(prob["m"])[sel] if m != 0})
        return tuple(sorted({C + t0, C + 1, C + 3, C + 7} | set(cams) | set(mars)))
    if kind == "rig":
        return tuple(range(1, C)) + tuple(C + T + m for m in range(1, M))   # n_r = 0: only the times are free
    raise ValueError(kind)


KINDS = ["one_each", "markers", "cameras", "times", "rig"]
SWITCHES = [{}, {"RSBA_MT_ACC_MFMA": "0"}, {"RSBA_MT_FORK": "0"}, {"RSBA_MT_SPLIT": "0"}, {"RSBA_MT_SOLVE_LDS": "0"},
            {"RSBA_MT_SPLIT_BACKSUB": "0"}, {"RSBA_MT_SPLIT_BACKSUB": "0", "RSBA_MT_BACKSUB_WG": "0"}]
_ids = lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default"   # noqa: E731


# ---- which path runs (these fail where constant blocks veto the elimination)
@pytest.mark.parametrize("schur_impl,shape", [(2, (4, 40, 6)), (1, (4, 60, 8))], ids=["schur_impl2", "automatic_above_384"])
def test_constant_blocks_take_the_time_eliminating_path(schur_impl, shape):
    prob = _rig(shape)
    C, T, M = prob["C"], prob["T"], prob["M"]
    assert 6 * (C + T + M) > 384 or schur_impl == 2
    got = _solve(prob, capi.MODEL_MARKER_CHAIN, schur_impl, "none", _const_set(prob, "one_each"), expect_elim=True, profile=True,
                 max_num_iterations=5)
    stats = got[4]
    assert not any("k_marker_system" in k for k in stats), stats
    assert any(k.startswith("k_mc_") or k.startswith("k_time_") for k in stats), stats


def test_time_elimination_query():
    prob = _rig((4, 40, 6))
    pr = capi.Problem.marker_chain(prob)
    try:
        for impl, want in ((0, 0), (2, 1)):
            s = capi.Solver(pr, _options(impl, "none"))
            try:
                assert s.eliminates_times() == want
            finally:
                s.close()
    finally:
        pr.close()
    lib = capi.load()
    assert lib.rsba_solver_time_elimination(None, None) == capi.ERR_ARG
    # the point model has no time blocks: RSBA_ERR_UNSUPPORTED
    pp = capi.Problem.points(syn.make_problem(4, 200, 3, seed=5))
    try:
        s = capi.Solver(pp)
        try:
            v = capi.C.c_int32(7)
            assert lib.rsba_solver_time_elimination(s.h, capi.C.byref(v)) == capi.ERR_UNSUPPORTED
            assert v.value == 7
        finally:
            s.close()
    finally:
        pp.close()


def _report_counts(text):
    """Original / reduced columns of the report's parameter-block and parameter rows."""
    out = {}
    for ln in text.splitlines():
        for key in ("Parameter blocks", "Parameters", "Residual blocks"):
            if ln.startswith(key) and ln[len(key):len(key) + 1] == " ":
                out[key] = tuple(int(v) for v in ln[len(key):].split())
    return out


def test_full_report_counts_constant_blocks():
    """Ceres' summary counts: the constant blocks leave the reduced program, on both paths alike; a constant block no residual uses
    (camera 0) is in neither column."""
    prob = _rig((6, 50, 9))
    C, T, M = prob["C"], prob["T"], prob["M"]
    const = (0, 2, C + 4, C + 9, C + T + 3)
    # camera 0 and marker 0 are not part of RSBA_MODEL_MARKER_CHAIN's residuals
    ub = {int(c) for c in prob["c"] if c != 0} | {C + int(t) for t in prob["t"]} | {C + T + int(m) for m in prob["m"] if m != 0}
    used, nconst = len(ub), len(ub & set(const))
    assert nconst == 4
    reports = {}
    for impl, elim in ((0, 0), (2, 1)):
        pr = capi.Problem.marker_chain(prob)
        try:
            for b in const:
                pr.set_parameter_block_constant(6 * b)
            s = capi.Solver(pr, _options(impl, "none", max_num_iterations=3))
            try:
                assert s.eliminates_times() == elim
                s.run()
                reports[impl] = _report_counts(s.full_report())
            finally:
                s.close()
        finally:
            pr.close()
    want = {"Parameter blocks": (used, used - nconst), "Parameters": (6 * used, 6 * (used - nconst)), "Residual blocks": (prob["N"], prob["N"])}
    assert reports[0] == want and reports[2] == want, reports


# ---- committed data against marker_loss_ref
@pytest.mark.parametrize("loss", ["none", "huber", "cauchy"])
def test_hongo_constant_blocks(loss):
    prob = ref.hongo()
    C, T = prob["C"], prob["T"]
    _check(prob, capi.MODEL_MARKER_CHAIN, 2, loss, (2, C + 3, C + T + 5), ("hongo", loss))


@pytest.mark.parametrize("loss", ["none", "huber", "cauchy"])
def test_test2_constant_blocks(loss):
    prob = ref.test2()
    C, T = prob["C"], prob["T"]
    _check(prob, capi.MODEL_MARKER_CHAIN_TEST2, 2, loss, (1, C + 2, C + T + 3), ("test2", loss))


# ---- synthetic rigs: every constant set under every elimination switch and back-substitution selection
@pytest.mark.parametrize("env", SWITCHES, ids=_ids)
@pytest.mark.parametrize("loss", ["none", "huber", "cauchy"])
@pytest.mark.parametrize("kind", KINDS)
def test_small_rig_every_switch(kind, loss, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = _rig((4, 40, 6))
    _check(prob, capi.MODEL_MARKER_CHAIN, 2, loss, _const_set(prob, kind), ((4, 40, 6), kind, loss))


@pytest.mark.parametrize("env", SWITCHES, ids=_ids)
@pytest.mark.parametrize("loss", ["none", "huber", "cauchy"])
@pytest.mark.parametrize("kind", KINDS)
def test_12x40x20(kind, loss, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = _rig((12, 40, 20))
    _check(prob, capi.MODEL_MARKER_CHAIN, 2, loss, _const_set(prob, kind), ((12, 40, 20), kind, loss))


# (the eliminating numpy reference: about five seconds a linearisation at this size)
@pytest.mark.parametrize("env", [{}, {"RSBA_MT_SPLIT": "0"}], ids=_ids)
@pytest.mark.parametrize("kind,loss", [("markers", "none"), ("times", "huber"), ("rig", "none")])
def test_8x400x16(kind, loss, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = _rig((8, 400, 16))
    _check(prob, capi.MODEL_MARKER_CHAIN, 2, loss, _const_set(prob, kind), ((8, 400, 16), kind, loss), sparse=True)


def test_dense_and_eliminated_gpu_paths_agree():
    prob = _rig((12, 40, 20))
    const = _const_set(prob, "times")
    a = _solve(prob, capi.MODEL_MARKER_CHAIN, 0, "huber", const, expect_elim=False)
    b = _solve(prob, capi.MODEL_MARKER_CHAIN, 2, "huber", const, expect_elim=True)
    assert np.array_equal(a[1][:, 7], b[1][:, 7])
    assert np.all(np.abs(a[1][:, 1] - b[1][:, 1]) <= 1e-9 * np.abs(a[1][:, 1]))
    pa, pb = a[2].reshape(-1, 6), b[2].reshape(-1, 6)
    assert np.max(np.abs(pa - pb).max(axis=1) / np.maximum(np.abs(pa).max(axis=1), 1e-12)) < 1e-6
    assert abs(a[3] - b[3]) <= 1e-4


# ---- invariants
@pytest.mark.parametrize("loss", ["none", "cauchy"])
def test_a_constant_block_no_residual_uses_changes_nothing(loss):
    """Camera 0 and marker 0 are not part of RSBA_MODEL_MARKER_CHAIN's residuals: making them constant gives the same bits."""
    prob = syn.make_marker_chain(6, 60, 9, seed=36)
    C, T = prob["C"], prob["T"]
    s0, log0, x0, rms0, _ = _solve(prob, capi.MODEL_MARKER_CHAIN, 2, loss)
    s1, log1, x1, rms1, _ = _solve(prob, capi.MODEL_MARKER_CHAIN, 2, loss, (0, C + T), expect_elim=True)
    assert log0.shape[0] > 2
    np.testing.assert_array_equal(log0, log1)
    np.testing.assert_array_equal(x0, x1)
    assert rms0 == rms1


def test_repeated_runs_are_bit_identical():
    prob = _rig((8, 400, 16))
    pr = capi.Problem.marker_chain(prob)
    try:
        for b in _const_set(prob, "times"):
            pr.set_parameter_block_constant(6 * b)
        s = capi.Solver(pr, _options(2, "huber"))
        try:
            runs = []
            for _ in range(2):
                s.run()
                s.download()
                runs.append((s.iterations(), pr.params.copy()))
            np.testing.assert_array_equal(runs[0][0], runs[1][0])
            np.testing.assert_array_equal(runs[0][1], runs[1][1])
        finally:
            s.close()
    finally:
        pr.close()


# ---- at the benchmarked size, against the eliminating numpy reference (the path is asserted before the solve)
@pytest.mark.parametrize("kind", ["markers", "cameras_and_times"])
def test_scale_8x5000x16(kind):
    prob = syn.make_marker_chain(8, 5000, 16, seed=11)
    C, T, M = prob["C"], prob["T"], prob["M"]
    const = tuple(C + T + m for m in range(1, M)) if kind == "markers" else (2, 5) + tuple(C + t for t in range(0, 5000, 50))
    it = 1   # (one LM iteration: two linearisations of the numpy reference, about a minute each at this size)
    smc = sref.SparseMarkerChain(prob, 0, "none", 0.0, const)
    x, summary, rows = sref.minimise(smc, max_num_iterations=it)
    got = _solve(prob, capi.MODEL_MARKER_CHAIN, 1, "none", const, expect_elim=True, max_num_iterations=it)
    _assert_matches(prob, got, summary, rows, smc.mc.full(x), smc.mc.free_blocks)


# ---- covariance on this path
@pytest.mark.parametrize("apply_loss", [1, 0])
def test_covariance_with_constant_blocks(apply_loss):
    prob = _rig((5, 40, 8))
    C, T, M = prob["C"], prob["T"], prob["M"]
    const = (2, C + 4, C + T + 3)
    pr = capi.Problem.marker_chain(prob)
    try:
        for b in const:
            pr.set_parameter_block_constant(6 * b)
        s = capi.Solver(pr, _options(2, "cauchy", max_num_iterations=20))
        try:
            assert s.eliminates_times() == 1
            s.run()
            s.download()
            s.covariance_compute(apply_loss_function=apply_loss)
            x = pr.params.copy()
            mc = ref.MarkerChain(dict(prob, params=x), 0, "cauchy" if apply_loss else "none", 2.0, const)
            cov, free = ref.covariance(mc, mc.x0())
            at = {b: 6 * i for i, b in enumerate(free)}
            blocks = [b for b in list(range(1, C)) + [C + T + m for m in range(1, M)]]
            for p in blocks:
                for q in blocks:
                    got = s.covariance_block(6 * p, 6 * q)
                    if p in const or q in const:
                        assert np.all(got == 0.0), (p, q)
                        continue
                    want = cov[at[p]:at[p] + 6, at[q]:at[q] + 6]
                    assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max(), (p, q)
        finally:
            s.close()
    finally:
        pr.close()
