"""rsba_solver_covariance_blocks and rsba_solver_time_covariances (Covariance::GetCovarianceBlock for any pair of blocks) against the
numpy references: tests/marker_loss_ref.py / tests/marker_weight_ref.py (marker chain, time blocks included) and
tests/covariance_ref.py (point model, camera x point and point x point').

The bar is tests/test_gpu_covariance.py's: max|got - ref| <= 1e-8 max|ref block|, each block against its own largest entry.  The
reference resolves it: its dense inverse and its Schur-formula route agree to 1e-10 at every shape used here
(tests/test_covariance_cross_ref_cpu.py).  The dense and the time-eliminating path agree to 1e-10 of the block, the bar
test_gpu_covariance.py holds the two paths to.  Every case prints its worst error / bar."""
import ctypes as C

import numpy as np
import pytest

import covariance_cross_ref as xr
import covariance_ref as cr
import marker_loss_ref as ref
import marker_weight_ref as wref
from realsensecalibration_amd import capi

pytestmark = pytest.mark.gpu
TOL = 1e-8
PATHS = 1e-10
C_VOID = C.c_void_p


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = capi.load()
    assert lib.rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


def _options(schur_impl, loss="none", a=0.0, **kw):
    return capi.default_options(schur_impl=schur_impl, huber_delta=a if loss != "none" else 0.0, loss_type=1 if loss == "cauchy" else 0, **kw)


def _code(call):
    try:
        call()
        return capi.OK
    except capi.RsbaError as e:
        return e.code


# ------------------------------------------------------------------------------------------------ marker chain
class Marker:
    """A marker-chain problem on a solver, optionally solved, with the covariance computed; closes both."""

    def __init__(self, prob, schur_impl, loss="none", a=0.0, const=(), weights=None, run=True, compute=True, iters=20, **cov):
        self.prob, self.C, self.T, self.M = prob, prob["C"], prob["T"], prob["M"]
        self.pr = capi.Problem.marker_chain(prob)
        for b in const:
            self.pr.set_parameter_block_constant(6 * b)
        if weights is not None:
            self.pr.set_observation_weights(weights)
        self.s = capi.Solver(self.pr, _options(schur_impl, loss, a, max_num_iterations=iters))
        assert self.s.eliminates_times() == (1 if schur_impl == 2 else 0)
        if run:
            self.s.run()
            self.s.download()
        self.x = self.pr.params.copy()
        if compute:
            self.s.covariance_compute(**cov)

    def close(self):
        self.s.close()
        self.pr.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _marker_reference(prob, x, loss="none", a=0.0, const=(), weights=None):
    p = dict(prob, params=x)
    mc = wref.WeightedMarkerChain(p, weights, 0, loss, a, const) if weights is not None else ref.MarkerChain(p, 0, loss, a, const)
    cov, free = ref.covariance(mc, mc.x0())
    return cov, {int(b): 6 * i for i, b in enumerate(free)}


def _check_marker_pairs(s, pairs, cov, at, label, const=()):
    """One covariance_blocks call for the block pairs; each against the reference's block -> worst relative error."""
    got = s.covariance_blocks([(6 * p, 6 * q) for p, q in pairs])
    worst = 0.0
    for (p, q), g in zip(pairs, got):
        assert g.shape == (6, 6)
        if p in const or q in const:
            assert np.all(g == 0.0), (p, q)
            continue
        want = cov[at[p]:at[p] + 6, at[q]:at[q] + 6]
        err = np.abs(g - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err <= TOL, (label, p, q, err)
    print("%s: %d pairs, worst error / bar %.3e (bar %.0e)" % (label, len(pairs), worst / TOL, TOL))
    return got


def _check_time_marginals(m, const=()):
    """time_covariances() equals the (t, t) blocks bit for bit; zeros for a constant time."""
    tc = m.s.time_covariances()
    assert tc.shape == (m.T, 6, 6)
    tt = m.s.covariance_blocks([(m.s.time_offset(t), m.s.time_offset(t)) for t in range(m.T)])
    for t in range(m.T):
        np.testing.assert_array_equal(tc[t], tt[t])
        np.testing.assert_array_equal(tc[t], tc[t].T)
        assert np.all(tc[t] == 0.0) == (m.C + t in const)
    np.testing.assert_array_equal(m.s.time_covariances(), tc)
    return tc


def _paths_agree(a, b, label):
    worst = max(np.abs(g2 - g0).max() / np.abs(g0).max() for g2, g0 in zip(a, b) if np.any(g0 != 0.0))
    print("%s: time-eliminating against dense, worst difference / bar %.3e (bar %.0e)" % (label, worst / PATHS, PATHS))
    assert worst <= PATHS


def test_hongo_all_pairs_on_both_paths():
    """All 19 x 19 pairs of free blocks (6 times, 3 cameras, 10 markers) after a solve, on the time-eliminating path and on the dense
    path at the same parameters."""
    prob = ref.hongo()
    C, T, M = prob["C"], prob["T"], prob["M"]
    with Marker(prob, 2) as m2:
        cov, at = _marker_reference(prob, m2.x)
        free = sorted(at)
        assert len(free) == 19 and sum(C <= b < C + T for b in free) == 6
        pairs = [(p, q) for p in free for q in free]
        g2 = _check_marker_pairs(m2.s, pairs, cov, at, "hongo time-eliminating")
        _check_time_marginals(m2)
        with Marker(dict(prob, params=m2.x), 0, run=False) as m0:
            g0 = _check_marker_pairs(m0.s, pairs, cov, at, "hongo dense")
            _check_time_marginals(m0)
        _paths_agree(g2, g0, "hongo")


def test_more_than_64_rows_per_time():
    """(8, 12, 16): 78 to 111 rows in every time, the second chunk of 64 rows.  All time marginals, all (time, camera / marker) and all
    (t, t'), and the dense path at the same parameters."""
    prob = xr.marker_rig(xr.MC_TWO_CHUNKS)
    C, T, M = prob["C"], prob["T"], prob["M"]
    assert xr.rows_per_time(prob).min() > 64
    times = [C + t for t in range(T)]
    reduced = list(range(1, C)) + [C + T + k for k in range(1, M)]
    pairs = [(p, q) for p in times for q in times] + [(p, q) for p in times for q in reduced] + [(q, p) for p in times for q in reduced]
    with Marker(prob, 2) as m2:
        cov, at = _marker_reference(prob, m2.x)
        g2 = _check_marker_pairs(m2.s, pairs, cov, at, "8x12x16 time-eliminating")
        _check_time_marginals(m2)
        with Marker(dict(prob, params=m2.x), 0, run=False) as m0:
            g0 = _check_marker_pairs(m0.s, pairs, cov, at, "8x12x16 dense")
        _paths_agree(g2, g0, "8x12x16")


def test_80_times():
    """(5, 80, 8): 80 marginals, every (t, x), and (t, t') of the first 5 times against all others."""
    prob = xr.marker_rig(xr.MC_LONG)
    C, T, M = prob["C"], prob["T"], prob["M"]
    times = [C + t for t in range(T)]
    reduced = list(range(1, C)) + [C + T + k for k in range(1, M)]
    pairs = [(p, p) for p in times] + [(p, q) for p in times for q in reduced] + [(p, q) for p in times[:5] for q in times if q != p]
    with Marker(prob, 2) as m:
        cov, at = _marker_reference(prob, m.x)
        _check_marker_pairs(m.s, pairs, cov, at, "5x80x8 time-eliminating")
        _check_time_marginals(m)


@pytest.mark.parametrize("schur_impl", [2, 0])
def test_huber_weights_and_constant_blocks(schur_impl):
    """(3, 70, 5): Huber 2 px, weights with zeros, a constant time block and a constant marker block, with and without the loss."""
    cs = xr.weighted_case()
    prob, const = cs["prob"], cs["constant_blocks"]
    C, T, M = prob["C"], prob["T"], prob["M"]
    assert const == (3 + 4, 3 + 70 + 2)
    times = [C + t for t in range(T)]
    reduced = list(range(1, C)) + [C + T + k for k in range(1, M)]
    probe = times[:8]   # (the constant time, C + 4, among them)
    pairs = [(p, p) for p in times] + [(p, q) for p in times for q in reduced] + [(q, p) for p in probe for q in reduced] \
        + [(p, q) for p in probe for q in times] + [(p, q) for p in reduced for q in reduced]
    with Marker(prob, schur_impl, cs["loss"], cs["a"], const, cs["weights"]) as m:
        for apply_loss in (1, 0):
            if not apply_loss:
                m.s.covariance_compute(apply_loss_function=0)
            cov, at = _marker_reference(prob, m.x, cs["loss"], cs["a"], const, cs["weights"]) if apply_loss else _marker_reference(prob, m.x, const=const)
            assert not any(b in at for b in const)
            _check_marker_pairs(m.s, pairs, cov, at, "3x70x5 schur_impl %d apply_loss %d" % (schur_impl, apply_loss), const)
            tc = _check_time_marginals(m, const)
            assert np.all(tc[4] == 0.0)


def test_failed_compute_leaves_no_result():
    cs = wref.case("4x40x6_time7_huber")   # every row of time 7 has weight 0
    with Marker(cs["prob"], 2, cs["loss"], cs["a"], weights=cs["weights"], compute=False) as m:
        assert _code(m.s.covariance_compute) == capi.ERR_RANK_DEFICIENT
        assert _code(lambda: m.s.covariance_blocks([(m.s.time_offset(1), m.s.time_offset(1))])) == capi.ERR_ARG
        assert _code(m.s.time_covariances) == capi.ERR_ARG


def test_no_compute_and_dropped_results():
    prob = xr.marker_rig(xr.MC_TWO_CHUNKS)
    with Marker(prob, 2, "huber", 2.0, run=False, compute=False) as m:
        q = [(m.s.time_offset(0), m.s.marker_offset(1))]
        assert _code(lambda: m.s.covariance_blocks(q)) == capi.ERR_ARG and _code(m.s.time_covariances) == capi.ERR_ARG
        m.s.covariance_compute()
        first = m.s.covariance_blocks(q)[0]
        m.s.set_parameters(m.x)
        assert _code(lambda: m.s.covariance_blocks(q)) == capi.ERR_ARG and _code(m.s.time_covariances) == capi.ERR_ARG
        m.s.covariance_compute()
        again = m.s.covariance_blocks(q)[0]   # (a second compute: k_cov_mc_lin's atomic sums may differ in the last bits)
        assert np.abs(again - first).max() <= PATHS * np.abs(first).max()
        m.s.set_observation_weights(np.ones(prob["N"]))
        assert _code(lambda: m.s.covariance_blocks(q)) == capi.ERR_ARG and _code(m.s.time_covariances) == capi.ERR_ARG


# ------------------------------------------------------------------------------------------------ point model
class Points:
    """A point problem (camera 0 and point 0 constant) on a solver, optionally solved, with the covariance computed."""

    def __init__(self, prob, huber=0.0, cauchy=False, run=True, iters=20):
        self.prob, self.C, self.P = prob, prob["C"], prob["P"]
        self.pr = capi.Problem.points(prob)
        self.pr.set_camera_constant(0)
        self.pr.set_point_constant(0)
        self.s = capi.Solver(self.pr, capi.default_options(schur_impl=1, huber_delta=huber, loss_type=1 if cauchy else 0, max_num_iterations=iters))
        if run:
            self.s.run()
            self.s.download()
        self.x = self.pr.params.copy()
        self.s.covariance_compute()

    def close(self):
        self.s.close()
        self.pr.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _check_point_pairs(s, C, pairs, cov, keep, label, const=((0,), (0,))):
    """pairs of ("c", i) / ("p", j); one covariance_blocks call, each block against covariance_ref's."""
    off = lambda b: s.camera_offset(b[1]) if b[0] == "c" else s.point_offset(b[1])   # noqa: E731
    pos = {int(k): i for i, k in enumerate(keep)}
    got = s.covariance_blocks([(off(a), off(b)) for a, b in pairs])
    worst = 0.0
    for (a, b), g in zip(pairs, got):
        na, nb = (6 if a[0] == "c" else 3), (6 if b[0] == "c" else 3)
        assert g.shape == (na, nb)
        if any(blk[1] in const[0 if blk[0] == "c" else 1] for blk in (a, b)):
            assert np.all(g == 0.0), (a, b)
            continue
        oa, ob = (6 * a[1] if a[0] == "c" else 6 * C + 3 * a[1]), (6 * b[1] if b[0] == "c" else 6 * C + 3 * b[1])
        want = cov[np.ix_([pos[oa + t] for t in range(na)], [pos[ob + t] for t in range(nb)])]
        err = np.abs(g - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err <= TOL, (label, a, b, err)
    print("%s: %d pairs, worst error / bar %.3e (bar %.0e)" % (label, len(pairs), worst / TOL, TOL))
    return got


def _point_reference(oracle, prob, x, huber=0.0, cauchy=False):
    cov, keep, kappa = cr.point_covariance(oracle, prob, x, (0,), (0,), huber, cauchy)
    print("kappa(J'J) = %.3e" % kappa)
    assert kappa < 1e10
    return cov, keep


@pytest.mark.parametrize("shape", [xr.PT_SMALL, xr.PT_TWO_CHUNKS], ids=["6x40x4", "70x24x70"])
def test_point_model_all_pairs(oracle, shape):
    """Every camera x point (both orientations), every point x point' and every camera x camera'; (70, 24, 70): 70 views per point, the
    second chunk of views."""
    prob = xr.point_problem(shape)
    C, P = prob["C"], prob["P"]
    with Points(prob) as m:
        cov, keep = _point_reference(oracle, prob, m.x)
        cams, pts = [("c", c) for c in range(C)], [("p", j) for j in range(P)]
        pairs = [(a, b) for a in cams for b in pts] + [(b, a) for a in cams for b in pts] + [(a, b) for a in pts for b in pts] + [(a, b) for a in cams for b in cams]
        _check_point_pairs(m.s, C, pairs, cov, keep, "points %dx%dx%d" % shape[:3])


@pytest.mark.parametrize("cauchy", [False, True], ids=["huber", "cauchy"])
def test_point_model_robust_loss(oracle, cauchy):
    prob = xr.point_problem(xr.PT_ROBUST)
    C, P = prob["C"], prob["P"]
    rng = np.random.default_rng(200)
    pp = [(("p", int(j)), ("p", int(k))) for j, k in zip(rng.integers(1, P, 200), rng.integers(1, P, 200))]
    with Points(prob, 2.0, cauchy) as m:
        cov, keep = _point_reference(oracle, prob, m.x, 2.0, cauchy)
        pairs = [(("c", c), ("p", j)) for c in range(C) for j in range(P)] + pp
        _check_point_pairs(m.s, C, pairs, cov, keep, "points 8x200x5 %s" % ("cauchy" if cauchy else "huber"))


# ------------------------------------------------------------------------------------------------ the state a result belongs to
def test_snapshot_marker_chain():
    """compute at the uploaded start, query, run, query again: the same bits (the queries re-linearise from the compute's snapshot)."""
    prob = xr.marker_rig(xr.MC_TWO_CHUNKS)
    C, T, M = prob["C"], prob["T"], prob["M"]
    with Marker(prob, 2, run=False) as m:
        s = m.s
        q = [(s.time_offset(t), s.time_offset(u)) for t in range(3) for u in range(T)] + [(s.time_offset(t), s.marker_offset(k)) for t in range(T) for k in (1, M - 1)] \
            + [(s.camera_offset(1), s.time_offset(5)), (s.camera_offset(1), s.marker_offset(2))]
        before = s.covariance_blocks(q)
        s.run()
        s.download()
        assert not np.array_equal(m.pr.params, m.x)
        after = s.covariance_blocks(q)
        for a, b in zip(before, after):
            np.testing.assert_array_equal(a, b)
        tc = s.time_covariances()   # formed after the run, from the snapshot
        for t in range(3):
            np.testing.assert_array_equal(tc[t], before[t * T + t])


def test_snapshot_point_model():
    prob = xr.point_problem(xr.PT_SMALL)
    C, P = prob["C"], prob["P"]
    with Points(prob, run=False) as m:
        s = m.s
        q = [(s.camera_offset(c), s.point_offset(j)) for c in range(1, C) for j in range(1, P)] + [(s.point_offset(j), s.point_offset(j + 1)) for j in range(1, P - 1)]
        before = s.covariance_blocks(q)
        s.run()
        s.download()
        assert not np.array_equal(m.pr.params, m.x)
        for a, b in zip(before, s.covariance_blocks(q)):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------ repeatability, symmetry, the old call
def _twice_and_transposed(s, pairs):
    a, b = s.covariance_blocks(pairs), s.covariance_blocks(pairs)
    t = s.covariance_blocks([(q, p) for p, q in pairs])
    for x, y, z in zip(a, b, t):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(z, x.T)
        assert np.any(x != 0.0)
    return a


@pytest.mark.parametrize("schur_impl", [2, 0])
def test_repeatable_symmetric_and_the_old_call_marker_chain(schur_impl):
    prob = xr.marker_rig(xr.MC_TWO_CHUNKS)
    C, T, M = prob["C"], prob["T"], prob["M"]
    with Marker(prob, schur_impl) as m:
        s = m.s
        tt = [(s.time_offset(t), s.time_offset(t)) for t in range(T)]
        tu = [(s.time_offset(t), s.time_offset(u)) for t in range(4) for u in range(T) if u != t]
        tx = [(s.time_offset(t), x) for t in range(T) for x in (s.camera_offset(1), s.camera_offset(C - 1), s.marker_offset(1), s.marker_offset(M - 1))]
        old = [(6 * p, 6 * q) for p in list(range(1, C)) + [C + T + k for k in range(1, M)] for q in (1, C + T + 3)]
        _twice_and_transposed(s, tt + tu + tx)
        for (a, b), g in zip(old, _twice_and_transposed(s, old)):
            np.testing.assert_array_equal(g, s.covariance_block(a, b))   # the bits of the single-pair call
        # an unreferenced (base) block in any pair: RSBA_ERR_ARG for the whole call, nothing written
        for bad in (s.camera_offset(0), s.marker_offset(0), 6 * (C + T + M), -6, 3):
            oa = np.array([s.time_offset(0), s.time_offset(1), bad], np.int64)
            ob = np.array([s.time_offset(0), bad, s.marker_offset(1)], np.int64)
            out = np.full(3 * 36, 7.5)
            rc = capi.load().rsba_solver_covariance_blocks(s.h, 3, oa.ctypes.data_as(C_VOID), ob.ctypes.data_as(C_VOID), out.ctypes.data_as(C_VOID))
            assert rc == capi.ERR_ARG and np.all(out == 7.5), bad
        assert capi.load().rsba_solver_covariance_blocks(s.h, -1, oa.ctypes.data_as(C_VOID), ob.ctypes.data_as(C_VOID), out.ctypes.data_as(C_VOID)) == capi.ERR_ARG
        assert capi.load().rsba_solver_covariance_blocks(s.h, 1, None, ob.ctypes.data_as(C_VOID), out.ctypes.data_as(C_VOID)) == capi.ERR_ARG
        assert capi.load().rsba_solver_covariance_blocks(s.h, 1, oa.ctypes.data_as(C_VOID), ob.ctypes.data_as(C_VOID), None) == capi.ERR_ARG
        assert capi.load().rsba_solver_covariance_blocks(s.h, 0, oa.ctypes.data_as(C_VOID), ob.ctypes.data_as(C_VOID), out.ctypes.data_as(C_VOID)) == capi.OK
        assert np.all(out == 7.5) and s.covariance_blocks([]) == []
        assert capi.load().rsba_solver_time_covariances(s.h, None) == capi.ERR_ARG
        assert _code(lambda: s.covariance_block(s.time_offset(0), s.time_offset(0))) == capi.ERR_UNSUPPORTED   # the old call's contract


def test_repeatable_symmetric_and_the_old_call_point_model():
    prob = xr.point_problem(xr.PT_SMALL)
    C, P = prob["C"], prob["P"]
    with Points(prob) as m:
        s = m.s
        cp = [(s.camera_offset(c), s.point_offset(j)) for c in range(1, C) for j in range(1, P)]
        pq = [(s.point_offset(j), s.point_offset(k)) for j in range(1, P) for k in range(1, P) if j != k]
        _twice_and_transposed(s, cp + pq)
        cc = [(s.camera_offset(a), s.camera_offset(b)) for a in range(1, C) for b in range(1, C)]
        for (a, b), g in zip(cc, _twice_and_transposed(s, cc)):
            np.testing.assert_array_equal(g, s.covariance_block(a, b))
        pc = s.point_covariances()
        for j, g in enumerate(s.covariance_blocks([(s.point_offset(j), s.point_offset(j)) for j in range(P)])):
            np.testing.assert_array_equal(g, pc[j])
            np.testing.assert_array_equal(g, s.covariance_block(s.point_offset(j), s.point_offset(j)))
        assert _code(s.time_covariances) == capi.ERR_UNSUPPORTED
        for bad in (6 * C + 1, 6 * C + 3 * P, 1, -3):
            oa = np.array([s.camera_offset(1), bad], np.int64)
            ob = np.array([s.point_offset(2), s.point_offset(3)], np.int64)
            out = np.full(2 * 36, 7.5)
            rc = capi.load().rsba_solver_covariance_blocks(s.h, 2, oa.ctypes.data_as(C_VOID), ob.ctypes.data_as(C_VOID), out.ctypes.data_as(C_VOID))
            assert rc == capi.ERR_ARG and np.all(out == 7.5), bad


def test_unreferenced_camera_is_an_argument_error_point_model():
    prob = xr.point_problem(xr.PT_SMALL)
    keep = prob["cam_idx"] != 5   # camera 5 observes nothing
    prob = dict(prob, cam_idx=np.ascontiguousarray(prob["cam_idx"][keep]), pt_idx=np.ascontiguousarray(prob["pt_idx"][keep]),
                obs=np.ascontiguousarray(prob["obs"].reshape(-1, 2)[keep].reshape(-1)), N=int(keep.sum()))
    with Points(prob, run=False) as m:
        assert _code(lambda: m.s.covariance_blocks([(m.s.camera_offset(1), m.s.point_offset(3)), (m.s.camera_offset(5), m.s.point_offset(3))])) == capi.ERR_ARG
        assert np.all(np.isfinite(m.s.covariance_blocks([(m.s.camera_offset(1), m.s.point_offset(3))])[0]))


# ------------------------------------------------------------------------------------------------ non-interference
def _log_and_params(s, pr):
    s.run()
    s.download()
    return s.iterations(), pr.params.copy()


def test_non_interference_marker_chain():
    """run -> compute -> queries -> run gives the log and the parameters of run -> run, bit for bit."""
    prob = xr.marker_rig(xr.MC_TWO_CHUNKS)
    T, M = prob["T"], prob["M"]
    runs = []
    for with_cov in (True, False):
        with Marker(prob, 2, run=False, compute=False, iters=3) as m:
            _log_and_params(m.s, m.pr)
            if with_cov:
                m.s.covariance_compute()
                m.s.time_covariances()
                m.s.covariance_blocks([(m.s.time_offset(t), m.s.time_offset(u)) for t in range(T) for u in range(T)] + [(m.s.time_offset(t), m.s.marker_offset(k)) for t in range(T) for k in range(1, M)])
            runs.append(_log_and_params(m.s, m.pr))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])


def test_non_interference_point_model():
    prob = xr.point_problem(xr.PT_TWO_CHUNKS)
    C, P = prob["C"], prob["P"]
    runs = []
    for with_cov in (True, False):
        pr = capi.Problem.points(prob)
        pr.set_camera_constant(0)
        pr.set_point_constant(0)
        s = capi.Solver(pr, capi.default_options(schur_impl=1, max_num_iterations=3))
        _log_and_params(s, pr)
        if with_cov:
            s.covariance_compute()
            s.covariance_blocks([(s.camera_offset(c), s.point_offset(j)) for c in range(C) for j in range(P)] + [(s.point_offset(j), s.point_offset(k)) for j in range(P) for k in range(P)])
        runs.append(_log_and_params(s, pr) + (s.schedule_info(),))
        s.close()
        pr.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2]


# ------------------------------------------------------------------------------------------------ sharded point model
def test_sharded_point_model(oracle):
    """A 2-rank loopback group: camera x point on the owning rank, point x point' within a shard, and pairs with camera 3, which only
    rank 1's shard observes, on rank 0 — all against the whole-problem reference."""
    import test_gpu_sharded_queries as tsq
    keep = lambda sh, r, lo: (sh["cam_idx"] != 4) & ((sh["cam_idx"] != 3) | (r != 0))   # noqa: E731
    c = tsq.Case(5, 70, 4, 32, 2, keep=keep)
    assert 3 not in c.shards[0]["cam_idx"] and 3 in c.shards[1]["cam_idx"]
    cov, keepc, kappa = cr.point_covariance(oracle, c.whole, c.x0, c.const_cams, c.const_pts)
    assert kappa < 1e10
    pos = {int(k): i for i, k in enumerate(keepc)}
    Cn = c.C
    with c.group() as g:
        assert g.run(lambda r, s, pr: _code(s.covariance_compute)) == [capi.OK] * 2

        def query(r, s, pr):
            P = pr.num_points
            live = [j for j in range(P) if c.lo[r] + j not in c.const_pts]
            pairs = [(("c", a), ("p", j)) for a in (1, 2, 3) for j in live] + [(("p", j), ("c", 3)) for j in live[:5]] \
                + [(("p", j), ("p", k)) for j in live[:12] for k in live[:12]] + [(("c", 0), ("p", live[0]))]
            off = lambda b: s.camera_offset(b[1]) if b[0] == "c" else s.point_offset(b[1])   # noqa: E731
            first = s.covariance_blocks([(off(a), off(b)) for a, b in pairs])
            for x, y in zip(first, s.covariance_blocks([(off(a), off(b)) for a, b in pairs])):
                np.testing.assert_array_equal(x, y)
            bad = _code(lambda: s.covariance_blocks([(s.camera_offset(4), s.point_offset(live[0]))]))   # camera 4: no rank references it
            return pairs, first, bad, _code(s.time_covariances)
        worst = 0.0
        for r, (pairs, got, bad, tcode) in enumerate(g.run(query)):
            assert bad == capi.ERR_ARG and tcode == capi.ERR_UNSUPPORTED
            for (a, b), blk in zip(pairs, got):
                if a == ("c", 0):
                    assert np.all(blk == 0.0)
                    continue
                oa, na = (6 * a[1], 6) if a[0] == "c" else (6 * Cn + 3 * (c.lo[r] + a[1]), 3)
                ob, nb = (6 * b[1], 6) if b[0] == "c" else (6 * Cn + 3 * (c.lo[r] + b[1]), 3)
                want = cov[np.ix_([pos[oa + t] for t in range(na)], [pos[ob + t] for t in range(nb)])]
                err = np.abs(blk - want).max() / np.abs(want).max()
                worst = max(worst, err)
                assert err <= TOL, (r, a, b, err)
        print("sharded 5x70x4: worst error / bar %.3e (bar %.0e)" % (worst / TOL, TOL))
