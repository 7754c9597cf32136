"""rsba_solver_evaluate / rsba_solver_set_parameters (ceres::Problem::Evaluate without the Jacobian; values changed in place) on the
GPU against the numpy reference of tests/evaluate_ref.py: cost, EVERY residual and EVERY gradient entry, in three states of one
solver — before any run, after a run, after set_parameters to a seeded perturbation of the start.

Bars (rounding bounds, computed on the CPU side only; u = 2^-53):
  residuals        rbar = 16 x max(d_r, 4 ulp(max |observation coordinate|)), d_r the largest difference between the reference
                   taken with the oracle's default build and with its -ffp-contract=off build.  The floor is there because the two
                   builds may agree exactly; 4 ulp because a residual is a difference of two pixel-sized numbers; 16 x because the
                   GPU differs from the oracle in more ways than the oracle's builds from each other (contraction, its own
                   reciprocal, device sin / cos).
  gradient entry k sum_i |J_ik| rbar + (64 + n_k) u sum_i |J_ik r_i|, n_k the number of terms: the residual error carried through,
                   then the rows' own relative error and any summation order.
  cost             rbar sum |r| + N u cost.
Every test prints its largest error / bar ratios (DESIGN §7b records them).

Shapes: the smallest at which each thing can go wrong (the table in DESIGN §7b).  The observation rows of every synthetic point
problem are shuffled with a seeded permutation, so the solver's `order` is never the identity.  P1 at schur_impl 0 and P4 (whose
duplicate selects schur_impl 0) keep the constant CAMERA only: constant point blocks need the tiled Schur kernel
(rsba_problem_set_point_constant), the solver cannot be created with them there.
"""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import evaluate_ref as er
import marker_loss_ref as mlr
import oracle_lib
from realsensecalibration_amd import capi
from realsensecalibration_amd import synthetic as syn

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
RUN_ITERATIONS = 4
P2_POINTS = 2304


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


# ------------------------------------------------------------------------------------------------ cases
def _rows(prob, keep):
    return dict(prob, cam_idx=np.ascontiguousarray(prob["cam_idx"][keep]), pt_idx=np.ascontiguousarray(prob["pt_idx"][keep]),
                obs=np.ascontiguousarray(prob["obs"].reshape(-1, 2)[keep].reshape(-1)), N=int(np.count_nonzero(keep) if keep.dtype == bool else len(keep)))


def _shuffled(prob, seed):
    return _rows(prob, np.random.default_rng(seed).permutation(prob["N"]))


def _p1():
    prob = syn.make_problem(5, 70, 4, seed=41)
    prob = _rows(prob, (prob["cam_idx"] != 4) & (prob["pt_idx"] != 17))   # camera 4 and point 17 unreferenced
    if prob["N"] % 2 == 0:
        prob = _rows(prob, np.arange(1, prob["N"]))
    assert prob["N"] % 2 == 1 and prob["N"] > 64
    return prob


def _subsampled(C, P, seed, views, outlier_frac):
    """make_problem with every camera seeing every point, then point j keeps views[j] cameras drawn with the seed."""
    prob = syn.make_problem(C, P, C, seed=seed, outlier_frac=outlier_frac)
    rng = np.random.default_rng([seed, 7])
    keep = np.zeros(prob["N"], bool)
    for j in range(P):   # (rows are point-major, C per point, cameras ascending)
        keep[j * C + rng.permutation(C)[:views[j]]] = True
    return _rows(prob, keep)


def _case(name):
    if name in _CASES:
        return _CASES[name]
    c = SimpleNamespace(name=name, kind="points", model=capi.MODEL_POINTS, variant=0, loss="none", a=0.0, const_cams=(), const_pts=(),
                        const_blocks=())
    if name in ("P1", "P1_atomic"):
        c.prob = _shuffled(_p1(), 1)
        c.const_cams, c.const_pts = (0,), ((3, 69) if name == "P1" else ())
        c.schur_impl = 1 if name == "P1" else 0
    elif name == "P2":
        # (the balanced point order needs 4 chunks of 512 points: BalancedPointOrder keeps the file order below 2048)
        rng = np.random.default_rng(52)
        views = 2 + np.floor(38.999 * rng.random(P2_POINTS) ** 6).astype(int)   # 2 .. 40, uneven
        views[:2] = (2, 40)
        c.prob = _shuffled(_subsampled(40, P2_POINTS, 42, views, 0.05), 2)
        c.loss, c.a, c.schur_impl = "huber", 1.5, 1
        c.const_cams, c.const_pts = (0,), (0,)   # the gauge: the covariance of the non-interference test exists
    elif name == "P3":
        views = np.where(np.arange(600) % 10 == 0, 72, 3)   # every 10th point: more views than a wavefront has lanes
        c.prob = _shuffled(_subsampled(72, 600, 43, views, 0.05), 3)
        c.loss, c.a, c.schur_impl = "cauchy", 2.0, 1
    elif name == "P4":
        prob = _p1()
        dup = 5
        prob = dict(prob, cam_idx=np.append(prob["cam_idx"], prob["cam_idx"][dup]).astype(np.int32),
                    pt_idx=np.append(prob["pt_idx"], prob["pt_idx"][dup]).astype(np.int32),
                    obs=np.append(prob["obs"], prob["obs"][2 * dup:2 * dup + 2] + (0.75, -0.5)), N=prob["N"] + 1)
        c.dup = (dup, prob["N"] - 1)
        perm = np.random.default_rng(4).permutation(prob["N"])
        c.dup = tuple(int(np.nonzero(perm == d)[0][0]) for d in c.dup)   # where the two rows went
        c.prob = _rows(prob, perm)
        c.const_cams, c.schur_impl = (0,), 1   # (asked for the tiled kernel: the duplicate selects the atomic one)
    elif name in ("M1_dense", "M1_elim"):
        c.kind, c.model, c.prob = "marker", capi.MODEL_MARKER_CHAIN, mlr.hongo()
        c.schur_impl = 0 if name == "M1_dense" else 2
    elif name == "M2":
        c.kind, c.model, c.variant, c.prob = "marker", capi.MODEL_MARKER_CHAIN_TEST2, 1, mlr.test2()
        assert np.all(c.prob["params"].reshape(-1, 6)[c.prob["C"] + c.prob["T"]:, :3] == 0.0)   # marker rvecs 0: the small-angle branch
        c.schur_impl, c.const_blocks = 0, (c.prob["C"] + c.prob["T"] + c.prob["M"] - 1,)
    elif name in ("M3_elim", "M3_dense"):
        prob = mlr.displace_corners(syn.make_marker_chain(3, 70, 5, seed=44), 0.05, 12.0, seed=5)
        c.kind, c.model, c.prob = "marker", capi.MODEL_MARKER_CHAIN, prob
        c.loss, c.a = "huber", 2.0
        c.schur_impl = 2 if name == "M3_elim" else 0
        c.const_blocks = (prob["C"] + 7, prob["C"] + prob["T"] + 2)   # one time block, one marker block
    else:
        raise KeyError(name)
    if c.kind == "marker":
        c.prob = dict(c.prob, obs=np.ascontiguousarray(c.prob["obs"], float).reshape(-1, 8), intr=np.ascontiguousarray(c.prob["intr"], float))
    c.x0 = np.array(c.prob["params"], float)
    rng = np.random.default_rng([99, len(c.x0)])
    c.x1 = c.x0 + 1e-3 * rng.standard_normal(len(c.x0))   # the seeded perturbation of the start
    _CASES[name] = c
    return c


_CASES = {}


def _solver(c, params=None, schur_impl=None, **kw):
    prob = c.prob if params is None else dict(c.prob, params=np.ascontiguousarray(params, float))
    if c.kind == "points":
        pr = capi.Problem.points(prob)
        for cam in c.const_cams:
            pr.set_camera_constant(cam)
        for p in c.const_pts:
            pr.set_point_constant(p)
    else:
        pr = capi.Problem.marker_chain(prob, c.model)
        for b in c.const_blocks:
            pr.set_parameter_block_constant(6 * b)
    kw.setdefault("max_num_iterations", RUN_ITERATIONS)
    o = capi.default_options(schur_impl=c.schur_impl if schur_impl is None else schur_impl, huber_delta=c.a if c.loss != "none" else 0.0,
                             loss_type=1 if c.loss == "cauchy" else 0, **kw)
    return pr, capi.Solver(pr, o)


# ------------------------------------------------------------------------------------------------ reference and bars
_REF = {}


def _reference(c, x, apply_loss):
    """-> (reference, residual bar); the oracle's rows are taken once per (problem, state) and shared."""
    key = (id(c.prob), x.tobytes())
    if key not in _REF:
        rows = er.point_rows if c.kind == "points" else (lambda o, p, v: er.marker_rows(o, p, v, c.variant))
        _REF[key] = (rows(oracle_lib.load(), c.prob, x), rows(oracle_lib.load_nocontract(), c.prob, x))
    const = er.point_constant_offsets(c.prob, c.const_cams, c.const_pts) if c.kind == "points" else [(6 * b, 6) for b in c.const_blocks]
    ref, alt = (er.finish(rw, len(x), const, c.loss, c.a, apply_loss) for rw in _REF[key])
    d_r = np.abs(ref.residuals - alt.residuals).max() if len(ref.residuals) else 0.0
    rbar = 16.0 * max(d_r, 4.0 * np.spacing(np.abs(c.prob["obs"]).max()))
    return ref, rbar


def _bars(c, ref, rbar):
    gbar = ref.abs_J * rbar + (64 + ref.n_terms) * U * ref.abs_Jr
    cbar = rbar * np.abs(ref.residuals).sum() + c.prob["N"] * U * ref.cost
    return gbar, cbar


def _check_state(c, s, x, label):
    """cost, every residual and every gradient entry at x against the reference; masked slots; repeatability; partial outputs."""
    for apply_loss in ((True, False) if c.loss != "none" else (True,)):
        ref, rbar = _reference(c, x, apply_loss)
        gbar, cbar = _bars(c, ref, rbar)
        cost, r, g = s.evaluate(apply_loss_function=apply_loss)
        cost2, r2, g2 = s.evaluate(apply_loss_function=apply_loss)
        assert cost == cost2
        np.testing.assert_array_equal(r, r2)
        np.testing.assert_array_equal(g, g2)
        assert r.shape == (s.num_residuals,) and s.num_residuals == (2 if c.kind == "points" else 8) * c.prob["N"]
        q_r = np.abs(r - ref.residuals).max() / rbar
        live = ref.live
        q_g = (np.abs(g - ref.gradient)[live] / gbar[live]).max()
        q_c = abs(cost - ref.cost) / cbar
        print("evaluate %s %s apply_loss=%d: error / bar  residual %.3f  gradient %.3f  cost %.3f   (rbar %.2e)" % (c.name, label, apply_loss, q_r, q_g, q_c, rbar))
        assert q_r <= 1.0 and q_g <= 1.0 and q_c <= 1.0, (q_r, q_g, q_c)
        assert np.all(g[~live] == 0.0) and np.all(ref.gradient[~live] == 0.0)
        # residual-only and gradient-only calls answer the same question
        cost3, r3, g3 = s.evaluate(gradient=False, apply_loss_function=apply_loss)
        assert g3 is None and np.abs(r3 - ref.residuals).max() <= rbar and abs(cost3 - ref.cost) <= cbar
        cost4, r4, g4 = s.evaluate(residuals=False, apply_loss_function=apply_loss)
        assert r4 is None and cost4 == cost
        np.testing.assert_array_equal(g4, g)
    return ref


def _masked_slots(c):
    if c.kind == "points":
        C = c.prob["C"]
        cams = set(c.const_cams) | (set(range(C)) - set(int(v) for v in c.prob["cam_idx"]))
        pts = set(c.const_pts) | (set(range(c.prob["P"])) - set(int(v) for v in c.prob["pt_idx"]))
        return [k for cam in cams for k in range(6 * cam, 6 * cam + 6)] + [k for p in pts for k in range(6 * C + 3 * p, 6 * C + 3 * p + 3)]
    C, T = c.prob["C"], c.prob["T"]
    blocks = set(c.const_blocks) | {0} | ({C + T} if c.variant == 0 else set())
    return [k for b in blocks for k in range(6 * b, 6 * b + 6)]


@pytest.mark.parametrize("name", ["P1", "P1_atomic", "P2", "P3", "P4", "M1_dense", "M1_elim", "M2", "M3_elim"])
def test_against_reference_in_three_states(name):
    c = _case(name)
    pr, s = _solver(c)
    if c.kind == "marker":
        assert s.eliminates_times() == (1 if c.schur_impl == 2 else 0)
    elif name in ("P1_atomic", "P4"):
        assert s.schedule_info()["schur_impl"] == 0
    else:
        assert s.schedule_info()["schur_impl"] == 1
    masked = _masked_slots(c)
    if name == "P1":
        C = c.prob["C"]
        assert sorted(masked) == sorted(list(range(0, 6)) + list(range(24, 30)) + [6 * C + 3 * p + e for p in (3, 17, 69) for e in range(3)])
    # --- before any run: the uploaded start
    ref = _check_state(c, s, c.x0, "start")
    assert set(masked) <= set(np.nonzero(~ref.live)[0])
    if c.kind == "points":
        assert sorted(np.nonzero(~ref.live)[0]) == sorted(masked)
    if name == "P4":
        # both rows of the duplicated (camera, point) pair have their own residuals: they differ by the detections' difference
        _, r, _ = s.evaluate(gradient=False)
        a, b = c.dup
        _, rbar = _reference(c, c.x0, True)
        obs = c.prob["obs"].reshape(-1, 2)
        assert np.abs((r[2 * b:2 * b + 2] - r[2 * a:2 * a + 2]) - (obs[a] - obs[b])).max() <= 2 * rbar and np.abs(obs[a] - obs[b]).min() >= 0.5
    # --- after a run: the solution
    s.run()
    s.download()
    x = pr.params.copy()
    assert not np.array_equal(x, c.x0)
    ref = _check_state(c, s, x, "solved")
    # consistency with the solve: its final cost, and the gradient norm of its last iteration
    _, rbar = _reference(c, x, True)
    gbar, cbar = _bars(c, ref, rbar)
    cost, _, g = s.evaluate(residuals=False)
    log = s.iterations()
    print("final cost %.15e evaluate %.15e (bar %.2e); gradient_max_norm %.15e evaluate %.15e (bar %.2e)" %
          (s.final_costs()[0], cost, cbar, log[-1, 3], np.abs(g).max(), gbar[ref.live].max()))
    assert abs(cost - s.final_costs()[0]) <= cbar
    assert abs(np.abs(g).max() - log[-1, 3]) <= gbar[ref.live].max()
    # --- after set_parameters: every block takes the new values, constant and unreferenced ones too
    s.set_parameters(c.x1)
    np.testing.assert_array_equal(pr.params, x)   # the problem's own array is not touched ...
    s.download()
    np.testing.assert_array_equal(pr.params, c.x1)   # ... until the download, which returns x1 exactly (point by point: pt_perm)
    _check_state(c, s, c.x1, "set")
    np.testing.assert_array_equal(s.iterations(), log)   # the iteration log stays until the next run
    s.close()
    pr.close()


def test_p2_runs_the_balanced_point_order():
    """P2 is the case for a solver whose internal point order is not the problem's (pt_perm: the gradient's and set_parameters'
    scatter, the camera index's device positions).  A child process creates P2's solver with RSBA_DEBUG set and must report the
    balanced order; the three-state, re-solve and non-interference tests then run on that shape."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import test_gpu_evaluate as t; c = t._case('P2'); pr, s = t._solver(c); print(s.schedule_info()); s.close(); pr.close()"
    env = dict(os.environ, RSBA_DEBUG="1", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], cwd=here, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rsba: point order balanced" in r.stderr and "rsba: point order kept" not in r.stderr, r.stderr[-4000:]


def _run_log(s, pr):
    s.run()
    s.download()
    return s.iterations()[:, 1:], pr.params.copy()


@pytest.mark.parametrize("name", ["P2", "M1_dense", "M1_elim"])
def test_non_interference(name):
    """run -> evaluate -> run gives the iteration log and the parameters of run -> run, bit for bit; evaluate after
    covariance_compute leaves the covariance blocks unchanged."""
    c = _case(name)
    runs = []
    for with_eval in (True, False):
        pr, s = _solver(c)
        _run_log(s, pr)
        if with_eval:
            s.evaluate()
            s.evaluate(gradient=False, apply_loss_function=False)
        runs.append(_run_log(s, pr))
        if with_eval:
            s.covariance_compute()
            a = 6 * (1 if c.kind == "points" else 2)
            before = s.covariance_block(a, a + 6)
            pts = s.point_covariances() if c.kind == "points" else None
            s.evaluate()
            np.testing.assert_array_equal(s.covariance_block(a, a + 6), before)
            if pts is not None:
                np.testing.assert_array_equal(s.point_covariances(), pts)
        s.close()
        pr.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("name", ["P2", "M1_dense", "M1_elim"])
def test_resolve_from_set_parameters_equals_a_new_solver(name):
    """A: created at x0, set_parameters(x1), run.  B: created from a problem holding x1, run.  The plan depends on the indices alone
    and the solve is bitwise reproducible: logs (cost, gradient norm, step norm, radius, accept flags) and parameters are identical."""
    c = _case(name)
    pa, sa = _solver(c)
    sa.run()   # (a run in between: what it leaves behind must not matter either)
    sa.set_parameters(c.x1)
    la, xa = _run_log(sa, pa)
    pb, sb = _solver(c, params=c.x1)
    lb, xb = _run_log(sb, pb)
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(xa, xb)
    assert len(la) > 1 and sa.schedule_info() == sb.schedule_info()
    for h in (sa, sb, pa, pb):
        h.close()


@pytest.mark.parametrize("dense,elim", [("M1_dense", "M1_elim"), ("M3_dense", "M3_elim")])
def test_marker_paths_return_identical_bits(dense, elim):
    """One kernel family for both paths: the dense-path and the time-eliminating solver agree bit for bit before any run."""
    out = []
    for name in (dense, elim):
        c = _case(name)
        pr, s = _solver(c)
        assert s.eliminates_times() == (1 if name == elim else 0)
        out.append(s.evaluate())
        out.append(s.evaluate(apply_loss_function=False))
        s.close()
        pr.close()
    for a, b in ((out[0], out[2]), (out[1], out[3])):
        assert a[0] == b[0]
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[2], b[2])


def test_errors():
    import ctypes as C
    c = _case("P1")
    pr, s = _solver(c)
    lib = capi.load()
    assert lib.rsba_solver_evaluate(s.h, None, None, None, None) == capi.OK   # all outputs NULL: nothing to do
    cost = C.c_double()
    assert lib.rsba_solver_evaluate(s.h, None, C.byref(cost), None, None) == capi.OK   # NULL options: the defaults
    before = s.evaluate()
    assert cost.value == before[0]
    s.covariance_compute()
    bad = c.x1.copy()
    bad[len(bad) // 2] = np.nan
    with pytest.raises(capi.RsbaError) as e:
        s.set_parameters(bad)
    assert e.value.code == capi.ERR_ARG
    bad[len(bad) // 2] = np.inf
    with pytest.raises(capi.RsbaError) as e:
        s.set_parameters(bad)
    assert e.value.code == capi.ERR_ARG
    after = s.evaluate()   # a refused call changes nothing: the same bits, and the covariance is still there
    assert before[0] == after[0]
    np.testing.assert_array_equal(before[1], after[1])
    np.testing.assert_array_equal(before[2], after[2])
    s.covariance_block(6, 6)
    assert lib.rsba_solver_set_parameters(s.h, None) == capi.ERR_ARG
    s.set_parameters(c.x1)   # an accepted call drops the covariance of the old values
    with pytest.raises(capi.RsbaError) as e:
        s.covariance_block(6, 6)
    assert e.value.code == capi.ERR_ARG
    s.close()
    pr.close()
