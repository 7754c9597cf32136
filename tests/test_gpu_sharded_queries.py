"""rsba_solver_evaluate, rsba_solver_set_parameters and rsba_solver_covariance_* on a SHARDED solver (point model): a loopback group
of N ranks on the one GPU (capi.ShardedLoopbackGroup: one host thread per rank, the live solvers kept between calls), checked
against the numpy references on the WHOLE problem — tests/evaluate_ref.py and tests/covariance_ref.py, as the single-rank tests
(tests/test_gpu_evaluate.py, tests/test_gpu_covariance.py).  Shards come from syn.make_problem(..., point_range=rd.shard_range(...)),
the whole problem from the same call without point_range; every case asserts that the whole problem's rows are the shards' rows in
rank order.

Bars, none of them new (u = 2^-53):
  residuals        rbar = 16 x max(d_r, 4 ulp(max |observation coordinate|)), d_r the largest difference between the reference taken
                   with the oracle's default build and with its -ffp-contract=off build (test_gpu_evaluate.py's docstring).
  gradient entry k sum_i |J_ik| rbar + (64 + n_k) u sum_i |J_ik r_i|, n_k the number of terms.
  cost             rbar sum |r| + N u cost.
  covariance       relative block error <= 1e-8 of the reference block's largest entry, with kappa(J'J) < 1e10 (test_gpu_covariance.py).
n_k is NOT extended by the number of ranks: no case needed it.  Every case prints its worst error / bar ratios.

What the group must also hold, bit for bit: the concatenated residuals are the single-rank solver's on the whole problem at the same
values (the same per-observation function); cost and camera slots are the same on every rank; two consecutive calls agree; camera x
camera covariance blocks are the same on every rank and block(b, a) == block(a, b)'.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import covariance_ref as cr
import evaluate_ref as er
import oracle_lib
from realsensecalibration_amd import capi
from realsensecalibration_amd import distributed as rd
from realsensecalibration_amd import synthetic as syn

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
TOL = 1e-8
LOSSES = {"none": dict(), "huber": dict(huber_delta=1.5), "cauchy": dict(huber_delta=2.0, loss_type=1)}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


# ------------------------------------------------------------------------------------------------ problems
def _rows(prob, keep):
    return dict(prob, cam_idx=np.ascontiguousarray(prob["cam_idx"][keep]), pt_idx=np.ascontiguousarray(prob["pt_idx"][keep]),
                obs=np.ascontiguousarray(prob["obs"].reshape(-1, 2)[keep].reshape(-1)), N=int(np.count_nonzero(keep)))


def _split(C, P, k, seed, world, outlier_frac=0.0, keep=None):
    """-> (whole, shards, point offsets).  keep(prob, r) -> row mask of shard r (r None: not used); the whole problem is then the
    shards' kept rows in rank order."""
    shards = [syn.make_problem(C, P, k, seed, point_range=rd.shard_range(P, r, world), outlier_frac=outlier_frac) for r in range(world)]
    whole = syn.make_problem(C, P, k, seed, outlier_frac=outlier_frac)
    lo = [rd.shard_range(P, r, world)[0] for r in range(world)]
    if keep is not None:
        masks = [keep(sh, r, lo[r]) for r, sh in enumerate(shards)]
        shards = [_rows(sh, m) for sh, m in zip(shards, masks)]
        whole = _rows(whole, np.concatenate(masks))
    # the whole problem's observation rows are the shards' rows concatenated in rank order
    np.testing.assert_array_equal(whole["cam_idx"], np.concatenate([sh["cam_idx"] for sh in shards]))
    np.testing.assert_array_equal(whole["pt_idx"], np.concatenate([sh["pt_idx"] + o for sh, o in zip(shards, lo)]))
    np.testing.assert_array_equal(whole["obs"], np.concatenate([sh["obs"] for sh in shards]))
    np.testing.assert_array_equal(whole["params"], _stitch(C, [sh["params"] for sh in shards]))
    assert whole["N"] == sum(sh["N"] for sh in shards) and whole["P"] == sum(sh["P"] for sh in shards)
    return whole, shards, lo


def _stitch(C, parts):
    """Per-rank parameter-layout vectors -> the whole problem's: rank 0's camera slots, then every rank's point slots."""
    return np.concatenate([parts[0][:6 * C]] + [p[6 * C:] for p in parts])


def _slices(C, shards, x):
    """The whole problem's vector -> every rank's."""
    out, at = [], 6 * C
    for sh in shards:
        out.append(np.concatenate([x[:6 * C], x[at:at + 3 * sh["P"]]]))
        at += 3 * sh["P"]
    return out


class Case:
    """Whole problem + shards + constant blocks (whole-problem point indices) + options."""

    def __init__(self, C, P, k, seed, world, loss="none", const_cams=(0,), const_pts=(0,), outlier_frac=0.0, keep=None, **optkw):
        self.C, self.world, self.loss = C, world, loss
        self.whole, self.shards, self.lo = _split(C, P, k, seed, world, outlier_frac, keep)
        self.const_cams, self.const_pts = tuple(const_cams), tuple(const_pts)
        self.optkw = dict(schur_impl=1, **LOSSES[loss], **optkw)
        self.x0 = np.array(self.whole["params"], float)
        self.x1 = self.x0 + 1e-3 * np.random.default_rng([99, len(self.x0)]).standard_normal(len(self.x0))

    def local_const_pts(self, r):
        hi = self.lo[r] + self.shards[r]["P"]
        return [p - self.lo[r] for p in self.const_pts if self.lo[r] <= p < hi]

    def prepare(self, r, pr):
        for c in self.const_cams:
            pr.set_camera_constant(c)
        for p in self.local_const_pts(r):
            pr.set_point_constant(p)

    def group(self, shards=None, **optkw):
        return capi.ShardedLoopbackGroup(shards or self.shards, dict(self.optkw, **optkw), self.prepare)

    def single(self, **optkw):
        """The whole problem on a solver without a communicator."""
        pr = capi.Problem.points(self.whole)
        for c in self.const_cams:
            pr.set_camera_constant(c)
        for p in self.const_pts:
            pr.set_point_constant(p)
        return pr, capi.Solver(pr, capi.default_options(**dict(self.optkw, **optkw)))

    def shards_at(self, x):
        return [dict(sh, params=v) for sh, v in zip(self.shards, _slices(self.C, self.shards, x))]


# ------------------------------------------------------------------------------------------------ references and bars
_ROWS = {}


def _reference(c, x, apply_loss):
    """-> (reference of the whole problem at x, residual bar, gradient bars, cost bar): test_gpu_evaluate.py's formulas."""
    key = (id(c.whole), x.tobytes())
    if key not in _ROWS:
        _ROWS[key] = (er.point_rows(oracle_lib.load(), c.whole, x), er.point_rows(oracle_lib.load_nocontract(), c.whole, x))
    const = er.point_constant_offsets(c.whole, c.const_cams, c.const_pts)
    a = LOSSES[c.loss].get("huber_delta", 0.0)
    ref, alt = (er.finish(rw, len(x), const, c.loss, a, apply_loss) for rw in _ROWS[key])
    d_r = np.abs(ref.residuals - alt.residuals).max()
    rbar = 16.0 * max(d_r, 4.0 * np.spacing(np.abs(c.whole["obs"]).max()))
    gbar = ref.abs_J * rbar + (64 + ref.n_terms) * U * ref.abs_Jr
    cbar = rbar * np.abs(ref.residuals).sum() + c.whole["N"] * U * ref.cost
    return ref, rbar, gbar, cbar


def _evaluate_twice(apply_loss):
    def fn(r, s, pr):
        a = s.evaluate(apply_loss_function=apply_loss)
        b = s.evaluate(apply_loss_function=apply_loss)
        assert a[0] == b[0]   # two consecutive calls: identical bits on this rank
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[2], b[2])
        return a
    return fn


def _check_evaluate(c, g, x, label, single=None):
    """The group's evaluate at the whole-problem values x against the reference (and, bit for bit, against `single`)."""
    C = c.C
    for apply_loss in ((True, False) if c.loss != "none" else (True,)):
        ref, rbar, gbar, cbar = _reference(c, x, apply_loss)
        ranks = g.run(_evaluate_twice(apply_loss))
        for cost, _, grad in ranks[1:]:   # cost and camera slots: the same bits on every rank
            assert cost == ranks[0][0]
            np.testing.assert_array_equal(grad[:6 * C], ranks[0][2][:6 * C])
        res = np.concatenate([rk[1] for rk in ranks])
        grad = _stitch(C, [rk[2] for rk in ranks])
        if single is not None:
            single.set_parameters(x)
            np.testing.assert_array_equal(res, single.evaluate(gradient=False, apply_loss_function=apply_loss)[1])
        live = ref.live
        q_r = np.abs(res - ref.residuals).max() / rbar
        q_g = (np.abs(grad - ref.gradient)[live] / gbar[live]).max()
        q_c = abs(ranks[0][0] - ref.cost) / cbar
        print("sharded evaluate %s apply_loss=%d: error / bar  residual %.3f  gradient %.3f  cost %.3f   (rbar %.2e)" % (label, apply_loss, q_r, q_g, q_c, rbar))
        assert q_r <= 1.0 and q_g <= 1.0 and q_c <= 1.0, (q_r, q_g, q_c)
        assert np.all(grad[~live] == 0.0) and np.all(ref.gradient[~live] == 0.0)
        # the partial requests: residuals alone (local, no collective) and cost + gradient
        part = g.run(lambda r, s, pr: (s.evaluate(residuals=False, apply_loss_function=apply_loss), _residuals_only(s, apply_loss)))
        for (full, ronly), rk in zip(part, ranks):
            assert full[0] == rk[0]
            np.testing.assert_array_equal(full[2], rk[2])
            np.testing.assert_array_equal(ronly, rk[1])
    return ranks


def _residuals_only(s, apply_loss=True):
    import ctypes as C
    o = capi.EvaluateOptions(apply_loss_function=1 if apply_loss else 0)
    r = np.zeros(s.num_residuals)
    assert capi.load().rsba_solver_evaluate(s.h, C.byref(o), None, r.ctypes.data_as(C.c_void_p), None) == capi.OK
    return r


def _run(r, s, pr):
    s.run()
    s.download()
    return s.iterations()[:, 1:], pr.params.copy()


def _code(call):
    try:
        call()
        return capi.OK
    except capi.RsbaError as e:
        return e.code


def _check_covariance(c, g, x, label, cams=None):
    """covariance_compute on every rank at the whole-problem values x; every camera x camera block and every rank's point
    marginals against covariance_ref on the whole problem."""
    C = c.C
    lossd = LOSSES[c.loss]
    cov, keep, kappa = cr.point_covariance(oracle_lib.load(), c.whole, x, c.const_cams, c.const_pts, lossd.get("huber_delta", 0.0), c.loss == "cauchy")
    print("kappa(J'J) = %.3e" % kappa)
    assert kappa < 1e10
    assert g.run(lambda r, s, pr: _code(s.covariance_compute)) == [capi.OK] * c.world
    cams = list(range(C)) if cams is None else cams
    blocks = g.run(lambda r, s, pr: {(a, b): s.covariance_block(6 * a, 6 * b) for a in cams for b in cams})
    worst = 0.0
    pos = {int(k): i for i, k in enumerate(keep)}
    for a in cams:
        for b in cams:
            got = blocks[0][a, b]
            for rk in blocks[1:]:
                np.testing.assert_array_equal(rk[a, b], got)   # the same bits on every rank
            np.testing.assert_array_equal(blocks[0][b, a], got.T)   # block(b, a) == block(a, b)'
            if a in c.const_cams or b in c.const_cams:
                assert np.all(got == 0.0)
                continue
            ref = cov[np.ix_([pos[6 * a + t] for t in range(6)], [pos[6 * b + t] for t in range(6)])]   # (= cr.block)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            assert err <= TOL, (a, b, err)
    pcs = g.run(lambda r, s, pr: (s.point_covariances(), s.covariance_block(s.point_offset(pr.num_points - 1), s.point_offset(pr.num_points - 1))))
    for r, (pc, last) in enumerate(pcs):
        assert pc.shape == (c.shards[r]["P"], 3, 3)
        np.testing.assert_array_equal(last, pc[-1])   # block(p, p), by the owning rank's offsets, is the same marginal
        for j in range(len(pc)):
            p = c.lo[r] + j
            if p in c.const_pts:
                assert np.all(pc[j] == 0.0)
                continue
            ia = [pos[6 * C + 3 * p + t] for t in range(3)]
            ref = cov[np.ix_(ia, ia)]
            err = np.abs(pc[j] - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            assert err <= TOL, (r, j, err)
    print("sharded covariance %s: worst relative block error %.3e (error / bar %.3f)" % (label, worst, worst / TOL))
    return blocks


# ------------------------------------------------------------------------------------------------ S1: evaluate
def test_s1_evaluate_in_three_states():
    """6 cameras x 40 points x 4 views in 2 shards, camera 0 constant, a constant point on each rank, Huber 1.5: before a run,
    after a 4-iteration run, after set_parameters to a seeded perturbation; with and without the loss."""
    c = Case(6, 40, 4, 31, 2, loss="huber", const_pts=(0, 23), outlier_frac=0.05, max_num_iterations=4)
    assert c.local_const_pts(0) == [0] and c.local_const_pts(1) == [3]
    ps, single = c.single()
    with c.group() as g:
        _check_evaluate(c, g, c.x0, "S1 start", single)
        xs = _stitch(c.C, [x for _, x in g.run(_run)])
        assert not np.array_equal(xs, c.x0)
        _check_evaluate(c, g, xs, "S1 solved", single)
        x1 = _slices(c.C, c.shards, c.x1)
        assert g.run(lambda r, s, pr: _code(lambda: s.set_parameters(x1[r]))) == [capi.OK] * 2
        for r, x in enumerate(g.run(lambda r, s, pr: (s.download(), pr.params.copy())[1])):
            np.testing.assert_array_equal(x, x1[r])
        _check_evaluate(c, g, c.x1, "S1 set", single)
    single.close()
    ps.close()


# ------------------------------------------------------------------------------------------------ S2: a camera of one shard, of none
def test_s2_camera_seen_by_one_shard_only_and_by_none():
    """5 cameras x 70 points x 4 views in 2 shards; camera 3's rows removed from rank 0's shard only, camera 4's from both.  Camera
    3's slots on rank 0 carry rank 1's sum (the zero mask comes from the summed flags), camera 4's are exactly 0.0 everywhere."""
    keep = lambda sh, r, lo: (sh["cam_idx"] != 4) & ((sh["cam_idx"] != 3) | (r != 0))   # noqa: E731
    c = Case(5, 70, 4, 32, 2, keep=keep)
    assert 3 not in c.shards[0]["cam_idx"] and 3 in c.shards[1]["cam_idx"] and 4 not in c.whole["cam_idx"]
    with c.group() as g:
        ranks = _check_evaluate(c, g, c.x0, "S2 start")
        ref, rbar, gbar, _ = _reference(c, c.x0, True)
        g0, g1 = ranks[0][2], ranks[1][2]
        np.testing.assert_array_equal(g0[18:24], g1[18:24])
        assert np.all(g0[18:24] != 0.0) and np.all(np.abs(g0[18:24] - ref.gradient[18:24]) <= gbar[18:24])
        assert np.all(g0[24:30] == 0.0) and np.all(g1[24:30] == 0.0) and not np.any(np.signbit(g0[24:30]))
        _check_covariance(c, g, c.x0, "S2 start", cams=[0, 1, 2, 3])
        codes = g.run(lambda r, s, pr: (_code(lambda: s.covariance_block(24, 6)), _code(lambda: s.covariance_block(6, 24)),
                                        _code(lambda: s.covariance_block(18, 18))))
        assert codes == [(capi.ERR_ARG, capi.ERR_ARG, capi.OK)] * 2   # camera 4: no rank references it; camera 3: available on rank 0 too


# ------------------------------------------------------------------------------------------------ S3: covariance
@pytest.mark.parametrize("loss", ["none", "cauchy"])
def test_s3_covariance_after_a_solve(loss):
    """13 cameras x 700 points x 7 views in 3 shards (uneven: 233, 233, 234), gauge fixed by camera 0 and point 0."""
    c = Case(13, 700, 7, 33, 3, loss=loss, outlier_frac=0.05 if loss != "none" else 0.0, max_num_iterations=20)
    assert len({sh["P"] for sh in c.shards}) == 2
    with c.group() as g:
        first = g.run(_run)
        xs = _stitch(c.C, [x for _, x in first])
        _check_covariance(c, g, xs, "S3 %s" % loss)
        # run -> covariance -> evaluate -> run against run -> run
        g.run(lambda r, s, pr: s.evaluate())
        second = g.run(_run)
    with c.group() as g:
        g.run(_run)
        plain = g.run(_run)
    for (la, xa), (lb, xb) in zip(second, plain):
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(xa, xb)


# ------------------------------------------------------------------------------------------------ S4: > 64 views, > 64 cameras
def test_s4_more_than_one_wavefront_of_views_and_more_than_64_cameras():
    """72 cameras x 600 points in 2 shards; every 10th point sees all 72 cameras, the rest 3 (test_gpu_evaluate.py's P3)."""
    C, P = 72, 600
    views = np.where(np.arange(P) % 10 == 0, 72, 3)
    rng = np.random.default_rng([43, 7])
    mask = np.zeros(P * C, bool)
    for j in range(P):   # (rows are point-major, C per point, cameras ascending)
        mask[j * C + rng.permutation(C)[:views[j]]] = True
    keep = lambda sh, r, lo: mask[lo * C:(lo + sh["P"]) * C]   # noqa: E731
    c = Case(C, P, C, 43, 2, loss="cauchy", outlier_frac=0.05, keep=keep, max_num_iterations=4)
    assert c.whole["N"] == 60 * 72 + 540 * 3
    with c.group() as g:
        xs = _stitch(C, [x for _, x in g.run(_run)])
        _check_evaluate(c, g, xs, "S4 solved")
        _check_covariance(c, g, xs, "S4 solved")


# ------------------------------------------------------------------------------------------------ S5: re-solve
def test_s5_resolve_from_set_parameters_equals_a_group_created_there():
    c = Case(6, 40, 4, 35, 2, loss="huber", outlier_frac=0.05, max_num_iterations=6)
    x1 = _slices(c.C, c.shards, c.x1)
    with c.group() as g:
        before = g.run(lambda r, s, pr: s.evaluate())
        # cameras that differ in ONE bit on ONE rank: refused by every rank, nothing changed on any
        odd = x1[1].copy()
        odd[7] = np.nextafter(odd[7], np.inf)
        codes = g.run(lambda r, s, pr: _code(lambda: s.set_parameters(odd if r == 1 else x1[r])))
        assert codes == [capi.ERR_ARG] * 2
        # a non-finite value on one rank alone: the same
        nan = x1[0].copy()
        nan[-1] = np.nan
        codes = g.run(lambda r, s, pr: _code(lambda: s.set_parameters(nan if r == 0 else x1[r])))
        assert codes == [capi.ERR_ARG] * 2
        for a, b in zip(before, g.run(lambda r, s, pr: s.evaluate())):
            assert a[0] == b[0]
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(a[2], b[2])
        g.run(_run)   # (a run in between: what it leaves behind must not matter either)
        assert g.run(lambda r, s, pr: _code(lambda: s.set_parameters(x1[r]))) == [capi.OK] * 2
        set_there = g.run(_run)
    with c.group(c.shards_at(c.x1)) as g:
        created_there = g.run(_run)
    for (la, xa), (lb, xb) in zip(set_there, created_there):
        assert len(la) > 1
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(xa, xb)


# ------------------------------------------------------------------------------------------------ S6: agreement and degeneracy
def test_s6_disagreement_is_refused_by_every_rank():
    c = Case(6, 40, 4, 36, 2, max_num_iterations=6)
    with c.group() as g:
        codes = g.run(lambda r, s, pr: _code(lambda: s.evaluate(residuals=False, gradient=(r == 0))))
        assert codes == [capi.ERR_ARG] * 2
        # different entry points, different options: the same
        codes = g.run(lambda r, s, pr: _code(s.covariance_compute if r == 0 else lambda: s.evaluate()))
        assert codes == [capi.ERR_ARG] * 2
        codes = g.run(lambda r, s, pr: _code(lambda: s.covariance_compute(min_reciprocal_condition_number=1e-14 if r == 0 else 1e-13)))
        assert codes == [capi.ERR_ARG] * 2
        codes = g.run(lambda r, s, pr: _code(lambda: s.covariance_compute(min_reciprocal_condition_number=-1.0 if r == 1 else 1e-14)))
        assert codes == [capi.ERR_ARG] * 2
        # ... and the following matching calls succeed
        ranks = g.run(lambda r, s, pr: s.evaluate())
        assert ranks[0][0] == ranks[1][0] and ranks[0][0] > 0.0
        assert g.run(lambda r, s, pr: _code(s.covariance_compute)) == [capi.OK] * 2


def test_s6_all_free_problem_is_rank_deficient_on_every_rank_then_run_unchanged():
    c = Case(6, 40, 4, 37, 2, const_cams=(), const_pts=(), max_num_iterations=6)
    with c.group() as g:
        assert g.run(lambda r, s, pr: _code(s.covariance_compute)) == [capi.ERR_RANK_DEFICIENT] * 2
        assert g.run(lambda r, s, pr: _code(lambda: s.covariance_block(0, 0))) == [capi.ERR_ARG] * 2   # no result after a failed compute
        after = g.run(_run)
    with c.group() as g:
        plain = g.run(_run)
    for (la, xa), (lb, xb) in zip(after, plain):
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(xa, xb)


def test_a_rank_that_raises_releases_the_others():
    """The helper's own promise: a rank whose function raises aborts the communicator, the rank waiting in the collective leaves
    with RSBA_ERR_COMM at once, and the caller sees the first failure."""
    c = Case(6, 40, 4, 38, 2)

    def fn(r, s, pr):
        if r == 1:
            raise ValueError("rank 1 gives up")
        return s.evaluate()
    with c.group() as g:
        with pytest.raises(RuntimeError, match="rank 1 failed: rank 1 gives up"):
            g.run(fn)
        with pytest.raises(RuntimeError):
            g.run(_run)


# ------------------------------------------------------------------------------------------------ S7: the one-rank communicator
def _s7_child():
    """Runs in a child process with RSBA_FORCE_COMM=1: S1's WHOLE problem on a solver with the one-rank RCCL communicator against
    the same calls on a solver without one."""
    c = Case(6, 40, 4, 31, 2, loss="huber", const_pts=(0, 23), outlier_frac=0.05, max_num_iterations=4)
    assert os.environ.get("RSBA_FORCE_COMM") == "1"
    pc, with_comm = c.single()
    del os.environ["RSBA_FORCE_COMM"]
    pn, without = c.single()
    os.environ["RSBA_FORCE_COMM"] = "1"
    assert with_comm.schedule_info()["comm_kind"] == "rccl" and without.schedule_info()["comm_kind"] == "none"
    for s in (with_comm, without):
        s.set_parameters(c.x1)
    for apply_loss in (True, False):
        ref, rbar, gbar, cbar = _reference(c, c.x1, apply_loss)
        a, b = with_comm.evaluate(apply_loss_function=apply_loss), without.evaluate(apply_loss_function=apply_loss)
        q_c, q_g = abs(a[0] - b[0]) / cbar, (np.abs(a[2] - b[2])[ref.live] / gbar[ref.live]).max()
        print("S7 evaluate apply_loss=%d: difference / bar  gradient %.3f  cost %.3f" % (apply_loss, q_g, q_c))
        assert q_c <= 1.0 and q_g <= 1.0 and np.all(a[2][~ref.live] == 0.0)
        np.testing.assert_array_equal(a[1], b[1])
        for got in (a, b):
            assert abs(got[0] - ref.cost) <= cbar and np.all(np.abs(got[2] - ref.gradient)[ref.live] <= gbar[ref.live])
    worst = 0.0
    for s in (with_comm, without):
        s.covariance_compute()
    for i in range(c.C):
        for j in range(c.C):
            a, b = with_comm.covariance_block(6 * i, 6 * j), without.covariance_block(6 * i, 6 * j)
            if 0 in (i, j):
                assert np.all(a == 0.0) and np.all(b == 0.0)
                continue
            worst = max(worst, np.abs(a - b).max() / np.abs(b).max())
    pa, pb = with_comm.point_covariances(), without.point_covariances()
    live = np.abs(pb).max(axis=(1, 2)) > 0.0
    worst = max(worst, (np.abs(pa - pb).max(axis=(1, 2))[live] / np.abs(pb).max(axis=(1, 2))[live]).max())
    assert np.all(pa[~live] == 0.0)
    print("S7 covariance: worst relative block difference %.3e" % worst)
    assert worst <= TOL
    for h in (with_comm, without, pc, pn):
        h.close()
    print("S7 ok")


def test_s7_one_rank_communicator():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, RSBA_FORCE_COMM="1", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_sharded_queries as t; t._s7_child()"], cwd=here, env=env, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "S7 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
