"""The marker-chain step measure (tests/marker_step_accuracy.py) is neither vacuous nor false: without a GPU, on every case shape of
tests/test_gpu_marker_step.py,

  * both numpy references' own fp64 steps — marker_sparse_ref.SparseMarkerChain.step (the eliminated algorithm) and the dense Cholesky
    inside marker_loss_ref.minimise — pass through the same x1 = fl(x0 + delta) round trip and stay within the bar;
  * three mutations of the eliminated reference each exceed it: one residual block left out of one time's W_t, one time's
    (V_t + D_t)^-1 rounded to float32, the last chunk's partial sum of W'EW left out of the reduced system.

No shape is thinned or skipped: the cases' distinct (problem, wiring, loss, constant set, radius, state) combinations are all checked,
and their count is asserted."""
import numpy as np
import pytest

import marker_loss_ref as ref
import marker_sparse_ref as sref
import marker_step_accuracy as msa

SHAPES = {}
for _c in msa.CASES:
    SHAPES.setdefault(msa.shape_key(_c), _c)
SHAPE_CASES = list(SHAPES.values())
ONE_STEP = dict(max_num_iterations=1, function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0)
_CHECKED = set()


def eliminated_step(smc, lin, scale, radius, mutation=None):
    """SparseMarkerChain.step, operation for operation (asserted below), with the three mutations as hooks."""
    _, _, Jt, U, g_r, V, gt, W, _ = lin
    nr, nt = smc.nr, smc.nt
    if mutation == "w_block":
        # the first residual block with a free time and a reduced column: its 6 x 6 products leave that time's W
        k = int(np.flatnonzero((smc.tim_f >= 0) & ((smc.cam_r >= 0) | (smc.mar_r >= 0)))[0])
        W = W.copy()
        Jtm = Jt[k][:, 6:12]
        for blk, cols in ((smc.cam_r[k], slice(0, 6)), (smc.mar_r[k], slice(12, 18))):
            if blk >= 0:
                W[smc.tim_f[k], :, 6 * blk:6 * blk + 6] -= Jtm.T @ Jt[k][:, cols]
    sr, st = scale[:nr], scale[nr:].reshape(nt, 6)
    Us = U * np.outer(sr, sr)
    Ur = Us + np.diag(np.clip(np.diag(Us), msa.MIN_LM, msa.MAX_LM) / radius)
    Vs = V * st[:, :, None] * st[:, None, :]
    dV = np.clip(np.einsum("tii->ti", Vs), msa.MIN_LM, msa.MAX_LM) / radius
    Vd = Vs + dV[:, :, None] * np.eye(6)[None]
    Ws = W * st[:, :, None] * sr[None, None, :]
    bt = st * gt
    Vi = np.linalg.inv(Vd)
    if mutation == "inverse_float32":
        Vi[0] = Vi[0].astype(np.float32).astype(np.float64)
    sel = slice(None)
    if mutation == "last_chunk":
        sel = slice(0, np.array_split(np.arange(nt), min(nt, 8))[-1][0])   # chunks of consecutive times; the last one's partial is lost
    S = Ur - np.einsum("tar,tab,tbq->rq", Ws[sel], Vi[sel], Ws[sel])
    rhs = sr * g_r - np.einsum("tar,tab,tb->r", Ws[sel], Vi[sel], bt[sel])
    L = np.linalg.cholesky(S)
    yr = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    yt = np.einsum("tab,tb->ta", Vi, bt - np.einsum("tar,r->ta", Ws, yr))
    delta = np.zeros(smc.mc.n)
    delta[smc.x_red] = -sr * yr
    delta[smc.x_tim] = -(st * yt).ravel()
    return delta


_CONVERGED = {}


def _start(case):
    if case.state != "second":
        return msa.problem(case.prob)
    key = (case.prob, case.variant, case.loss, case.const)
    if key not in _CONVERGED:
        mc = msa.chain(case)
        x, summary, _ = ref.minimise(mc)
        assert summary["termination"] == "CONVERGENCE"
        _CONVERGED[key] = mc.full(x).ravel()
    return msa.start_problem(case, _CONVERGED[key])


@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c.name for c in SHAPE_CASES])
def test_references_within_the_bar_and_mutations_above_it(case):
    prob = _start(case)
    mc = msa.chain_at(case, prob)
    x0 = mc.x0()
    assert np.linalg.norm(x0) > 1.0   # (parameter_tolerance = -1 ends a run only below |x| = 1)
    sysm = msa.System(mc, x0, case.radius, dense=False)
    dense = msa.System(mc, x0, case.radius, dense=True)
    smc = sref.SparseMarkerChain(prob, case.variant, case.loss, mc.a, msa.constant_blocks(case, prob))
    lin = smc.linearise(x0)
    scale = 1.0 / (1.0 + np.sqrt(smc.diag(lin)))
    d_el = smc.step(lin, scale, case.radius, msa.MIN_LM, msa.MAX_LM)
    np.testing.assert_array_equal(d_el, eliminated_step(smc, lin, scale, case.radius))
    # the dense Cholesky inside marker_loss_ref.minimise, accepted whatever its gain
    x_dense, _, rows = ref.minimise(mc, initial_radius=case.radius, min_relative_decrease=-1e300, **ONE_STEP)
    assert rows[1]["successful"] == 1
    # the case's force flag says whether the default threshold would reject this step
    assert case.force == (not rows[1]["relative_decrease"] > 1e-3), rows[1]
    got = {"eliminated": sysm.check(x0 + d_el), "dense": dense.check(x_dense)}
    line = "%-34s n %4d m %6d kappa_t %9.2e kappa_s %9.2e |" % (case.name, sysm.n, sysm.m, sysm.kappa_t, sysm.kappa_s)
    for k, r in got.items():
        line += " %s eta %.2e bar %.2e eta/bar %.3f |" % (k, r["eta"], r["bar"], r["ratio"])
    mut = {k: sysm.check(x0 + eliminated_step(smc, lin, scale, case.radius, k)) for k in ("w_block", "inverse_float32", "last_chunk")}
    for k, r in mut.items():
        line += " %s %.1e" % (k, r["ratio"])
    print("\n" + line)
    for k, r in got.items():
        assert r["eta"] <= r["bar"], (k, r)
    for k, r in mut.items():
        assert r["eta_max"] > sysm.forming + sysm.solve + 4 * msa.U and r["ratio"] > 1.0, (k, r, "the bar does not see this mutation")
    # the reference's scalars pass the scalar tolerances through the same round trip
    nd, tol = sysm.step_norm_tolerance(x0 + d_el)
    assert abs(np.linalg.norm(d_el) - nd) <= tol
    if case.loss != "none":
        r = mc.residuals(mc.full(x0))
        past = int(np.sum(np.sum(r * r, axis=1) > msa.LOSS_A ** 2))
        assert 0 < past < mc.N, past
    _CHECKED.add(msa.shape_key(case))


def test_every_listed_shape_was_checked():
    assert len(_CHECKED) == len(SHAPE_CASES) == len({msa.shape_key(c) for c in msa.CASES}), (len(_CHECKED), len(SHAPE_CASES))


def test_case_list_covers_the_paths():
    """The path each case names is the one the thresholds of PlanMarkerChain (csrc/ba_marker_plan.hpp) give for its structure."""
    want = {"minimal_2x3x2": (12, "mfma3", "lds"), "minimal_2x3x2_test2": (18, "mfma3", "lds"),
            "width_13x8x13": (144, "mfma3", "lds"), "width_13x8x14": (150, "mfma8", "lds"), "width_21x6x21": (240, "mfma8", "panel"),
            "width_21x6x22": (246, "valu_mem", "panel"), "width_14x8x14": (156, "mfma8", "lds"), "width_14x8x15": (162, "mfma8", "panel"),
            "width_33x6x33": (384, "valu_mem", "panel"), "width_33x6x34": (390, "valu_mem", "multi"),
            "wide_60x3x60": (708, "valu_mem", "multi"), "wide_62x3x62": (732, "", "multi")}
    byname = {c.name: c for c in msa.CASES}
    assert len(byname) == len(msa.CASES)
    for nm, (nr, acc, solve) in want.items():
        mc = msa.chain(byname[nm])
        p = msa.expected_path(byname[nm], mc)
        assert (msa.structure(mc)[0], p["acc"], p["solve"]) == (nr, acc, solve), (nm, msa.structure(mc), p)
    assert msa.expected_path(byname["wide_62x3x62"], msa.chain(byname["wide_62x3x62"]))["elim"] == "k_time_eliminate"
    assert msa.structure(msa.chain(byname["wide_60x3x60"]))[2] == 118 and msa.structure(msa.chain(byname["wide_62x3x62"]))[2] == 122
    assert msa.structure(msa.chain(byname["wide_8x6x12"]))[3] == 96
    p = msa.expected_path(byname["wide_8x6x12_backsub_wg"], msa.chain(byname["wide_8x6x12_backsub_wg"]))
    assert p["backsub"] == "wg"
    for nm, elim, backsub in (("switch_8x24x12_SPLIT=0", "k_time_eliminate", "wg"), ("switch_8x24x12_BACKSUB_WG=0,SPLIT_BACKSUB=0", "split", "terms"),
                              ("switch_8x24x12_ACC_MFMA=0", "split", "split"), ("loss_8x24x12_huber", "split", "split")):
        p = msa.expected_path(byname[nm], msa.chain(byname[nm]))
        assert (p["elim"], p["backsub"]) == (elim, backsub), (nm, p)
    assert msa.expected_path(byname["switch_8x24x12_ACC_MFMA=0"], msa.chain(byname["switch_8x24x12_ACC_MFMA=0"]))["acc"] == "valu_lds"
    assert msa.expected_path(byname["switch_8x24x12_SOLVE_LDS=0"], msa.chain(byname["switch_8x24x12_SOLVE_LDS=0"]))["solve"] == "panel"
