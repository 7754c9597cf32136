"""The maths of rsba_solver_covariance_blocks in numpy (tests/covariance_cross_ref.py: the Schur-formula route) against the dense
inverse, at every shape tests/test_gpu_covariance_cross.py uses: the two must agree to 1e-10 of each block's largest entry, two
decades below the bar the device is held to (1e-8).  And the shape properties the GPU tests rely on."""
import numpy as np
import pytest

import covariance_cross_ref as xr
import covariance_ref as cr
import marker_loss_ref as ref
import marker_weight_ref as wref

BAR = 1e-10


def _marker(mc):
    _, _, _, H, _, _ = mc.linearise(mc.x0())
    red, elim = xr.marker_split(mc)
    assert len(elim) > 0 and len(red) + 6 * len(elim) == H.shape[0]
    worst = xr.worst_block_difference(xr.schur_covariance(H, red, elim), np.linalg.inv(H), [6] * (H.shape[0] // 6))
    print("kappa %.2e, Schur route against the dense inverse: %.2e of a block (bar %.0e)" % (np.linalg.cond(H), worst, BAR))
    assert worst <= BAR


def test_hongo():
    _marker(ref.MarkerChain(ref.hongo()))


@pytest.mark.parametrize("shape", [xr.MC_TWO_CHUNKS, xr.MC_LONG], ids=["8x12x16", "5x80x8"])
def test_marker_rigs(shape):
    _marker(ref.MarkerChain(xr.marker_rig(shape)))


@pytest.mark.parametrize("apply_loss", [1, 0])
def test_weighted_rig_with_constant_blocks(apply_loss):
    cs = xr.weighted_case()
    if apply_loss:
        _marker(wref.WeightedMarkerChain(cs["prob"], cs["weights"], 0, cs["loss"], cs["a"], cs["constant_blocks"]))
    else:
        _marker(ref.MarkerChain(cs["prob"], 0, "none", 0.0, cs["constant_blocks"]))


@pytest.mark.parametrize("shape,huber,cauchy", [(xr.PT_SMALL, 0.0, False), (xr.PT_TWO_CHUNKS, 0.0, False), (xr.PT_ROBUST, 2.0, False), (xr.PT_ROBUST, 2.0, True)],
                         ids=["6x40x4", "70x24x70", "8x200x5_huber", "8x200x5_cauchy"])
def test_point_problems(oracle, shape, huber, cauchy):
    prob = xr.point_problem(shape)
    C, P = prob["C"], prob["P"]
    J = cr.point_jacobian(oracle, prob, prob["params"], huber, cauchy)
    keep = np.concatenate([np.arange(6, 6 * C), np.arange(6 * C + 3, 6 * C + 3 * P)])   # camera 0 and point 0 constant
    H = J[:, keep].T @ J[:, keep]
    nr = 6 * (C - 1)
    elim = [np.arange(nr + 3 * j, nr + 3 * j + 3) for j in range(P - 1)]
    worst = xr.worst_block_difference(xr.schur_covariance(H, np.arange(nr), elim), np.linalg.inv(H), [6] * (C - 1) + [3] * (P - 1))
    print("kappa %.2e, Schur route against the dense inverse: %.2e of a block (bar %.0e)" % (np.linalg.cond(H), worst, BAR))
    assert worst <= BAR


def test_shapes_the_gpu_tests_rely_on():
    k = xr.rows_per_time(xr.marker_rig(xr.MC_TWO_CHUNKS))
    assert k.min() >= 78 and k.max() <= 111, (k.min(), k.max())   # every time has a second chunk of 64 rows
    prob = xr.point_problem(xr.PT_TWO_CHUNKS)
    assert np.all(np.bincount(prob["pt_idx"], minlength=prob["P"]) == 70)   # every point a second chunk of views
    cs = xr.weighted_case()
    w, t = cs["weights"], np.asarray(cs["prob"]["t"])
    assert np.any(w == 0.0) and all(np.any(w[t == q] > 0.0) for q in range(cs["prob"]["T"]))
    h = ref.hongo()
    assert (h["C"], h["T"], h["M"]) == (4, 6, 11)   # 6 times and 13 free camera / marker blocks
