"""The back-substitution of eliminated blocks into the reduced inverse, in numpy: what rsba_solver_covariance_blocks and
rsba_solver_time_covariances compute on the device, written from the same formulas and checked against the dense inverse
(tests/test_covariance_cross_ref_cpu.py).  With e an eliminated block (a time block on the marker chain's time-eliminating path, a
point on the point model), V_e its diagonal block of H = J'J, W_e = H[reduced, e], Y_e = W_e V_e^-1 and Sigma = S^-1,
S = H[reduced, reduced] - sum_e W_e V_e^-1 W_e':

    cov(e, e)  = V_e^-1 + Y_e' Sigma Y_e        cov(e, e') = Y_e' Sigma Y_e'        cov(x, e) = -Sigma[x, :] Y_e

Also the shapes that the CPU and the GPU tests share (the GPU tests rely on their row / view counts).
"""
import numpy as np

import marker_loss_ref as ref

# (C, T, M, seed) of the synthetic marker-chain rigs; MC_TWO_CHUNKS has more than 64 rows in every time
MC_TWO_CHUNKS = (8, 12, 16, 31)
MC_LONG = (5, 80, 8, 21)
MC_WEIGHTED = (3, 70, 5, 5)
# (C, P, k, seed, outlier_frac) of the point problems; PT_TWO_CHUNKS has 70 views of every point
PT_SMALL = (6, 40, 4, 16, 0.0)
PT_TWO_CHUNKS = (70, 24, 70, 41, 0.0)
PT_ROBUST = (8, 200, 5, 12, 0.05)


def marker_rig(shape):
    from realsensecalibration_amd import synthetic as syn
    C, T, M, seed = shape
    return syn.make_marker_chain(C, T, M, seed=seed)


def point_problem(shape):
    from realsensecalibration_amd import synthetic as syn
    C, P, k, seed, outl = shape
    return syn.make_problem(C, P, k, seed=seed, outlier_frac=outl)


def schur_covariance(H, reduced, eliminated):
    """inv(H) by the Schur route.  reduced: the column indices of the reduced blocks; eliminated: a list of index arrays, one per
    eliminated block (H has no entries between two of them).  -> the full n x n covariance."""
    n = H.shape[0]
    reduced = np.asarray(reduced, int)
    S = H[np.ix_(reduced, reduced)].copy()
    Y, Vi = [], []
    for e in eliminated:
        W = H[np.ix_(reduced, e)]
        vi = np.linalg.inv(H[np.ix_(e, e)])
        S -= W @ vi @ W.T
        Y.append(W @ vi)
        Vi.append(vi)
    sigma = np.linalg.inv(S)
    cov = np.zeros((n, n))
    cov[np.ix_(reduced, reduced)] = sigma
    for i, e in enumerate(eliminated):
        x = -sigma @ Y[i]
        cov[np.ix_(reduced, e)] = x
        cov[np.ix_(e, reduced)] = x.T
        z = sigma @ Y[i]
        for k, f in enumerate(eliminated):
            cov[np.ix_(f, e)] = Y[k].T @ z + (Vi[i] if k == i else 0.0)
    return cov


def marker_split(mc):
    """A MarkerChain's free columns split as the time-eliminating path splits them -> (reduced columns, [columns of each free time])."""
    at = {int(b): 6 * i for i, b in enumerate(mc.free_blocks)}
    red = [at[b] + k for b in at if not mc.C <= b < mc.C + mc.T for k in range(6)]
    elim = [np.arange(at[b], at[b] + 6) for b in at if mc.C <= b < mc.C + mc.T]
    return np.array(sorted(red)), elim


def worst_block_difference(a, b, sizes):
    """max over the blocks (consecutive, of the given sizes) of max|a - b| / max|b| of the block."""
    edges = np.concatenate([[0], np.cumsum(sizes)])
    worst = 0.0
    for i in range(len(sizes)):
        for j in range(len(sizes)):
            ra, rb = slice(edges[i], edges[i + 1]), slice(edges[j], edges[j + 1])
            worst = max(worst, np.abs(a[ra, rb] - b[ra, rb]).max() / np.abs(b[ra, rb]).max())
    return worst


def rows_per_time(prob):
    return np.bincount(np.asarray(prob["t"]), minlength=prob["T"])


def weighted_case():
    """MC_WEIGHTED with 5 % of its corners 40 px off, Huber 2 px, fractional weights with zeros on the hit rows (never every row of a
    time), a constant time block (C + 4) and a constant marker block (C + T + 2)."""
    import marker_weight_ref as wref
    clean = marker_rig(MC_WEIGHTED)
    prob = ref.displace_corners(clean, 0.05, 40.0, 5)
    hit = wref.hit_rows(clean, prob)
    w = np.random.default_rng(7).choice([0.25, 1.0, 4.0], prob["N"]) * wref.mask_of(hit)
    C, T = prob["C"], prob["T"]
    return dict(prob=prob, weights=w, loss="huber", a=2.0, constant_blocks=(C + 4, C + T + 2), hit=hit)
