"""Backward error of a solve of the reduced camera system, and the bar any correct fp64 factorisation meets (host code).

The point model's step solves S y = rhs, S the Jacobi-scaled, LM-damped 6C x 6C reduced camera system (SPD), with a blocked
Cholesky factorisation: 32-wide panels, the 32 x 32 diagonal factors L_kk inverted explicitly (T_k = L_kk^-1, DiagFactorInverse
in ba_cholesky.hpp), the panels below them and the right-hand side formed as products with T_k' and the back-substitution
x_k = T_k' y_k, partly on the matrix cores.  The kernels hand back dcam = -scale_c * y.

Measure (Oettli-Prager, componentwise in the metric of S's own diagonal), per free row i:

    eta_i = |rhs_i - sum_j S_ij y_j| / ( sqrt(S_ii) * sum_j sqrt(S_jj) |y_j| + |rhs_i| )

evaluated in np.longdouble (80-bit x87 on x86-64: 64-bit mantissa, eps ~1.1e-19, so the residual of an fp64 solution is exact to
well below the bar).  eta_i is the smallest epsilon with (S + dS) y = rhs + d, |dS_ij| <= epsilon sqrt(S_ii S_jj), |d_i| <= epsilon
|rhs_i|.

Bar.  Plain Cholesky, n = 6C: (S + dS) y^ = rhs with |dS| <= gamma_{3n+1} |R'||R| (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., Thm 10.4; gamma_k = k u / (1 - k u), u = 2^-53).  By Cauchy-Schwarz (|R'||R|)_ij <= ||r_i|| ||r_j||, and
||r_i||^2 = (R'R)_ii <= S_ii / (1 - gamma_{n+1}) for the computed factor (Thm 10.3), so eta <= gamma_{3n+1} / (1 - gamma_{n+1}),
whatever the conditioning of S.  The kernels replace the triangular substitutions with the diagonal blocks by products with
their computed inverses: x^ = T^ b with T^ L = I + E, |E| <= c u |T^||L| (Higham sec. 14.2 / sec. 13.3), which is a backward
perturbation of L_kk of norm at most kappa_inf(L_kk) times what a substitution commits.  Every term of the bound that runs through
a diagonal block therefore stretches by at most (1 + kappa_inf(L_kk)):

    bar = gamma_{3n+1} / (1 - gamma_{n+1}) * (1 + max_k kappa_inf(L_kk)) + 8 u

with L_kk the 32 x 32 diagonal blocks (the last one partial) of the host's Cholesky factor of S.  The 8 u cover what lies outside
the factorisation: y recovered as -dcam / scale_c (two roundings in dcam = -scale_c * y and one in the division) and S formed
apart from the factorisation's own copy (a rounding per entry, S_ij = raw_ij * (s_i s_j) + damping).  Nothing here is fitted to a
measurement.

What the measure sees.  A wrong entry of relative size delta in block k changes eta by about delta times the share of block k in
sum_j sqrt(S_jj)|y_j| — a local error is diluted by the rest of the solution, a global one is not.
"""
import numpy as np

U = 2.0 ** -53
PB = 32   # the kernels' panel width (RSBA_PB)


def longdouble_ok():
    return np.finfo(np.longdouble).eps < 1e-18


def gamma(k):
    return k * U / (1.0 - k * U)


def diag_block_kappas(S, pb=PB):
    """kappa_inf of the pb x pb diagonal blocks of the Cholesky factor of S (host, fp64); inf when S is not positive definite."""
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return np.array([np.inf])
    out = []
    for k in range(0, S.shape[0], pb):
        Lk = L[k:k + pb, k:k + pb]
        Tk = np.linalg.inv(Lk)
        out.append(np.abs(Lk).sum(axis=1).max() * np.abs(Tk).sum(axis=1).max())
    return np.array(out)


def bar(S, pb=PB):
    """The bar above for S (n = S.shape[0]); returns (bar, max kappa_inf(L_kk))."""
    n = S.shape[0]
    kappa = float(diag_block_kappas(S, pb).max())
    return gamma(3 * n + 1) / (1.0 - gamma(n + 1)) * (1.0 + kappa) + 8 * U, kappa


def backward_errors(S, rhs, y, rows=None):
    """eta_i for the rows `rows` (default: all), in np.longdouble."""
    Sl = np.asarray(S, dtype=np.longdouble)
    yl = np.asarray(y, dtype=np.longdouble)
    bl = np.asarray(rhs, dtype=np.longdouble)
    r = bl - Sl @ yl
    d = np.sqrt(np.maximum(np.diagonal(Sl), 0))
    den = d * np.sum(d * np.abs(yl)) + np.abs(bl)
    eta = np.abs(r) / np.where(den > 0, den, 1)
    eta = np.where(den > 0, eta, np.where(r == 0, 0, np.inf))
    if rows is not None:
        eta = eta[rows]
    return eta.astype(np.float64)


def free_rows(C, cam_free=None):
    """Row indices of the free cameras (cam_free[c] == 0: constant camera, excluded)."""
    if cam_free is None:
        return np.arange(6 * C)
    return np.concatenate([np.arange(6 * c, 6 * c + 6) for c in range(C) if cam_free[c]] or [np.zeros(0, dtype=int)])


def check(S, rhs, y, rows=None):
    """(max eta over `rows`, bar, kappa) for a solution y of S y = rhs."""
    assert longdouble_ok()
    b, kappa = bar(S)
    eta = backward_errors(S, rhs, y, rows)
    return float(eta.max()) if eta.size else 0.0, b, kappa
