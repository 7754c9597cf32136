"""numpy reference of the Jacobian of ceres::Problem::Evaluate as rsba_solver_jacobian_structure / rsba_solver_evaluate_jacobian
return it: a compressed-row matrix, rows in the problem's observation order, column index = parameter offset.

Rows come from evaluate_ref.point_rows / marker_rows (the oracle's per-observation functions, pinned to the reference's committed
outputs).  The blocks of a row are sorted by offset, constant offsets are dropped (the base blocks of the marker-chain models never
appear: the functor has no such parameter), and with a loss applied the rows of a residual block are multiplied by sqrt(rho'(s)) of
that block (marker_loss_ref.rho_and_rho1), Ceres' corrector for rho'' <= 0.  All rows of an observation have the same width, so its
values are one contiguous piece, row after row."""
from types import SimpleNamespace

import numpy as np

import marker_loss_ref as mlr


def assemble(rows, num_parameters, constant_offsets=(), loss="none", a=0.0, apply_loss=True):
    """rows -> shape, indptr (int64), indices (int32), values, and per value: `obs` (its observation) and `scale` (the largest |J|
    of its observation's residual block, corrected as the values are; what an entry's error is taken relative to); `s`: the squared
    norm of every residual block."""
    N = len(rows)
    d = len(rows[0][0]) if N else 0
    raw = np.array([r for r, _ in rows], float).reshape(N, d)
    constant = {int(off) for off, _ in constant_offsets}
    indptr, indices, values, obs, scale = [0], [], [], [], []
    for i, (_, blocks) in enumerate(rows):
        kept = sorted(((int(off), np.asarray(J, float)) for off, J in blocks if int(off) not in constant), key=lambda b: b[0])
        cols = [off + k for off, J in kept for k in range(J.shape[1])]
        vals = np.concatenate([J for _, J in kept], axis=1) if kept else np.zeros((d, 0))
        top = float(np.abs(vals).max()) if vals.size else 0.0
        for row in range(d):
            indices.extend(cols)
            values.extend(vals[row])
            indptr.append(len(indices))
        obs.extend([i] * (d * len(cols)))
        scale.extend([top] * (d * len(cols)))
    ref = SimpleNamespace(shape=(N * d, int(num_parameters)), indptr=np.array(indptr, np.int64), indices=np.array(indices, np.int32),
                          values=np.array(values, float), obs=np.array(obs, np.int64), scale=np.array(scale, float),
                          s=np.sum(raw * raw, axis=1))
    return corrected(ref, loss, a) if apply_loss else ref


def corrected(ref, loss, a):
    """The raw matrix (apply_loss False) with every residual block's rows multiplied by sqrt(rho'(s)): one rounding per value."""
    sq = np.sqrt(mlr.rho_and_rho1(ref.s, loss, a)[1])[ref.obs] if len(ref.obs) else np.zeros(0)
    return SimpleNamespace(**dict(vars(ref), values=sq * ref.values, scale=sq * ref.scale))


def dense(shape, indptr, indices, values):
    """The matrix as a dense array (duplicates would add up; a row never names a column twice)."""
    J = np.zeros(shape)
    for r in range(shape[0]):
        for q in range(indptr[r], indptr[r + 1]):
            J[r, indices[q]] += values[q]
    return J


def transpose_times(shape, indptr, indices, values, r):
    """J'r, one term at a time in row order."""
    g = np.zeros(shape[1])
    row = np.repeat(np.arange(shape[0]), np.diff(indptr))
    np.add.at(g, indices, values * np.asarray(r, float)[row])
    return g
