"""The numpy reference of the CRS Jacobian (tests/jacobian_ref.py) against what it must agree with on the CPU alone: an independent
dense assembly of the same oracle rows (exactly), the gradient of tests/evaluate_ref.py (J'r within (n_k + 2) u sum_i |J_ik r_i|: the
same products, summed in another order), and the structural rules — a row whose blocks are all constant is empty, the columns of
constant blocks and of the marker-chain models' fixed base blocks hold nothing."""
import numpy as np
import pytest

import evaluate_ref as er
import jacobian_ref as jr
import marker_loss_ref as mlr
import oracle_lib
from test_gpu_evaluate import _case

U = 2.0 ** -53


def _setup(name):
    c = _case(name)
    o = oracle_lib.load()
    if c.kind == "points":
        rows = er.point_rows(o, c.prob, c.x1)
        # camera 0 and the point of camera 0's first row: that observation has no free block
        first = int(np.nonzero(c.prob["cam_idx"] == 0)[0][0])
        const_pts = tuple(sorted(set(c.const_pts) | {int(c.prob["pt_idx"][first])}))
        const = er.point_constant_offsets(c.prob, (0,), const_pts)
        return c, rows, const, first
    rows = er.marker_rows(o, c.prob, c.x1, c.variant)
    return c, rows, [(6 * b, 6) for b in c.const_blocks], None


@pytest.mark.parametrize("name", ["P1", "M1_dense", "M2", "M3_dense"])
@pytest.mark.parametrize("apply_loss", [True, False])
def test_reference_against_dense_assembly_and_gradient(name, apply_loss):
    c, rows, const, all_const_obs = _setup(name)
    loss, a = (c.loss, c.a) if c.loss != "none" else ("huber", 1.0)   # (a loss everywhere: the corrector is part of what is checked)
    n = len(c.x1)
    ref = jr.assemble(rows, n, const, loss, a, apply_loss)
    ev = er.finish(rows, n, const, loss, a, apply_loss)
    d = 2 if c.kind == "points" else 8
    assert ref.shape == (d * c.prob["N"], n) and len(ref.indptr) == ref.shape[0] + 1 and ref.indptr[-1] == len(ref.values) == len(ref.indices)
    # --- an independent dense assembly of the same rows
    s = np.array([float(np.sum(np.square(r))) for r, _ in rows])
    sq = np.sqrt(mlr.rho_and_rho1(s, loss, a)[1]) if apply_loss else np.ones_like(s)
    assert not apply_loss or np.any(sq != 1.0)
    const_cols = {k for off, size in const for k in range(off, off + size)}
    J = np.zeros(ref.shape)
    for i, (_, blocks) in enumerate(rows):
        for off, Jb in blocks:
            if off not in const_cols:
                J[d * i:d * i + d, off:off + Jb.shape[1]] = sq[i] * Jb
    np.testing.assert_array_equal(jr.dense(ref.shape, ref.indptr, ref.indices, ref.values), J)
    # --- structure: ascending columns inside a row, rows of one observation alike, constant and base columns empty
    for r in range(ref.shape[0]):
        cols = ref.indices[ref.indptr[r]:ref.indptr[r + 1]]
        assert np.all(np.diff(cols) > 0)
        np.testing.assert_array_equal(cols, ref.indices[ref.indptr[r - r % d]:ref.indptr[r - r % d + 1]])
    used = set(int(k) for k in ref.indices)
    assert not (used & const_cols)
    if c.kind == "marker":
        base = set(range(6)) | (set(range(6 * (c.prob["C"] + c.prob["T"]), 6 * (c.prob["C"] + c.prob["T"]) + 6)) if c.variant == 0 else set())
        assert not (used & base)
        assert set(np.unique(np.diff(ref.indptr))) <= {0, 6, 12, 18}
    else:
        i = all_const_obs
        assert ref.indptr[2 * i] == ref.indptr[2 * i + 1] == ref.indptr[2 * i + 2]   # every block constant: two empty rows
        assert set(np.unique(np.diff(ref.indptr))) == {0, 3, 6, 9}
    # --- J'r is evaluate_ref's gradient
    g = jr.transpose_times(ref.shape, ref.indptr, ref.indices, ref.values, ev.residuals)
    bar = (ev.n_terms + 2) * U * ev.abs_Jr
    live = ev.live
    assert np.all(np.abs(g - ev.gradient)[live] <= bar[live])
    assert np.all(g[~live] == 0.0) and np.all(ev.gradient[~live] == 0.0)
    q = np.abs(g - ev.gradient)[live] / np.maximum(bar[live], 1e-300)
    print("jacobian reference %s apply_loss=%d: J'r against the gradient, worst error / bar %.3f" % (name, apply_loss, q.max()))
