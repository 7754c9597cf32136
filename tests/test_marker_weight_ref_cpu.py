"""tests/marker_weight_ref.py (the numpy reference with per-observation weights) pinned by properties that need no product code, and
the decision margins of every case tests/test_gpu_marker_weights.py compares accept / reject sequences on.  No GPU.
"""
import numpy as np
import pytest

import marker_loss_ref as ref
import marker_weight_ref as wref


def _unweighted(prob, cs):
    mc = ref.MarkerChain(prob, cs["variant"], cs["loss"], cs["a"], cs["constant_blocks"])
    x, summary, rows = ref.minimise(mc)
    return mc, summary, rows, mc.full(x)


def _decisions(rows):
    return [rw["valid"] + 2 * rw["successful"] for rw in rows]


# every case of the table whose weights are 0 / 1
@pytest.mark.parametrize("name", ["hongo_mask_none", "hongo_mask_huber", "test2_mask_cauchy", "4x40x6_mask_none", "12x40x20_mask_none"])
def test_weights_zero_one_equal_removal(name):
    """Weight 0 on some rows is the unweighted problem without those rows: the same free blocks, the same accept / reject sequence,
    final parameters within 1e-14, costs within 4e-13 relative (measured; the two differ by the order of the sums alone)."""
    cs, mc, summary, rows, final = wref.reference_run(name)
    keep = np.flatnonzero(cs["weights"] != 0.0)
    assert 0 < keep.size < cs["prob"]["N"] and set(np.unique(cs["weights"])) == {0.0, 1.0}
    mc0, summary0, rows0, final0 = _unweighted(wref.select_rows(cs["prob"], keep), cs)
    np.testing.assert_array_equal(mc.free_blocks, mc0.free_blocks)
    assert (summary["termination"], summary["reason"]) == (summary0["termination"], summary0["reason"])
    assert _decisions(rows) == _decisions(rows0)
    assert np.abs(final - final0).max() <= 1e-14
    for rw, rw0 in zip(rows, rows0):
        assert abs(rw["cost"] - rw0["cost"]) <= 4e-13 * rw0["cost"]
    # the raw sum of squares is not weighted: the removed rows still count in it
    assert summary["final_sumsq"] > summary0["final_sumsq"]


def test_masked_cases_discriminate():
    """The unweighted run of a masked case ends far from the weighted one (5e-4 to 0.34 in the parameters against the device test's
    bar of 1e-6): ignoring the weights cannot pass."""
    for name in ["hongo_mask_none", "hongo_mask_huber", "test2_mask_cauchy", "4x40x6_mask_none"]:
        cs, mc, summary, rows, final = wref.reference_run(name)
        _, _, _, final0 = _unweighted(cs["prob"], cs)
        assert np.abs(final - final0).max() > 1e-4, name


def test_weight_two_equals_duplication():
    """Weight 2 on every third row is the unweighted problem with those rows listed twice (1e-10 on the parameters, the same iteration
    counts)."""
    clean, prob = wref.rig((4, 40, 6))
    w = np.ones(prob["N"])
    w[::3] = 2.0
    mc = wref.WeightedMarkerChain(prob, w, 0, "huber", 2.0)
    x, summary, rows = ref.minimise(mc)
    index = np.concatenate([np.arange(prob["N"]), np.arange(0, prob["N"], 3)])
    mc0 = ref.MarkerChain(wref.select_rows(prob, index), 0, "huber", 2.0)
    x0, summary0, rows0 = ref.minimise(mc0)
    assert _decisions(rows) == _decisions(rows0)
    assert np.abs(mc.full(x) - mc0.full(x0)).max() <= 1e-10
    assert abs(summary["final_cost"] - summary0["final_cost"]) <= 1e-12 * summary0["final_cost"]


def test_time_with_zero_weights_keeps_its_bits_and_leaves_the_system_singular():
    cs, mc, summary, rows, final = wref.reference_run("4x40x6_time7_huber")
    C = cs["prob"]["C"]
    at7 = np.asarray(cs["prob"]["t"]) == 7
    assert int(np.sum(at7)) == 17 and not np.any(cs["weights"][at7])
    np.testing.assert_array_equal(final[C + 7], np.asarray(cs["prob"]["params"]).reshape(-1, 6)[C + 7])
    H = mc.linearise(final[mc.free_blocks].ravel())[3]
    assert H.shape == (288, 288) and np.linalg.matrix_rank(H) == 282


@pytest.mark.parametrize("name", wref.TABLE + wref.EXTRA)
def test_decision_margins(name):
    """A condition on the cases, so that comparing accept / reject sequences with the device never rests on a coin flip: on every valid
    step that reaches the test, relative_decrease stays 1e-2 away from min_relative_decrease = 1e-3 and |cost_change| stays 1e-3
    (relative) away from function_tolerance x cost = 1e-6 cost."""
    cs, mc, summary, rows, final = wref.reference_run(name)
    assert summary["termination"] == "CONVERGENCE" and len(rows) > 3
    m_rel, m_fun = np.inf, np.inf
    for j, rw in enumerate(rows[1:], 1):
        if not rw["valid"]:
            continue
        last = j == len(rows) - 1
        if last and summary["reason"] == "parameter":
            continue   # (ended before the cost change was looked at)
        before = rw["cost"] + rw["cost_change"] if rw["successful"] else rw["cost"]
        m_fun = min(m_fun, abs(abs(rw["cost_change"]) / (1e-6 * before) - 1.0))
        if last and summary["reason"] == "function":
            continue   # (ended before the relative decrease was formed)
        m_rel = min(m_rel, abs(rw["relative_decrease"] - 1e-3))
    print("%s: %d iterations, %d successful, margins %.3g (relative decrease) %.3g (function tolerance)"
          % (name, len(rows) - 1, sum(rw["successful"] for rw in rows), m_rel, m_fun))
    assert m_rel > 1e-2 and m_fun > 1e-3
