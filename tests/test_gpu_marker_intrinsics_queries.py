"""The queries of a marker-chain solver with free intrinsics under the extended layout (rsba_solver_set_extended_layout): evaluate,
set_parameters and the covariance, on the dense path (schur_impl = 1) and the time-eliminating one (schur_impl = 3), against
tests/marker_intrinsics_query_ref.py — a numpy reference that shares no code with the product, pinned without a device by
tests/test_marker_intrinsics_query_ref_cpu.py.

Three states of one solver: before a run, after a run, after set_parameters to a seeded perturbation (poses, fx fy by 1 %, cx cy by
3 px, k1 k2 by 0.01 — every slot, held or not).

Bars.  Evaluate: those of tests/test_gpu_evaluate.py's docstring — rbar = 16 x max(d_r, 4 ulp(max |observation coordinate|)), per
gradient entry sum_i |J_ik| rbar + (64 + n_k) u sum_i |J_ik r_i|, the cost rbar sum |r| + N u cost.  The oracle has no free
intrinsics, so d_r is the numpy reference's own rounding: the largest difference between its float64 raw residuals and the same
formulas run in np.longdouble (its functions carry the dtype; asserted in the reference).  Slots that are zeros by definition are
compared as bits.  Covariance: tests/test_gpu_covariance.py's bar, 1e-8 of the reference block's largest entry, taken only where the
reference is itself stable: np.linalg.inv(H) and the Cholesky inverse of the Jacobi-scaled H must agree on every block within 1e-9
of the block's largest entry, asserted as a condition.  Every test prints its largest error / bar.
"""
import numpy as np
import pytest

import marker_intrinsics_query_ref as qref
import marker_intrinsics_ref as iref
from realsensecalibration_amd import capi, synthetic

pytestmark = pytest.mark.gpu

NAMES = ["3x12x4_0f", "3x12x4_3f", "3x70x5_mixed_all", "rig5_65rows", "rig6_six_masks"]
IMPLS = [1, 3]
_CASES, _REFS, _SESSIONS = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert capi.load().rsba_device_count() > 0, "GPU tests need a HIP device; the product has no CPU path"


def _rig_case(C, T, M, masks):
    prob, truth_six, truth = iref.rig(C, T, M, masks)
    return dict(prob=prob, dist=prob["dist"], masks=list(masks), variant=0, loss="none", a=0.0, weights=None, constant_blocks=(), pose_masks={},
                priors={}, truth_six=truth_six, truth=truth)


def _case(name):
    if name not in _CASES:
        if name == "rig5_65rows":
            cs = _rig_case(5, 3, 14, [0x3F] * 5)
            rows = np.bincount(np.asarray(cs["prob"]["t"]), minlength=3)
            assert cs["prob"]["N"] == 166 and rows.max() == 65 and rows.max() > 64, rows   # a second trip of the 64-row chunk loop, one valid lane
        elif name == "rig6_six_masks":
            cs = _rig_case(6, 2, 12, [0x0F, 0x3F, 0, 0x33, 0x3F, 0x01])
            assert sorted(np.bincount(np.asarray(cs["prob"]["t"]), minlength=2).tolist()) == [53, 61]
        else:
            cs = iref.case(name)
        _CASES[name] = cs
    return _CASES[name]


def _options(cs, schur_impl, **kw):
    return capi.default_options(schur_impl=schur_impl, huber_delta=cs["a"] if cs["loss"] != "none" else 0.0, loss_type=1 if cs["loss"] == "cauchy" else 0, **kw)


def _problem(cs, masks="case"):
    pr = capi.Problem.marker_chain(cs["prob"], capi.MODEL_MARKER_CHAIN_TEST2 if cs["variant"] == 1 else capi.MODEL_MARKER_CHAIN)
    for b in cs["constant_blocks"]:
        pr.set_parameter_block_constant(6 * b)
    if cs["weights"] is not None:
        pr.set_observation_weights(cs["weights"])
    for b, m in cs["pose_masks"].items():
        pr.set_parameter_subset_constant(6 * b, m)
    for b, (A, v) in cs["priors"].items():
        pr.set_block_prior(6 * b, A, v)
    for k, m in enumerate(cs["masks"] if masks == "case" else []):
        if m:
            pr.set_intrinsics_free(k, m)
    return pr


def _extended_state(pr):
    d = pr.distortion
    d = np.zeros((pr.num_cameras, 5)) if d is None else d
    return np.concatenate([pr.params.ravel(), np.concatenate([pr.intrinsics, d[:, :2]], axis=1).ravel()])


def _ref(name, key, xe):
    if (name, key) not in _REFS:
        _REFS[(name, key)] = qref.Queries(_case(name), xe)
    return _REFS[(name, key)]


def _blocks_of(cs, with_times):
    """Offsets of the referenced camera, marker and intrinsics blocks (and the time blocks)."""
    p = cs["prob"]
    C, T, M = p["C"], p["T"], p["M"]
    c, t, m = (np.asarray(p[k]) for k in ("c", "t", "m"))
    cams = sorted(set(c[c != 0].tolist()))
    mars = sorted(set((m if cs["variant"] == 1 else m[m != 0]).tolist()))
    times = sorted(set(t.tolist())) if with_times else []
    intr = sorted(set(c.tolist()))
    return [6 * b for b in cams] + [6 * (C + b) for b in times] + [6 * (C + T + b) for b in mars] + [6 * (C + T + M) + 6 * k for k in intr]


def _session(name, impl):
    """One solver per (case, path), its three states queried once: -> dict(state -> dict(xe, cost, r, g, cov, ...))."""
    if (name, impl) in _SESSIONS:
        return _SESSIONS[(name, impl)]
    cs = _case(name)
    out = {}
    pr = _problem(cs)
    try:
        s = capi.Solver(pr, _options(cs, impl))
        try:
            assert s.eliminates_times() == (1 if impl == 3 else 0)
            s.set_extended_layout(True)
            nx = s.num_extended_parameters()
            assert nx == pr.num_parameters + 6 * pr.num_cameras

            def query(xe):
                cost, r, g = s.evaluate()
                again = s.evaluate()
                assert (cost, r.tobytes(), g.tobytes()) == (again[0], again[1].tobytes(), again[2].tobytes()), "two calls, two answers"
                assert g.shape == (nx,)
                only = s.evaluate(residuals=False, gradient=False)
                assert only[0] == cost and only[1] is None and only[2] is None
                offs = _blocks_of(cs, with_times=impl != 3)
                s.covariance_compute()
                pairs = [(a, b) for a in offs for b in offs]
                blocks = s.covariance_blocks(pairs)
                d = dict(xe=xe, cost=cost, r=r, g=g, offs=offs, cov={p: b for p, b in zip(pairs, blocks)})
                d["single"] = s.covariance_block(offs[0], offs[-1]) if impl == 3 else None
                d["times"] = s.time_covariances() if impl != 3 else None
                return d

            out["start"] = query(qref.extended_x0(cs))
            summ = s.run()
            s.download()
            out["run"] = query(_extended_state(pr))
            out["run"]["final_costs"] = s.final_costs()
            out["run"]["summary"] = summ
            xp = qref.perturbed(cs)
            s.set_parameters(xp)
            out["set"] = query(xp)
        finally:
            s.close()
    finally:
        pr.close()
    _SESSIONS[(name, impl)] = out
    return out


# ------------------------------------------------------------------------------------------------ 1. evaluate
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", NAMES)
def test_evaluate_matches_the_reference(name, impl):
    ses = _session(name, impl)
    worst = [0.0, 0.0, 0.0]
    for state in ("start", "run", "set"):
        d = ses[state]
        q = _ref(name, state if state != "run" else (state, impl), d["xe"])
        rbar = q.rbar()
        r_ref, g_ref = q.residuals(), q.gradient()
        assert d["r"].shape == r_ref.shape and d["g"].shape == g_ref.shape == (q.next,)
        rerr = np.abs(d["r"] - r_ref).max() / rbar
        gbar = q.gradient_bars(rbar)
        comp = q.computed()
        assert d["g"][~comp].tobytes() == np.zeros(int((~comp).sum())).tobytes(), "a slot that is zero by definition is not +0.0"
        gerr = (np.abs(d["g"] - g_ref)[comp] / gbar[comp]).max()
        cerr = abs(d["cost"] - q.cost()) / q.cost_bar(rbar)
        worst = [max(a, b) for a, b in zip(worst, (rerr, gerr, cerr))]
        assert rerr <= 1.0 and gerr <= 1.0 and cerr <= 1.0, (state, rerr, gerr, cerr)
        # every intrinsics slot is covered: computed ones above, the others as bits
        assert comp[q.npar:].reshape(-1, 6).tolist() == [[bool((m >> c) & 1) for c in range(6)] for m in _case(name)["masks"]]
        if state == "run":
            assert abs(d["cost"] - d["final_costs"][0]) <= q.cost_bar(rbar), (d["cost"], d["final_costs"])
    print("EVALINTR %s impl %d: d_r %.2e rbar %.2e; largest error / bar: residuals %.3f gradient %.3f cost %.3f (d_r: float64 against longdouble)" % (
        name, impl, q.raw_rounding(), rbar, *worst))


@pytest.mark.parametrize("name", NAMES)
def test_both_paths_return_identical_bits_at_identical_values(name):
    a, b = _session(name, 1), _session(name, 3)
    for state in ("start", "set"):
        assert a[state]["cost"] == b[state]["cost"] and a[state]["r"].tobytes() == b[state]["r"].tobytes() and a[state]["g"].tobytes() == b[state]["g"].tobytes(), state


# ------------------------------------------------------------------------------------------------ 2. two product paths
@pytest.mark.parametrize("name", ["3x12x4_3f", "3x70x5_mixed_all"])
def test_residuals_equal_those_of_a_solver_without_masks_at_the_same_values(name):
    cs = _case(name)
    xp = qref.perturbed(cs)
    at = qref.case_at(cs, xp)
    pr = _problem(at, masks=None)
    try:
        s = capi.Solver(pr, _options(cs, 1))
        try:
            with pytest.raises(capi.RsbaError) as e:
                s.set_extended_layout(True)          # no free intrinsics: no state slot
            assert e.value.code == capi.ERR_UNSUPPORTED
            cost, r, _ = s.evaluate()
        finally:
            s.close()
    finally:
        pr.close()
    rbar = _ref(name, "set", xp).rbar()
    for impl in IMPLS:
        d = _session(name, impl)["set"]
        err = np.abs(d["r"] - r).max()
        print("CROSS %s impl %d: %.2e (rbar %.2e)" % (name, impl, err, rbar))
        assert err <= rbar and abs(d["cost"] - cost) <= _ref(name, "set", xp).cost_bar(rbar)


# ------------------------------------------------------------------------------------------------ 3. set and re-solve
def _run_bits(pr, s):
    """The log and everything rsba_solver_download writes: the parameters, the whole intrinsics array and the whole distortion
    array (the state's six values of every camera, p1 p2 k3 as the problem had them), the summary."""
    summ = s.run()
    s.download()
    d = pr.distortion
    d = np.zeros((pr.num_cameras, 5)) if d is None else d
    return (s.iterations().tobytes(), pr.params.tobytes(), pr.intrinsics.tobytes(), d.tobytes(), (summ.termination_type, summ.num_iterations, summ.final_cost))


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", NAMES)
def test_set_then_run_gives_the_bits_of_a_solver_created_there(name, impl):
    cs = _case(name)
    xp = qref.perturbed(cs)
    pr = _problem(cs)
    try:
        s = capi.Solver(pr, _options(cs, impl))
        try:
            s.set_extended_layout(True)
            with pytest.raises(ValueError):
                s.set_parameters(xp[:pr.num_parameters])
            bad = xp.copy()
            bad[-1] = np.nan
            with pytest.raises(capi.RsbaError) as e:
                s.set_parameters(bad)
            assert e.value.code == capi.ERR_ARG
            s.set_parameters(xp)
            got = _run_bits(pr, s)
        finally:
            s.close()
    finally:
        pr.close()
    at = qref.case_at(cs, xp)
    pr = _problem(at)
    try:
        if not np.asarray(at["dist"]).any():
            pytest.fail("the perturbation left no coefficient")
        s = capi.Solver(pr, _options(cs, impl))
        try:
            want = _run_bits(pr, s)
        finally:
            s.close()
    finally:
        pr.close()
    assert got == want
    assert got[4][1] >= 1


# ------------------------------------------------------------------------------------------------ 4. covariance
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", NAMES)
def test_covariance_matches_the_reference(name, impl):
    ses = _session(name, impl)
    cs = _case(name)
    worst, worst_ref = 0.0, 0.0
    for state in ("start", "run", "set"):
        d = ses[state]
        q = _ref(name, state if state != "run" else (state, impl), d["xe"])
        Ca, Cb = q.covariance("inv"), q.covariance("chol")
        offs = d["offs"]
        assert any(o >= q.npar for o in offs) and len(offs) >= 4
        for a in offs:
            for b in offs:
                ra, rb = q.block(Ca, a, b), q.block(Cb, a, b)
                got = d["cov"][(a, b)]
                top = np.abs(ra).max()
                assert d["cov"][(b, a)].tobytes() == np.ascontiguousarray(got.T).tobytes(), (a, b)
                if top == 0.0:      # a constant block or a camera with mask 0
                    assert got.tobytes() == np.zeros((6, 6)).tobytes(), (state, a, b)
                    continue
                worst_ref = max(worst_ref, np.abs(ra - rb).max() / top)
                assert np.abs(ra - rb).max() <= 1e-9 * top, "the reference itself is not stable here: %s %d %d" % (state, a, b)
                worst = max(worst, np.abs(got - ra).max() / (1e-8 * top))
                ha, hb = q.held6(a), q.held6(b)
                assert got[ha].tobytes() == np.zeros((int(ha.sum()), 6)).tobytes() and got[:, hb].tobytes() == np.zeros((6, int(hb.sum()))).tobytes(), (state, a, b)
        if d["single"] is not None:
            assert d["single"].tobytes() == d["cov"][(offs[0], offs[-1])].tobytes()
        if d["times"] is not None:
            p = cs["prob"]
            for t in range(p["T"]):
                o = 6 * (p["C"] + t)
                want = d["cov"][(o, o)] if o in offs else np.zeros((6, 6))
                assert d["times"][t].tobytes() == want.tobytes(), t
    print("COVINTR %s impl %d: largest error / bar %.3f (bar: 1e-8 of the block's largest entry); reference inv against Cholesky %.2e (condition: 1e-9)" % (
        name, impl, worst, worst_ref))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 5. rank deficiency
@pytest.mark.parametrize("impl", IMPLS)
def test_unobservable_intrinsics_are_reported_not_inverted(impl):
    """2 cameras, 1 time, 1 marker, both masks 0x3F: camera 1's pose, the time and two intrinsics blocks are 24 kept unknowns against
    16 residuals — singular by counting."""
    cs = _rig_case(2, 1, 1, [0x3F, 0x3F])
    assert cs["prob"]["N"] == 2
    opts = dict(max_num_iterations=3)
    outs = []
    for attempt in (False, True):
        pr = _problem(cs)
        try:
            s = capi.Solver(pr, _options(cs, impl, **opts))
            try:
                s.set_extended_layout(True)
                if attempt:
                    with pytest.raises(capi.RsbaError) as e:
                        s.covariance_compute(min_reciprocal_condition_number=1e-10)
                    assert e.value.code == capi.ERR_RANK_DEFICIENT
                    with pytest.raises(capi.RsbaError) as e:
                        s.covariance_block(s.intrinsics_offset(0), s.intrinsics_offset(0))
                    assert e.value.code == capi.ERR_ARG
                outs.append(_run_bits(pr, s))
            finally:
                s.close()
        finally:
            pr.close()
    assert outs[0] == outs[1]


# ------------------------------------------------------------------------------------------------ 6. non-interference
@pytest.mark.parametrize("impl", IMPLS)
def test_queries_leave_the_run_alone_and_a_result_is_dropped_when_it_should(impl):
    cs = _case("3x70x5_mixed_all")
    outs = []
    for queries in (False, True):
        pr = _problem(cs)
        try:
            s = capi.Solver(pr, _options(cs, impl))
            try:
                first = _run_bits(pr, s)
                if queries:
                    s.set_extended_layout(True)
                    s.evaluate()
                    s.covariance_compute()
                    i0 = s.intrinsics_offset(0)
                    kept = s.covariance_block(i0, i0)
                second = _run_bits(pr, s)
                outs.append((first, second))
                if queries:
                    assert s.covariance_block(i0, i0).tobytes() == kept.tobytes()      # survives a run
                    s.set_parameters(qref.extended_x0(cs))
                    with pytest.raises(capi.RsbaError) as e:
                        s.covariance_block(i0, i0)
                    assert e.value.code == capi.ERR_ARG
                    s.covariance_compute()
                    s.covariance_block(i0, i0)
                    s.set_extended_layout(False)
                    with pytest.raises(capi.RsbaError) as e:
                        s.covariance_block(6, 6)
                    assert e.value.code == capi.ERR_ARG
            finally:
                s.close()
        finally:
            pr.close()
    assert outs[0] == outs[1] and outs[0][0] == outs[0][1]


# ------------------------------------------------------------------------------------------------ 7. refusals and defaults
def _refused(call, code):
    with pytest.raises(capi.RsbaError) as e:
        call()
    assert e.value.code == code, (e.value.code, code)


@pytest.mark.parametrize("impl", IMPLS)
def test_refusals_and_defaults(impl):
    cs = _case("3x12x4_0f")
    pr = _problem(cs)
    try:
        s = capi.Solver(pr, _options(cs, impl))
        try:
            nx = s.num_extended_parameters()
            for call in (lambda: s.evaluate(), lambda: s.evaluate_jacobian(), lambda: s.jacobian_structure(), lambda: s.covariance_compute(),
                         lambda: s.set_parameters(pr.params.copy())):
                _refused(call, capi.ERR_UNSUPPORTED)                   # the layout is off by default
            s.set_extended_layout(True)
            _refused(lambda: s.evaluate_jacobian(), capi.ERR_UNSUPPORTED)
            _refused(lambda: s.jacobian_structure(), capi.ERR_UNSUPPORTED)
            s.covariance_compute()
            i1 = s.intrinsics_offset(1)
            assert i1 == pr.num_parameters + 6
            _refused(lambda: s.covariance_blocks([(i1 + 1, i1)]), capi.ERR_ARG)       # starts no block
            _refused(lambda: s.covariance_blocks([(nx, i1)]), capi.ERR_ARG)           # behind the last block
            _refused(lambda: s.covariance_block(i1, nx), capi.ERR_ARG)
            t0 = s.time_offset(0)
            if impl == 3:
                _refused(lambda: s.covariance_blocks([(t0, i1)]), capi.ERR_UNSUPPORTED)
                _refused(lambda: s.covariance_blocks([(t0, t0)]), capi.ERR_UNSUPPORTED)
                _refused(lambda: s.time_covariances(), capi.ERR_UNSUPPORTED)
            else:
                assert np.abs(s.covariance_blocks([(t0, i1)])[0]).max() > 0 and s.time_covariances().any()
            s.set_extended_layout(False)
            _refused(lambda: s.evaluate(), capi.ERR_UNSUPPORTED)
        finally:
            s.close()
    finally:
        pr.close()


def test_the_layout_is_refused_where_there_is_no_state_slot():
    pp = capi.Problem.points(synthetic.make_problem(3, 20, 3, seed=1))
    try:
        s = capi.Solver(pp, capi.default_options())
        try:
            _refused(lambda: s.set_extended_layout(True), capi.ERR_UNSUPPORTED)
            _refused(lambda: s.set_extended_layout(False), capi.ERR_UNSUPPORTED)
            assert s.num_extended_parameters() == pp.num_parameters
        finally:
            s.close()
    finally:
        pp.close()
    cs = _case("3x12x4_0f")
    pr = _problem(cs, masks=None)
    try:
        s = capi.Solver(pr, _options(cs, 1))
        try:
            _refused(lambda: s.set_extended_layout(True), capi.ERR_UNSUPPORTED)
            s.evaluate()                                                 # and it answers as it always did
        finally:
            s.close()
    finally:
        pr.close()


@pytest.mark.parametrize("impl", IMPLS)
def test_a_camera_no_observation_names(impl):
    """Camera 2's observations dropped, its mask 0: its intrinsics slot exists, its gradient is 0.0, its covariance block ERR_ARG."""
    cs = dict(_case("3x12x4_3f"))
    prob = cs["prob"]
    keep = np.asarray(prob["c"]) != 2
    cs["prob"] = dict(prob, N=int(keep.sum()), t=prob["t"][keep], c=prob["c"][keep], m=prob["m"][keep], obs=np.asarray(prob["obs"])[keep])
    cs["masks"] = [0x3F, 0x3F, 0]
    pr = _problem(cs)
    try:
        s = capi.Solver(pr, _options(cs, impl))
        try:
            s.set_extended_layout(True)
            _, _, g = s.evaluate()
            i2 = s.intrinsics_offset(2)
            assert g[i2:i2 + 6].tobytes() == np.zeros(6).tobytes() and g[12:18].tobytes() == np.zeros(6).tobytes()
            assert g[s.intrinsics_offset(0):s.intrinsics_offset(0) + 6].all()
            s.covariance_compute()
            i0 = s.intrinsics_offset(0)
            assert np.abs(s.covariance_blocks([(i0, i0)])[0]).max() > 0
            _refused(lambda: s.covariance_blocks([(i2, i0)]), capi.ERR_ARG)
            _refused(lambda: s.covariance_block(i0, i2), capi.ERR_ARG)
        finally:
            s.close()
    finally:
        pr.close()
