"""LM steps of the point model that FOLLOW a rejected step, on the GPU, held as linear solves (tests/step_sequence.py has the patterns,
the cases and how the public API observes such a step; tests/point_step_accuracy.py the measure and the bar;
tests/test_step_sequence_cpu.py shows the cases' patterns and margins in the reference and six mutations above the bar).

tests/test_gpu_point_step.py holds the first and second ACCEPTED step.  What runs after a rejection is other code: the damping
kernel queued on the device's own decision must damp the KEPT linearisation again (not the candidate's, which the fused
back-substitution has just written), at radius / decrease_factor with the host's doubling factor handed over each step; the buffers
do not flip; after an acceptance the factor is 2 again.  For a pattern of length L ('RA', 'RRA', 'ARA', 'ARRA'; 'AA' on the
scale-visible case) fresh solvers run 1 .. L iterations with min_relative_decrease between the reference's relative decreases:
  1. rows 0 .. k of the longest run equal the k-iteration run's bit for bit, and the flags spell the pattern;
  2. a run that ends on a rejection returns the bits of its base point; a rejected row carries the base point's cost and gradient
     bits, and its radius is the previous row's / 2, / 4 ...: exactly;
  3. every accepted step, the ones behind rejections among them, solves the full damped normal equations at its base point (the
     previous run's x) with the radius the previous row reports and iteration 0's scale, within the derived bar on every free row,
     camera and point rows reported apart; its row's scalars within point_step_accuracy.scalar_checks' tolerances;
  4. the scale-visible cases (min_lm_diagonal = 0.999: the clip is active, iteration 0's scale enters the later systems) hold a
     stale or re-taken Jacobi scale to the same bar;
  5. constant and unreferenced blocks keep their bits, every free block moves with an accepted step, a second solver returns the
     same bits, no stall or fallback.
One child process per setting (tests/point_sequence_worker.py): the defaults with every case, and 'RA' and 'ARRA' on v64 under
RSBA_BACKSUB_PROJ=0, RSBA_FUSED_LIN=0, RSBA_DECIDED_DAMP=0, RSBA_PIPELINE=0 and RSBA_FORCE_COMM=1.  schur_impl = 0 runs 'RA' and 'RRA':
two of its solvers differ in the last bits, so what is compared ACROSS runs there is the iteration, radius and flags of the rows, a
rejected row's cost and gradient lie within the scalars' tolerances of the previous row's, and the only base point known exactly
is x0.  The form of the point back-substitution printed with a case is the one PlanStep's rule predicts for the setting
(point_step_accuracy.expected_form), not an observation: the kernel statistics name all forms alike, as in test_gpu_point_step.py.
Every held step prints case, pattern, step, radius, eta, bar and eta / bar; profiles/step_sequence_backward_error.txt is that
table from an MI355X.

Still held per solve only: a step after an INVALID step (a failed factorisation or a non-positive model cost change), termination."""
import json
import os
import subprocess
import sys

import pytest

import step_sequence as ss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(env, impl, cases):
    child_env = dict(os.environ)
    child_env.update(env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "point_sequence_worker.py"), str(impl)] + cases, env=child_env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res = {}
    for ln in out.stdout.splitlines():
        if ln.startswith("{"):
            r = json.loads(ln)
            res[r["name"]] = r
    return res, out.stderr


def _tag(env, impl):
    return (" ".join("%s=%s" % (k[5:], v) for k, v in sorted(env.items())) or "defaults") + ("" if impl else " schur_impl=0")


@pytest.mark.parametrize("env,impl,cases", ss.POINT_SETTINGS, ids=["%s %s" % (_tag(e, i), c[0]) for e, i, c in ss.POINT_SETTINGS])
def test_steps_behind_rejections_within_their_backward_error_bars(env, impl, cases):
    res, err = _run(env, impl, cases)
    assert "stalled" not in err and "falling back" not in err, err[-3000:]
    failures = []
    for nm in cases:
        assert nm in res, (nm, err[-3000:])
        r = res[nm]
        case = ss.POINT_BY_NAME[nm]
        for h in r["held"]:
            for cls in ("cam", "pt"):
                q = h[cls]
                print("\nPTSEQ %-20s %-24s %-26s %-5s step %d %-3s radius %-12.6g eta %.2e bar %.2e eta/bar %.2e" % (
                    nm, _tag(env, impl), r["form"], case.pattern, h["step"], cls, h["radius"], q["eta"], q["bar"], q["ratio"]), end="")
                if not q["eta"] <= q["bar"]:
                    failures.append("%s: step %d %s rows above the bar: %s" % (nm, h["step"], cls, q))
        print("\n       %s flags %s rho %s (thr %g) %.1f s" % (nm, r.get("flags"), " ".join("%.5f" % v for v in r.get("rho", [])), case.thr, r.get("seconds", 0.0)))
        for k, fig in r["scalars"].items():
            print("       step %s scalars: " % k + "  ".join("%s %.1e" % kv for kv in fig.items()))
        failures += ["%s: %s" % (nm, f) for f in r["failures"]]
        held = [h["step"] for h in r["held"]]
        want = [k + 1 for k, c in enumerate(case.pattern) if c == "A"]
        if held != want:
            failures.append("%s: held steps %s, expected %s" % (nm, held, want))
    assert not failures, "\n".join(failures)
