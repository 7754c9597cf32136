"""One and two LM steps of the point model on the GPU, held as linear solves (tests/point_step_accuracy.py has the measure, the
bar's derivation and the case list; tests/test_point_step_accuracy_cpu.py shows the bar is neither vacuous nor false).

Whole solves hide an inexact step: Levenberg-Marquardt corrects it.  tests/test_gpu_reduced_solve.py holds the step as far as the
reduced camera system; here the rest of it — the point back-substitution in its three forms and every template instance of the
projective one, with view counts mixed inside a slice so that padding lanes sit beside valid ones and the register, LDS and
streamed slots are all walked; the second trip of its slice loop; and what it leaves for the NEXT step (the candidate's V, g_p
and sqrt(rho'), the fix for constant points, the damping kernel queued on the device's decision) — is held through the public API:
  1. x1 - x0 solves the full damped normal equations of the numpy reference within the derived bar on every free row, camera and
     point rows reported apart; the scalars of log rows 0 and 1 within marker_step_accuracy.py's tolerances;
  2. (schur_impl = 1) a two-step run's rows 0 and 1 equal the one-step run's bit for bit, so it went through the same x1; x2 - x1
     is then held to the system at x1 with the radius the log gives and iteration 0's scale, and its scalars likewise;
  3. constant cameras, constant points and unreferenced points keep their bits through both steps, every other block moved, a second
     one-step solver returns the same bits, no stall or fallback.
One child process per setting (tests/point_step_worker.py).  Every case prints the form PlanStep picks for it (stated from the rule
tests/test_step_plan_host.py holds: the kernel statistics name all forms alike), n, m, kappa, and eta, bar and eta / bar of both
row classes and steps; profiles/point_step_backward_error.txt is that table from an MI355X.

A step after a REJECTED one, and the radius updates behind it, are observable through the public API too (min_relative_decrease set
between the reference's relative decreases): tests/test_gpu_point_sequence.py holds them.  Still held per solve only: a step after an
INVALID one (a failed factorisation or a non-positive model cost change), termination."""
import json
import os
import subprocess
import sys

import pytest

import point_step_accuracy as psa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(env, impl, cases):
    child_env = dict(os.environ)
    child_env.update(env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "point_step_worker.py"), str(impl)] + cases, env=child_env,
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


def _line(tag, r):
    s = "PTSTEP %-16s %-34s %-28s n %6d m %5d kappa_s %8.3g kappa_p %8.3g |" % (r["name"], tag, r["form"], r["n"], r["m"], r["kappa_s"], r["kappa_p"])
    for step in ("step1", "step2"):
        if step in r:
            for cls in ("cam", "pt"):
                q = r[step][cls]
                s += " %s %s eta %.2e bar %.2e eta/bar %.2e |" % (step[-1], cls, q["eta"], q["bar"], q["ratio"])
    return s


@pytest.mark.parametrize("env,impl,cases", psa.SETTINGS, ids=["%s %s" % (_tag(e, i), c[0]) for e, i, c in psa.SETTINGS])
def test_steps_within_their_backward_error_bars(env, impl, cases):
    res, err = _run(env, impl, cases)
    assert "stalled" not in err and "falling back" not in err, err[-3000:]
    failures = []
    for nm in cases:
        assert nm in res, (nm, err[-3000:])
        r = res[nm]
        print("\n" + _line(_tag(env, impl), r))
        for step in ("scalars1", "scalars2"):
            if step in r:
                print("       %s: " % step + "  ".join("%s %.1e" % kv for kv in r[step].items()))
        print("       worst rows: " + "; ".join("%s %s: %s" % (st, cls, r[st][cls]["row"]) for st in ("step1", "step2") if st in r for cls in ("cam", "pt")))
        failures += ["%s: %s" % (nm, f) for f in r["failures"]]
        steps = ("step1",) if impl == 0 else ("step1", "step2")
        for st in steps:
            if st not in r:
                failures.append("%s: %s was not measured" % (nm, st))
                continue
            for cls in ("cam", "pt"):
                if not r[st][cls]["eta"] <= r[st][cls]["bar"]:
                    failures.append("%s: %s %s rows above the bar: %s" % (nm, st, cls, r[st][cls]))
    assert not failures, "\n".join(failures)
