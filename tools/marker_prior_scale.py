"""The cost of Gaussian priors on camera and marker blocks (ceres::NormalPrior) on the marker chain at scale: three configurations of
tools/marker_chain_scale.py, the parent commit's library beside this one's, in one session with the repetitions alternating between
them and their order reversed every other repetition (profiles/marker_prior_scale.jsonl).

    python tools/marker_prior_scale.py PARENT_TREE [reps=6] [shape=8,5000,16] [sigma=0.02] [out=PATH]
        PARENT_TREE: a checkout of the parent commit with its library built (its own tools/marker_chain_scale.py runs there)

One line per configuration: marker_chain_scale's output of the first repetition (the per-kernel times are the solver's own event
timing of a profiled run, profile_kernels = 1), and in front of it `line` (what ran), every repetition's ms_per_iteration, their mean
and their spread (max - min).  Without priors this commit runs the parent's kernels (profiles/marker_prior_kernel_resources.txt): its
difference to the parent is to be read against the PARENT's own spread, which is why the parent is repeated as often as the others.
The priors line is reported, not bounded: a solver with priors runs the loss instances of the kernels (rho(s) = s), as a solver with
observation weights does, plus the two prior kernels.  A child that fails ends the measurement.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
ARGS = [a for a in sys.argv[1:] if "=" not in a]
if len(ARGS) != 1:
    raise SystemExit(__doc__)
PARENT = os.path.abspath(ARGS[0])
REPS = int(KW.get("reps", 6))
SHAPE = KW.get("shape", "8,5000,16").split(",")
SIGMA = KW.get("sigma", "0.02")
NFREE = int(SHAPE[0]) - 1 + int(SHAPE[2]) - 1
CONFIGS = [("parent commit", PARENT, []),
           ("this commit, no priors", ROOT, []),
           ("this commit, priors on all %d free camera / marker blocks" % NFREE, ROOT, ["priors=" + SIGMA])]

results = {name: [] for name, _, _ in CONFIGS}
for rep in range(REPS):
    for name, tree, extra in (CONFIGS if rep % 2 == 0 else CONFIGS[::-1]):   # (no configuration always follows the same neighbour)
        env = dict(os.environ)
        env.pop("RSBA_LIB", None)   # each tree loads its own library
        out = subprocess.run([sys.executable, os.path.join("tools", "marker_chain_scale.py")] + SHAPE + extra, cwd=tree, env=env,
                             stdout=subprocess.PIPE, text=True, timeout=300, check=True).stdout
        results[name].append(json.loads(out.strip().splitlines()[-1]))
        print("repetition %d  %-70s %.4f ms per iteration" % (rep + 1, name, results[name][-1]["ms_per_iteration"]), file=sys.stderr)
lines = []
for name, _, _ in CONFIGS:
    ms = [round(r["ms_per_iteration"], 4) for r in results[name]]
    first = dict(results[name][0])
    first.pop("roofline", None)
    lines.append(json.dumps(dict({"line": name, "ms_per_iteration_repetitions": ms, "ms_per_iteration_mean": round(sum(ms) / len(ms), 4),
                                  "ms_per_iteration_spread": round(max(ms) - min(ms), 4)}, **first)))
text = "\n".join(lines) + "\n"
if "out" in KW:
    open(KW["out"], "w").write(text)
sys.stdout.write(text)
