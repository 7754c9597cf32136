"""The host-only plan of the marker chain's time elimination (csrc/ba_marker_plan.hpp) under the host sanitizers:
tests/marker_plan_driver.cpp, a stand-alone program, is compiled with -fsanitize=address,undefined and run as a child process.  For
every case of tests/marker_step_accuracy.py that eliminates the times the problem's wiring goes to the driver in a text file, the
driver plans it under the case's switches, checks the contracts the kernels rely on (offsets, slots, orders, block lists, flags) and
prints the path and the structure it planned; they are held against marker_step_accuracy.expected_path and structure, the statement
of the rules the GPU tests hold the library's kernel statistics to.  What those cases cannot express — subset masks, priors, n_r = 0,
a constant time, a time without slots, the unsupported returns, 8 CUs, RSBA_MT_CHUNKS against T — the driver builds and checks
itself and exits non-zero on a violation.  Nothing loaded into Python is sanitised."""
import json
import os
import subprocess

import numpy as np
import pytest

import marker_step_accuracy as msa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsensecalibration_amd", "csrc")
SWITCHES = ("RSBA_MT_SPLIT", "RSBA_MT_ACC_MFMA", "RSBA_MT_CHUNKS", "RSBA_MT_BACKSUB_WG", "RSBA_MT_SPLIT_BACKSUB", "RSBA_MT_FORK", "RSBA_MT_SOLVE_LDS",
            "RSBA_CHOL_TILES", "RSBA_DEBUG")   # MarkerSwitches::FromEnv
CASES = [c for c in msa.CASES if c.impl != 0]
CUS = 256   # the driver's chip


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("marker_plan") / "marker_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "marker_plan_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, env, args=()):
    child = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    child.update(env, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=child, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "marker plan driver: ok" in r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    return [json.loads(ln) for ln in r.stdout.splitlines()]


def write_wiring(path, case, subset=(), priors=()):
    """C T M variant loss N | the constant blocks | (block, mask) pairs | the blocks with a prior | camera time marker per observation"""
    prob = msa.problem(case.prob)
    const = msa.constant_blocks(case, prob)
    rows = np.stack([prob["c"], prob["t"], prob["m"]], 1).astype(int)
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d\n" % (prob["C"], prob["T"], prob["M"], case.variant, int(case.loss != "none" or len(priors) > 0), prob["N"]))
        f.write(" ".join(str(v) for v in (len(const),) + tuple(const)) + "\n")
        f.write(" ".join(str(v) for v in (len(subset),) + tuple(x for bm in subset for x in bm)) + "\n")
        f.write(" ".join(str(v) for v in (len(priors),) + tuple(priors)) + "\n")
        f.write("\n".join("%d %d %d" % tuple(r) for r in rows) + "\n")


def check_line(line, case, mc, **rules):
    want = msa.expected_path(case, mc, **rules)
    nr, dmax, pmax, widest = msa.structure(mc)
    assert line["rc"] == 0
    got = {k: line[k] for k in ("elim", "acc", "solve", "backsub")}
    assert got == {k: want[k] for k in got}, (case.name, line, want)
    assert (line["nr"], line["dmax"], line["pmax"], line["widest"], bool(line["loss"])) == (nr, dmax, pmax, widest, want["loss"]), (case.name, line)
    # chunks of times: at most one per CU, or RSBA_MT_CHUNKS, where the chunk sums live in LDS (every accumulation but 'valu_mem')
    if want["acc"] not in ("", "valu_mem"):
        assert 1 <= line["G"] <= min(line["T"], max(1, int(dict(case.env).get("RSBA_MT_CHUNKS", CUS))))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_planned_path_is_the_reference_path(driver, tmp_path, case):
    wiring = str(tmp_path / "wiring.txt")
    write_wiring(wiring, case)
    (line,) = run_driver(driver, dict(case.env), [wiring])
    check_line(line, case, msa.chain(case))


@pytest.mark.parametrize("env", [{}, {"RSBA_MT_SPLIT": "0"}, {"RSBA_MT_SPLIT_BACKSUB": "0", "RSBA_MT_BACKSUB_WG": "1"}], ids=["default", "SPLIT=0", "SPLIT_BACKSUB=0"])
def test_subset_masks_and_priors_keep_the_split_paths(driver, tmp_path, env):
    """The two rules the cases do not carry, through the same file: a subset mask on a free camera, a prior on a free marker."""
    case = next(c for c in CASES if c.name == "switch_8x24x12_default")._replace(env=tuple(sorted(env.items())))
    prob, mc = msa.problem(case.prob), msa.chain(case)
    wiring = str(tmp_path / "wiring.txt")
    write_wiring(wiring, case, subset=[(3, 0b000101)])
    (line,) = run_driver(driver, env, [wiring])
    check_line(line, case, mc, subset=True)
    assert (line["elim"], line["backsub"]) == ("split", "split")
    write_wiring(wiring, case, priors=[prob["C"] + prob["T"] + 2])
    (line,) = run_driver(driver, env, [wiring])
    check_line(line, case, mc, priors=True)
    assert line["elim"] == "split" and line["loss"] == 1 and line["backsub"] == ("split" if not env.get("RSBA_MT_SPLIT_BACKSUB") else "terms")


def test_cases_the_reference_does_not_express(driver):
    assert run_driver(driver, {}) == []
