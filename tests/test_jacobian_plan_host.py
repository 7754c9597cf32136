"""The Jacobian structure plan of csrc/ba_evaluate_plan.cpp (rsba_solver_jacobian_structure, the tables of k_eval_jacobian_*) under the
host sanitizers: it is compiled with -fsanitize=address,undefined together with tests/jacobian_plan_driver.cpp, a stand-alone program
that checks the plan's contracts — row pointers monotone and ending at the number of nonzeros, widths in {0, 3, 6, 9} / {0, 6, 12, 18},
columns ascending and inside the named blocks, every free named block exactly once per row, constant and base blocks absent — on the
hongo indices, a seeded random point shape with an unreferenced camera, an unreferenced point, a constant camera and a constant
point, the empty problem, one observation and an observation all of whose blocks are constant.  The program runs as a child process;
nothing loaded into Python is sanitised."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsensecalibration_amd", "csrc")


def test_jacobian_plan_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "jacobian_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "jacobian_plan_driver.cpp"),
                           os.path.join(CSRC, "ba_evaluate_plan.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "hongo", "correspondence.txt")], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "jacobian plan driver: ok" in r.stdout and "hongo: 68 observations checked" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
