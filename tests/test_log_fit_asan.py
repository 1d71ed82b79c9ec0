"""The fit's host twin and its step under AddressSanitizer + UndefinedBehaviorSanitizer: tools/log_fit_asan.cpp, a program of its
own (host code only, no device, nothing loaded into Python), built with the build line at its top -- the sanitizers' runtimes
linked into the program itself, so that it runs in the environment as it is -- and run once.  Any sanitizer report aborts the
program, which fails the test."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fit_twin_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "log_fit_asan")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(REPO, "tools", "log_fit_asan.cpp"),
                    os.path.join(REPO, "ibdgem_amd", "csrc", "ibdg_states_host.cpp")], check=True, cwd=REPO)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert [l.split(":")[0] for l in lines] == ["1 windows", "2 windows", "257 windows", "1279 windows"]
