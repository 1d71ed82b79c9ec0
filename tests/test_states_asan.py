"""`ibdgem --states` and `hiddengem --summary-list` under AddressSanitizer + UndefinedBehaviorSanitizer: the fixture
runs and the golden lists of tests/test_states_cli.py (and its hand-made tables) against ibdgem_asan / hiddengem_asan,
the same mechanism as tests/test_host_asan.py (IBDGEM_EXE / HIDDENGEM_EXE).  Any sanitizer report aborts the program,
which fails the test that ran it."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")


@pytest.mark.skipif(os.environ.get("IBDGEM_EXE") is not None, reason="already inside the sanitizer rerun")
def test_states_tests_pass_under_asan_and_ubsan():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST, "asan"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ,
               IBDGEM_EXE=os.path.join(HOST, "ibdgem_asan"), HIDDENGEM_EXE=os.path.join(HOST, "hiddengem_asan"),
               # the HIP runtime the engine library pulls in keeps allocations until exit: leak checking off
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "not gpu", "-p", "no:cacheprovider",
                        "tests/test_states_cli.py"], cwd=REPO, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout
