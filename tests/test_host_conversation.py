"""The host program's conversation with the engine, on the CPU: `make -C ibdgem_amd/host stub` links the program against the
recording stand-in of tests/engine_stub instead of the engine library.  Every route through the code that talks to a
context for a comparison individual (site list, batch, look-ahead, statistics, tables, slices, pileup list) is run on the
synA input; the library calls each context saw, with their arguments, and the SHA-256 of every output file must be the ones
in tests/golden/host_conversation/ -- recorded with the host program as it was before that code was restructured
(`python tests/test_host_conversation.py --record` writes them; it is not run again for a change that is meant to keep
the conversation as it is).  The same routes run under AddressSanitizer + UndefinedBehaviorSanitizer, and the ones with
several contexts -- the shard threads -- under ThreadSanitizer; the stand-in is compiled with the same flags, so a buffer
shorter than what the library is entitled to write shows too."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")
INPUT = os.path.join(REPO, "tests", "golden", "synA", "input")
GOLD = os.path.join(REPO, "tests", "golden", "host_conversation")
INPUT_FILES = ["panel.hap.gz", "panel.legend.gz", "panel.indv", "reads.pileup.gz"]
PANEL = ["-H", "panel.hap.gz", "-L", "panel.legend.gz", "-I", "panel.indv"]
ONE = PANEL + ["-P", "reads.pileup.gz"]
LOGS = ["--LD", "--log-stats", "--states", "--posteriors", "--segments", "--arm-stats", "30000,40000", "-w", "16"]


def _ids(n):
    return ["-s", ",".join(f"ind{i}" for i in range(n))]


# name: (arguments, --devices, extra environment)
ROUTES = {
    "default_tables_1ctx": (ONE + _ids(3), "0", {}),
    "default_tables_2ctx": (ONE + _ids(3), "0,0", {}),
    "ld_summary_1ctx": (ONE + ["--LD", "--summary-only", "-w", "16"] + _ids(31), "0", {}),
    "ld_summary_2ctx": (ONE + ["--LD", "--summary-only", "-w", "16"] + _ids(31), "0,0", {}),
    "ld_log_summary_1ctx": (ONE + ["--LD", "--summary-only", "--log-summary", "-w", "16"] + _ids(31), "0", {}),
    "ld_log_summary_2ctx": (ONE + ["--LD", "--summary-only", "--log-summary", "-w", "16"] + _ids(31), "0,0", {}),
    "ld_arm_stats_only_1ctx": (ONE + ["--LD", "--arm-stats", "30000,40000", "--stats-only", "-w", "16"] + _ids(61), "0", {}),
    "ld_arm_stats_only_2ctx": (ONE + ["--LD", "--arm-stats", "30000,40000", "--stats-only", "-w", "16"] + _ids(61), "0,0", {}),
    "log_calls_stats_only_1ctx": (ONE + LOGS + ["--stats-only"] + _ids(31), "0", {}),
    "log_calls_summary_2ctx": (ONE + LOGS + ["--summary-only"] + _ids(31), "0,0", {}),
    "varsites_device_1ctx": (ONE + ["--LD", "-v"] + _ids(3), "0", {}),
    "varsites_host_1ctx": (ONE + ["--LD", "-v"] + _ids(3), "0", {"IBDGEM_VARSITES": "host"}),
    "ld_slices_3ctx": (ONE + ["--LD", "-w", "16"] + _ids(2), "0,0,0", {}),
    "pileup_list_1ctx": (PANEL + ["--LD", "--summary-only", "--pileup-list", "pileups.txt"] + _ids(3), "0", {}),
}
THREADED = [k for k, v in ROUTES.items() if "," in v[1]]
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
           "TSAN_OPTIONS": "halt_on_error=1:exitcode=66"}
_built = set()


def _exe(name):
    if name not in _built:
        subprocess.run(["make", "-C", HOST, name], check=True, stdout=subprocess.DEVNULL)
        _built.add(name)
    return os.path.join(HOST, name)


def converse(exe, route, work):
    """Run one route in `work`; what it left: exit code, messages, each context's calls, each file's SHA-256.  The program is
    started as ./ibdgem beside links to the inputs and writes to ./out, so that the command line its tables echo is fixed."""
    args, devices, extra = ROUTES[route]
    os.makedirs(os.path.join(work, "out"))
    os.makedirs(os.path.join(work, "trace"))
    for fn in INPUT_FILES:
        os.symlink(os.path.join(INPUT, fn), os.path.join(work, fn))
    os.symlink(exe, os.path.join(work, "ibdgem"))
    with open(os.path.join(work, "pileups.txt"), "w") as fh:
        fh.write("first reads.pileup.gz\nsecond reads.pileup.gz\n")
    # (the orderly way out for the plain build too: every build's trace ends with the contexts' destruction)
    env = dict(os.environ, IBDG_STUB_TRACE=os.path.join(work, "trace"), IBDGEM_KEEP_TEARDOWN="1", **SAN_ENV, **extra)
    r = subprocess.run(["./ibdgem"] + args + ["--devices", devices, "--threads", "4", "-O", "out"], cwd=work, env=env,
                       capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr, r.stderr[-4000:]
    traces = []
    for fn in sorted(os.listdir(os.path.join(work, "trace"))):
        with open(os.path.join(work, "trace", fn)) as fh:
            traces.append(fh.read().splitlines())
    files = {}
    for fn in sorted(os.listdir(os.path.join(work, "out"))):
        with open(os.path.join(work, "out", fn), "rb") as fh:
            files[fn] = hashlib.sha256(fh.read()).hexdigest()
    # the contexts beyond the first are created side by side and the shard threads interleave freely: per context, the order
    # of its own calls is what counts
    return {"returncode": r.returncode, "stderr": [l for l in r.stderr.splitlines() if not l.startswith("Run time:")],
            "traces": sorted(traces), "files": files}


def _check(exe_name, route, tmp_path):
    with open(os.path.join(GOLD, route + ".json")) as fh:
        want = json.load(fh)
    got = converse(_exe(exe_name), route, str(tmp_path))
    assert got["returncode"] == want["returncode"] == 0, got["stderr"][-20:]
    assert len(got["traces"]) == len(want["traces"])
    for have, exp in zip(got["traces"], want["traces"]):
        assert have == exp
    assert got["files"] == want["files"]
    assert got["stderr"] == want["stderr"]


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_conversation_is_the_recorded_one(route, tmp_path):
    _check("ibdgem_stub", route, tmp_path)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_conversation_under_asan_and_ubsan(route, tmp_path):
    _check("ibdgem_stub_asan", route, tmp_path)


@pytest.mark.parametrize("route", sorted(THREADED))
def test_shard_threads_under_tsan(route, tmp_path):
    _check("ibdgem_stub_tsan", route, tmp_path)


if __name__ == "__main__":
    import tempfile
    assert sys.argv[1:] == ["--record"], "usage: test_host_conversation.py --record"
    os.makedirs(GOLD, exist_ok=True)
    for name in sorted(ROUTES):
        with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
            rec = converse(_exe("ibdgem_stub"), name, a)
            assert rec == converse(_exe("ibdgem_stub"), name, b), name + ": two runs differ"
            assert rec["returncode"] == 0, rec["stderr"]
        with open(os.path.join(GOLD, name + ".json"), "w") as fh:
            json.dump(rec, fh, indent=0)
            fh.write("\n")
        print(name, len(rec["traces"]), "contexts,", sum(map(len, rec["traces"])), "calls,", len(rec["files"]), "files")
