"""--pileup-list: several pileups against one panel in one run (CPU tier: --plan and the no-device non-LD path).

For every entry the run must write what `ibdgem <same options> -P PATH -N NAME` writes, and print that run's
per-pileup messages, in list order.  The device tier is tests/test_gpu_pileup_list.py."""
import os
import subprocess

import pytest

import golden_io as G
import pileup_list_util as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")
EXE = os.path.join(HOST, "ibdgem")
FIX_IN = os.path.join(G.GOLD, "ibdgem-test", "input")
FIX_OUT = os.path.join(G.GOLD, "ibdgem-test", "output")
FIX_PANEL = ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv"]
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST, "ibdgem"], check=True, stdout=subprocess.DEVNULL)
    return EXE


def _fixture_list(tmp_path, entries=((1, "test1.pileup"), (2, "test2.pileup"), (3, "test3.pileup"))):
    return U.write_list(tmp_path / "pileups.txt", [(f"sample{k}", p) for k, p in entries])


def _check_fixture_files(out_dir, samples):
    got = U.output_files(out_dir)
    want = {f"sample{k}.sample{t}.{kind}.txt" for k in samples for t in (1, 2, 3) for kind in ("tab", "summary")}
    assert set(got) == want
    for fn, data in got.items():
        ref = open(os.path.join(FIX_OUT, fn), "rb").read()
        if fn.endswith(".tab.txt"):
            ref = ref.split(b"\n", 1)[1]
        assert data == ref, fn


def test_one_list_run_writes_all_files_of_the_reference_fixture(exe, tmp_path):
    """The reference's own test (three pileups, one panel, three invocations) as one run without a device: all 18
    files byte for byte from line 2 of the tab files on, summary files whole; messages in list order."""
    lst = _fixture_list(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    r = U.run(exe, FIX_PANEL + ["--pileup-list", lst, "-O", str(out)], FIX_IN, env=NO_DEVICE)
    assert r.returncode == 0, r.stderr
    _check_fixture_files(out, (1, 2, 3))
    running = [l for l in r.stderr.splitlines() if l.startswith("Running ")]
    assert running == [f"Running sample{k}-vs-sample{t} comparison..." for k in (1, 2, 3) for t in (1, 2, 3)]
    assert r.stderr.count("computed on the host") == 1


def test_list_messages_equal_the_single_runs_in_list_order(exe, tmp_path):
    """per-pileup stderr (here: the -D message and the comparisons) is each single run's, in list order"""
    lst = _fixture_list(tmp_path, ((2, "test2.pileup"), (1, "test1.pileup")))
    args = FIX_PANEL + ["-D", "50", "--plan"]
    r = U.run(exe, args + ["--pileup-list", lst], FIX_IN)
    assert r.returncode == 0, r.stderr
    want_err, want_out = [], ""
    for k in (2, 1):
        s = U.run(exe, args + ["-P", f"test{k}.pileup", "-N", f"sample{k}"], FIX_IN)
        assert s.returncode == 0, s.stderr
        want_err += [l for l in s.stderr.splitlines() if not l.startswith("Run time")]
        want_out += s.stdout
    assert [l for l in r.stderr.splitlines() if not l.startswith("Run time")] == want_err
    assert "Observed depth is lower than target depth -D" in r.stderr
    assert r.stdout == want_out


PLAN_CASES = ["ld_default", "ld_varsites", "ld_downsample", "ld_positions", "ld_af_file", "ld_bg20_w64", "ld_pu_in_panel",
              "nonld_flags"]


@pytest.mark.parametrize("case", PLAN_CASES)
def test_plan_over_a_list_is_the_single_runs_plans_joined(exe, case, tmp_path):
    meta = G.cases("synA")
    args = U.strip_pileup_args(meta["base_args"] + meta["cases"][case])
    inp = os.path.join(G.GOLD, "synA", "input")
    paths = U.thinned_pileups("synA", tmp_path, 4)
    names = ["ind5", "p1", "ind9", "p3"] if case == "ld_pu_in_panel" else ["p0", "p1", "p2", "p3"]
    lst = U.write_list(tmp_path / "l.txt", list(zip(names, paths)))
    r = U.run(exe, args + ["--plan", "--pileup-list", lst], inp)
    assert r.returncode == 0, r.stderr
    want = ""
    for name, path in zip(names, paths):
        s = U.run(exe, args + ["--plan", "-P", path, "-N", name], inp)
        assert s.returncode == 0, s.stderr
        want += s.stdout
    assert r.stdout == want
    assert r.stdout.count("## PLAN ") == len(names) * r.stdout.count("## PLAN p1 ")


def test_downsampling_restarts_the_read_thinning_stream_per_pileup(exe, tmp_path):
    """-D thins with glibc's rand() stream from its start in every process: one pileup listed three times under three
    names is thinned the same way each time, as three single runs would thin it"""
    meta = G.cases("synA")
    args = U.strip_pileup_args(meta["base_args"] + meta["cases"]["ld_downsample"]) + ["--plan"]
    inp = os.path.join(G.GOLD, "synA", "input")
    lst = U.write_list(tmp_path / "l.txt", [(f"q{k}", "reads.pileup.gz") for k in range(3)])
    r = U.run(exe, args + ["--pileup-list", lst], inp)
    assert r.returncode == 0, r.stderr
    single = U.run(exe, args + ["-P", "reads.pileup.gz", "-N", "q0"], inp)
    assert single.returncode == 0
    parts = r.stdout.split("## PLAN q")
    assert len(parts) == 1 + 3 * 2
    assert r.stdout == single.stdout + single.stdout.replace("## PLAN q0 ", "## PLAN q1 ") + \
        single.stdout.replace("## PLAN q0 ", "## PLAN q2 ")
    assert "cull_p=1.000000" not in single.stdout


@pytest.mark.parametrize("lines,extra,message", [
    (["a test1.pileup"], ["-P", "test1.pileup"], "does not go with -P or -N"),
    (["a test1.pileup"], ["-N", "x"], "does not go with -P or -N"),
    (["# nothing", "", "   "], [], "names no pileup"),
    (["a test1.pileup", "b test2.pileup extra"], [], "Line 2 of the pileup list"),
    (["a test1.pileup", "lonely"], [], "Line 2 of the pileup list"),
    (["a test1.pileup", "# x", "b test2.pileup", "a test3.pileup"], [], "Pileup name 'a' appears twice in the pileup list"),
])
def test_list_refusals(exe, tmp_path, lines, extra, message):
    """refused with one line and exit status 1 before any genotype file is read (the -H here does not exist)"""
    lst = tmp_path / "l.txt"
    lst.write_text("\n".join(lines) + "\n")
    r = U.run(exe, ["-H", "missing.hap", "-L", "missing.legend", "-I", "missing.indv", "--pileup-list", str(lst)] + extra,
              FIX_IN, env=NO_DEVICE)
    assert r.returncode == 1
    assert message in r.stderr
    assert len(r.stderr.strip().splitlines()) == 1, r.stderr
    if "twice" in message:
        assert "(lines 1 and 4)" in r.stderr


def test_missing_list_file_is_refused(exe, tmp_path):
    r = U.run(exe, FIX_PANEL + ["--pileup-list", str(tmp_path / "nope.txt")], FIX_IN, env=NO_DEVICE)
    assert r.returncode == 1 and "Cannot open the pileup list" in r.stderr


def test_a_failing_entry_stops_the_list(exe, tmp_path):
    """an unsorted pileup in the middle: the message and exit status of its single run; the entry before it is complete,
    neither it nor the one after it leaves a file (and the one after it is never run)"""
    text = open(os.path.join(FIX_IN, "test2.pileup")).read().splitlines(keepends=True)
    bad = tmp_path / "unsorted.pileup"
    bad.write_text("".join([text[1], text[0]] + text[2:]))
    single = U.run(exe, FIX_PANEL + ["-P", str(bad), "-N", "sample2", "-O", str(tmp_path)], FIX_IN, env=NO_DEVICE)
    assert single.returncode == 1 and "mpileup lines not sorted!" in single.stderr
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".txt")]
    lst = _fixture_list(tmp_path, ((1, "test1.pileup"), (2, str(bad)), (3, "test3.pileup")))
    out = tmp_path / "out"
    out.mkdir()
    r = U.run(exe, FIX_PANEL + ["--pileup-list", lst, "-O", str(out)], FIX_IN, env=NO_DEVICE)
    assert r.returncode == single.returncode == 1
    _check_fixture_files(out, (1,))
    assert "Running sample3" not in r.stderr
    tail = r.stderr[r.stderr.index("Running sample1-vs-sample3 comparison..."):]
    assert "mpileup lines not sorted!" in tail and "ERROR parsing Pileup data" in tail


def test_a_missing_pileup_in_the_list(exe, tmp_path):
    lst = _fixture_list(tmp_path, ((1, "test1.pileup"), (2, "no-such.pileup")))
    out = tmp_path / "out"
    out.mkdir()
    r = U.run(exe, FIX_PANEL + ["--pileup-list", lst, "-O", str(out)], FIX_IN, env=NO_DEVICE)
    assert r.returncode == 1 and "Failed to open no-such.pileup." in r.stderr
    _check_fixture_files(out, (1,))


def test_list_run_is_race_free_under_tsan_with_the_panel_cache(exe, tmp_path):
    """ThreadSanitizer build: the fixture as a list with --panel-cache as a FILE (a first run writes it, a second maps it
    from the threads that read the panel's rows: formatters, host arithmetic) and --threads 4, the next pileup read and
    filtered beside the current one's work.  No report; the reference's files."""
    subprocess.run(["make", "-C", HOST, "ibdgem_tsan"], check=True, stdout=subprocess.DEVNULL)
    env = dict(NO_DEVICE, IBDGEM_MT_MIN_BYTES="1", TSAN_OPTIONS="halt_on_error=1:exitcode=66", IBDGEM_KEEP_TEARDOWN="1")
    lst = _fixture_list(tmp_path)
    cache = tmp_path / "panel.cache"
    for k in range(2):
        out = tmp_path / f"out{k}"
        out.mkdir()
        r = U.run(os.path.join(HOST, "ibdgem_tsan"), FIX_PANEL + ["--pileup-list", lst, "--panel-cache", str(cache),
                                                                  "--threads", "4", "-O", str(out)], FIX_IN, env=env)
        assert "ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, r.stderr[-2000:]
        assert cache.exists()
        _check_fixture_files(out, (1, 2, 3))
