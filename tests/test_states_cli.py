"""CPU tier: `ibdgem --states` (the IBD-state path of every comparison, found inside its output job) through the
no-device non-LD path, and `hiddengem --summary-list`.

Bar: a *.hiddengem.txt is byte for byte what `hiddengem -s` prints for the same run's *.summary.txt -- this
project's program, the committed golden (tests/golden/states, written by the reference programs through
make_golden_states.py) and, where oracle/_ref/hiddengem exists, the reference binary itself; ibdstates.txt and
--fractions are the rows and totals of the reference's bin/sum-hiddengem.py."""
import gzip
import json
import os
import subprocess

import pytest

import golden_io as G
import pileup_list_util as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")
# IBDGEM_EXE / HIDDENGEM_EXE: other builds of the two programs (tests/test_states_asan.py: the sanitizer builds)
IBDGEM = os.environ.get("IBDGEM_EXE") or os.path.join(HOST, "ibdgem")
HIDDENGEM = os.environ.get("HIDDENGEM_EXE") or os.path.join(HOST, "hiddengem")
REF = os.path.join(REPO, "oracle", "_ref", "hiddengem")
STATES = os.path.join(G.GOLD, "states")
FIX_IN = os.path.join(G.GOLD, "ibdgem-test", "input")
FIX_PANEL = ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv"]
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", IBDGEM_KEEP_TEARDOWN="1")
HEAD = "# SEGMENT\tSTART\tEND\tLIBD0\tLIBD1\tLIBD2\tNUM_SITES\n"
STATES_HEADER = b"# ID\tN_SEGMENTS\tN_IBD0\tN_IBD1\tN_IBD2\tFRAC_IBD0\tFRAC_IBD1\tFRAC_IBD2\n"
FRAC_HEADER = b"CHROM\tN_SEGMENTS\tN_IBD0\tN_IBD1\tN_IBD2\tFRAC_IBD0\tFRAC_IBD1\tFRAC_IBD2\n"


@pytest.fixture(scope="module", autouse=True)
def programs():
    if not os.environ.get("IBDGEM_EXE"):
        subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
        subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)


def meta():
    with open(os.path.join(STATES, "states.json")) as fh:
        return json.load(fh)


def ibdgem(args, out, cwd=FIX_IN, expect_ok=True):
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([IBDGEM] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, env=NO_DEVICE)
    if expect_ok:
        assert res.returncode == 0, res.stderr
    return res


def hiddengem(*args):
    return subprocess.run([HIDDENGEM, *args], capture_output=True)


def fixture_args(k):
    return FIX_PANEL + ["-P", f"test{k}.pileup", "-N", f"sample{k}"]


def golden_states_file(sname, pu):
    """what ibdstates.txt must be: the script's rows and totals under this program's header"""
    data = open(os.path.join(STATES, "fixture", sname, f"{pu}.fractions.txt"), "rb").read()
    assert data.startswith(FRAC_HEADER)
    return STATES_HEADER + data[len(FRAC_HEADER):]


def check_states_agree_with_paths(states, paths):
    """ibdstates.txt against the three '#% IBDk (n = ...)' lines of each individual's path file, in order"""
    lines = states.decode().splitlines()
    rows = [l.split("\t") for l in lines[1:-4]]
    assert len(rows) == len(paths)
    tot = [0, 0, 0]
    for row, (ind, path) in zip(rows, paths):
        tail = path.decode().splitlines()[-3:]
        n = [int(t.split("(n = ")[1].split(")")[0]) for t in tail]
        assert row[0] == ind and [int(x) for x in row[1:5]] == [sum(n)] + n, (row, tail)
        for k in range(3):
            assert row[5 + k] == ("%.3f" % (n[k] / sum(n)) if sum(n) else "nan")
            tot[k] += n[k]
    assert lines[-4] == f"# Total segments = {sum(tot)}"
    for k in range(3):
        assert lines[-3 + k] == f"# Total IBD{k} (%) = " + ("%.3f" % (tot[k] / sum(tot) * 100) if sum(tot) else "nan")


@pytest.mark.parametrize("k", [1, 2, 3])
def test_fixture_paths_equal_hiddengem_on_the_runs_own_summaries(k, tmp_path):
    m = meta()
    pu = f"sample{k}"
    ibdgem(fixture_args(k), tmp_path / "plain")
    ibdgem(fixture_args(k) + ["--states"], tmp_path / "st")
    plain, st = U.output_files(tmp_path / "plain"), U.output_files(tmp_path / "st")
    assert set(st) == set(plain) | {f"{pu}.{i}.hiddengem.txt" for i in m["individuals"]} | {f"{pu}.ibdstates.txt"}
    for fn, data in plain.items():                       # the summaries and tables of a run without --states
        assert st[fn] == data, fn
    paths = []
    for ind in m["individuals"]:
        got = st[f"{pu}.{ind}.hiddengem.txt"]
        summ = str(tmp_path / "st" / f"{pu}.{ind}.summary.txt")
        ours = hiddengem("-s", summ)
        assert ours.returncode == 0 and got == ours.stdout, ind
        assert got == open(os.path.join(STATES, "fixture", "default", f"{pu}.{ind}.hiddengem.txt"), "rb").read(), ind
        if os.path.exists(REF):
            assert got == subprocess.run([REF, "-s", summ], capture_output=True).stdout, ind
        paths.append((ind, got))
    states = st[f"{pu}.ibdstates.txt"]
    assert states == golden_states_file("default", pu)
    check_states_agree_with_paths(states, paths)


def test_penalties_and_the_modes_that_leave_files_out(tmp_path):
    m = meta()
    pen = m["sets"]["pen"]
    ibdgem(fixture_args(2) + ["--states"] + pen, tmp_path / "pen")
    st = U.output_files(tmp_path / "pen")
    for ind in m["individuals"]:
        got = st[f"sample2.{ind}.hiddengem.txt"]
        assert got == open(os.path.join(STATES, "fixture", "pen", f"sample2.{ind}.hiddengem.txt"), "rb").read(), ind
        assert got == hiddengem("-s", str(tmp_path / "pen" / f"sample2.{ind}.summary.txt"), *pen).stdout
    assert st["sample2.ibdstates.txt"] == golden_states_file("pen", "sample2")
    # --stats-only --states: the table alone, same bytes
    ibdgem(fixture_args(2) + ["--states", "--stats-only"] + pen, tmp_path / "only")
    assert U.output_files(tmp_path / "only") == {"sample2.ibdstates.txt": st["sample2.ibdstates.txt"]}
    # ... beside the arm statistics
    ibdgem(fixture_args(2) + ["--states", "--stats-only", "--arm-stats", "10,20"] + pen, tmp_path / "both")
    both = U.output_files(tmp_path / "both")
    assert sorted(both) == ["sample2.armstats.txt", "sample2.ibdstates.txt"]
    assert both["sample2.ibdstates.txt"] == st["sample2.ibdstates.txt"]
    # --summary-only --states: everything but the per-site tables
    ibdgem(fixture_args(2) + ["--states", "--summary-only"] + pen, tmp_path / "sum")
    assert U.output_files(tmp_path / "sum") == {fn: d for fn, d in st.items() if not fn.endswith(".tab.txt")}


@pytest.mark.parametrize("slots", ["1", "2"])
def test_fewer_output_slots_give_the_same_files(slots, tmp_path):
    ibdgem(fixture_args(1) + ["--states"], tmp_path / "a")
    os.makedirs(tmp_path / "b")
    res = subprocess.run([IBDGEM] + fixture_args(1) + ["--states", "-O", str(tmp_path / "b")], cwd=FIX_IN, capture_output=True,
                         text=True, env=dict(NO_DEVICE, IBDGEM_OUT_SLOTS=slots))
    assert res.returncode == 0, res.stderr
    assert U.output_files(tmp_path / "a") == U.output_files(tmp_path / "b")


def test_pileup_list_gives_each_entrys_single_run(tmp_path):
    lst = U.write_list(tmp_path / "pileups.txt", [(f"sample{k}", f"test{k}.pileup") for k in (3, 1, 2)])
    res = ibdgem(FIX_PANEL + ["--pileup-list", lst, "--states"], tmp_path / "list")
    got = U.output_files(tmp_path / "list")
    want = {}
    for k in (1, 2, 3):
        ibdgem(fixture_args(k) + ["--states"], tmp_path / f"single{k}")
        want.update(U.output_files(tmp_path / f"single{k}"))
    assert got == want and len(got) == 3 * (3 * 3 + 1)
    running = [l for l in res.stderr.splitlines() if l.startswith("Running ")]
    assert running == [f"Running sample{k}-vs-sample{t} comparison..." for k in (3, 1, 2) for t in (1, 2, 3)]


def test_a_synthetic_case_with_many_windows_and_a_sample_list(tmp_path):
    """window 2 over the synthetic panel: hundreds of windows per individual; IBDGEM_MT_MIN_BYTES=1 sends a table of
    that size through the formatter's team of threads, as a chromosome's table goes by default"""
    meta_a = G.cases("synA")
    args = meta_a["base_args"] + meta_a["cases"]["nonld_all_targets_w2"]
    inp = os.path.join(G.GOLD, "synA", "input")
    os.makedirs(tmp_path / "o")
    res = subprocess.run([IBDGEM] + args + ["--states", "--threads", "5", "-O", str(tmp_path / "o")], cwd=inp, capture_output=True,
                         text=True, env=dict(NO_DEVICE, IBDGEM_MT_MIN_BYTES="1"))
    assert res.returncode == 0, res.stderr
    files = U.output_files(tmp_path / "o")
    paths = []
    for fn in sorted(files):
        if fn.endswith(".summary.txt"):
            ind = fn.split(".")[1]
            got = files[f"UNKWN.{ind}.hiddengem.txt"]
            assert len(got.splitlines()) > 400
            assert got == hiddengem("-s", str(tmp_path / "o" / fn)).stdout
            if os.path.exists(REF):
                assert got == subprocess.run([REF, "-s", str(tmp_path / "o" / fn)], capture_output=True).stdout
            paths.append((ind, got))
    assert len(paths) >= 2
    order = [l.split("\t")[0] for l in files["UNKWN.ibdstates.txt"].decode().splitlines()[1:-4]]
    check_states_agree_with_paths(files["UNKWN.ibdstates.txt"], sorted(paths, key=lambda p: order.index(p[0])))


def test_refusals(tmp_path):
    r = ibdgem(fixture_args(1) + ["--p01", "0.5"], tmp_path / "a", expect_ok=False)
    assert r.returncode == 1 and "--states" in r.stderr and not os.listdir(tmp_path / "a")
    r = ibdgem(fixture_args(1) + ["--p12", "0.5", "--summary-only"], tmp_path / "a", expect_ok=False)
    assert r.returncode == 1 and "--states" in r.stderr
    r = ibdgem(fixture_args(1) + ["--states", "--plan"], tmp_path / "b", expect_ok=False)
    assert r.returncode == 1 and "--plan" in r.stderr and r.stdout == "" and not os.listdir(tmp_path / "b")
    r = ibdgem(fixture_args(1) + ["--stats-only"], tmp_path / "c", expect_ok=False)
    assert r.returncode == 1 and "--arm-stats" in r.stderr
    # a directory that cannot be written stops the run before the first comparison
    missing = tmp_path / "not" / "there"
    r = subprocess.run([IBDGEM] + fixture_args(1) + ["--states", "-O", str(missing)], cwd=FIX_IN, capture_output=True,
                       text=True, env=NO_DEVICE)
    assert r.returncode == 1 and "Cannot open" in r.stderr and "sample1.ibdstates.txt" in r.stderr
    assert "Running " not in r.stderr
    # an individual's path file that cannot be opened: the message names it, the run stops, its stale files are emptied
    out = tmp_path / "d"
    ibdgem(fixture_args(1) + ["--states"], out)
    os.remove(out / "sample1.sample2.hiddengem.txt")
    os.mkdir(out / "sample1.sample2.hiddengem.txt")
    r = ibdgem(fixture_args(1) + ["--states"], out, expect_ok=False)
    assert r.returncode == 1 and "sample1.sample2.hiddengem.txt" in r.stderr and "Cannot open" in r.stderr
    assert (out / "sample1.sample2.summary.txt").stat().st_size == 0
    assert "--states" in subprocess.run([IBDGEM, "-h"], capture_output=True, text=True).stderr


# ---- hiddengem --summary-list ------------------------------------------------------------------------------------

def hidden_cases():
    with open(os.path.join(G.GOLD, "hidden", "cases.json")) as fh:
        return {c["name"]: c for c in json.load(fh)}


def write_summary_list(fn, names):
    cases = hidden_cases()
    with open(fn, "w") as fh:
        for k, n in enumerate(names):
            fh.write(n + ("\t" if k % 2 else "  ") + os.path.join(G.GOLD, cases[n]["input"]) + "\n")
    return str(fn)


@pytest.mark.parametrize("lname", ["default35", "case035", "case036", "case037", "case038"])
def test_summary_list_over_the_golden_cases(lname, tmp_path):
    names = meta()["lists"][lname]
    cases = hidden_cases()
    assert sum(len(v) for v in meta()["lists"].values()) == len(cases) == 39
    args = cases[names[0]]["args"]
    assert all(cases[n]["args"] == args for n in names)
    lst = write_summary_list(tmp_path / "list.txt", names)
    want_frac = open(os.path.join(STATES, "lists", lname + ".fractions.txt"), "rb").read()
    for threads in ("1", "8"):
        out, frac = tmp_path / f"t{threads}", tmp_path / f"frac{threads}.txt"
        out.mkdir()
        r = hiddengem("--summary-list", lst, "--out-dir", str(out), "--fractions", str(frac), "--threads", threads, *args)
        assert r.returncode == 0 and r.stdout == b"" and r.stderr == b"", r.stderr
        assert sorted(os.listdir(out)) == sorted(n + ".hiddengem.txt" for n in names)
        for n in names:
            assert (out / (n + ".hiddengem.txt")).read_bytes() == open(os.path.join(G.GOLD, "hidden", n + ".out"), "rb").read(), n
        assert frac.read_bytes() == want_frac


def test_summary_list_defaults(tmp_path):
    """no --out-dir: the current directory; no --fractions: the tables alone; default threads"""
    lst = write_summary_list(tmp_path / "list.txt", ["case031", "case034"])
    r = subprocess.run([HIDDENGEM, "--summary-list", lst], cwd=tmp_path, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["case031.hiddengem.txt", "case034.hiddengem.txt", "list.txt"]
    assert (tmp_path / "case034.hiddengem.txt").read_bytes() == open(os.path.join(G.GOLD, "hidden", "case034.out"), "rb").read()


def test_summary_list_refusals(tmp_path):
    good = os.path.join(G.GOLD, "hidden", "one_window.summary.txt")
    frac = tmp_path / "frac.txt"

    def run(text, *extra):
        (tmp_path / "l.txt").write_text(text)
        r = subprocess.run([HIDDENGEM, "--summary-list", str(tmp_path / "l.txt"), "--out-dir", str(tmp_path), "--fractions",
                            str(frac), *extra], capture_output=True, text=True)
        assert not frac.exists()
        return r

    r = run(f"a\t{good}\nb\t{good}\na\t{good}\n")
    assert r.returncode == 1 and "line 3" in r.stderr and "'a'" in r.stderr
    r = run(f"a\t{good}\njust_a_name\n")
    assert r.returncode == 1 and "line 2" in r.stderr
    r = run(f"a\t{good}\textra\n")
    assert r.returncode == 1 and "line 1" in r.stderr
    r = run(f"a\t{good}\n\nb\t{good}\n")
    assert r.returncode == 1 and "line 2" in r.stderr
    r = run("")
    assert r.returncode == 1 and "lists no summary file" in r.stderr
    r = run(f"a\t{good}\nb\t{tmp_path / 'missing.summary.txt'}\nc\t{good}\n", "--threads", "3")
    assert r.returncode == 1 and "line 2" in r.stderr and "missing.summary.txt" in r.stderr
    r = subprocess.run([HIDDENGEM, "--summary-list", str(tmp_path / "nope.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Failed to open ")
    r = subprocess.run([HIDDENGEM, "--summary-list", str(tmp_path / "l.txt"), "-s", good], capture_output=True, text=True)
    assert r.returncode == 1 and "--summary-list" in r.stderr and r.stdout == ""
    r = subprocess.run([HIDDENGEM, "-s", good, "--fractions", str(frac)], capture_output=True, text=True)
    assert r.returncode == 1 and "--summary-list" in r.stderr and r.stdout == "" and not frac.exists()
    r = subprocess.run([HIDDENGEM, "-h"], capture_output=True, text=True)
    assert "--summary-list" in r.stderr and "--fractions" in r.stderr


# ---- hand-made tables through the two programs ---------------------------------------------------------------------

def list_equals_single(summary_fn, tmp_path, *args):
    """--summary-list on one file = -s on it; returns the table"""
    (tmp_path / "one.txt").write_text(f"x {summary_fn}\n")
    r = hiddengem("--summary-list", str(tmp_path / "one.txt"), "--out-dir", str(tmp_path), "--fractions",
                  str(tmp_path / "x.frac"), *args)
    assert r.returncode == 0, r.stderr
    single = hiddengem("-s", str(summary_fn), *args)
    assert single.returncode == 0 and (tmp_path / "x.hiddengem.txt").read_bytes() == single.stdout
    return single.stdout


def test_nan_zero_and_skipped_rows(tmp_path):
    rows = ["1\t10\t90\t-nan\t-nan\t1.000000e-12\t100", "2\t100\t190\tnan\t1.000000e-22\tinf\t100",
            "3\t200\t290\t0.000000e+00\t0.000000e+00\t0.000000e+00\t100", "not a row", "4\t300\tx\t1e-3\t1e-9\t1e-9\t12",
            "5\t400\t490\t1.000000e-25\t1.000000e-21\t1.000000e-26\t57", "6\t500\t590\t4.940656e-324\t0.000000e+00\t1.000000e-310\t3"]
    fn = tmp_path / "t.summary.txt"
    fn.write_text(HEAD + "\n".join(rows) + "\n")
    table = list_equals_single(fn, tmp_path).decode().splitlines()
    assert len(table) == 1 + 5 + 3 and [l.split("\t")[0] for l in table[1:6]] == ["1", "2", "3", "4", "5"]
    frac = (tmp_path / "x.frac").read_text().splitlines()
    assert frac[1].split("\t")[:2] == ["x", "5"] and frac[-4] == "# Total segments = 5"
    if os.path.exists(REF):
        assert "\n".join(table) + "\n" == subprocess.run([REF, "-s", str(fn)], capture_output=True, text=True).stdout


def test_a_single_window_and_an_empty_table(tmp_path):
    one = os.path.join(G.GOLD, "hidden", "one_window.summary.txt")
    assert list_equals_single(one, tmp_path) == open(os.path.join(G.GOLD, "hidden", "case031.out"), "rb").read()
    assert (tmp_path / "x.frac").read_text().splitlines()[1] == "x\t1\t0\t1\t0\t0.000\t1.000\t0.000"
    empty = tmp_path / "e.summary.txt"
    empty.write_text(HEAD)
    assert len(list_equals_single(empty, tmp_path).splitlines()) == 4
    assert (tmp_path / "x.frac").read_text().splitlines()[1:] == [
        "x\t0\t0\t0\t0\tnan\tnan\tnan", "# Total segments = 0", "# Total IBD0 (%) = nan", "# Total IBD1 (%) = nan",
        "# Total IBD2 (%) = nan"]


def test_forty_thousand_windows(tmp_path):
    """more windows than the reference's fixed arrays hold: the scores of the first 12288 rows are those of the table
    cut there (tests/test_hiddengem.py), through the list as through -s; a gzip copy gives the same bytes"""
    rows = [f"{i + 1}\t{100 * i}\t{100 * i + 99}\t{10.0 ** -(20 + i % 7):e}\t{10.0 ** -(22 - i % 5):e}\t1e-30\t100\n"
            for i in range(40000)]
    long_fn, cut_fn, gz_fn = tmp_path / "long.summary.txt", tmp_path / "cut.summary.txt", tmp_path / "long.summary.txt.gz"
    long_fn.write_text(HEAD + "".join(rows))
    cut_fn.write_text(HEAD + "".join(rows[:12288]))
    with gzip.open(gz_fn, "wt") as fh:
        fh.write(HEAD + "".join(rows))
    (tmp_path / "l.txt").write_text(f"long {long_fn}\ncut {cut_fn}\ngz {gz_fn}\n")
    r = hiddengem("--summary-list", str(tmp_path / "l.txt"), "--out-dir", str(tmp_path), "--fractions", str(tmp_path / "f.txt"),
                  "--threads", "3")
    assert r.returncode == 0, r.stderr
    la = (tmp_path / "long.hiddengem.txt").read_text().splitlines()
    lb = (tmp_path / "cut.hiddengem.txt").read_text().splitlines()
    assert len(la) == 1 + 40000 + 3 and len(lb) == 1 + 12288 + 3
    assert [l.split("\t")[:4] for l in la[1:12289]] == [l.split("\t")[:4] for l in lb[1:12289]]
    assert (tmp_path / "gz.hiddengem.txt").read_bytes() == (tmp_path / "long.hiddengem.txt").read_bytes()
    assert (tmp_path / "long.hiddengem.txt").read_bytes() == hiddengem("-s", str(long_fn)).stdout
    frac = (tmp_path / "f.txt").read_text().splitlines()
    assert [l.split("\t")[:2] for l in frac[1:4]] == [["long", "40000"], ["cut", "12288"], ["gz", "40000"]]
    assert frac[-4] == "# Total segments = 92288"
    if os.path.exists(REF):
        assert subprocess.run([REF, "-s", str(cut_fn)], capture_output=True).stdout == (tmp_path / "cut.hiddengem.txt").read_bytes()
