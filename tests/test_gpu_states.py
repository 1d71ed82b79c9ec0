"""GPU tier: `ibdgem --LD --states` on a device -- the IBD-state path of every comparison individual, found on the host
inside the individual's output job from the window table the device returned, in every mode a table reaches the host.

Bar: every *.hiddengem.txt is byte for byte what `hiddengem -s` prints for the same run's *.summary.txt (this project's
program, and the reference binary where oracle/_ref/hiddengem travelled with the tree); ibdstates.txt agrees with them;
the bytes do not depend on the number of contexts, on --summary-only / --stats-only or on running as a --pileup-list.
Every program runs under its own `timeout -k 10`; a test ends at the first failing exit status."""
import os
import subprocess

import pytest

import golden_io as G
import pileup_list_util as U
from test_states_cli import check_states_agree_with_paths

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")
IBDGEM = os.path.join(HOST, "ibdgem")
HIDDENGEM = os.path.join(HOST, "hiddengem")
REF = os.path.join(REPO, "oracle", "_ref", "hiddengem")
LIMIT = ["timeout", "-k", "10", "300"]


def run(cmd, cwd=None):
    res = subprocess.run(LIMIT + cmd, cwd=cwd, capture_output=True)
    assert res.returncode == 0, (cmd, res.returncode, res.stderr[-3000:])
    return res


def ibdgem(tag, extra, out):
    """the case's whole panel as comparison individuals (no -S / -s)"""
    os.makedirs(out, exist_ok=True)
    run([IBDGEM] + G.cases(tag)["base_args"] + ["--LD"] + extra + ["-O", str(out)], cwd=os.path.join(G.GOLD, tag, "input"))
    return U.output_files(out)


def check_run(files, out, name="UNKWN", pen=(), expect_ref=True):
    """every path file of a run against hiddengem on the run's own summary; ibdstates.txt against them.  Returns the
    path files and the table."""
    states = files[f"{name}.ibdstates.txt"]
    order = [l.split("\t")[0] for l in states.decode().splitlines()[1:-4]]
    summaries = [fn for fn in files if fn.startswith(name + ".") and fn.endswith(".summary.txt")]
    assert sorted(fn.split(".")[1] for fn in summaries) == sorted(order) and len(order) >= 60
    paths = {}
    for ind in order:
        got = files[f"{name}.{ind}.hiddengem.txt"]
        summ = str(out / f"{name}.{ind}.summary.txt")
        assert got == run([HIDDENGEM, "-s", summ, *pen]).stdout, ind
        if os.path.exists(REF):
            assert got == run([REF, "-s", summ, *pen]).stdout, ind
        paths[ind] = got
    check_states_agree_with_paths(states, [(ind, paths[ind]) for ind in order])
    return paths, states


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """synA / synV, whole panel, one context: checked once, the runs below are compared with it"""
    made = {}
    for tag in ("synA", "synV"):
        out = tmp_path_factory.mktemp(tag)
        files = ibdgem(tag, ["--states"], out)
        made[tag] = (files,) + check_run(files, out)
    return made


@pytest.mark.parametrize("tag", ["synA", "synV"])
def test_whole_panel_paths_equal_hiddengem_on_the_runs_summaries(base, tag):
    files, paths, states = base[tag]
    n = len(paths)
    assert len(files) == 3 * n + 1
    assert len({p for p in paths.values()}) > 1              # (the individuals' paths are not all the same table)
    print(f"{tag}: {n} individuals, reference binary {'present' if os.path.exists(REF) else 'absent'}")


@pytest.mark.parametrize("tag", ["synA", "synV"])
@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
def test_same_bytes_over_several_contexts(base, tag, devices, tmp_path):
    files = ibdgem(tag, ["--states", "--devices", devices], tmp_path)
    want = base[tag][0]
    assert sorted(files) == sorted(want)
    check_run(files, tmp_path)
    for fn in want:                                          # (a window's values do not depend on where the site list is cut)
        if not fn.endswith(".tab.txt"):
            assert files[fn] == want[fn], fn


@pytest.mark.parametrize("tag", ["synA", "synV"])
def test_same_bytes_with_summary_only_and_stats_only(base, tag, tmp_path):
    want = base[tag][0]
    files = ibdgem(tag, ["--states", "--summary-only"], tmp_path / "sum")
    assert files == {fn: d for fn, d in want.items() if not fn.endswith(".tab.txt")}
    only = ibdgem(tag, ["--states", "--stats-only"], tmp_path / "only")
    assert only == {"UNKWN.ibdstates.txt": want["UNKWN.ibdstates.txt"]}
    both = ibdgem(tag, ["--states", "--stats-only", "--arm-stats", "20000,30000", "--devices", "0,0"], tmp_path / "both")
    assert sorted(both) == ["UNKWN.armstats.txt", "UNKWN.ibdstates.txt"]
    two = ibdgem(tag, ["--states", "--summary-only", "--devices", "0,0"], tmp_path / "two")
    check_run(two, tmp_path / "two")
    assert both["UNKWN.ibdstates.txt"] == two["UNKWN.ibdstates.txt"]


def test_reference_order_and_other_penalties(tmp_path):
    pen = ["--p01", "0.5", "--p02", "0.25", "--p12", "0.9"]
    files = ibdgem("synA", ["--states", "--reference-order", "--summary-only"] + pen, tmp_path)
    check_run(files, tmp_path, pen=pen)


def test_every_entry_of_a_pileup_list(base, tmp_path):
    paths = U.thinned_pileups("synA", tmp_path, 3)
    names = ["UNKWN", "second", "third"]
    lst = U.write_list(tmp_path / "l.txt", list(zip(names, paths)))
    args = U.strip_pileup_args(G.cases("synA")["base_args"]) + ["--LD", "--states", "--summary-only"]
    inp = os.path.join(G.GOLD, "synA", "input")
    for devices in ("0", "0,0"):
        out = tmp_path / ("list" + devices.replace(",", "_"))
        out.mkdir()
        res = run([IBDGEM] + args + ["--pileup-list", lst, "--devices", devices, "-O", str(out)], cwd=inp)
        running = [l.split()[1].split("-vs-")[0] for l in res.stderr.decode().splitlines() if l.startswith("Running ")]
        assert running == [n for n in names for _ in range(70)]      # messages in list order
        files = U.output_files(out)
        for name in names:
            check_run(files, out, name=name)
        want = base["synA"][0]                               # the first entry is the case's own pileup
        for fn, data in files.items():
            if fn.startswith("UNKWN."):
                assert data == want[fn], fn
        for name, path in zip(names[1:], paths[1:]):          # the others: their single runs
            single = tmp_path / f"single_{name}_{devices.replace(',', '_')}"
            single.mkdir()
            run([IBDGEM] + args + ["-P", path, "-N", name, "-O", str(single)], cwd=inp)
            for fn, data in U.output_files(single).items():
                assert files[fn] == data, fn


def test_windows_that_underflow_and_nan_windows(tmp_path):
    """-e 1e-12 -w 300: LIBD2 of an unrelated individual underflows to 0.000000e+00; a background that holds the compared
    individual alone: LIBD0 / LIBD1 are -nan.  The path is still hiddengem's on that text."""
    files = ibdgem("synA", ["--states", "--summary-only", "-e", "1e-12", "-w", "300"], tmp_path / "under")
    zero = [fn for fn, d in files.items() if fn.endswith(".summary.txt") and b"\t0.000000e+00\t" in d]
    assert len(zero) >= 30
    check_run(files, tmp_path / "under")
    meta = G.cases("synA")
    out = tmp_path / "nan"
    out.mkdir()
    run([IBDGEM] + meta["base_args"] + meta["cases"]["ld_bg_self_nan"] + ["--states", "-O", str(out)],
        cwd=os.path.join(G.GOLD, "synA", "input"))
    files = U.output_files(out)
    assert b"nan" in files["UNKWN.ind3.summary.txt"]
    got = files["UNKWN.ind3.hiddengem.txt"]
    assert got == run([HIDDENGEM, "-s", str(out / "UNKWN.ind3.summary.txt")]).stdout
    if os.path.exists(REF):
        assert got == run([REF, "-s", str(out / "UNKWN.ind3.summary.txt")]).stdout
    check_states_agree_with_paths(files["UNKWN.ibdstates.txt"], [("ind3", got)])
    only = tmp_path / "nan_only"
    only.mkdir()
    run([IBDGEM] + meta["base_args"] + meta["cases"]["ld_bg_self_nan"] + ["--states", "--stats-only", "-O", str(only)],
        cwd=os.path.join(G.GOLD, "synA", "input"))
    assert U.output_files(only) == {"UNKWN.ibdstates.txt": files["UNKWN.ibdstates.txt"]}
