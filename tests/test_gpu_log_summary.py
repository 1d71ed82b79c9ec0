"""GPU tier: ibdgem --log-summary on the committed synA / synB fixtures.

The logsummary rows carry the summary's columns 1-3 and 7 byte for byte; the three logs lie within the bars of
tests/hp_log_ref.py (plus 5e-7 for the %.6f) of the long-double truths -- the --LD columns from the panel and the run's own
read counts, the others from the committed 17-digit per-site tables --; and the files do not depend on how the run was
made: 1-3 contexts, --summary-only, --pileup-list, IBDGEM_VARSITES=host."""
import os

import numpy as np
import pytest

import golden_io as G
import hp_log_ref as HL
import pileup_list_util as U
from test_log_summary_cli import read_log_summary, tab_truth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
CASES = ["synA/ld_default", "synA/ld_varsites", "synA/nonld_all_targets_w2", "synB/ld_w37"]
_PANELS = {}


def case_args(key):
    tag, case = key.split("/")
    meta = G.cases(tag)
    return tag, case, meta["base_args"] + meta["cases"][case], os.path.join(G.GOLD, tag, "input")


def run(args, cwd, out, env=None):
    os.makedirs(out, exist_ok=True)
    r = U.run(EXE, args + ["-O", str(out)], cwd, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return U.output_files(out)


def logs_of(files):
    return {fn: data for fn, data in files.items() if fn.endswith(".logsummary.txt")}


@pytest.mark.parametrize("key", CASES)
def test_logsummary_against_the_truths(key, tmp_path):
    tag, case, args, inp = case_args(key)
    window = int(args[args.index("-w") + 1]) if "-w" in args else 100
    run(args + ["--log-summary"], inp, tmp_path)
    panel = _PANELS.setdefault(tag, G.load_syn_panel(tag))
    gold = os.path.join(G.GOLD, tag, case)
    stems = sorted(fn[:-len(".tab.txt.gz")] for fn in os.listdir(gold) if fn.endswith(".tab.txt.gz"))
    assert stems and sorted(logs_of(U.output_files(tmp_path))) == [s + ".logsummary.txt" for s in stems]
    for stem in stems:
        got = read_log_summary(str(tmp_path / f"{stem}.logsummary.txt"), str(tmp_path / f"{stem}.summary.txt")).astype(HL.LD)
        s, a = tab_truth(os.path.join(gold, stem + ".tab.txt.gz"), window)         # the 17-digit per-site values
        assert got.shape == s.shape
        cols = (2,) if "--LD" in args else (0, 1, 2)
        for k in cols:
            err = np.abs(got[:, k] - s[:, k])
            assert (err <= 5e-7 + HL.rows_bar(s[:, k], a[:, k])).all(), (stem, k, float(err.max()))
        if "--LD" in args:
            rows = [l.split("\t") for l in G.read_lines(str(tmp_path / f"{stem}.tab.txt")) if l and not l.startswith("#")]
            alle = panel.alleles[[panel.row_of_pos[int(r[2])] for r in rows]]
            nr, na = np.array([int(r[7]) for r in rows]), np.array([int(r[8]) for r in rows])
            tr = HL.ld_log2_truth(alle, nr, na, panel.index(stem.split(".", 1)[1]), window, 0.02, 20)
            for k, key2 in ((0, "log0"), (1, "log1")):
                err = np.abs(got[:, k] - tr[key2])
                assert (err <= 5e-7 + HL.ld_bar(tr[key2], len(panel.names))).all(), (stem, k, float(err.max()))


@pytest.mark.parametrize("key", CASES)
def test_logsummary_does_not_depend_on_how_the_run_was_made(key, tmp_path):
    tag, case, args, inp = case_args(key)
    base = logs_of(run(args + ["--log-summary"], inp, tmp_path / "base"))
    assert base
    ways = {"two contexts": (["--devices", "0,0"], None), "three contexts": (["--devices", "0,0,0"], None),
            "summary only": (["--summary-only"], None)}
    if "-v" in args:
        ways["site lists made on the host"] = ([], dict(os.environ, IBDGEM_VARSITES="host"))
    for i, (what, (extra, env)) in enumerate(ways.items()):
        assert logs_of(run(args + ["--log-summary"] + extra, inp, tmp_path / str(i), env=env)) == base, what


@pytest.mark.parametrize("key", ["synA/ld_default", "synB/ld_w37"])
def test_logsummary_of_a_pileup_list_equals_the_single_runs(key, tmp_path):
    tag, case, args, inp = case_args(key)
    U.thinned_pileups(tag, tmp_path, 3)
    paths = [os.path.join(inp, "reads.pileup.gz")] + [str(tmp_path / (f"{tag}_v{k}.pileup" + (".gz" if k % 2 else ""))) for k in (1, 2)]
    names = ["p0", "p1", "p2"]
    args = U.strip_pileup_args(args) + ["--log-summary"]
    want = {}
    for name, path in zip(names, paths):
        want.update(logs_of(run(args + ["-P", path, "-N", name], inp, tmp_path / "single")))
    lst = U.write_list(tmp_path / "l.txt", list(zip(names, paths)))
    got = logs_of(run(args + ["--pileup-list", lst, "--devices", "0,0"], inp, tmp_path / "list"))
    assert sorted(got) == sorted(want) and len(got) >= 6
    assert got == want


@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_batches_of_individuals_with_summary_only_equal_the_single_runs(devices, tmp_path):
    """31 individuals with --log-summary --summary-only and every log-domain statistic: a batch of 30 whose linear and log2
    tables leave the device in one copy each while the batch of one is queued ahead, on one context and cut over two.  Every
    file of an individual is that of its run alone, byte for byte, and so is its line of every statistics file."""
    import batch_cases as B
    got = B.run(["--log-summary", "--summary-only", "--devices", devices], B.NAMES, tmp_path)
    own = {fn: data for fn, data in got.items() if fn not in B.STATS_FILES}
    want = {fn: data for name in B.NAMES for fn, data in B.singles()[name].items() if fn not in B.STATS_FILES}
    assert sorted(own) == sorted(want) and len(own) == 31 * 5
    for fn in want:
        assert own[fn] == want[fn], fn
    B.check_statistics(got)
