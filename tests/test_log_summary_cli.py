"""CPU tier: ibdgem --log-summary without a HIP device (a non-LD run fills the logs on the host as long-double sums of
log2l of its per-site values), and the combinations it refuses."""
import os
import subprocess

import numpy as np
import pytest

import golden_io as G
import hp_log_ref as HL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
FIX_IN = os.path.join(G.GOLD, "ibdgem-test", "input")
FIX = ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv", "-P", "test1.pileup", "-N", "sample1"]
HEADER = "# SEGMENT\tSTART\tEND\tLOG2_LIBD0\tLOG2_LIBD1\tLOG2_LIBD2\tNUM_SITES"


def _run(args, cwd, out, expect_ok=True):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", IBDGEM_KEEP_TEARDOWN="1")
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([EXE] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, env=env)
    if expect_ok:
        assert res.returncode == 0, res.stderr
    return res


def read_log_summary(path, summary_path):
    """The rows of a logsummary file as [n_win][3] doubles, after checking its header and that columns 1-3 and 7 are the
    summary's own bytes."""
    lg = [l.split("\t") for l in G.read_lines(path)]
    sm = [l.split("\t") for l in G.read_lines(summary_path)]
    assert "\t".join(lg[0]) == HEADER and len(lg) == len(sm)
    for a, b in zip(lg[1:], sm[1:]):
        assert len(a) == 7 and a[:3] == b[:3] and a[6] == b[6], (a, b)
        for x in a[3:6]:
            assert x == "nan" or len(x.split(".")[1]) == 6, x          # %.6f
    return np.array([[float(x) for x in r[3:6]] for r in lg[1:]], dtype=np.float64).reshape(-1, 3)


def tab_truth(tab_path, window):
    """Long-double sums of log2 of a table's per-site values over its windows of `window` rows with reads."""
    rows = [l.split("\t") for l in G.read_lines(tab_path) if l and not l.startswith("#")]
    nr = np.array([int(r[7]) for r in rows])
    na = np.array([int(r[8]) for r in rows])
    site = np.array([[float(x) for x in r[11:14]] for r in rows], dtype=np.float64).reshape(-1, 3)
    return HL.rows_log2_truth(site, nr, na, window)


@pytest.mark.parametrize("case", ["nonld_flags", "nonld_all_targets_w2"])
def test_no_device_logs_are_the_sums_over_the_committed_per_site_values(case, tmp_path):
    """The committed tables carry 17 digits: their values ARE the run's doubles."""
    meta = G.cases("synA")
    args = meta["base_args"] + meta["cases"][case]
    window = int(args[args.index("-w") + 1]) if "-w" in args else 100
    _run(args + ["--log-summary"], os.path.join(G.GOLD, "synA", "input"), tmp_path)
    ref = os.path.join(G.GOLD, "synA", case)              # (the 17-digit files; ref7 holds the six-digit ones)
    seen = 0
    for fn in sorted(os.listdir(ref)):
        if not fn.endswith(".tab.txt.gz"):
            continue
        stem = fn[:-len(".tab.txt.gz")]
        got = read_log_summary(str(tmp_path / f"{stem}.logsummary.txt"), str(tmp_path / f"{stem}.summary.txt"))
        s, a = tab_truth(os.path.join(ref, fn), window)
        assert got.shape == s.shape
        err = np.abs(got.astype(HL.LD) - s)
        assert (err <= 5e-7 + HL.rows_bar(s, a)).all(), (fn, float(err.max()))
        seen += 1
    assert seen >= 1


def test_reference_fixture_without_a_device(tmp_path):
    """supplementary/ibdgem-test, non-LD: a file per individual; the logs against the sums over the run's own per-site
    table (six digits: each term within 2.5e-7 / ln 2 x 2 of its double's log2)."""
    _run(FIX + ["--log-summary"], FIX_IN, tmp_path)
    for t in (1, 2, 3):
        got = read_log_summary(str(tmp_path / f"sample1.sample{t}.logsummary.txt"), str(tmp_path / f"sample1.sample{t}.summary.txt"))
        s, a = tab_truth(str(tmp_path / f"sample1.sample{t}.tab.txt"), 100)
        rows = np.array([int(l.split("\t")[6]) for l in G.read_lines(str(tmp_path / f"sample1.sample{t}.summary.txt"))[1:]])
        assert (np.abs(got.astype(HL.LD) - s) <= 5e-7 + 1e-6 * rows[:, None]).all()
        lin = np.array([[float(x) for x in l.split("\t")[3:6]]
                        for l in G.read_lines(str(tmp_path / f"sample1.sample{t}.summary.txt"))[1:]])
        assert np.allclose(np.exp2(got), lin, rtol=1e-5)


def test_summary_only_gives_the_same_files(tmp_path):
    _run(FIX + ["--log-summary"], FIX_IN, tmp_path / "a")
    _run(FIX + ["--log-summary", "--summary-only"], FIX_IN, tmp_path / "b")
    names = sorted(n for n in os.listdir(tmp_path / "a") if not n.endswith(".tab.txt"))
    assert sorted(os.listdir(tmp_path / "b")) == names and sum(n.endswith(".logsummary.txt") for n in names) == 3
    for n in names:
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes(), n


def test_no_flag_no_file(tmp_path):
    _run(FIX, FIX_IN, tmp_path)
    assert not [n for n in os.listdir(tmp_path) if "logsummary" in n]


@pytest.mark.parametrize("other,word", [(["--plan"], "--plan"), (["--arm-stats", "100,200", "--stats-only"], "--stats-only")])
def test_refused_combinations(other, word, tmp_path):
    res = _run(FIX + ["--log-summary"] + other, FIX_IN, tmp_path, expect_ok=False)
    lines = [l for l in res.stderr.splitlines() if "ERROR" in l]
    assert res.returncode == 1 and len(lines) == 1 and "--log-summary" in lines[0] and word in lines[0], res.stderr
    assert not os.listdir(tmp_path)


def test_ld_without_a_device_stops_with_the_engines_error(tmp_path):
    res = _run(FIX + ["--log-summary", "--LD"], FIX_IN, tmp_path, expect_ok=False)
    assert res.returncode != 0 and "no HIP device" in res.stderr
