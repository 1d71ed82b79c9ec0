"""The host program's --fit-penalties without a device: the non-LD run on the reference's three-sample fixture keeps every
individual's log table on the host and iterates the update of --switches over them after the last one.  logibdfit.txt against the
binding (ibdg_log2_fit_host over the tables the run wrote) on every byte; the cross-check with --switches; --threads 1 against
--threads 4; --stats-only; --pileup-list, a fit per pileup; --chain-gap and --switch-scale; every refusal with its message; every
other file unchanged."""
import os
import subprocess

import numpy as np
import pytest

import pileup_list_util as PL
from ibdgem_amd import engine as E
from test_chain_gap_cli import starts_from
from test_log_states_host import host_log_table
from test_switch_scale_cli import shifts_from
from test_switches_cli import BASE, FIX, FIX_IN, HOST, IBDGEM, INDS, NO_DEVICE, P, W, files, ibdgem

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = ["# Iteration", "P01", "P02", "P12", "E_SW01", "E_SW02", "E_SW12", "PRIOR01", "PRIOR02", "PRIOR12", "COUNTED01", "COUNTED02",
          "COUNTED12", "RATIO01", "RATIO02", "RATIO12"]


@pytest.fixture(scope="module", autouse=True)
def programs():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)


def fit_text(rows, stood, fitted, T):
    """logibdfit.txt as the program writes it, from the binding's rows."""
    text = "\t".join(HEADER) + "\n"
    for i, r in enumerate(rows):
        cells = [str(i + 1)] + ["%.6e" % x for x in r["p"]] + ["%.6f" % x for x in r["total"]] + ["%.6f" % x for x in r["prior"]]
        cells += [str(int(c)) for c in r["counted"]]
        for k in range(3):
            ok = np.isfinite(r["total"][k]) and np.isfinite(r["prior"][k]) and r["total"][k] > 0 and r["prior"][k] > 0
            cells.append("%.6f" % (r["total"][k] / (float(T) * r["prior"][k])) if ok else "nan")
        text += "\t".join(cells) + "\n"
    text += f"# Individuals\t{T}\n# Iterations\t{len(rows)}\t{'stood' if stood else 'limit'}\n"
    return text + "# Fitted\t" + "\t".join("%.17g" % x for x in fitted) + "\n"


def tables_of(got, out_dir, name="sample1", inds=INDS, gap=None, scale=None, window=W):
    """The individuals' log tables as the run wrote them, and the chain starts and shifts of the list they share."""
    tabs, kw = [], {}
    for ind in inds:
        tabs.append(host_log_table(out_dir / f"{name}.{ind}.tab.txt", window))
        pos = np.array([[int(x) for x in l.split("\t")[1:3]] for l in got[f"{name}.{ind}.summary.txt"].decode().splitlines()[1:]],
                       dtype=np.uint64)
        kw = dict(starts=starts_from(pos[:, 0], pos[:, 1], gap) if gap else None,
                  shift=shifts_from(pos[:, 0], pos[:, 1], scale) if scale else None)
    return tabs, kw


def run_pair(tmp_path, extra, n_iter, run=None, name="sample1"):
    """A run with --fit-penalties and one without: the new file is there and no other file differs."""
    run = run or (lambda args, out: ibdgem(BASE + args, out))
    res = run(extra + ["--fit-penalties", str(n_iter)], tmp_path / "a")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    res = run(extra, tmp_path / "plain")
    assert res.returncode == 0, res.stderr
    plain = files(tmp_path / "plain")
    assert sorted(got) == sorted(list(plain) + [f"{name}.logibdfit.txt"])
    for fn, data in plain.items():
        assert got[fn] == data, fn
    return got


def test_the_file_is_the_bindings_fit(tmp_path):
    got = run_pair(tmp_path, [], 40)
    tabs, _ = tables_of(got, tmp_path / "a")
    rows, stood, fitted = E.log2_fit_host(tabs, P, 40)
    text = got["sample1.logibdfit.txt"].decode()
    assert text == fit_text(rows, stood, fitted, 3)
    assert len(rows) >= 2 and text.splitlines()[0].split("\t") == HEADER
    # # Fitted passed back reproduces the doubles
    assert [float(x) for x in text.splitlines()[-1].split("\t")[1:]] == fitted.tolist()
    # a limit below: the same rows, `limit`
    res = ibdgem(BASE + ["--fit-penalties", "2"], tmp_path / "two")
    assert res.returncode == 0, res.stderr
    r2, s2, f2 = E.log2_fit_host(tabs, P, 2)
    assert not s2 and files(tmp_path / "two")["sample1.logibdfit.txt"].decode() == fit_text(r2, s2, f2, 3)
    assert "# Iterations\t2\tlimit\n" in fit_text(r2, s2, f2, 3)


def test_the_cross_check_with_switches(tmp_path):
    """Row 1 shows the text of logibdswitches.txt's # Total, # Prior and # Counted, and row 2's penalties are its # Next: two
    code paths (the output jobs' calls and the fit's loop) over the same tables."""
    res = ibdgem(BASE + ["--switches", "--fit-penalties", "3"], tmp_path)
    assert res.returncode == 0, res.stderr
    got = files(tmp_path)
    sw = {l.split("\t")[0]: l.split("\t")[1:] for l in got["sample1.logibdswitches.txt"].decode().splitlines() if l.startswith("# ")}
    fit = [l.split("\t") for l in got["sample1.logibdfit.txt"].decode().splitlines()]
    assert fit[1][1:4] == sw["# Penalties"] and fit[1][4:7] == sw["# Total"] and fit[1][7:10] == sw["# Prior"]
    assert fit[1][10:13] == sw["# Counted"] and fit[2][1:4] == sw["# Next"]
    # and the other files are those of the run with --switches alone
    res = ibdgem(BASE + ["--switches"], tmp_path / "plain")
    assert res.returncode == 0, res.stderr
    plain = files(tmp_path / "plain")
    assert sorted(got) == sorted(list(plain) + ["sample1.logibdfit.txt"])
    assert all(got[fn] == data for fn, data in plain.items() if not os.path.isdir(tmp_path / fn))


def test_threads_and_stats_only_give_the_same_bytes(tmp_path):
    want = None
    for i, extra in enumerate((["--threads", "1"], ["--threads", "4"], ["--threads", "3", "--stats-only"], ["--summary-only"])):
        res = ibdgem(BASE + extra + ["--fit-penalties", "40"], tmp_path / str(i))
        assert res.returncode == 0, res.stderr
        got = files(tmp_path / str(i))
        want = want or got["sample1.logibdfit.txt"]
        assert got["sample1.logibdfit.txt"] == want, extra
        if "--stats-only" in extra:
            assert sorted(got) == ["sample1.logibdfit.txt", "sample1.logibdstates.txt"]
    assert b"# Iterations\t" in want


def test_pileup_list_a_fit_per_pileup(tmp_path):
    lst = PL.write_list(tmp_path / "pileups.txt", [(f"sample{k}", f"test{k}.pileup") for k in (1, 2, 3)])
    out = tmp_path / "out"
    out.mkdir()
    args = FIX[:6] + BASE + ["--fit-penalties", "40"]
    res = subprocess.run([IBDGEM] + args + ["--pileup-list", lst, "-O", str(out)], cwd=FIX_IN, capture_output=True, text=True, env=NO_DEVICE)
    assert res.returncode == 0, res.stderr
    got = files(out)
    fits = set()
    for k in (1, 2, 3):
        os.makedirs(tmp_path / f"s{k}")
        single = subprocess.run([IBDGEM] + FIX[:6] + ["-P", f"test{k}.pileup", "-N", f"sample{k}"] + BASE +
                                ["--fit-penalties", "40", "-O", str(tmp_path / f"s{k}")], cwd=FIX_IN, capture_output=True, text=True,
                                env=NO_DEVICE)
        assert single.returncode == 0, single.stderr
        one = files(tmp_path / f"s{k}")
        assert got[f"sample{k}.logibdfit.txt"] == one[f"sample{k}.logibdfit.txt"]
        tabs, _ = tables_of(one, tmp_path / f"s{k}", name=f"sample{k}")
        assert one[f"sample{k}.logibdfit.txt"].decode() == fit_text(*E.log2_fit_host(tabs, P, 40), 3)
        fits.add(one[f"sample{k}.logibdfit.txt"])
    assert len(fits) == 3                                                     # each pileup its own fit


def test_chain_gap_and_switch_scale_beside_it(tmp_path):
    """--chain-gap 50 on the fixture: every window starts a chain, nothing is counted, the update keeps p and the first step
    stands with nan ratios.  --switch-scale 200: the shifts cap p01 and p12 at the start, so only pair 02 is counted at first."""
    got = run_pair(tmp_path / "gap", ["--chain-gap", "50"], 10)
    tabs, kw = tables_of(got, tmp_path / "gap" / "a", gap=50)
    rows, stood, fitted = E.log2_fit_host(tabs, P, 10, **kw)
    text = got["sample1.logibdfit.txt"].decode()
    assert text == fit_text(rows, stood, fitted, 3) and len(rows) == 1 and stood and fitted.tolist() == list(P)
    assert text.splitlines()[1].split("\t")[10:] == ["0", "0", "0", "nan", "nan", "nan"]
    got = run_pair(tmp_path / "scale", ["--switch-scale", "200"], 10)
    tabs, kw = tables_of(got, tmp_path / "scale" / "a", scale=200.0)
    rows, stood, fitted = E.log2_fit_host(tabs, P, 10, **kw)
    assert got["sample1.logibdfit.txt"].decode() == fit_text(rows, stood, fitted, 3)
    n = len(tabs[0])
    assert rows["counted"][0].tolist() == [0, n - 1, 0]
    # both, on the input with gaps of test_chain_gap_cli.py, beside every other option
    import test_chain_gap_cli as G
    run = lambda args, out: G.ibdgem(["--log-stats", "--states"] + args, out, tmp_path / "in")
    extra = ["--posteriors", "--segments", "--sample-paths", "5", "--switches", "--chain-gap", "10000", "--switch-scale", "2000.5"]
    got = run_pair(tmp_path / "both", extra, 25, run, "pu")
    tabs, kw = tables_of(got, tmp_path / "both" / "a", name="pu", inds=G.INDS, gap=10000, scale=2000.5, window=G.W)
    rows, stood, fitted = E.log2_fit_host(tabs, G.PEN, 25, **kw)
    assert got["pu.logibdfit.txt"].decode() == fit_text(rows, stood, fitted, len(G.INDS))
    assert kw["starts"] and len(rows) >= 2


def test_refusals(tmp_path):
    for args, text in ((["--fit-penalties", "5", "--states"], "--fit-penalties needs --log-stats and --states"),
                       (["--fit-penalties", "5", "--log-stats", "--arm-stats", "300,600"], "--fit-penalties needs --log-stats and --states"),
                       (["--fit-penalties", "5", "--plan"], "--fit-penalties writes a file --plan does not make"),
                       (["--fit-penalties", "5", "--log-stats", "--states", "--plan"], "--plan does not make"),
                       (["--fit-penalties", "5", "--log-stats", "--states", "-v"], "--fit-penalties cannot be combined with -v"),
                       (["--fit-penalties", "5", "--log-stats", "--states", "-D", "2"], "--fit-penalties cannot be combined with -D"),
                       (["--fit-penalties", "0", "--log-stats", "--states"], "(--fit-penalties) '0' (must be an integer in 1 .. 1000)"),
                       (["--fit-penalties", "1001", "--log-stats", "--states"], "(--fit-penalties) '1001'"),
                       (["--fit-penalties", "3.5", "--log-stats", "--states"], "(--fit-penalties) '3.5'"),
                       (["--fit-penalties", "-2", "--log-stats", "--states"], "(--fit-penalties) '-2'")):
        r = ibdgem(args, tmp_path)
        assert r.returncode == 1 and text in r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []


def test_usage_names_the_option():
    r = subprocess.run([IBDGEM], capture_output=True, text=True, env=NO_DEVICE)
    assert "--fit-penalties N" in r.stdout + r.stderr and "logibdfit.txt" in r.stdout + r.stderr
