"""The host program's --switches without a device: the non-LD run on the reference's three-sample fixture (the output job calls
ibdg_log2_switches_host on the table the host made, and once more on the table that says nothing for the prior), the two files'
formats, # Next against the update function, --chain-gap and --switch-scale, the refusals, and every other file unchanged."""
import os
import subprocess

import numpy as np
import pytest

from ibdgem_amd import engine as E
from test_chain_gap_cli import starts_from
from test_log_states_host import host_log_table
from test_switch_scale_cli import shifts_from

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")
IBDGEM = os.path.join(HOST, "ibdgem")
FIX_IN = os.path.join(REPO, "tests", "golden", "ibdgem-test", "input")
FIX = ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv", "-P", "test1.pileup", "-N", "sample1"]
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", IBDGEM_KEEP_TEARDOWN="1")
INDS = ("sample1", "sample2", "sample3")
W = 7
PEN = ("--p01", "0.5", "--p02", "0.25", "--p12", "0.5")
P = (0.5, 0.25, 0.5)
BASE = ["-w", str(W), "--log-stats", "--states", *PEN]


@pytest.fixture(scope="module", autouse=True)
def programs():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)


def ibdgem(args, out):
    os.makedirs(out, exist_ok=True)
    return subprocess.run([IBDGEM] + FIX + args + ["-O", str(out)], cwd=FIX_IN, capture_output=True, text=True, env=NO_DEVICE)


def files(d):
    """The files of a run; a *.tab.txt without its first line, which repeats the command."""
    out = {fn: (d / fn).read_bytes() for fn in sorted(os.listdir(d))}
    for fn in out:
        if fn.endswith(".tab.txt"):
            out[fn] = out[fn].split(b"\n", 1)[1]
    return out


def run_pair(tmp_path, extra, run=None, name="sample1", inds=INDS):
    """A run with --switches and one without: the new files are there and no other file differs.  run(args, out): the program on
    an input (default: the reference's fixture with BASE)."""
    run = run or (lambda args, out: ibdgem(BASE + args, out))
    res = run(extra + ["--switches"], tmp_path / "a")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    res = run(extra, tmp_path / "plain")
    assert res.returncode == 0, res.stderr
    plain = files(tmp_path / "plain")
    assert sorted(got) == sorted(list(plain) + [f"{name}.logibdswitches.txt"] + [f"{name}.{ind}.logswitches.txt" for ind in inds])
    for fn, data in plain.items():                                            # without the option no file changes by a byte
        assert got[fn] == data, fn
    return got


def files_are_the_twins(got, out_dir, gap=None, scale=None, name="sample1", inds=INDS, window=W, pen=P):
    """Both files against the twin and the update function; returns (the individuals' sw, the run file's lines, the last
    individual's starts and shifts)."""
    run = [l.split("\t") for l in got[f"{name}.logibdswitches.txt"].decode().splitlines()]
    assert run[0] == ["# ID", "N_WIN", "E_SW01", "E_SW02", "E_SW12"] and len(run) == 9
    total, sws = np.zeros(3), {}
    for i, ind in enumerate(inds):
        tab = host_log_table(out_dir / f"{name}.{ind}.tab.txt", window)
        pos = np.array([[int(x) for x in l.split("\t")[1:3]] for l in got[f"{name}.{ind}.summary.txt"].decode().splitlines()[1:]],
                       dtype=np.uint64)
        n = len(tab)
        assert len(pos) == n
        kw = dict(starts=starts_from(pos[:, 0], pos[:, 1], gap) if gap else None,
                  shift=shifts_from(pos[:, 0], pos[:, 1], scale) if scale else None)
        sw, expect, counted = E.log2_switches_host(tab, *pen, **kw)
        sws[ind] = sw
        text = "Segment\tSw_01\tSw_02\tSw_12\tP_Switch\n"
        for w in range(n):
            text += "%d\t%.6f\t%.6f\t%.6f\t%.6f\n" % (w + 1, *sw[w], (sw[w, 0] + sw[w, 1]) + sw[w, 2])
        assert got[f"{name}.{ind}.logswitches.txt"].decode() == text, ind
        assert text.splitlines()[1] == "1\t0.000000\t0.000000\t0.000000\t0.000000"
        assert run[1 + i] == [ind, str(n)] + ["%.6f" % e for e in expect], ind
        total = total + expect                                                # in the order of the panel
        _, prior, counted0 = E.log2_switches_host(None, *pen, want_sw=False, n_win=n, **kw)
        assert counted0.tolist() == counted.tolist()
    assert run[4] == ["# Total"] + ["%.6f" % x for x in total]
    assert run[5] == ["# Prior"] + ["%.6f" % x for x in prior]               # one site list: the same for the three
    assert run[6] == ["# Counted"] + [str(int(c)) for c in counted]
    assert run[7] == ["# Penalties"] + ["%.6e" % p for p in pen]
    assert run[8] == ["# Next"] + ["%.6e" % x for x in E.switch_penalty_update(pen, total, len(inds), prior)]
    return sws, run, kw


def test_cli_switches_without_a_device(tmp_path):
    got = run_pair(tmp_path, [])
    sws, run, _ = files_are_the_twins(got, tmp_path / "a")
    n = len(sws[INDS[0]])
    assert run[6] == ["# Counted"] + [str(n - 1)] * 3
    assert any((sw > 1e-3).any() for sw in sws.values())                       # the fixture does switch
    # --stats-only: the run's file alone, the same bytes
    res = ibdgem(BASE + ["--switches", "--stats-only"], tmp_path / "b")
    assert res.returncode == 0, res.stderr
    only = files(tmp_path / "b")
    assert sorted(only) == ["sample1.logibdstates.txt", "sample1.logibdswitches.txt"]
    for fn, data in only.items():
        assert got[fn] == data, fn


def test_cli_switches_on_the_fixture_with_chains_and_steps(tmp_path):
    """The fixture's windows are 700 bp apart with 100 bp between them.  --chain-gap 50: every window starts a chain, no step is
    counted, the prior is 0 and # Next is the penalties themselves.  --switch-scale 200: every step's shift is log2(3.5) bits,
    which caps p01 = p12 = 0.5 at 1 (not counted) and leaves p02 = 0.25 below it (counted)."""
    sws, run, kw = files_are_the_twins(run_pair(tmp_path / "gap", ["--chain-gap", "50"]), tmp_path / "gap" / "a", gap=50)
    n = len(sws[INDS[0]])
    assert kw["starts"] == list(range(1, n))
    assert run[4][1:] == run[5][1:] == ["0.000000"] * 3 and run[6][1:] == ["0"] * 3 and run[8][1:] == run[7][1:]
    sws, run, kw = files_are_the_twins(run_pair(tmp_path / "scale", ["--switch-scale", "200"]), tmp_path / "scale" / "a", scale=200.0)
    assert run[6][1:] == ["0", str(n - 1), "0"] and run[8][1] == run[7][1] and run[8][3] == run[7][3] and run[8][2] != run[7][2]


def test_cli_switches_with_every_other_option_on_an_input_with_gaps(tmp_path):
    """The input of test_chain_gap_cli.py (a gap on a window border, one inside a window): --switches beside --posteriors,
    --segments, --sample-paths, --chain-gap and --switch-scale."""
    import test_chain_gap_cli as G
    run = lambda args, out: G.ibdgem(["--log-stats", "--states"] + args, out, tmp_path / "in")
    extra = ["--posteriors", "--segments", "--sample-paths", "5", "--chain-gap", "10000", "--switch-scale", "2000.5"]
    got = run_pair(tmp_path, extra, run, "pu", G.INDS)
    sws, lines, kw = files_are_the_twins(got, tmp_path / "a", gap=10000, scale=2000.5, name="pu", inds=G.INDS, window=G.W, pen=G.PEN)
    n = len(sws[G.INDS[0]])
    assert kw["starts"] == [G.BORDER // G.W] and (kw["shift"][1:] < 0).any() and (kw["shift"][1:] > 0).any()
    assert all(int(c) == n - 2 for c in lines[6][1:])                          # penalties of 1e-3 and 1e-6: no shift caps them


def test_cli_switches_refusals(tmp_path):
    r = ibdgem(["--switches", "--states"], tmp_path)
    assert r.returncode == 1 and "--switches needs --log-stats and --states" in r.stderr
    r = ibdgem(["--switches", "--log-stats", "--arm-stats", "300,600"], tmp_path)
    assert r.returncode == 1 and "--switches needs --log-stats and --states" in r.stderr
    r = ibdgem(["--switches", "--log-stats", "--states", "--plan"], tmp_path)
    assert r.returncode == 1 and "--plan does not make" in r.stderr
    assert os.listdir(tmp_path) == []


def test_usage_names_the_option():
    r = subprocess.run([IBDGEM], capture_output=True, text=True, env=NO_DEVICE)
    assert "--switches" in r.stdout + r.stderr and "logibdswitches.txt" in r.stdout + r.stderr
