"""The host program's --sample-paths without a device: the non-LD run on the reference's three-sample fixture (the output job
calls ibdg_log2_samples_host on the table the host made, keyed by the individual's index in the panel), the two files' formats,
the quantile rule, --seed, and the refusals."""
import os
import subprocess

import numpy as np
import pytest

from ibdgem_amd import engine as E
from test_log_states_host import host_log_table

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
HEADER = ["# ID", "N_SEGMENTS", "K"] + [f"IBD{s}_{q}_{k}" for s in range(3) for q in ("WIN", "SEG", "BP")
                                      for k in ("MEAN", "Q025", "Q500", "Q975")] + ["P_ANY_IBD12"]
DRAW_HEADER = ("Sample\tWIN_IBD0\tWIN_IBD1\tWIN_IBD2\tSEG_IBD0\tSEG_IBD1\tSEG_IBD2\tBP_IBD0\tBP_IBD1\tBP_IBD2\t"
               "LONGEST_BP_IBD0\tLONGEST_BP_IBD1\tLONGEST_BP_IBD2\n")


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


def columns(v, K):
    """The four columns of K integers: the mean of the integer sum, the three order statistics."""
    v = sorted(int(x) for x in v)
    return ["%.3f" % (sum(v) / K), str(v[(K - 1) // 40]), str(v[(K - 1) // 2]), str(v[(K - 1) - (K - 1) // 40])]


def row_of(name, n, nine, K):
    """A row of logibdsamples.txt from nine [K][9]: windows, segments and base pairs per state."""
    row = [name, str(n), str(K)]
    for s in range(3):
        for q in range(3):
            row += columns(nine[:, 3 * q + s], K)
    return row + ["%.6f" % (int(((nine[:, 4] + nine[:, 5]) > 0).sum()) / K)]


@pytest.mark.parametrize("K,seed", [(41, None), (1, None), (41, 12345678901234567890)])
def test_cli_samples_without_a_device(tmp_path, K, seed):
    assert ((K - 1) // 40, (K - 1) // 2, (K - 1) - (K - 1) // 40) == ((1, 20, 39) if K == 41 else (0, 0, 0))
    base = ["-w", str(W), "--log-stats", "--states", *PEN]
    opt = ["--sample-paths", str(K)] + ([] if seed is None else ["--seed", str(seed)])
    res = ibdgem(base + opt, tmp_path / "a")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    res = ibdgem(base, tmp_path / "plain")
    assert res.returncode == 0, res.stderr
    plain = files(tmp_path / "plain")
    new = ["sample1.logibdsamples.txt"] + [f"sample1.{ind}.logsamples.txt" for ind in INDS]
    assert sorted(got) == sorted(list(plain) + new)
    for fn, data in plain.items():                                            # without the option no file changes by a byte
        assert got[fn] == data, fn
    summary = [l.split("\t") for l in got["sample1.logibdsamples.txt"].decode().splitlines()]
    assert summary[0] == HEADER and len(summary) == 5
    total = np.zeros((K, 9), dtype=np.uint64)
    for i, ind in enumerate(INDS):
        tab = host_log_table(tmp_path / "a" / f"sample1.{ind}.tab.txt", W)
        pos = np.array([[int(x) for x in l.split("\t")[1:3]] for l in
                        got[f"sample1.{ind}.summary.txt"].decode().splitlines()[1:]], dtype=np.uint64)
        n = len(tab)
        assert len(pos) == n
        _, rec = E.log2_samples_host(tab, *P, K, 1 if seed is None else seed, i, pos_first=pos[:, 0].copy(), pos_last=pos[:, 1].copy())
        text = DRAW_HEADER + "".join("%d\t%s\n" % (k + 1, "\t".join(str(int(x)) for x in list(rec[k, :6]) + list(rec[k, 9:])))
                                     for k in range(K))
        assert got[f"sample1.{ind}.logsamples.txt"].decode() == text, ind
        nine = np.concatenate([rec[:, :6], rec[:, 9:12]], axis=1)
        assert summary[1 + i] == row_of(ind, n, nine, K), ind
        total += nine
    assert summary[4] == row_of("# Total", 3 * n, total, K)
    if K == 41:
        assert len({tuple(r) for r in summary[1:4]}) == 3                      # three individuals, three streams
    # --stats-only: the run's file alone, the same bytes
    res = ibdgem(base + opt + ["--stats-only"], tmp_path / "b")
    assert res.returncode == 0, res.stderr
    only = files(tmp_path / "b")
    assert sorted(only) == ["sample1.logibdsamples.txt", "sample1.logibdstates.txt"]
    for fn, data in only.items():
        assert got[fn] == data, fn


def test_seed_changes_the_sample_files_and_no_other(tmp_path):
    base = ["-w", str(W), "--log-stats", "--states", "--posteriors", "--segments", "--chain-gap", "300", "--switch-scale", "500", *PEN,
            "--sample-paths", "41"]
    runs = {}
    for name, seed in (("default", []), ("one", ["--seed", "1"]), ("two", ["--seed", "2"])):
        res = ibdgem(base + seed, tmp_path / name)
        assert res.returncode == 0, res.stderr
        runs[name] = files(tmp_path / name)
    sampled = ["sample1.logibdsamples.txt"] + [f"sample1.{ind}.logsamples.txt" for ind in INDS]
    assert all(fn in runs["one"] and len(runs["one"][fn].splitlines()) >= 5 for fn in sampled)
    assert runs["default"] == runs["one"]                                       # the default seed is 1
    assert sorted(runs["one"]) == sorted(runs["two"])
    for fn in runs["one"]:
        assert (runs["one"][fn] != runs["two"][fn]) == ("samples" in fn), fn


def test_cli_samples_refusals(tmp_path):
    r = ibdgem(["--sample-paths", "5", "--states"], tmp_path)
    assert r.returncode == 1 and "--sample-paths needs --log-stats and --states" in r.stderr
    r = ibdgem(["--sample-paths", "5", "--log-stats", "--arm-stats", "300,600"], tmp_path)
    assert r.returncode == 1 and "--sample-paths needs --log-stats and --states" in r.stderr
    r = ibdgem(["--sample-paths", "5", "--log-stats", "--states", "--plan"], tmp_path)
    assert r.returncode == 1 and "--plan does not make" in r.stderr
    r = ibdgem(["--seed", "5", "--log-stats", "--states"], tmp_path)
    assert r.returncode == 1 and "--seed is the seed of --sample-paths" in r.stderr
    for bad in ("0", "65537", "-1", "ten", "3x"):
        r = ibdgem(["--sample-paths", bad, "--log-stats", "--states"], tmp_path)
        assert r.returncode == 1 and "Invalid number of draws (--sample-paths)" in r.stderr, bad
    r = ibdgem(["--sample-paths", "5", "--seed", "-3", "--log-stats", "--states"], tmp_path)
    assert r.returncode == 1 and "Invalid seed (--seed)" in r.stderr
    assert os.listdir(tmp_path) == []
