"""The host program's --posteriors without a device: the non-LD run on the reference's three-sample fixture (the output job
calls ibdg_log2_posteriors_host on the table the host made), and the refusals."""
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
            assert out[fn].startswith(b"# Entered command: ")
            out[fn] = out[fn].split(b"\n", 1)[1]
    return out


@pytest.mark.parametrize("pen", [(), ("--p01", "0.5", "--p02", "0.25", "--p12", "0.5")])
def test_cli_posteriors_without_a_device(tmp_path, pen):
    W = 7
    base = ["-w", str(W), "--log-stats", "--states", *pen]
    res = ibdgem(base + ["--posteriors"], tmp_path / "a")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    res = ibdgem(base, tmp_path / "plain")
    assert res.returncode == 0, res.stderr
    plain = files(tmp_path / "plain")
    new = ["sample1.logibdposteriors.txt"] + [f"sample1.{ind}.logposteriors.txt" for ind in INDS]
    assert sorted(got) == sorted(list(plain) + new)
    for fn, data in plain.items():                                            # nothing else changes by a byte
        assert got[fn] == data, fn
    p = tuple(float(x) for x in pen[1::2]) or (1e-3, 1e-6, 1e-3)
    summary = [l.split("\t") for l in got["sample1.logibdposteriors.txt"].decode().splitlines()]
    assert summary[0] == "# ID\tN_SEGMENTS\tE_IBD0\tE_IBD1\tE_IBD2\tFRAC_IBD0\tFRAC_IBD1\tFRAC_IBD2\tLOG2_Z".split("\t")
    states = {l.split("\t")[0]: l.split("\t") for l in got["sample1.logibdstates.txt"].decode().splitlines() if not l.startswith("#")}
    total = np.zeros(3)
    for k, ind in enumerate(INDS):
        tab = host_log_table(tmp_path / "a" / f"sample1.{ind}.tab.txt", W)
        post, expect, log2_z = E.log2_posteriors_host(tab, *p)
        n = len(tab)
        text = "Segment\tPost_IBD0\tPost_IBD1\tPost_IBD2\tMax_State\n"
        for w in range(n):
            text += "%d\t%.6f\t%.6f\t%.6f\t%d\n" % (w + 1, *post[w], int(np.argmax(post[w])))   # (argmax: the first of equals)
        assert got[f"sample1.{ind}.logposteriors.txt"].decode() == text, ind
        row = summary[1 + k]
        assert row[0] == ind and row[1] == str(n) == states[ind][1]           # N_SEGMENTS is the summary's and the path's
        assert row[2:5] == ["%.3f" % e for e in expect] and row[5:8] == ["%.6f" % (e / n) for e in expect]
        assert row[8] == "%.6f" % log2_z
        assert abs(expect.sum() - n) <= 1e-9 * n                              # the expectations add up to the windows
        assert abs(sum(float(x) for x in row[2:5]) - n) <= 0.0015 and abs(sum(float(x) for x in row[5:8]) - 1) <= 1.5e-6
        total += expect
        assert len(open(tmp_path / "a" / f"sample1.{ind}.summary.txt").read().splitlines()) == n + 1
    tail = got["sample1.logibdposteriors.txt"].decode().splitlines()[4:]
    assert tail[0] == "# Total segments = %d" % (3 * n)
    assert tail[1:] == ["# Total E_IBD%d = %.3f (%.3f %%)" % (s, total[s], total[s] / (3 * n) * 100) for s in range(3)]
    # --stats-only: the run's file alone, the same bytes
    res = ibdgem(base + ["--posteriors", "--stats-only"], tmp_path / "b")
    assert res.returncode == 0, res.stderr
    only = files(tmp_path / "b")
    assert sorted(only) == ["sample1.logibdposteriors.txt", "sample1.logibdstates.txt"]
    for fn, data in only.items():
        assert got[fn] == data, fn


def test_cli_posteriors_refusals(tmp_path):
    r = ibdgem(["--posteriors", "--states"], tmp_path)
    assert r.returncode == 1 and "--posteriors needs --log-stats and --states" in r.stderr
    r = ibdgem(["--posteriors", "--log-stats", "--arm-stats", "300,600"], tmp_path)
    assert r.returncode == 1 and "--posteriors needs --log-stats and --states" in r.stderr
    r = ibdgem(["--posteriors", "--log-stats", "--states", "--plan"], tmp_path)
    assert r.returncode == 1 and "--plan does not make" in r.stderr
    assert os.listdir(tmp_path) == []
