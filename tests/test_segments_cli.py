"""The host program's --segments without a device: the non-LD run on the reference's three-sample fixture (the output job
calls ibdg_log2_segments_host on the table the host made), and the refusals."""
import os
import subprocess

import numpy as np
import pytest

import segments_check as S
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


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("pen", [(), ("--p01", "0.5", "--p02", "0.25", "--p12", "0.5"), ("--p01", "1", "--p02", "1", "--p12", "1")])
def test_cli_segments_without_a_device(tmp_path, pen, post):
    W = 7
    base = ["-w", str(W), "--log-stats", "--states", *pen] + (["--posteriors"] if post else [])
    res = ibdgem(base + ["--segments"], tmp_path / "a")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    res = ibdgem(base, tmp_path / "plain")
    assert res.returncode == 0, res.stderr
    plain = files(tmp_path / "plain")
    new = ["sample1.logibdsegments.txt"] + [f"sample1.{ind}.logsegments.txt" for ind in INDS]
    assert sorted(got) == sorted(list(plain) + new)
    for fn, data in plain.items():                                            # nothing else changes by a byte
        assert got[fn] == data, fn
    p = tuple(float(x) for x in pen[1::2]) or (1e-3, 1e-6, 1e-3)
    lines, n_rows = {}, 0
    for ind in INDS:
        seg_file = got[f"sample1.{ind}.logsegments.txt"]
        lines[ind] = S.individual_consistent(seg_file, got[f"sample1.{ind}.loghiddengem.txt"], got[f"sample1.{ind}.summary.txt"],
                                             post, ind)
        # the file is the twin's records over the table the host made, printed as the option says
        tab = host_log_table(tmp_path / "a" / f"sample1.{ind}.tab.txt", W)
        seg, n_seg, summary = E.log2_segments_host(tab, *p, with_post=post)
        _, rows = S.rows_of(seg_file)
        assert len(rows) == n_seg
        for row, r in zip(rows, seg):
            e = [int(x) for x in r["e"]]
            s = int(r["state"])
            lr = e[s] - max(e[(s + 1) % 3], e[(s + 2) % 3])
            assert row[9:13] == ["%.4f" % (np.longdouble(x) / 65536) for x in e + [lr]]
            if post:
                assert row[13] == "%.6f" % (np.longdouble(int(r["post_q"])) / (np.longdouble(int(r["n_win"])) * 2 ** 32))
                assert row[14] == "%.6f" % float(r["post_min"])
        assert lines[ind][:6] == [int(x) for x in summary[:6]]
        n_rows += n_seg
    S.run_consistent(got["sample1.logibdsegments.txt"], lines)
    if pen and pen[1] == "1":
        assert n_rows > 3                                                     # (without penalties the paths do switch)
    # --stats-only: the run's file alone, the same bytes
    res = ibdgem(base + ["--segments", "--stats-only"], tmp_path / "b")
    assert res.returncode == 0, res.stderr
    only = files(tmp_path / "b")
    assert sorted(only) == sorted(["sample1.logibdsegments.txt", "sample1.logibdstates.txt"] +
                                  (["sample1.logibdposteriors.txt"] if post else []))
    for fn, data in only.items():
        assert got[fn] == data, fn


def test_cli_segments_refusals(tmp_path):
    r = ibdgem(["--segments", "--states"], tmp_path)
    assert r.returncode == 1 and "--segments needs --log-stats and --states" in r.stderr
    r = ibdgem(["--segments", "--log-stats", "--arm-stats", "300,600"], tmp_path)
    assert r.returncode == 1 and "--segments needs --log-stats and --states" in r.stderr
    r = ibdgem(["--segments", "--log-stats", "--states", "--plan"], tmp_path)
    assert r.returncode == 1 and "--plan does not make" in r.stderr
    assert os.listdir(tmp_path) == []


def test_usage_names_the_option():
    r = subprocess.run([IBDGEM, "--help"], capture_output=True, text=True, env=NO_DEVICE)
    text = r.stdout + r.stderr
    assert "--segments" in text and "logsegments.txt" in text and "logibdsegments.txt" in text
