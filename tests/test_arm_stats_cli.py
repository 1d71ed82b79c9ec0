"""CPU tier: ibdgem --arm-stats / --stats-only without a HIP device (non-LD runs take the host's arithmetic).

The chromosome-arm sums of log2(LIBD2/LIBD0) and log2(LIBD1/LIBD0) must print what the reference's bin/chrarm-stats.py
prints for the same run's summary files (tests/golden/armstats, from the committed 17-digit summaries)."""
import os
import subprocess

import numpy as np
import pytest

import armstats_check as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
NONLD = ["synA/nonld_flags", "synA/nonld_all_targets_w2"]
RANGES = ["both", "p_nan", "p_zero", "c0_at_end", "c1_at_start"]


def _run(args, cwd, out, expect_ok=True):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", IBDGEM_KEEP_TEARDOWN="1")
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([EXE] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, env=env)
    if expect_ok:
        assert res.returncode == 0, res.stderr
    return res


def _rng(key, rname):
    c0, c1 = A.golden()["cases"][key]["ranges"][rname]["range"]
    return f"{c0},{c1}"


@pytest.mark.parametrize("key", NONLD)
@pytest.mark.parametrize("rname", RANGES)
def test_no_device_arm_stats_match_the_script(key, rname, tmp_path):
    args, inp = A.run_args(key)
    _run(args + ["--arm-stats", _rng(key, rname)], inp, tmp_path)
    A.check(A.read_armstats(str(tmp_path / "UNKWN.armstats.txt")), key, rname)


def test_stats_only_writes_the_armstats_file_alone(tmp_path):
    key = "synA/nonld_all_targets_w2"
    args, inp = A.run_args(key)
    _run(args + ["--arm-stats", _rng(key, "both"), "--stats-only"], inp, tmp_path)
    assert sorted(os.listdir(tmp_path)) == ["UNKWN.armstats.txt"]
    A.check(A.read_armstats(str(tmp_path / "UNKWN.armstats.txt")), key, "both")


def test_armstats_file_does_not_depend_on_summary_only(tmp_path):
    key = "synA/nonld_flags"
    args, inp = A.run_args(key)
    rng = ["--arm-stats", _rng(key, "c1_at_start")]
    _run(args + rng, inp, tmp_path / "a")
    _run(args + rng + ["--summary-only"], inp, tmp_path / "b")
    _run(args + rng + ["--stats-only"], inp, tmp_path / "c")
    a = (tmp_path / "a" / "UNKWN.armstats.txt").read_bytes()
    assert a == (tmp_path / "b" / "UNKWN.armstats.txt").read_bytes() == (tmp_path / "c" / "UNKWN.armstats.txt").read_bytes()
    assert sorted(os.listdir(tmp_path / "b")) == ["UNKWN.armstats.txt", "UNKWN.ind3.summary.txt"]


def test_q_arm_is_nan_when_no_window_follows_the_centromere(tmp_path):
    """A range past the last window: the p-arm is every window (the script would raise at end of file)."""
    key = "synA/nonld_all_targets_w2"
    args, inp = A.run_args(key)
    _run(args + ["--arm-stats", "900000000,900000001"], inp, tmp_path / "past")
    rows = A.read_armstats(str(tmp_path / "past" / "UNKWN.armstats.txt"))
    assert [r[0] for r in rows] == ["ind0", "ind69"]
    for r in rows:
        assert r[3] == r[5] == "nan" and "nan" not in (r[2], r[4]), r
    # the p-arm over every window = the q-arm of a range before the first window (END_0 > 1: p is nan, q every window)
    _run(args + ["--arm-stats", "1,1"], inp, tmp_path / "all_q")
    q_all = A.read_armstats(str(tmp_path / "all_q" / "UNKWN.armstats.txt"))
    for r, q in zip(rows, q_all):
        assert q[2] == q[4] == "nan" and (q[3], q[5]) == (r[2], r[4]), (r, q)


def test_no_windows_gives_nan_everywhere(tmp_path):
    key = "synA/nonld_flags"
    args, inp = A.run_args(key)
    pos = tmp_path / "pos.txt"
    pos.write_text("7\t1\n")                                      # no panel site: no row, no window
    _run(args + ["-p", str(pos), "--arm-stats", "10,20"], inp, tmp_path / "o")
    rows = A.read_armstats(str(tmp_path / "o" / "UNKWN.armstats.txt"))
    assert rows == [["ind3", "7", "nan", "nan", "nan", "nan"]]


@pytest.mark.parametrize("bad", ["", "5", "5,", ",5", "a,b", "5,3", "-1,5", "1;2", "1,2,3", "1, 2", "+1,2"])
def test_malformed_range_is_refused(bad, tmp_path):
    key = "synA/nonld_flags"
    args, inp = A.run_args(key)
    res = _run(args + ["--arm-stats", bad], inp, tmp_path, expect_ok=False)
    assert res.returncode == 1 and "--arm-stats" in res.stderr
    assert not os.listdir(tmp_path)


def test_stats_only_needs_arm_stats(tmp_path):
    key = "synA/nonld_flags"
    args, inp = A.run_args(key)
    res = _run(args + ["--stats-only"], inp, tmp_path, expect_ok=False)
    assert res.returncode == 1 and "--arm-stats" in res.stderr
    assert not os.listdir(tmp_path)


def test_stored_long_double_sums_are_plain_decimals_that_print_the_script_line():
    """Every stored sum parses as a long double and prints (%.3e) what the script printed: the tolerance at a rounding
    boundary (armstats_check.check_value) has the script's own value to work from."""
    n = 0
    for key, c in A.golden()["cases"].items():
        for rname, r in c["ranges"].items():
            for ind, e in r["individuals"].items():
                fields = e["line"].split("\t")[1:]
                for text, want in zip(e["sums"], fields):
                    v = np.longdouble(text)
                    assert ("nan" if np.isnan(v) else "%.3e" % v) == want, (key, rname, ind, text, want)
                    n += 1
    assert n == 4 * 75


def test_rounding_boundary_tolerance():
    """The boundary branch of the text comparison, on synthetic values: 1.2345e2 + 1e-12 rounds to 1.235e+02 in the
    script; a sum off by 1e-11 may print 1.234e+02, but nothing else, and not when no boundary is within the bound."""
    assert A.check_value("1.234e+02", "1.234e+02", "123.4", 0.0) == 0
    assert A.check_value("1.234e+02", "1.235e+02", "123.450000000001", 1e-11) == 1
    with pytest.raises(AssertionError, match="no %.3e boundary"):
        A.check_value("1.234e+02", "1.235e+02", "123.450000000001", 1e-13)
    with pytest.raises(AssertionError, match="neither rounding"):
        A.check_value("1.233e+02", "1.235e+02", "123.450000000001", 1e-11)
    with pytest.raises(AssertionError):
        A.check_value("nan", "1.235e+02", "123.450000000001", 1e-11)


def test_stats_only_with_plan_is_refused(tmp_path):
    key = "synA/nonld_flags"
    args, inp = A.run_args(key)
    res = _run(args + ["--plan", "--arm-stats", "10,20", "--stats-only"], inp, tmp_path, expect_ok=False)
    assert res.returncode == 1 and "--plan" in res.stderr
    assert not os.listdir(tmp_path)
