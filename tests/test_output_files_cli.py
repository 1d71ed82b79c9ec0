"""The lifecycle of a comparison individual's output files (IND_FILES in host/ibdgem.c), without a device, on the reference's
three-sample fixture: they are opened without truncation and emptied by the job that writes them, so a rerun into a used
directory must leave nothing of the earlier run, and a run that fails must leave no complete-looking file of an earlier one."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")
IBDGEM = os.path.join(HOST, "ibdgem")
FIX_IN = os.path.join(REPO, "tests", "golden", "ibdgem-test", "input")
FIX = ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv", "-P", "test1.pileup", "-N", "sample1"]
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", IBDGEM_KEEP_TEARDOWN="1")
LOG_OPTS = ["--log-stats", "--states", "--posteriors", "--segments", "--log-summary", "--chain-gap", "300",
            "--p01", "0.5", "--p02", "0.25", "--p12", "0.5"]
KINDS = ("tab", "summary", "logsummary", "loghiddengem", "logposteriors", "logsegments", "logsamples")
RUN_KINDS = ("logibdstates", "logibdposteriors", "logibdsegments", "logibdsamples")


@pytest.fixture(scope="module", autouse=True)
def programs():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)


def ibdgem(args, out):
    os.makedirs(out, exist_ok=True)
    return subprocess.run([IBDGEM] + FIX + args + ["-O", str(out)], cwd=FIX_IN, capture_output=True, text=True, env=NO_DEVICE)


def files(d):
    """The files of a run; a *.tab.txt without its first line, which repeats the command and so the -O path."""
    out = {fn: (d / fn).read_bytes() for fn in sorted(os.listdir(d))}
    for fn in out:
        if fn.endswith(".tab.txt"):
            out[fn] = out[fn].split(b"\n", 1)[1]
    return out


def test_a_rerun_into_a_used_directory_leaves_nothing_of_the_earlier_run(tmp_path):
    first = ["-w", "7"] + LOG_OPTS + ["--sample-paths", "41"]
    second = ["-w", "50"] + LOG_OPTS + ["--sample-paths", "2"]
    for args, d in ((first, "a"), (second, "a"), (second, "b")):
        res = ibdgem(args, tmp_path / d)
        assert res.returncode == 0, res.stderr
    a, b = files(tmp_path / "a"), files(tmp_path / "b")
    assert sorted(a) == sorted(b) and len(a) == 25
    assert [fn for fn in a if a[fn] != b[fn]] == []


def blocked_rerun(tmp, opts, kind):
    """A complete run, then the same run with sample2's file of one kind replaced by a directory: the failing run's result."""
    res = ibdgem(opts, tmp)
    assert res.returncode == 0, res.stderr
    blocked = tmp / f"sample1.sample2.{kind}.txt"
    if blocked.exists():
        os.remove(blocked)
    os.mkdir(blocked)
    res = ibdgem(opts, tmp)
    assert res.returncode == 1
    line = [l for l in res.stderr.splitlines() if "Cannot open" in l]
    assert len(line) == 1 and f"'{blocked}'" in line[0], res.stderr
    if kind in ("tab", "summary"):
        assert (f"Cannot open '{tmp}/sample1.sample2.tab.txt' and/or '{tmp}/sample1.sample2.summary.txt' for writing."
                in line[0])
    others = [fn for fn in sorted(os.listdir(tmp)) if fn.startswith("sample1.sample2.") and (tmp / fn).is_file()]
    return others, {fn: (tmp / fn).stat().st_size for fn in others}


@pytest.mark.parametrize("kind", KINDS)
def test_a_failing_run_empties_every_file_it_opened(tmp_path, kind):
    others, size = blocked_rerun(tmp_path, ["-w", "7"] + LOG_OPTS + ["--sample-paths", "5"], kind)
    assert others == sorted(f"sample1.sample2.{k}.txt" for k in KINDS if k != kind)
    assert size == dict.fromkeys(others, 0)
    for k in RUN_KINDS:
        assert (tmp_path / f"sample1.{k}.txt").stat().st_size == 0


@pytest.mark.parametrize("opts,kinds", [(["--states"], ("tab", "hiddengem")),
                                        (["--states", "--summary-only"], ("hiddengem",))])
def test_a_failing_run_empties_its_files_without_the_log_options(tmp_path, opts, kinds):
    """The /dev/null in the table's place (--summary-only: it is not emptied, and no *.tab.txt appears) and the states file's name
    without --log-stats."""
    others, size = blocked_rerun(tmp_path, opts, "summary")
    assert others == sorted(f"sample1.sample2.{k}.txt" for k in kinds)
    assert size == dict.fromkeys(others, 0)
    assert (tmp_path / "sample1.ibdstates.txt").stat().st_size == 0
