"""-v site lists made on the device: what can be checked without one (CPU tier).

The four entry points are declared, exported and bound; the host program's -v path without a device (the host's own
scan of the panel rows, which the device path leaves in place) still writes the reference's files, also under the
sanitizer builds."""
import os
import re
import subprocess

import pytest

import golden_io as G
from ibdgem_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")
FIX_IN = os.path.join(G.GOLD, "ibdgem-test", "input")
NEW = ["ibdg_upload_candidates", "ibdg_num_candidates", "ibdg_select_variable_sites", "ibdg_get_site_candidates"]
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", IBDGEM_KEEP_TEARDOWN="1")


def _build(*targets):
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST, *targets], check=True, stdout=subprocess.DEVNULL)


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "ibdgem_hip.h")).read()
    lib = E.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in E.SYMBOLS, name
        assert hasattr(lib, name), name
    for method in ("upload_candidates", "select_variable_sites", "site_candidates", "n_candidates"):
        assert hasattr(E.Engine, method), method
    assert lib.ibdg_abi_version() == 5 and re.search(r"#define IBDG_ABI_VERSION 5\b", header)
    # without a context the calls fail or answer 0, they do not crash
    assert lib.ibdg_num_candidates(None) == 0
    assert lib.ibdg_upload_candidates(None, None, None, None, None, 0) != 0
    assert lib.ibdg_select_variable_sites(None, 0, 100) != 0
    assert lib.ibdg_get_site_candidates(None, None) != 0


def _read(path):
    return G.read_lines(path)


def _run(exe, args, cwd, out, env=None):
    res = subprocess.run([exe] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True,
                         env=dict(os.environ, **NO_DEVICE, **(env or {})), timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return res


def _check_fixture_v(out, k):
    """-v on the reference's fixture: the rows of the reference's own table at which the comparison individual is not 0/0
    (src/ibdgem.c:584), same text; the skipped rows are counted as skipped"""
    for t in (1, 2, 3):
        fn = f"sample{k}.sample{t}.tab.txt"
        got = [l for l in _read(str(out / fn)) if not l.startswith("#") and l]
        want_all = [l for l in _read(os.path.join(G.GOLD, "ibdgem-test", "output", fn)) if not l.startswith("#") and l]
        want = [l for l in want_all if l.split("\t")[9:11] != ["0", "0"]]
        assert 0 < len(want) < len(want_all), fn
        assert got == want, fn
        full = G.TabFile(os.path.join(G.GOLD, "ibdgem-test", "output", fn))
        mine = G.TabFile(str(out / fn))
        assert mine.processed == len(want)
        assert mine.processed + mine.skipped == full.processed + full.skipped


def _check_golden_v(out, tag, case):
    ref = os.path.join(G.GOLD, tag, case, "ref7")
    n = 0
    for fn in sorted(os.listdir(ref)):
        if not fn.endswith(".tab.txt.gz"):
            continue                    # (--LD cases run without --LD here: the per-site table does not depend on it)
        assert _read(str(out / fn[:-3]))[1:] == _read(os.path.join(ref, fn)), f"{tag}/{case}/{fn}"
        n += 1
    assert n >= 1


V_GOLDENS = [("synA", "ld_varsites"), ("synV", "vcf_ld_varsites_w50")]


def _golden_args(tag, case):
    meta = G.cases(tag)
    args = meta["base_args"] + meta["cases"][case]
    assert "-v" in args
    return [a for a in args if a != "--LD"], os.path.join(G.GOLD, tag, "input")


@pytest.mark.parametrize("varsites", [None, "host"])
def test_v_without_a_device_writes_the_reference_files(varsites, tmp_path):
    _build("ibdgem")
    exe = os.path.join(HOST, "ibdgem")
    env = {"IBDGEM_VARSITES": varsites} if varsites else {}
    fix = tmp_path / "fix"
    fix.mkdir()
    res = _run(exe, ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv", "-P", "test2.pileup", "-N", "sample2", "-v"],
               FIX_IN, fix, dict(env, IBDGEM_TIMING="1"))
    _check_fixture_v(fix, 2)
    assert "per individual: site list" in res.stderr and "site list on the device" not in res.stderr
    for tag, case in V_GOLDENS:
        d = tmp_path / case
        d.mkdir()
        args, cwd = _golden_args(tag, case)
        _run(exe, args, cwd, d, env)
        _check_golden_v(d, tag, case)


def test_v_without_a_device_under_the_sanitizer_builds(tmp_path):
    _build("ibdgem_asan", "ibdgem_tsan")
    builds = [("ibdgem_asan", dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
                                   UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")),
              ("ibdgem_tsan", dict(TSAN_OPTIONS="halt_on_error=1:exitcode=66", IBDGEM_MT_MIN_BYTES="1"))]
    for name, env in builds:
        exe = os.path.join(HOST, name)
        fix = tmp_path / (name + "_fix")
        fix.mkdir()
        res = _run(exe, ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv", "-P", "test1.pileup", "-N", "sample1", "-v",
                         "--threads", "4"], FIX_IN, fix, env)
        assert "Sanitizer" not in res.stderr, res.stderr[-2000:]
        _check_fixture_v(fix, 1)
        for tag, case in V_GOLDENS:
            d = tmp_path / (name + "_" + case)
            d.mkdir()
            args, cwd = _golden_args(tag, case)
            res = _run(exe, args + ["--threads", "3"], cwd, d, env)
            assert "Sanitizer" not in res.stderr, res.stderr[-2000:]
            _check_golden_v(d, tag, case)
