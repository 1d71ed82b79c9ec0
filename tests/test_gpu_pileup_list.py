"""--pileup-list on the device (GPU tier): every entry's files equal its single run's, for 1-3 contexts; and the engine's
state that belongs to a site list is reset when a context's site list is replaced, whatever the old list had reached."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import golden_io as G
import pileup_list_util as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")
EXE = os.path.join(HOST, "ibdgem")
FIX_IN = os.path.join(G.GOLD, "ibdgem-test", "input")
FIX_OUT = os.path.join(G.GOLD, "ibdgem-test", "output")
FIX_PANEL = ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv"]
DEVICES = {1: "0", 2: "0,0", 3: "0,0,0"}


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST, "ibdgem"], check=True, stdout=subprocess.DEVNULL)
    return EXE


def _ok(r):
    assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("ld", [False, True])
@pytest.mark.parametrize("devices", ["0", "0,0,0"])
def test_fixture_as_a_list_on_the_device(exe, ld, devices, tmp_path):
    """the reference's three pileups in one run: non-LD, the reference's own 18 files; --LD, the three single runs' files"""
    lst = U.write_list(tmp_path / "l.txt", [(f"sample{k}", f"test{k}.pileup") for k in (1, 2, 3)])
    args = FIX_PANEL + (["--LD"] if ld else []) + ["--devices", devices]
    out = tmp_path / "list"
    out.mkdir()
    r = _ok(U.run(exe, args + ["--pileup-list", lst, "-O", str(out)], FIX_IN))
    running = [l for l in r.stderr.splitlines() if l.startswith("Running ")]
    assert running == [f"Running sample{k}-vs-sample{t} comparison..." for k in (1, 2, 3) for t in (1, 2, 3)]
    got = U.output_files(out)
    if ld:
        want_dir = tmp_path / "single"
        want_dir.mkdir()
        for k in (1, 2, 3):
            _ok(U.run(exe, args + ["-P", f"test{k}.pileup", "-N", f"sample{k}", "-O", str(want_dir)], FIX_IN))
        want = U.output_files(want_dir)
    else:
        want = {}
        for fn in os.listdir(FIX_OUT):
            data = open(os.path.join(FIX_OUT, fn), "rb").read()
            want[fn] = data.split(b"\n", 1)[1] if fn.endswith(".tab.txt") else data
    assert sorted(got) == sorted(want) and len(got) == 18
    for fn in want:
        assert got[fn] == want[fn], fn


def _arm_range(tag):
    pos = sorted(int(l.split("\t")[1]) for l in gzip.open(os.path.join(G.GOLD, tag, "input", "reads.pileup.gz"), "rt"))
    return f"{pos[len(pos) * 2 // 5]},{pos[len(pos) * 9 // 20]}"


LIST_CASES = [("synA", "ld_default", []), ("synA", "ld_varsites", []), ("synA", "ld_downsample", []),
              ("synA", "ld_bg20_w64", []), ("synA", "ld_pu_in_panel", []), ("synA", "ld_default", ["--summary-only"]),
              ("synA", "ld_default", ["--arm-stats", "ARM"]), ("synA", "ld_default", ["--stats-only", "--arm-stats", "ARM"]),
              ("synB", "ld_w37", []), ("synB", "ld_pu_named", ["--arm-stats", "ARM"])]
_single_cache = {}


def _pileup_messages(stderr):
    """stderr without what a run prints once for the panel (run time, the note of a run without a device)"""
    return [l for l in stderr.splitlines() if not l.startswith(("Run time", "No HIP device found"))]


def _singles(exe, tag, case, extra, names, paths, tmp_path_factory):
    """each entry's single run with one context: {file: bytes}, and its per-pileup stderr lines"""
    key = (tag, case, tuple(extra))
    if key not in _single_cache:
        meta = G.cases(tag)
        args = U.strip_pileup_args(meta["base_args"] + meta["cases"][case]) + extra
        d = tmp_path_factory.mktemp("single")
        err = []
        for name, path in zip(names, paths):
            r = _ok(U.run(exe, args + ["-P", path, "-N", name, "-O", str(d)], os.path.join(G.GOLD, tag, "input")))
            err += _pileup_messages(r.stderr)
        _single_cache[key] = (U.output_files(d), err)
    return _single_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("tag,case,extra", LIST_CASES)
@pytest.mark.parametrize("contexts", [1, 2, 3])
def test_every_entry_equals_its_single_run(exe, tag, case, extra, contexts, tmp_path, tmp_path_factory):
    extra = [_arm_range(tag) if a == "ARM" else a for a in extra]
    src = tmp_path_factory.getbasetemp() / f"pileups_{tag}"
    if not src.exists():
        src.mkdir()
        U.thinned_pileups(tag, src, 4)
    paths = [os.path.join(G.GOLD, tag, "input", "reads.pileup.gz")] + \
        [str(src / (f"{tag}_v{k}.pileup" + (".gz" if k % 2 else ""))) for k in range(1, 4)]
    sq = {"ld_pu_in_panel": "ind5", "ld_pu_named": "ind129"}.get(case)
    names = [sq or "p0", "p1", "ind9" if sq else "p2", "p3"]
    want, want_err = _singles(exe, tag, case, extra, names, paths, tmp_path_factory)
    meta = G.cases(tag)
    args = U.strip_pileup_args(meta["base_args"] + meta["cases"][case]) + extra
    lst = U.write_list(tmp_path / "l.txt", list(zip(names, paths)))
    out = tmp_path / "out"
    out.mkdir()
    r = _ok(U.run(exe, args + ["--pileup-list", lst, "--devices", DEVICES[contexts], "-O", str(out)],
                  os.path.join(G.GOLD, tag, "input")))
    got = U.output_files(out)
    assert sorted(got) == sorted(want)
    for fn in want:
        assert got[fn] == want[fn], fn
    assert _pileup_messages(r.stderr) == want_err
    if "--stats-only" in extra:
        assert all(fn.endswith(".armstats.txt") for fn in got) and len(got) == 4


@pytest.mark.gpu
def test_a_path_listed_under_two_names_gives_the_same_bits(exe, tmp_path):
    meta = G.cases("synA")
    args = U.strip_pileup_args(meta["base_args"] + meta["cases"]["ld_default"])
    lst = U.write_list(tmp_path / "l.txt", [("a", "reads.pileup.gz"), ("b", "reads.pileup.gz")])
    out = tmp_path / "out"
    out.mkdir()
    _ok(U.run(exe, args + ["--pileup-list", lst, "--devices", "0,0", "-O", str(out)], os.path.join(G.GOLD, "synA", "input")))
    got = U.output_files(out)
    a = {fn[2:]: v for fn, v in got.items() if fn.startswith("a.")}
    b = {fn[2:]: v for fn, v in got.items() if fn.startswith("b.")}
    assert a and a == b


@pytest.mark.gpu
@pytest.mark.parametrize("n_entries", [1, 2, 3])
def test_more_or_as_many_contexts_as_entries(exe, n_entries, tmp_path):
    """three contexts for one to three pileups: contexts that take no entry still have their panel upload joined before
    the program tears the contexts down (IBDGEM_KEEP_TEARDOWN: ibdg_destroy on each), and every entry equals its
    single run"""
    meta = G.cases("synB")
    inp = os.path.join(G.GOLD, "synB", "input")
    args = U.strip_pileup_args(meta["base_args"] + meta["cases"]["ld_w37"])
    paths = U.thinned_pileups("synB", tmp_path, n_entries)
    names = [f"e{k}" for k in range(n_entries)]
    want_dir = tmp_path / "single"
    want_dir.mkdir()
    for name, path in zip(names, paths):
        _ok(U.run(exe, args + ["-P", path, "-N", name, "-O", str(want_dir)], inp))
    out = tmp_path / "out"
    out.mkdir()
    lst = U.write_list(tmp_path / "l.txt", list(zip(names, paths)))
    r = _ok(U.run(exe, args + ["--pileup-list", lst, "--devices", "0,0,0", "-O", str(out)], inp,
                  env=dict(os.environ, IBDGEM_KEEP_TEARDOWN="1")))
    assert "ERROR" not in r.stderr
    assert U.output_files(out) == U.output_files(want_dir)


# ---------------------------------------------------------------------------------------------- engine level
def _problem(seed=11, n_rows=4000, n_ids=300):
    from ibdgem_amd.engine import pack_alleles_fast
    rng = np.random.default_rng(seed)
    f = np.clip(rng.beta(0.3, 1.0, size=n_rows), 1e-3, 0.999)
    alle = (rng.random((n_rows, 2 * n_ids)) < f[:, None]).astype(np.uint8)

    def sites(n, depth, s):
        r = np.random.default_rng(s)
        rows = np.sort(r.choice(n_rows, size=n, replace=False)).astype(np.uint32)
        cov = np.minimum(r.poisson(depth, size=n), 20)
        n_alt = r.binomial(cov, f[rows]).astype(np.uint8)
        return rows, (cov - n_alt).astype(np.uint8), n_alt

    return pack_alleles_fast(alle), n_ids, sites(3000, 2.0, seed + 1), sites(1700, 4.0, seed + 2)


PLAN_A = [[t] for t in range(30)] + [list(range(40, 55))] + [[3]]     # past ibd0_after (8), the re-layout (22), a group of 15
PLAN_B = [[7], [8], list(range(60, 75)), [9]]


def _sequence(eng, sites, plan, window=50):
    """upload a site list and run the plan; per run: every individual's window table, the last individual's site table,
    last_count_unit and ld_layout"""
    rows, nr, na = sites
    eng.upload_sites(rows, nr, na, window)
    out = []
    for targets in plan:
        eng.run(targets, ld=True)
        win = [eng.window_ll(t).view(np.uint64).copy() for t in range(len(targets))]
        out.append(dict(win=win, site=eng.site_ll(len(targets) - 1).view(np.uint64).copy(),
                        unit=eng.last_count_unit(), layout=eng.ld_layout()))
    first, last, ncov = eng.windows()
    return out, (first.copy(), last.copy(), ncov.copy())


def _same(a, b):
    ra, wa = a
    rb, wb = b
    assert all((x == y).all() for x, y in zip(wa, wb))
    assert len(ra) == len(rb)
    for k, (x, y) in enumerate(zip(ra, rb)):
        assert x["unit"] == y["unit"] and x["layout"] == y["layout"], k
        assert (x["site"] == y["site"]).all(), k
        assert len(x["win"]) == len(y["win"]) and all((p == q).all() for p, q in zip(x["win"], y["win"])), k


@pytest.mark.gpu
@pytest.mark.parametrize("pending", [False, True])
def test_replacing_the_site_list_resets_its_state(pending):
    """A context that has run list A past the IBD0 pass, the re-layout and a group of 15 takes list B (other length and
    coverage): B's results, window table, count unit and layout equal a fresh context's on B; back on A they equal the
    first results bit for bit.  `pending`: the switches come while a queued single run's finalising step is still pending."""
    import ibdgem_amd
    panel, n_ids, A, B = _problem()
    with ibdgem_amd.Engine(0, 0.02, 20) as fresh:
        fresh.upload_panel(panel, n_ids)
        ref_a = _sequence(fresh, A, PLAN_A)
    with ibdgem_amd.Engine(0, 0.02, 20) as fresh:
        fresh.upload_panel(panel, n_ids)
        ref_b = _sequence(fresh, B, PLAN_B)
    # what list A is there to stress, on the fresh context: the panel's own tiles first and the compacted ones after the
    # re-layout, single runs in the IBD1 form once the IBD0 pass exists, a group of 15; B is a list of another length
    runs = ref_a[0]
    assert runs[0]["layout"] == 1 and runs[-1]["layout"] == 2, [r["layout"] for r in runs]
    assert runs[0]["unit"] != 3 and any(r["unit"] == 3 for r in runs[8:30]), [r["unit"] for r in runs]
    assert len(runs[30]["win"]) == 15
    assert len(ref_b[1][0]) != len(ref_a[1][0])
    with ibdgem_amd.Engine(0, 0.02, 20) as eng:
        eng.upload_panel(panel, n_ids)
        _same(_sequence(eng, A, PLAN_A), ref_a)
        if pending:
            eng.set_option("async", 1)
            for t in (5, 6, 7):
                eng.run([t], ld=True)                   # queued: the last one's finalising step is left to "the next run"
            eng.set_option("async", 0)
        _same(_sequence(eng, B, PLAN_B), ref_b)
        if pending:
            eng.set_option("async", 1)
            eng.run([12], ld=True)
            eng.run([13], ld=True)
            eng.set_option("async", 0)
        _same(_sequence(eng, A, PLAN_A), ref_a)
