"""-v site lists made on the device (GPU tier): ibdg_upload_candidates / ibdg_select_variable_sites /
ibdg_get_site_candidates through ctypes, and the host program's -v path through them.

Every comparison is bit-exact / byte-identical: the selection feeds the unchanged preparation and kernels the arrays an
upload of the numpy-filtered list feeds them (a fresh context given that list is the reference throughout); one case goes
through the oracle with the bars of tests/test_gpu_parity.py."""
import os
import subprocess

import numpy as np
import pytest

import golden_io as G
import pileup_list_util as U
from ibdgem_amd import engine as E

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _alleles(rng, n_rows, n_ids):
    f = np.clip(rng.beta(0.3, 1.0, size=n_rows), 1e-3, 0.999)
    return (rng.random((n_rows, 2 * n_ids)) < f[:, None]).astype(np.uint8), f


def _depths(rng, f_rows, depth):
    cov = np.minimum(rng.poisson(depth, size=len(f_rows)), 20)          # (zeros included: rows that join no window)
    n_alt = rng.binomial(cov, f_rows).astype(np.uint8)
    return (cov - n_alt).astype(np.uint8), n_alt


def _not_hom_ref(alle, rows, t):
    return (alle[rows, 2 * t] | alle[rows, 2 * t + 1]) != 0


def _engine(alle, n_ids, options=None):
    e = E.Engine(0, 0.02, 20)
    for k, v in (options or {}).items():
        e.set_option(k, v)
    e.upload_panel(E.pack_alleles_fast(alle), n_ids)
    return e


def _run_outcome(e, t):
    try:
        e.run([t], ld=True)
        return "ok", e.window_ll(0).shape
    except E.EngineError as x:
        return "error", str(x)


# ------------------------------------------------------------------------------------------------ 1. selection
@pytest.mark.parametrize("n_ids", [1, 3, 63, 64, 65, 130, 2504])
def test_selection_equals_numpy_filter(n_ids):
    rng = np.random.default_rng(1000 + n_ids)
    L, W = 3000, 40
    alle, f = _alleles(rng, L, n_ids)
    zero = one = None
    if n_ids >= 63:
        zero, one = n_ids // 2, n_ids // 2 + 1
        alle[:, 2 * zero:2 * zero + 2] = 0              # 0/0 at every row: nothing is selected
        alle[:, 2 * one + (n_ids & 1)] = 1              # not 0/0 anywhere: every candidate is selected
    edge = np.array([0, 31, 32, 63, 64, 95, 96, L - 65, L - 64, L - 33, L - 32, L - 1])
    pick = np.union1d(rng.choice(L, size=2000, replace=False), edge).astype(np.uint32)
    lists = {"file order": pick, "not in file order": rng.permutation(pick).astype(np.uint32), "the panel's own rows": None}
    general = proper = 0
    with _engine(alle, n_ids) as eng, _engine(alle, n_ids) as ref:
        for what, rows in lists.items():
            n = L - 7 if rows is None else len(rows)
            r = np.arange(n, dtype=np.uint32) if rows is None else rows
            nr, na = _depths(rng, f[r], 1.5)
            assert (nr + na == 0).any()
            eng.upload_candidates(rows, nr, na)
            assert eng.n_candidates == n
            who = [0, n_ids - 1] + [int(t) for t in rng.choice(n_ids, size=min(2, n_ids), replace=False)]
            who += [t for t in (zero, one) if t is not None]
            for t in who:
                keep = _not_hom_ref(alle, r, t)
                eng.select_variable_sites(t, W)
                got = eng.site_candidates()
                assert got.dtype == np.uint32 and np.array_equal(got, np.flatnonzero(keep)), (what, t)
                assert eng.n_sites == keep.sum() and eng.n_candidates == n
                ref.upload_sites(r[keep], nr[keep], na[keep], W)
                assert eng.n_windows == ref.n_windows
                for a, b in zip(eng.windows(), ref.windows()):
                    assert np.array_equal(a, b), (what, t)
                if t == zero:
                    assert eng.n_sites == 0 and eng.n_windows == 0
                    assert _run_outcome(eng, t) == _run_outcome(ref, t)
                elif t == one:
                    assert eng.n_sites == n
                else:
                    general += 1
                    proper += 0 < keep.sum() < n
    assert general >= 6 and 2 * proper >= general, (proper, general)


# ------------------------------------------------------------------------------------------------ 2. results
def _problem(seed=5, n_rows=4000, n_ids=300, n_cand=3000, depth=2.0):
    rng = np.random.default_rng(seed)
    alle, f = _alleles(rng, n_rows, n_ids)
    rows = np.sort(rng.choice(n_rows, size=n_cand, replace=False)).astype(np.uint32)
    nr, na = _depths(rng, f[rows], depth)
    return rng, alle, n_ids, rows, nr, na


def _results(e, targets, ld, bg=None, pu=-1):
    e.run(targets, ld=ld, bg_count=bg, pu_id=pu)
    return dict(win=[bits(e.window_ll(k)).copy() for k in range(len(targets))],
                site=[bits(e.site_ll(k)).copy() for k in range(len(targets))], af=bits(e.site_af()).copy())


def _assert_same(a, b, what):
    assert np.array_equal(a["af"], b["af"]), what
    for k in ("win", "site"):
        assert len(a[k]) == len(b[k])
        for x, y in zip(a[k], b[k]):
            assert x.shape == y.shape and np.array_equal(x, y), (what, k)


CONFIGS = {
    "ld auto": dict(),
    "strict": dict(options={"ld_variant": 1}),
    "reference order": dict(options={"ld_variant": 3}),
    "never compacted": dict(options={"compact_tiles": -1}),
    "compacted by density": dict(options={"compact_tiles": 0}, depth=0.2),
    "always compacted": dict(options={"compact_tiles": 1}),
    "non-LD": dict(ld=False),
    "override": dict(fo=True),
    "background list and -N": dict(bg=True),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_results_equal_a_fresh_context_with_the_filtered_upload(name):
    cfg = CONFIGS[name]
    rng, alle, n_ids, rows, nr, na = _problem(depth=cfg.get("depth", 2.0))
    ld = cfg.get("ld", True)
    fo = None
    if cfg.get("fo"):
        fo = np.where(rng.random(len(rows)) < 0.5, np.nan, rng.uniform(0.01, 0.99, len(rows)))
    bg, pu = None, -1
    if cfg.get("bg"):
        bg = rng.integers(0, 3, size=n_ids).astype(np.uint8)
        pu = 17
    with _engine(alle, n_ids, cfg.get("options")) as eng, _engine(alle, n_ids, cfg.get("options")) as ref:
        eng.upload_candidates(rows, nr, na, fo)
        for t, other in ((7, 8), (250, 3)):
            keep = _not_hom_ref(alle, rows, t)
            assert 0 < keep.sum() < len(rows)
            eng.select_variable_sites(t, 50)
            ref.upload_sites(rows[keep], nr[keep], na[keep], 50, None if fo is None else fo[keep])
            assert eng.ld_layout() == ref.ld_layout()
            for tg in ([t], [other]):
                _assert_same(_results(eng, tg, ld, bg, pu), _results(ref, tg, ld, bg, pu), (name, t, tg))
                assert eng.last_ld_variant() == ref.last_ld_variant()


def test_selected_list_against_the_oracle(oracle):
    from test_gpu_parity import assert_bits, assert_ld_close
    rng, alle, n_ids, rows, nr, na = _problem(seed=9)
    t, W = 11, 100
    keep = _not_hom_ref(alle, rows, t)
    with _engine(alle, n_ids) as eng:
        eng.upload_candidates(rows, nr, na)
        eng.select_variable_sites(t, W)
        eng.run([t], ld=True)
        site, win = eng.site_ll(0), eng.window_ll(0)
        first, last, ncov = eng.windows()
    want = oracle.compare(alle[rows[keep]], nr[keep], na[keep], t, window=W, ld=True)
    assert np.array_equal(first, want["first"]) and np.array_equal(last, want["last"]) and np.array_equal(ncov, want["nsites"])
    assert_bits(site, want["site"], "per-site values")
    assert_bits(win[:, 2], want["win"][:, 2], "LIBD2")
    assert_ld_close(win[:, :2], want["win"][:, :2], "--LD LIBD0/LIBD1")


# ------------------------------------------------------------------------------------------------ 3. state
def test_selections_replace_each_other_and_uploads_leave_the_candidates():
    rng, alle, n_ids, rows, nr, na = _problem(seed=21)
    a, b = 4, 190
    other = np.sort(rng.choice(len(alle), size=1500, replace=False)).astype(np.uint32)
    o_nr, o_na = _depths(rng, np.full(len(other), 0.3), 3.0)
    with _engine(alle, n_ids) as eng, _engine(alle, n_ids) as ref:
        eng.upload_candidates(rows, nr, na)
        seen = []
        for t in (a, b, a):
            eng.select_variable_sites(t, 50)
            seen.append((eng.site_candidates().copy(), _results(eng, [t], True)))
        assert np.array_equal(seen[0][0], seen[2][0]) and not np.array_equal(seen[0][0], seen[1][0])
        _assert_same(seen[0][1], seen[2][1], "select(a) again")
        # a plain upload in between: a fresh context's results, and no map to ask for
        eng.upload_sites(other, o_nr, o_na, 50)
        ref.upload_sites(other, o_nr, o_na, 50)
        _assert_same(_results(eng, [b], True), _results(ref, [b], True), "plain upload after a selection")
        with pytest.raises(E.EngineError, match="ibdg_select_variable_sites"):
            eng.site_candidates()
        assert eng.n_candidates == len(rows)
        eng.select_variable_sites(a, 50)
        assert np.array_equal(eng.site_candidates(), seen[0][0])
        _assert_same(_results(eng, [a], True), seen[0][1], "selection after a plain upload")
        # a new panel drops the candidates
        eng.upload_panel(E.pack_alleles_fast(alle), n_ids)
        assert eng.n_candidates == 0
        with pytest.raises(E.EngineError, match="no candidates"):
            eng.select_variable_sites(a, 50)


def test_selection_waits_for_queued_runs_and_a_pending_finalising_step():
    rng, alle, n_ids, rows, nr, na = _problem(seed=22)
    with _engine(alle, n_ids) as eng, _engine(alle, n_ids) as ref:
        eng.upload_candidates(rows, nr, na)
        eng.select_variable_sites(30, 50)
        eng.set_option("async", 1)
        for t in (5, 6, 7):
            eng.run([t], ld=True)                   # queued: the last one's finalising step is left to "the next run"
        eng.select_variable_sites(31, 50)
        eng.run([31], ld=True)
        eng.run([32], ld=True)
        eng.set_option("async", 0)
        keep = _not_hom_ref(alle, rows, 31)
        ref.upload_sites(rows[keep], nr[keep], na[keep], 50)
        ref.run([32], ld=True)
        assert np.array_equal(bits(eng.window_ll(0)), bits(ref.window_ll(0)))
        assert np.array_equal(bits(eng.site_ll(0)), bits(ref.site_ll(0)))


def test_errors_leave_the_context_usable():
    rng, alle, n_ids, rows, nr, na = _problem(seed=23)
    with _engine(alle, n_ids) as eng, _engine(alle, n_ids) as ref:
        with pytest.raises(E.EngineError, match="no candidates"):
            eng.select_variable_sites(0, 50)
        bad = rows.copy()
        bad[10] = len(alle)
        with pytest.raises(E.EngineError, match=r"row_index\[10\]"):
            eng.upload_candidates(bad, nr, na)
        deep = nr.copy()
        deep[20] = 21
        with pytest.raises(E.EngineError, match="candidate 20"):
            eng.upload_candidates(rows, deep, na)
        assert eng.n_candidates == 0
        eng.upload_candidates(rows, nr, na)
        with pytest.raises(E.EngineError, match="outside the panel"):
            eng.select_variable_sites(n_ids, 50)
        with pytest.raises(E.EngineError, match="window size"):
            eng.select_variable_sites(0, 0)
        eng.upload_sites(rows, nr, na, 50)
        with pytest.raises(E.EngineError, match="ibdg_select_variable_sites"):
            eng.site_candidates()
        keep = _not_hom_ref(alle, rows, 12)
        eng.select_variable_sites(12, 50)
        ref.upload_sites(rows[keep], nr[keep], na[keep], 50)
        _assert_same(_results(eng, [12], True), _results(ref, [12], True), "after the errors")


# ------------------------------------------------------------------------------------------------ 4. host program
@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST, "ibdgem"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "ibdgem")


def _messages(stderr):
    return [l for l in stderr.splitlines() if not l.startswith(("Run time", "## "))]


def _both_paths(exe, args, cwd, tmp_path):
    """the run with the site lists made on the device and with IBDGEM_VARSITES=host: files, messages, which path ran"""
    res = {}
    for path in ("device", "host"):
        out = tmp_path / path
        out.mkdir()
        env = dict(os.environ, IBDGEM_TIMING="1")
        if path == "host":
            env["IBDGEM_VARSITES"] = "host"
        r = U.run(exe, args + ["-O", str(out)], cwd, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        phases = [l for l in r.stderr.splitlines() if l.startswith("## ") and "per individual: site list" in l]
        assert phases, r.stderr[-2000:]
        res[path] = (U.output_files(out), _messages(r.stderr), ["on the device" in l for l in phases])
    assert all(res["device"][2]) and not any(res["host"][2])
    assert sorted(res["device"][0]) == sorted(res["host"][0]) and res["device"][0]
    for fn in res["host"][0]:
        assert res["device"][0][fn] == res["host"][0][fn], fn
    assert res["device"][1] == res["host"][1]
    return res["device"][0]


@pytest.mark.parametrize("tag,case", [("synA", "ld_varsites"), ("synV", "vcf_ld_varsites_w50")])
def test_host_program_on_the_committed_goldens(exe, tag, case, tmp_path):
    meta = G.cases(tag)
    files = _both_paths(exe, meta["base_args"] + meta["cases"][case], os.path.join(G.GOLD, tag, "input"), tmp_path)
    ref = os.path.join(G.GOLD, tag, case, "ref7")
    tabs = [fn for fn in os.listdir(ref) if fn.endswith(".tab.txt.gz")]
    assert tabs
    for fn in tabs:               # (the per-site table does not depend on --LD's sums: the reference's own text)
        assert files[fn[:-3]].decode().splitlines() == G.read_lines(os.path.join(ref, fn)), fn


def _arm_range(tag):
    import gzip
    pos = sorted(int(l.split("\t")[1]) for l in gzip.open(os.path.join(G.GOLD, tag, "input", "reads.pileup.gz"), "rt"))
    return f"{pos[len(pos) * 2 // 5]},{pos[len(pos) * 9 // 20]}"


EXTRAS = [["-A", "af.txt", "--arm-stats", "ARM", "--states"], ["-B", "bg20.txt", "-w", "64"], ["--summary-only"],
          ["--stats-only", "--arm-stats", "ARM"], ["--reference-order", "-B", "bg_dup.txt"], ["-w", "7", "-N", "ind5"]]


@pytest.mark.parametrize("extra", EXTRAS, ids=lambda e: " ".join(e))
@pytest.mark.parametrize("as_list", [False, True])
def test_host_program_over_several_individuals(exe, extra, as_list, tmp_path):
    """-v --LD over ten comparison individuals of synA with the options that touch the site list, as a single run and as a
    --pileup-list of three pileups (the candidates are replaced per pileup)"""
    extra = [_arm_range("synA") if a == "ARM" else a for a in extra]
    inp = os.path.join(G.GOLD, "synA", "input")
    args = U.strip_pileup_args(G.cases("synA")["base_args"]) + ["--LD", "-v", "-s", ",".join(f"ind{k}" for k in range(0, 70, 7))]
    args += extra
    if as_list:
        src = tmp_path / "pileups"
        src.mkdir()
        paths = U.thinned_pileups("synA", src, 3)
        args = [a for a in args if a not in ("-N", "ind5")]
        args += ["--pileup-list", U.write_list(tmp_path / "l.txt", list(zip(["p0", "ind5", "p2"], paths)))]
    else:
        args += ["-P", "reads.pileup.gz"]
    files = _both_paths(exe, args, inp, tmp_path)
    assert len(files) >= (3 if as_list else 1)
