"""The site list's row table: one {LIBD0, LIBD1 under genotype 0, 1, 2} table per upload, made by the first --LD run that keeps
per-site results and used by every later --LD run, whatever its number of comparison individuals (ibdg_get_site_ll expands it
for the last run's individual t).  Whatever invalidates it -- new sites, a new panel, -A overrides, new alt counts -- must make
the next run rebuild it, and a queue of runs must leave the LAST run's individuals behind.

Per-site tables and LIBD2 of the windows are checked bit for bit against the oracle, the --LD window LIBD0/LIBD1 bit for bit
against the same run made in a fresh context.
"""
import numpy as np
import pytest

from ibdgem_amd import engine as E

pytestmark = pytest.mark.gpu

W = 100


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bits(got, want, what):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, what
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {(~same).sum()}/{same.size} differ, first at {i}: {got[i]!r} vs {want[i]!r}")


def synth(seed, L, N, cov_mean=2.0):
    rng = np.random.default_rng(seed)
    f = np.clip(rng.beta(0.3, 1.0, size=L), 1e-3, 0.999)
    alle = (rng.random((L, 2 * N)) < f[:, None]).astype(np.uint8)
    cov = np.minimum(rng.poisson(cov_mean, size=L), 20)
    n_alt = rng.binomial(cov, f)
    return alle, (cov - n_alt).astype(np.uint8), n_alt.astype(np.uint8)


def fresh_windows(alle, nr, na, targets, f_override=None):
    """The window tables of one synchronous run in a context of its own."""
    with E.Engine() as e:
        e.upload_panel(E.pack_alleles_fast(alle), alle.shape[1] // 2)
        e.upload_sites(np.arange(len(nr)), nr, na, W, f_override=f_override)
        e.run(targets, ld=True)
        return [e.window_ll(i) for i in range(len(targets))]


def check(eng, oracle, alle, nr, na, targets, what, f_override=None, windows=None):
    """Per-site tables and windows of the last run over `targets` against the oracle / a fresh context."""
    if windows is None:
        windows = fresh_windows(alle, nr, na, targets, f_override)
    for i, t in enumerate(targets):
        ref = oracle.compare(alle, nr, na, t, window=W, ld=True, f_override=f_override)
        assert_bits(eng.site_ll(i), ref["site"], f"{what}: per-site table of individual {t}")
        win = eng.window_ll(i)
        assert_bits(win[:, 2], ref["win"][:, 2], f"{what}: LIBD2 of individual {t}")
        assert_bits(win, windows[i], f"{what}: windows of individual {t} against a fresh context")


def test_queued_single_runs_leave_the_last_individual_s_table(oracle):
    """The bench's step: queued runs of one comparison individual each, two individuals taking turns.  After every queue
    length, site_ll(0) is the table of the individual of the LAST run."""
    N, L = 300, 5000
    alle, nr, na = synth(1101, L, N)
    a, b = 7, 8
    with E.Engine() as eng:
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        eng.upload_sites(np.arange(L), nr, na, W)
        eng.run([a], ld=True)
        site_a = eng.site_ll(0)
        eng.run([b], ld=True)
        site_b = eng.site_ll(0)
        assert not np.array_equal(bits(site_a), bits(site_b)), "the two individuals must differ for the test to mean anything"
        wins = {t: fresh_windows(alle, nr, na, [t])[0] for t in (a, b)}
        eng.set_option("async", 1)
        for n in range(1, 12):
            queue = [(a, b)[k % 2] for k in range(n)]
            for t in queue:
                eng.run([t], ld=True)
            check(eng, oracle, alle, nr, na, [queue[-1]], f"queue of {n}", windows=[wins[queue[-1]]])
        eng.set_option("async", 0)


def test_new_sites_with_the_same_row_count_rebuild_the_table(oracle):
    N, L = 200, 3000
    alle, nr, na = synth(1202, L, N)
    _, nr2, na2 = synth(1203, L, N)
    with E.Engine() as eng:
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        eng.set_option("async", 1)
        for k, (r, s) in enumerate([(nr, na), (nr2, na2), (nr, na)]):
            eng.upload_sites(np.arange(L), r, s, W)
            eng.run([5], ld=True)
            eng.run([6], ld=True)
            check(eng, oracle, alle, r, s, [6], f"upload {k}")


def test_a_new_panel_rebuilds_the_table(oracle):
    N, L = 200, 3000
    alle, nr, na = synth(1301, L, N)
    alle2 = synth(1302, L, N)[0]
    with E.Engine() as eng:
        for k, al in enumerate([alle, alle2, alle]):
            eng.upload_panel(E.pack_alleles_fast(al), N)
            eng.upload_sites(np.arange(L), nr, na, W)
            eng.run([9], ld=True)
            check(eng, oracle, al, nr, na, [9], f"panel {k}")


def test_allele_frequency_overrides_on_off_on(oracle):
    N, L = 150, 2500
    alle, nr, na = synth(1401, L, N)
    fo = np.full(L, np.nan)
    pick = np.random.default_rng(3).random(L) < 0.3
    fo[pick] = np.random.default_rng(4).uniform(0.01, 0.99, size=pick.sum())
    with E.Engine() as eng:
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        for k, f in enumerate([fo, None, fo]):
            eng.upload_sites(np.arange(L), nr, na, W, f_override=f)
            eng.run([11], ld=True)
            check(eng, oracle, alle, nr, na, [11], f"overrides {'on' if f is not None else 'off'} ({k})", f_override=f)


def test_alt_counts_recounted_inside_the_run(oracle):
    """Option count_in_run: the counts the table needs come from the run's own recount (stream2, before the table)."""
    N, L = 250, 4000
    alle, nr, na = synth(1501, L, N)
    alle2 = synth(1502, L, N)[0]
    with E.Engine() as eng:
        eng.set_option("count_in_run", 1)
        for k, al in enumerate([alle, alle2]):
            eng.upload_panel(E.pack_alleles_fast(al), N)
            eng.upload_sites(np.arange(L), nr, na, W)
            eng.set_option("async", 1)
            for t in (3, 4, 3):
                eng.run([t], ld=True)
            eng.set_option("async", 0)
            check(eng, oracle, al, nr, na, [3], f"panel {k}, counted in the run")


def test_site_results_toggled_between_queued_runs(oracle):
    N, L = 200, 3000
    alle, nr, na = synth(1601, L, N)
    with E.Engine() as eng:
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        eng.upload_sites(np.arange(L), nr, na, W)
        eng.set_option("async", 1)
        # the first run on the upload keeps nothing per row: a later one makes the table
        eng.set_option("site_results", 0)
        eng.run([1], ld=True)
        eng.set_option("site_results", 1)
        eng.run([2], ld=True)
        eng.set_option("site_results", 0)
        eng.run([3], ld=True)
        with pytest.raises(E.EngineError, match="no per-site results"):
            eng.site_ll(0)
        eng.set_option("site_results", 1)
        eng.run([4], ld=True)
        check(eng, oracle, alle, nr, na, [4], "0, 1, 0, 1")
        eng.set_option("async", 0)


def test_one_then_fifteen_then_one_individual(oracle):
    N, L = 300, 4000
    alle, nr, na = synth(1701, L, N)
    many = [(17 * i + 2) % N for i in range(15)]
    with E.Engine() as eng:
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        eng.upload_sites(np.arange(L), nr, na, W)
        for k, tg in enumerate([[21], many, [22]]):
            eng.run(tg, ld=True)
            check(eng, oracle, alle, nr, na, tg, f"run {k} of {len(tg)}")


def test_a_change_of_layout_in_the_middle_of_a_queue(oracle):
    """The runs on an upload re-lay the site list out (compacted tiles) once they have added up to option compact_targets:
    here in the second of a queue of runs.  The table (made by the first) and the later runs' windows stay right."""
    N, L = 200, 6000
    alle, nr, na = synth(1801, L, N)
    with E.Engine() as eng:
        eng.set_option("compact_targets", 20)
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        eng.upload_sites(np.arange(L), nr, na, W)
        assert eng.ld_layout() == 1
        eng.set_option("async", 1)
        for t in (30, 31, 30, 31, 32):
            eng.run([t], ld=True)
        assert eng.ld_layout() == 2
        check(eng, oracle, alle, nr, na, [32], "after the change of layout")
        eng.set_option("async", 0)
