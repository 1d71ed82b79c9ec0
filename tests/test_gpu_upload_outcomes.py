"""What an upload of sites leaves behind, outcome by outcome: the layout a site list gets (ibdg_ld_layout: 0 none -- the strict
kernel serves --, 1 the panel's own tiles, 2 the compacted tiles), the state of the context after a list whose layout was
refused, and every message of the upload group with the state it leaves.  The net under the upload path of ibdg_api.cpp
(build_segments: plan_layout, cut_segments, layout_refused, commit_layout; hand_over; upload_sites_core and the four entry points).

Pinned elsewhere and not repeated here:
  * rows out of file order: compacted tiles, or the strict kernel with compact_tiles -1, and ld_variant 2 "not applicable"
    then, against the oracle -- test_gpu_parity.test_kernel_selection_and_fallback;
  * rows more than 255 tile pairs apart, against the oracle -- test_gpu_parity.test_rows_tens_of_thousands_of_panel_rows_apart;
    the edge at 255 / 256 pairs -- test_gpu_tile_gaps (cases edge-255, edge-256);
  * compact_tiles 0 by density -- test_gpu_launch_trips (compact_density) and test_gpu_parity.test_sparse_pileup_rows_far_apart;
  * launch geometries bit for bit (ring, record budget, windows per wave), each on a context of its own --
    test_gpu_parity.test_exponent_counting_launch_geometries;
  * the first offending site in file order, through several scan blocks --
    test_gpu_parity.test_rows_in_any_order_and_the_first_offending_site;
  * the candidates' messages by fragment and the context after them -- test_gpu_variable_sites.test_errors_leave_the_context_usable;
  * the bounded poll of the hand-over -- ibdg_selftest("wait_info") (test_abi); no test here sets IBDG_WAIT_TIMEOUT_MS.

Not here: the refusal for power tables out of range (grow_pow_tables: a power of rho, sigma, tau or 1 - eps whose binary
exponent leaves +-2^31 / 3, i.e. reads x |log2 rho| > 6.7e8 in one window).  No context that ibdg_create accepts with the
plain binomial table reaches it before the LDS refusal does: the table is binomial only where eps^max_cov > 1e-280, so
|log2 rho| < 931 / max_cov, and a window passes the LDS check only with fewer than 4031 segments of at most 32 rows of at most
max_cov reads, so reads x |log2 rho| < 4031 x 32 x 931 = 1.2e8.

N = 70 individuals throughout, one panel of 130000 rows shared by the module (left unchanged).
"""
import numpy as np
import pytest

import depth_cases as DC
import gap_cases as GC
from ibdgem_amd import engine as E

pytestmark = pytest.mark.gpu

N, LP, T = 70, 130000, 5
SEG_BYTES = GC.SEG_BYTES


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{what}: {(~same).sum()}/{same.size} differ"


@pytest.fixture(scope="module")
def panel():
    rng = np.random.default_rng(4242)
    alle = (rng.random((LP, 2 * N)) < 0.3).astype(np.uint8)
    packed = E.pack_alleles_fast(alle)
    packed.setflags(write=False)
    return packed


def reads(seed, n):
    rng = np.random.default_rng(seed)
    cov = 1 + np.minimum(rng.poisson(1.5, size=n), 19)
    na = rng.binomial(cov, 0.3)
    return (cov - na).astype(np.uint8), na.astype(np.uint8)


def engine(panel, eps=0.02, **opts):
    eng = E.Engine(0, eps, 20)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.upload_panel(panel, N)
    return eng


def want_windows(nr, na, W):
    cov = np.flatnonzero(nr.astype(int) + na > 0)
    n_win = -(-len(cov) // W)
    first = cov[np.arange(n_win) * W]
    last = cov[np.minimum((np.arange(n_win) + 1) * W, len(cov)) - 1]
    ncov = np.minimum(W, len(cov) - np.arange(n_win) * W)
    return n_win, first, last, ncov


def after_upload(eng, lst, layout, what):
    rows, nr, na, W = lst
    n_win, first, last, ncov = want_windows(nr, na, W)
    assert eng.n_sites == len(nr), what
    assert eng.n_windows == n_win, what
    f, l, n = eng.windows()
    assert np.array_equal(f, first) and np.array_equal(l, last) and np.array_equal(n, ncov), what
    assert eng.ld_layout() == layout, (what, eng.ld_layout())


def tables(eng):
    eng.run([T], ld=True)
    return eng.last_ld_variant(), eng.site_ll(0).copy(), eng.window_ll(0).copy()


# --------------------------------------------------------------------------- 1. one context, every outcome in turn
def outcome_lists():
    nr, na = reads(1, 600)
    dense = (np.arange(1000, 1600, dtype=np.uint32), nr, na, 100)
    perm = np.arange(600)
    perm[[203, 204]] = perm[[204, 203]]
    swapped = (dense[0][perm], nr[perm], na[perm], 100)
    far = np.array([10, 11, 40000, 40001, 40002, 90000, 129998, 129999], dtype=np.uint32)
    fr, fa = reads(2, len(far))
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.uint8), 100)
    bare = (np.arange(5000, 5300, dtype=np.uint32), np.zeros(300, np.uint8), np.zeros(300, np.uint8), 100)
    # name, list, {compact_tiles: (layout, variant)}
    return [("dense", dense, {0: (1, 2), -1: (1, 2)}),
            ("two rows exchanged", swapped, {0: (2, 2), -1: (0, 1)}),
            ("rows far apart", (far, fr, fa, 3), {0: (2, 2), -1: (0, 1)}),
            ("empty", empty, {0: (0, 1), -1: (0, 1)}),
            ("no reads", bare, {0: (0, 1), -1: (0, 1)}),
            ("dense again", dense, {0: (1, 2), -1: (1, 2)})]


@pytest.mark.parametrize("tiles", [0, -1])
def test_one_context_through_every_layout_outcome(panel, tiles):
    """A refused attempt leaves nothing behind: after each upload the context answers as a fresh one given only that upload."""
    fresh = {}
    with engine(panel, compact_tiles=tiles) as eng:
        for name, lst, want in outcome_lists():
            layout, variant = want[tiles]
            what = f"compact_tiles {tiles}, {name}"
            eng.upload_sites(*lst[:3], lst[3])
            after_upload(eng, lst, layout, what)
            got = tables(eng)
            key = name.replace(" again", "")
            if key not in fresh:
                with engine(panel, compact_tiles=tiles) as ref:
                    ref.upload_sites(*lst[:3], lst[3])
                    after_upload(ref, lst, layout, what + " (fresh)")
                    fresh[key] = tables(ref)
            print(what, "layout", eng.ld_layout(), "variant", got[0], "fresh variant", fresh[key][0])
            assert got[0] == variant and fresh[key][0] == variant, what
            assert got[1].shape == (len(lst[1]), 3), what
            same_bits(got[1], fresh[key][1], what + ": per-site table")
            same_bits(got[2], fresh[key][2], what + ": window table")


# --------------------------------------------------------------------------- 2. the LDS refusal
def popcount_lds_bytes(max_seg, win_per_group, tab_len, tab_in_lds, ring_slots):
    """ld_popcount_lds_bytes(.., multi_target = 0) through ld_lds_layout (ibdg_ld_layout.h): records and window constants of
    8 words, tables of 16 bytes per entry, 8 waves, wave_sum2 scratch."""
    head = (max_seg * 8 + win_per_group * 8) * 4 + 15
    ring = (head + tab_len * 2 * (16 if tab_in_lds else 0) + 1023) & ~1023
    return ring + 8 * ring_slots * 1024 + 8 * 1024


def one_row_per_tile(n):
    k = np.arange(n)
    return (32 * k + (7 * k + 3) % 32).astype(np.uint32)


def test_lds_refusal_of_a_window_with_thousands_of_tiles(panel):
    """One window whose rows sit one per 32-row tile: as many segments as rows in its run of one window.  The smallest count at
    which the counting kernel's workgroup would need more than 150 KiB of LDS (ring of 2, tables in global memory: the window
    holds more than 767 reads) is refused on the panel's own tiles -- the strict kernel runs -- and one row fewer is not;
    the compacted tiles take the list."""
    n = next(n for n in range(768, 10000) if popcount_lds_bytes(n, 1, n + 1, False, 2) > 150 * 1024)
    assert popcount_lds_bytes(n - 1, 1, n, False, 2) <= 150 * 1024 and 32 * n <= LP
    print("rows in the window:", n)
    rows = one_row_per_tile(n)
    nr, na = reads(3, n)
    out = {}
    for tiles, layout, variant in ((-1, 0, 1), (0, 2, 2)):
        with engine(panel, compact_tiles=tiles) as eng:
            eng.upload_sites(rows, nr, na, n)
            print("compact_tiles", tiles, "layout", eng.ld_layout())
            after_upload(eng, (rows, nr, na, n), layout, f"compact_tiles {tiles}")
            out[tiles] = tables(eng)
            assert out[tiles][0] == variant
            if tiles == -1:
                # the threshold itself: one row (one segment) fewer fits
                eng.upload_sites(rows[:-1], nr[:-1], na[:-1], n - 1)
                print("one row fewer: layout", eng.ld_layout())
                assert eng.ld_layout() == 1
    same_bits(out[0][1], out[-1][1], "per-site table")
    same_bits(out[0][2][:, 2], out[-1][2][:, 2], "LIBD2")


# --------------------------------------------------------------------------- 3. a clamped P(D|G) table
NOT_APPLICABLE = ("[::] ERROR in ibdg_run: ld_variant 2 (exponent counting) is not applicable here "
                  "(clamped P(D|G) table, epsilon outside (0,1), max_cov > 50 or rows out of order)")


@pytest.mark.parametrize("tiles", [-1, 0, 1])
def test_clamped_table_gets_no_layout(panel, tiles):
    """epsilon 1e-30: e^a underflows and the reference clamps P(D|G) to DBL_MIN (test_kernel_selection_and_fallback): no
    layout whatever compact_tiles says, the strict kernel, ld_variant 2 refused, and the context usable afterwards."""
    name, lst, _ = outcome_lists()[0]
    with engine(panel, eps=1e-30, compact_tiles=tiles) as eng:
        eng.upload_sites(*lst[:3], lst[3])
        after_upload(eng, lst, 0, "clamped")
        first = tables(eng)
        assert first[0] == 1
        eng.set_option("ld_variant", 2)
        with pytest.raises(E.EngineError) as ei:
            eng.run([T], ld=True)
        assert str(ei.value) == NOT_APPLICABLE
        eng.set_option("ld_variant", 0)
        again = tables(eng)
        assert again[0] == 1 and eng.ld_layout() == 0
        same_bits(again[1], first[1], "per-site table")
        same_bits(again[2], first[2], "window table")


# --------------------------------------------------------------------------- 4. the record budget
def test_record_budget_halves_the_runs_and_the_context_goes_on(panel):
    """record_lds_bytes 1024 with runs of 16 windows (windows_per_wave 16; guided_runs 0, without which the runs of so few
    windows are one window long from the start): the records of a run of 16 windows do not fit, so the run length is halved
    and stage B's control words redone at least once.  Same bits as the default geometry, and the next upload on the same
    context, with the default budget again, is served as by a fresh one."""
    L, W = 3000, 100
    nr, na = reads(4, L)
    seg = DC.segments(nr, na, W)
    n_win = int(seg["win"][-1]) + 1
    per_run = np.diff(np.searchsorted(seg["win"], GC.run_begins(n_win, 16), side="left"))
    assert int(per_run.max()) * SEG_BYTES > 1024, per_run
    per_pair = np.diff(np.searchsorted(seg["win"], GC.run_begins(n_win, 2), side="left"))
    print("segments per run of 16:", per_run, "of 2:", per_pair)
    rows = np.arange(L, dtype=np.uint32)
    with engine(panel, ld_variant=2) as ref:
        ref.upload_sites(rows, nr, na, W)
        want = tables(ref)
        ref.upload_sites(rows[::2], nr[::2], na[::2], W)
        want2 = tables(ref)
    with engine(panel, ld_variant=2, record_lds_bytes=1024, windows_per_wave=16, guided_runs=0) as eng:
        eng.upload_sites(rows, nr, na, W)
        after_upload(eng, (rows, nr, na, W), 1, "small budget")
        got = tables(eng)
        assert got[0] == 2
        same_bits(got[1], want[1], "per-site table")
        same_bits(got[2], want[2], "window table")
        eng.set_option("record_lds_bytes", 12 * 1024)
        eng.upload_sites(rows[::2], nr[::2], na[::2], W)
        after_upload(eng, (rows[::2], nr[::2], na[::2], W), 1, "default budget again")
        got2 = tables(eng)
        assert got2[0] == 2
        same_bits(got2[1], want2[1], "second upload: per-site table")
        same_bits(got2[2], want2[2], "second upload: window table")


# --------------------------------------------------------------------------- 5. the messages, full text
def message(call, *args, **kw):
    with pytest.raises(E.EngineError) as ei:
        call(*args, **kw)
    return str(ei.value)


def raw_upload(eng, fn, row, ref, alt, n, window):
    """The entry point with the pointers as given (None = NULL)."""
    p = lambda a: None if a is None else a.ctypes.data
    eng._chk(getattr(eng.lib, fn)(eng.ctx, p(row), p(ref), p(alt), None, n, window))


def raw_candidates(eng, row, ref, alt, n):
    p = lambda a: None if a is None else a.ctypes.data
    eng._chk(eng.lib.ibdg_upload_candidates(eng.ctx, p(row), p(ref), p(alt), None, n))


def test_messages_and_what_they_leave(panel):
    """Every message of the group a caller can reach, word for word -- the checks shared by the entry points say
    ibdg_upload_sites whoever called them --, and the context after each: a call refused by its checks leaves the list
    before it (and the candidates) in place; a list stage A refuses leaves no sites, ld_layout 0 and "no sites" for a run."""
    _, lst, _ = outcome_lists()[0]
    rows, nr, na, W = lst
    one = np.ones(4, np.uint8)
    idx = np.arange(4, dtype=np.uint32)
    NO_PANEL = "[::] ERROR in ibdg_upload_sites: no panel uploaded"
    with E.Engine(0, 0.02, 20) as eng:
        assert message(eng.upload_sites, idx, one, one, 100) == NO_PANEL
        assert message(raw_upload, eng, "ibdg_upload_sites_dev", idx, one, one, 4, 100) == NO_PANEL     # (host pointers: never read)
        assert message(eng.upload_candidates, idx, one, one) == NO_PANEL
        assert message(eng.select_variable_sites, 0, 100) == "[::] ERROR in ibdg_select_variable_sites: no panel uploaded"
        assert eng.n_sites == 0 and eng.n_windows == 0 and eng.ld_layout() == 0 and eng.n_candidates == 0
        assert message(eng.run, [T], ld=True) == "[::] ERROR in ibdg_run: no panel uploaded"
    with engine(panel) as eng, engine(panel) as ref:
        ref.upload_sites(rows, nr, na, W)
        want = tables(ref)
        NO_SITES = "[::] ERROR in ibdg_run: no sites uploaded"
        assert message(eng.run, [T], ld=True) == NO_SITES
        assert message(eng.select_variable_sites, 0, 100) == "[::] ERROR in ibdg_select_variable_sites: no candidates uploaded"
        eng.upload_sites(rows, nr, na, W)

        def intact(what):
            after_upload(eng, lst, 1, what)
            got = tables(eng)
            same_bits(got[1], want[1], what + ": per-site table")
            same_bits(got[2], want[2], what + ": window table")

        # refused by the checks: the list before stays
        WINDOW = "[::] ERROR: Invalid window size (-w) of 0 (must be >= 1)."
        NULL = "[::] ERROR in ibdg_upload_sites: NULL input array"
        assert message(eng.upload_sites, idx, one, one, 0) == WINDOW
        assert message(raw_upload, eng, "ibdg_upload_sites_dev", idx, one, one, 4, 0) == WINDOW
        assert message(raw_upload, eng, "ibdg_upload_sites", idx, None, one, 4, 100) == NULL
        assert message(raw_upload, eng, "ibdg_upload_sites", idx, one, None, 4, 100) == NULL
        assert message(raw_upload, eng, "ibdg_upload_sites_dev", idx, None, one, 4, 100) == NULL
        assert message(raw_candidates, eng, idx, one, None, 4) == NULL
        assert (message(raw_upload, eng, "ibdg_upload_sites", idx, one, one, 2 ** 32, 100)
                == "[::] ERROR in ibdg_upload_sites: more than 2^32-1 rows in one call")              # (the arrays are never read)
        many = np.ones(LP + 1, np.uint8)
        IMPLICIT = f"[::] ERROR in ibdg_upload_sites: row_index[{LP}]={LP} outside the panel ({LP} rows)"
        assert message(eng.upload_sites, None, many, many, 100) == IMPLICIT
        assert message(eng.upload_candidates, None, many, many) == IMPLICIT
        intact("after the checks' refusals")
        # the candidates' own checks: the candidates before stay, and so does the list
        eng.upload_candidates(rows, nr, na)
        bad_rows = rows.copy()
        bad_rows[10] = LP + 7
        deep = nr.copy()
        deep[20] = 21
        assert (message(eng.upload_candidates, bad_rows, deep, na)
                == f"[::] ERROR in ibdg_upload_candidates: row_index[10]={LP + 7} outside the panel ({LP} rows)")
        assert (message(eng.upload_candidates, rows, deep, na)
                == f"[::] ERROR in ibdg_upload_candidates: candidate 20 has n_ref+n_alt={21 + int(na[20])} > max_cov=20")
        assert eng.n_candidates == len(rows)
        assert (message(eng.select_variable_sites, N, 100)
                == f"[::] ERROR in ibdg_select_variable_sites: individual {N} outside the panel ({N} individuals)")
        assert message(eng.select_variable_sites, 0, 0) == WINDOW
        intact("after the candidates' refusals")
        # refused by stage A: no sites are left
        for what, r, a, text in (
                ("row", bad_rows, nr, f"[::] ERROR in ibdg_upload_sites: row_index[10]={LP + 7} outside the panel ({LP} rows)"),
                ("reads", rows, deep, f"[::] ERROR in ibdg_upload_sites: site 20 has n_ref+n_alt={21 + int(na[20])} > max_cov=20"),
                ("row and reads of one site", bad_rows, np.where(np.arange(len(nr)) == 10, 21, nr).astype(np.uint8),
                 f"[::] ERROR in ibdg_upload_sites: row_index[10]={LP + 7} outside the panel ({LP} rows)"),
                ("reads before row", bad_rows, np.where(np.arange(len(nr)) == 9, 21, nr).astype(np.uint8),
                 f"[::] ERROR in ibdg_upload_sites: site 9 has n_ref+n_alt={21 + int(na[9])} > max_cov=20")):
            assert message(eng.upload_sites, r, a, na, W) == text, what
            assert eng.n_sites == 0 and eng.n_windows == 0 and eng.ld_layout() == 0, what
            assert message(eng.run, [T], ld=True) == NO_SITES, what
        # ... and a good upload works, from the host and from the candidates
        eng.upload_sites(rows, nr, na, W)
        intact("a good upload after stage A's refusals")
        eng.select_variable_sites(T, W)
        assert 0 < eng.n_sites < len(rows) and eng.ld_layout() in (1, 2)
        cand = eng.site_candidates()
        ref.upload_sites(rows[cand], nr[cand], na[cand], W)
        sel, sel_ref = tables(eng), tables(ref)
        same_bits(sel[1], sel_ref[1], "selected list: per-site table")
        same_bits(sel[2], sel_ref[2], "selected list: window table")
