"""GPU tier: every grid-stride kernel past its first trip, and the options no other test sets.

The rest of the seconds-scale tier runs at shapes where each kernel's work-distribution loop executes once (the only other
test whose loops wrap is tests/test_gpu_fullsize.py: minutes, one shape and one form per kernel).  Here:
  1. k_prep_scan (stage A, stage B and ibdg_select_variable_sites) past 1024 blocks of 1024 elements -- a second pass with
     carry_s -- and the atomicMin of an offending site from a block beyond the first pass;
  2. k_rows_windows<ROWS_TAB|ROWS_FULL> and k_win_ibd2 on several trips of `g += gridDim.x * 4`, against the oracle;
  3. k_alt_count<LOADS> past its block cap at upload and beside an --LD kernel, k_alt_count_long past its wave count, every
     one with a partial last group;
  4. k_llr_partial past LLR_MAX_BLOCKS items;
  5. the options sum_dpp 0, end_in_dispatch 0, reserve_compact 0, compact_density, stage_workers;
  6. ring_slots 2, 3, 4, 8 in every counting form (vector, matrix-core, IBD1, groups of four), tables in LDS and in memory.

Every multi-trip test restates the formula of its launch wrapper (next to the name of the lines it mirrors) and asserts the
trip count BEFORE it compares anything: a shape that stops wrapping must fail, not pass with one trip.  No numeric bar is
new: bit equality, the 1e-10 bar of assert_ld_close, the hp_ref bounds and the 2^-50 bound of the arm-stats model.

stage_workers: the test of staged_upload (tests/test_gpu_fullsize.py) needs a panel of 256 MB in host memory to reach
the staging team, which is no seconds-scale test, so it is left as it is; ibdg_upload_panel_fd goes through the same team at
any size, and the option is set there (1 and 3 threads, more pieces than threads)."""
import functools
import math

import numpy as np
import pytest

import hp_ref as H
from gap_cases import run_structure
from ibdgem_amd import engine as E
from test_gpu_arm_stats import check_against_model, random_case
from test_gpu_parity import assert_bits, assert_ld_close, synth, windows_numpy
from test_gpu_precision import FORMS, _shape_case, band_case, run_form, tab_in_lds

pytestmark = pytest.mark.gpu


def cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def n_cu():
    """The CU count the engine reads (ibdg_create: hipDeviceAttributeMultiprocessorCount, 256 where that fails)."""
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count
    return n if n > 0 else 256


# --------------------------------------------------------------------------- the launch wrappers, restated
def scan_passes(n):
    """k_prep_scan: blocks_for(n) = ceil(n / PREP_BLOCK) block totals (PREP_BLOCK = 256 threads x 4 items), scanned by one
    block of 1024 threads in passes of 1024 (`for (base = 0; base < n; base += 1024)`)."""
    return cdiv(cdiv(n, 1024), 1024)


def rows_trips(n_win, T, per_cu):
    """launch_rows_windows: a wave per group of IBDG_ROWS_WPW = 2 windows, four waves per block, `max_blocks` when given;
    the kernels' loop is `g = blockIdx.x * 4 + wave; g < n_groups; g += gridDim.x * 4`.  max_blocks (plan_run's
    P.row_blocks with site_blocks_per_cu in an --LD run without recount and without a matrix-core group; ibdg_run's
    `blocks` with rows_blocks_per_cu in a non-LD run) = max(1, n_cu * per_cu / T); per_cu 0: the full grid."""
    groups = cdiv(max(n_win, 1), 2)
    blocks = cdiv(groups, 4)
    if per_cu > 0:
        blocks = min(blocks, max(1, n_cu() * per_cu // T))
    return cdiv(groups, 4 * blocks)


def panel_stride(n_ids):
    """prepare_panel / pick_cpw: 64-bit words per device row = 2 * cpw * ceil(chunks / cpw), cpw = min(chunks, 5)."""
    chunks = cdiv(n_ids, 64)
    cpw = min(chunks, 5)
    return 2 * cpw * cdiv(chunks, cpw)


def alt_count_launch(n_ids, n_rows, max_blocks=0):
    """launch_alt_count: 16-byte units per row `pairs`, g = gcd(pairs, 64), 64 / g rows and pairs / g loads per group;
    the LDS form while loads * 64 * 4 <= 16 KiB, with min(groups, 256 * 32 * 4, max_blocks or inf) single-wave blocks
    (`grp += gridDim.x`); otherwise k_alt_count_long with min(ceil(rows / 4), 256 * 32) blocks of four waves, one row per
    wave and trip (`r += n_waves`)."""
    pairs = panel_stride(n_ids) // 2
    g = math.gcd(pairs, 64)
    loads = pairs // g
    if loads * 64 * 4 <= 16 * 1024:
        R = 64 // g
        groups = cdiv(n_rows, R)
        blocks = min(groups, 256 * 32 * 4)
        if max_blocks:
            blocks = min(blocks, max_blocks)
        return dict(form="lds", loads=loads, rows_per_group=R, trips=cdiv(groups, blocks), tail_rows=n_rows % R)
    blocks = min(cdiv(n_rows, 4), 256 * 32)
    return dict(form="long", loads=loads, trips=cdiv(n_rows, 4 * blocks))


def llr_launch(T, first, end):
    """ibdg_window_llr_sums / launch_llr_sums: nb = blocks of LLR_BLK = 2048 windows of the longest range (>= 1), one item
    per (individual, range, block), min(items, LLR_MAX_BLOCKS = 8192) blocks (`item += gridDim.x`)."""
    nb = max([1] + [cdiv(int(e) - int(f), 2048) for f, e in zip(first, end)])
    items = T * len(first) * nb
    return dict(nb=nb, items=items, trips=cdiv(items, min(items, 8192)))


# --------------------------------------------------------------------------- 1. the three-kernel scan past 1024 blocks
SCAN_N, SCAN_W = 3, 100


def pack_few(alle):
    """pack_alleles_fast's layout for up to 64 individuals without its [L][64][2] intermediate."""
    L, n_ids = alle.shape[0], alle.shape[1] // 2
    assert n_ids <= 64
    out = np.zeros((L, 2), dtype=np.uint64)
    for n in range(n_ids):
        out[:, 0] |= alle[:, 2 * n].astype(np.uint64) << np.uint64(n)
        out[:, 1] |= alle[:, 2 * n + 1].astype(np.uint64) << np.uint64(n)
    assert (out[:500] == E.pack_alleles_fast(alle[:500])).all()
    return out


_SCAN = {}


def scan_case(shape, oracle):
    """(a) 1 048 577 rows, every one covered: 1025 blocks for both scans, one element in the second pass; (b) 1 300 000 rows
    with synth's Poisson(2) depths: 1270 and 1099 blocks.  Made once, with the oracle's answers; nobody changes them."""
    if shape not in _SCAN:
        L = {"a": 1_048_577, "b": 1_300_000}[shape]
        alle, nr, na = synth(1, L, SCAN_N)
        if shape == "a":
            nr[(nr.astype(int) + na) == 0] = 1
        n_cov = int(((nr.astype(int) + na) > 0).sum())
        c = dict(L=L, alle=alle, nr=nr, na=na, n_cov=n_cov, packed=pack_few(alle), win=windows_numpy(nr, na, SCAN_W),
                 ld=oracle.compare(alle, nr, na, 1, window=SCAN_W, ld=True),
                 plain=oracle.compare(alle, nr, na, 1, window=SCAN_W, ld=False))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SCAN[shape] = c
    c = _SCAN[shape]
    # the precondition: a second pass of the site scan (rows) and of the segment scan (covered rows)
    assert scan_passes(c["L"]) == 2 and scan_passes(c["n_cov"]) == 2, (c["L"], c["n_cov"])
    if shape == "a":
        assert c["n_cov"] == c["L"] == 1024 * 1024 + 1
    else:
        assert c["n_cov"] > 1_048_576
    return c


@pytest.mark.parametrize("tiles", [-1, 1])
@pytest.mark.parametrize("shape", ["a", "b"])
def test_site_and_segment_scans_carry_into_a_second_pass(oracle, shape, tiles):
    """Stage A (k_prep_site_count, k_prep_scan, k_prep_site_scatter) and stage B (k_prep_seg_count, k_prep_scan,
    k_prep_seg_scatter; both seg_start forms: the panel's own tiles and the compacted ones) with more than 1024 block totals:
    the window bounds, an --LD run and a non-LD run of one individual against the oracle."""
    c = scan_case(shape, oracle)
    L = c["L"]
    with E.Engine(0, 0.02, 20) as eng:
        eng.set_option("compact_tiles", tiles)
        eng.upload_panel(c["packed"], SCAN_N)
        eng.upload_sites(np.arange(L, dtype=np.uint32), c["nr"], c["na"], SCAN_W)
        assert eng.n_sites == L
        first, last, ncov = eng.windows()
        assert len(first) == len(c["win"][0]) == cdiv(c["n_cov"], SCAN_W)
        for got, want in zip((first, last, ncov), c["win"]):
            assert np.array_equal(got, want)
        eng.run([1], ld=True)
        assert eng.last_ld_variant() == 2 and eng.ld_layout() == (2 if tiles == 1 else 1)
        site, win = eng.site_ll(0), eng.window_ll(0)
        assert_bits(site, c["ld"]["site"], f"shape {shape} --LD per-site values")
        assert_bits(win[:, 2], c["ld"]["win"][:, 2], f"shape {shape} LIBD2")
        assert_ld_close(win[:, :2], c["ld"]["win"][:, :2], f"shape {shape} tiles {tiles} --LD windows")
        eng.run([1], ld=False)
        assert_bits(eng.site_ll(0), c["plain"]["site"], f"shape {shape} non-LD per-site values")
        assert_bits(eng.window_ll(0), c["plain"]["win"], f"shape {shape} non-LD windows")


@pytest.mark.parametrize("shape", ["a", "b"])
def test_selection_scan_carries_into_a_second_pass(oracle, shape):
    """The same rows as -v candidates: k_sel_count, k_prep_scan and k_sel_scatter over more than 1024 blocks."""
    c = scan_case(shape, oracle)
    L, alle, nr, na = c["L"], c["alle"], c["nr"], c["na"]
    assert scan_passes(L) == 2
    with E.Engine(0, 0.02, 20) as eng, E.Engine(0, 0.02, 20) as ref:
        eng.upload_panel(c["packed"], SCAN_N)
        ref.upload_panel(c["packed"], SCAN_N)
        for rows in (None, np.arange(L, dtype=np.uint32)):
            eng.upload_candidates(rows, nr, na)
            assert eng.n_candidates == L
            for t in (0, 2):
                keep = (alle[:, 2 * t] | alle[:, 2 * t + 1]) != 0
                sel = np.flatnonzero(keep)
                assert 1024 * 256 < len(sel) < L                  # (a proper subset, so the ranks depend on every block total)
                eng.select_variable_sites(t, SCAN_W)
                assert np.array_equal(eng.site_candidates(), sel), (rows is None, t)
                ref.upload_sites(sel, nr[keep], na[keep], SCAN_W)
                assert eng.n_sites == ref.n_sites == len(sel) and eng.n_windows == ref.n_windows
                for a, b in zip(eng.windows(), ref.windows()):
                    assert np.array_equal(a, b), (rows is None, t)


def test_first_offending_site_beyond_the_first_pass(oracle):
    """Two offending sites in blocks 1171 and 1220 of k_prep_site_count: the smaller one is reported (atomicMin)."""
    c = scan_case("b", oracle)
    L = c["L"]
    lo, hi = 1_200_000, 1_250_000
    assert lo // 1024 >= 1024 and hi // 1024 > lo // 1024 and hi < L
    rows = np.arange(L, dtype=np.uint32)
    with E.Engine(0, 0.02, 20) as eng:
        eng.upload_panel(c["packed"], SCAN_N)
        bad_rows = rows.copy()
        bad_rows[hi], bad_rows[lo] = L, L + 3
        with pytest.raises(E.EngineError, match=rf"row_index\[{lo}\]={L + 3} outside the panel"):
            eng.upload_sites(bad_rows, c["nr"], c["na"], SCAN_W)
        bad_nr = c["nr"].copy()
        bad_nr[hi], bad_nr[lo] = 25, 21
        with pytest.raises(E.EngineError, match=rf"site {lo} has n_ref\+n_alt=2[1-9]"):
            eng.upload_sites(rows, bad_nr, c["na"], SCAN_W)
        with pytest.raises(E.EngineError, match="no sites"):
            eng.run([1], ld=True)
        eng.upload_sites(rows, c["nr"], c["na"], SCAN_W)          # and the context takes a good list afterwards
        assert eng.n_windows == len(c["win"][0])


# --------------------------------------------------------------------------- 2. k_rows_windows / k_win_ibd2 on several trips
ROWS_N, ROWS_W = 70, 2
_ROWS = {}


def rows_case(L):
    """Window 2 over synth's depths: thousands of windows, an odd number of them (the last group holds one window), rows
    without reads in front of window 0, between the windows and behind the last one -- in different trips."""
    if L not in _ROWS:
        seed = {12001: 201, 20001: 89}[L]
        alle, nr, na = synth(seed, L, ROWS_N)
        for v in (alle, nr, na):
            v.setflags(write=False)
        _ROWS[L] = dict(L=L, alle=alle, nr=nr, na=na, packed=E.pack_alleles_fast(alle), oracle={})
    c = _ROWS[L]
    cov = (c["nr"].astype(int) + c["na"]) > 0
    c["n_win"] = cdiv(int(cov.sum()), ROWS_W)
    assert c["n_win"] % 2 == 1, c["n_win"]
    assert not cov[-1] and not cov[0] and (~cov[1:-1]).any()
    return c


def rows_oracle(oracle, c, t, ld):
    if (t, ld) not in c["oracle"]:
        c["oracle"][t, ld] = oracle.compare(c["alle"], c["nr"], c["na"], t, window=ROWS_W, ld=ld)
    return c["oracle"][t, ld]


def rows_runs(c, opts, runs):
    """One context with `opts`; the runs [(targets, ld)] in turn on one upload.  Per run: the window tables, the per-site
    tables (None where none are kept) and the --LD variant."""
    out = []
    with E.Engine(0, 0.02, 20) as eng:
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.upload_panel(c["packed"], ROWS_N)
        eng.upload_sites(np.arange(c["L"], dtype=np.uint32), c["nr"], c["na"], ROWS_W)
        assert eng.n_windows == c["n_win"]
        for targets, ld in runs:
            eng.run(targets, ld=ld)
            keep = opts.get("site_results", 1) != 0
            out.append(dict(win=[eng.window_ll(i) for i in range(len(targets))],
                            site=[eng.site_ll(i) for i in range(len(targets))] if keep else None,
                            variant=eng.last_ld_variant()))
    return out


def rows_check(oracle, c, runs, got, full, checked, what):
    """Every run of `got` against the oracle for the checked individuals, and bit for bit against `full` (the full grid)."""
    for (targets, ld), g, f in zip(runs, got, full):
        assert g["variant"] == f["variant"] == (2 if ld else 0), what
        for i in range(len(targets)):
            assert_bits(g["win"][i], f["win"][i], f"{what}: windows of #{i} vs the full grid")
            if g["site"] is not None:
                assert_bits(g["site"][i], f["site"][i], f"{what}: per-site values of #{i} vs the full grid")
        for i in checked(len(targets)):
            res = rows_oracle(oracle, c, targets[i], ld)
            assert len(g["win"][i]) == len(res["win"]) == c["n_win"]
            if g["site"] is not None:
                assert_bits(g["site"][i], res["site"], f"{what}: per-site values of #{i}")
            if ld:
                assert_bits(g["win"][i][:, 2], res["win"][:, 2], f"{what}: LIBD2 of #{i}")
                assert_ld_close(g["win"][i][:, :2], res["win"][:, :2], f"{what}: --LD windows of #{i}")
            else:
                assert_bits(g["win"][i], res["win"], f"{what}: windows of #{i}")


ROWS_CASES = {
    # name: L, the option, its value, further options, the runs, the individuals checked against the oracle
    # ROWS_TAB builds the row table in the first run on an upload; the second run, of another individual, is k_win_ibd2
    "site_blocks 1: row table, then k_win_ibd2": (12001, "site_blocks_per_cu", 1, {}, [([7], True), ([33], True)],
                                                   lambda T: [0]),
    "site_blocks 1: k_win_ibd2 from the start": (12001, "site_blocks_per_cu", 1, {"site_results": 0}, [([7], True)],
                                                  lambda T: [0]),
    # nine individuals through the counting kernels: k_row_table, then k_win_ibd2 with gridDim.y = 9
    "site_blocks 2 (default), nine individuals": (12001, "site_blocks_per_cu", 2, {"mfma_targets": 0},
                                                  [([3, 69, 12, 40, 0, 55, 21, 8, 64], True)], lambda T: [0, 4, 8]),
    "rows_blocks 1, non-LD": (12001, "rows_blocks_per_cu", 1, {}, [([7], False), ([5, 69, 0, 33, 18], False)],
                              lambda T: range(T)),
    # no option set: beside the --LD kernel the per-row kernel already wraps past 4096 windows at 256 CUs
    "defaults, 8645 windows": (20001, "site_blocks_per_cu", None, {}, [([7], True), ([33], True)], lambda T: [0]),
}


@pytest.mark.parametrize("name", list(ROWS_CASES))
def test_row_and_window_kernels_on_several_trips(oracle, name):
    L, option, value, more, runs, checked = ROWS_CASES[name]
    c = rows_case(L)
    per_cu = 2 if value is None else value                # (ibdg_ctx::Options::site_blocks = 2)
    for targets, ld in runs:
        trips = rows_trips(c["n_win"], len(targets), per_cu)
        assert trips >= 2, (name, trips)
        if n_cu() == 256:
            assert trips >= 3, (name, trips)
        assert rows_trips(c["n_win"], len(targets), 0) == 1
    opts = dict(more) if value is None else dict(more, **{option: value})
    got = rows_runs(c, opts, runs)
    full = rows_runs(c, dict(more, **{option: 0}), runs)
    rows_check(oracle, c, runs, got, full, checked, name)


# --------------------------------------------------------------------------- 3. alt counts on several trips
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def random_words(seed, L, n_ids):
    """Packed rows made directly ([L][ibdg_row_words] 64-bit words; an (L, 2N) byte matrix would be gigabytes): every
    other row thinned, the lanes >= n_ids zero."""
    rng = np.random.default_rng(seed)
    chunks = cdiv(n_ids, 64)
    top = int(np.iinfo(np.uint64).max)
    w = rng.integers(0, top, size=(L, 2 * chunks), dtype=np.uint64, endpoint=True)
    w[::2] &= rng.integers(0, top, size=(cdiv(L, 2), 2 * chunks), dtype=np.uint64, endpoint=True)
    if n_ids % 64:
        w[:, -2:] &= np.uint64((1 << (n_ids % 64)) - 1)
    return w


def popcounts(words):
    return _POP8[words.view(np.uint8)].reshape(len(words), -1).sum(axis=1, dtype=np.uint32)


def test_upload_time_alt_count_past_its_block_cap():
    """One 16-byte unit per row, 64 rows per group: 32 770 groups for 32 768 blocks, the last group partial."""
    N, L = 3, 2_097_152 + 100
    k = alt_count_launch(N, L)
    assert k == dict(form="lds", loads=1, rows_per_group=64, trips=2, tail_rows=36), k
    words = random_words(3, L, N)
    want = popcounts(words)
    assert want.max() == 6 and want.min() == 0
    with E.Engine() as eng:
        eng.upload_panel(words, N)
        got = eng.alt_counts(0, L)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{len(bad)} rows, first {bad[0]} (group {bad[0] // 64}): {got[bad[0]]} vs {want[bad[0]]}"


@pytest.mark.parametrize("N,L,loads,rows_per_group", [(100, 20_011, 1, 32), (2504, 5003, 5, 8), (700, 20_011, 0, 64)])
def test_recount_beside_the_ld_kernel_on_several_trips(N, L, loads, rows_per_group):
    """count_in_run 1 with recount_blocks_per_cu 1: n_cu single-wave blocks of k_alt_count<LOADS> walk all groups, the last
    one partial (the unit_end clamp).  The counts exist only through the run (the option is set before the panel goes up),
    equal numpy's, give the AF column, and the run's results are those of a context that counted at upload."""
    k = alt_count_launch(N, L, n_cu() * 1)
    assert k["form"] == "lds" and k["rows_per_group"] == rows_per_group and k["tail_rows"] != 0, k
    assert k["loads"] == loads if loads else k["loads"] > 8, k           # (more than 8 loads: the LOADS == 0 form)
    assert k["trips"] >= 2, k
    words = random_words(N, L, N)
    want = popcounts(words)
    rng = np.random.default_rng(L)
    nr, na = rng.integers(0, 3, size=L).astype(np.uint8), rng.integers(0, 3, size=L).astype(np.uint8)
    out = {}
    for in_run in (0, 1):
        with E.Engine() as eng:
            if in_run:
                eng.set_option("count_in_run", 1)
                eng.set_option("recount_blocks_per_cu", 1)
            eng.upload_panel(words, N)
            if in_run:
                with pytest.raises(E.EngineError, match="counts not computed yet"):
                    eng.alt_counts(0, L)
            eng.upload_sites(None, nr, na, 100)
            eng.run([N - 1], ld=True)
            assert (eng.last_run_ms()["alt_count"] > 0) == bool(in_run)
            got = eng.alt_counts(0, L)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, f"in_run {in_run}: {len(bad)} rows, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
            assert_bits(eng.site_af(), want / float(2 * N), "AF")
            out[in_run] = (eng.last_ld_variant(), eng.site_ll(0), eng.window_ll(0))
    assert out[0][0] == out[1][0]
    assert_bits(out[1][1], out[0][1], "per-site values, recount in the run")
    assert_bits(out[1][2], out[0][2], "windows, recount in the run")


def test_wave_per_row_alt_count_past_its_wave_count():
    """k_alt_count_long at the smallest panel that takes it: 8192 blocks of four waves, 33 001 rows."""
    N = next(n for n in range(1, 1 << 14) if alt_count_launch(n, 1)["form"] == "long")
    assert alt_count_launch(N - 1, 1)["form"] == "lds" and alt_count_launch(N, 1)["loads"] * 256 > 16 * 1024
    L = 33_001
    assert alt_count_launch(N, L)["trips"] == 2
    words = random_words(5, L, N)
    assert words.shape[1] == 2 * cdiv(N, 64) < panel_stride(N)            # (the device rows are padded: units of zeros)
    want = popcounts(words)
    with E.Engine() as eng:
        eng.upload_panel(words, N)
        got = eng.alt_counts(0, L)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"N={N}: {len(bad)} rows, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


# --------------------------------------------------------------------------- 4. k_llr_partial past LLR_MAX_BLOCKS
def llr_ranges(n):
    pts = [2047, 2048, 2049, 4095, 4096, 4097]
    r = [(7, 7), (5, 6), (0, n)]                                          # empty, one window, the whole table
    r += [(0, p) for p in pts] + [(p, n) for p in pts] + [(p, q) for p in pts for q in pts if p < q]
    rng = np.random.default_rng(n)
    while len(r) < 50:
        a, b = sorted(int(x) for x in rng.integers(0, n + 1, size=2))
        r.append((a, b))
    return [a for a, _ in r], [b for _, b in r]


@pytest.mark.parametrize("ld", [True, False])
def test_llr_sums_past_the_block_cap(ld):
    """61 individuals x 50 ranges x 3 blocks of windows = 9150 items for 8192 blocks: red[][] reused by the blocks that take a
    second item.  The sums hold the model's bound, and the same ranges asked ten at a time (every launch short of a trip,
    other numbers of blocks per range) return the same bytes."""
    N, T = 70, 61
    alle, nr, na = random_case(31, N=N, L=12000)
    targets = [int(t) for t in np.random.default_rng(61).choice(N, size=T, replace=False)]
    with E.Engine(0, 0.02, 20) as e:
        e.upload_panel(E.pack_alleles_fast(alle), N)
        e.upload_sites(np.arange(len(nr)), nr, na, 2)
        n = e.n_windows
        first, end = llr_ranges(n)
        k = llr_launch(T, first, end)
        assert len(first) == 50 and k == dict(nb=3, items=9150, trips=2), (n, k)
        e.run(targets, ld=ld)
        _, got = check_against_model(e, T, first, end)
        assert (got[:, 0] == 0).all() and got[:, 1].any()
        beyond = got.reshape(-1, 4)[cdiv(8192, k["nb"]):]                  # (item = (t * n_seg + s) * nb + b)
        assert len(beyond) > 0 and np.count_nonzero(np.nan_to_num(beyond)) > len(beyond)
        parts = []
        for s in range(0, 50, 10):
            assert llr_launch(T, first[s:s + 10], end[s:s + 10])["trips"] == 1
            parts.append(e.window_llr_sums(first[s:s + 10], end[s:s + 10]))
        assert np.concatenate(parts, axis=1).tobytes() == got.tobytes()


# --------------------------------------------------------------------------- 5. the options no other test sets
DPP_FORMS = ["popcount mx1", "popcount IBD1 form", "popcount compacted"]


def dpp_input(which):
    if which == "bands":
        alle, nr, na = band_case(64, 100, 0.02)
        return alle, nr, na, 100, 0.02, 20, None, -1
    return _shape_case(which)


@pytest.mark.parametrize("which", [3, 7, "bands"])
def test_wave_sums_by_ds_swizzle(oracle, which):
    """sum_dpp 0: k_ld_popcount's second reduction path.  The hp_ref bound and the parity checks of run_form, the underflow
    bands, and the window tables of sum_dpp 1 bit for bit (the same additions).  The kernel reads the option only where the
    counts come from the matrix cores and the power tables sit in LDS: shape 7 and the bands must be such inputs (shape 3,
    whose windows hold thousands of reads, keeps its tables in memory: there the option must change nothing either)."""
    alle, nr, na, W, eps, M, refids, pu = dpp_input(which)
    L, N = alle.shape[0], alle.shape[1] // 2
    assert tab_in_lds(nr, na, W) == (which != 3), which               # the precondition: the swizzle path is reached
    for form in DPP_FORMS:
        spec = dict(FORMS[form], opts=dict(FORMS[form]["opts"], **{"sum_dpp": 0}))
        expect = None
        if form == "popcount IBD1 form":
            expect = dict(unit=3 if tab_in_lds(nr, na, W) else (2, 3))
        truths = run_form(oracle, form, alle, nr, na, W, eps, M, refids=refids, pu=pu, seed=1, expect=expect, spec=spec)
        if which == "bands":
            for key in ("ibd0", "ibd1"):
                counts = H.band_counts(truths[0][key])
                assert all(n >= 1 for n in counts.values()), (form, key, counts)
        tables = {}
        for dpp in (0, 1):
            with E.Engine(0, eps, M) as eng:
                for k, v in dict(FORMS[form]["opts"], **{"sum_dpp": dpp}).items():
                    eng.set_option(k, v)
                eng.upload_panel(E.pack_alleles_fast(alle), N)
                eng.upload_sites(np.arange(L), nr, na, W)
                eng.run([0], ld=True, pu_id=pu)
                assert eng.last_ld_variant() == 2 and eng.last_count_unit() in (2, 3)
                tables[dpp] = eng.window_ll(0)
        assert_bits(tables[0], tables[1], f"{form}: sum_dpp 0 vs 1")


# --------------------------------------------------------------------------- 6. every counting form at every ring depth
RING_DEPTHS = (2, 3, 4, 8)
# form -> FORMS entry, further options, comparison individuals, ibdg_last_count_unit with the power tables in LDS / in
# global memory (the IBD1 form needs them in LDS and falls back to the matrix-core form that counts everything).  Groups of
# four: T = 5 is one group in k_ld_popcount_mt plus one single launch, whose unit is the one reported (ibd0_after 1: the
# IBD1 form where it can be); T = 4 leaves no single launch (unit 0), so the group kernel is what ran.
RING_FORMS = {
    "vector": ("popcount mx0", {}, 1, 1, 1),
    "matrix all-terms": ("popcount mx1", {}, 1, 2, 2),
    "IBD1": ("popcount IBD1 form", {}, 1, 3, 2),
    "groups of four": ("popcount_mt T4", {"ibd0_after": 1}, 5, 3, 2),
}
# placement -> N, L, W, tables in LDS.  In LDS: N = 130 is three chunks, the last partial.  In global memory: a window of
# 1024 rows holds about 2000 reads, well past the 767 whose tables fit.
RING_PLACEMENTS = {"tables in LDS": (130, 3000, 100, True), "tables in global memory": (70, 2600, 1024, False)}
# uniform runs of 16 windows (guided_runs 0; windows_per_wave fixes the run length, ibdg_api.cpp build_segments), and a
# record budget that never halves them
RING_RUN_OPTS = {"windows_per_wave": 16, "guided_runs": 0, "record_lds_bytes": 96 * 1024}


@functools.lru_cache(maxsize=None)
def ring_case(placement):
    N, L = RING_PLACEMENTS[placement][:2]
    return synth(97, L, N, 2.0)


def ring_runs(nr, na, W):
    """make_runs (ibdg_api.cpp) without guided lengths: runs of windows_per_wave windows, the last one shorter; the run
    length stands while a run's records fit the budget, max_seg * (sizeof(Seg) + 8) <= record_lds_bytes (build_segments).
    Per run on the panel's own tiles (layout 1: row = position in the site list): tile pairs spanned.  (The model itself is
    gap_cases.run_structure, shared with the gap cases; it asserts the budget.)"""
    return run_structure(nr, na, W, RING_RUN_OPTS["windows_per_wave"], RING_RUN_OPTS["record_lds_bytes"])["pairs"]


def ring_run(form_opts, ring, alle, nr, na, W, eps, M, targets, unit, what):
    L, N = alle.shape[0], alle.shape[1] // 2
    with E.Engine(0, eps, M) as eng:
        for k, v in dict(form_opts, ring_slots=ring).items():
            eng.set_option(k, v)
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        eng.upload_sites(np.arange(L), nr, na, W)
        eng.run(targets, ld=True)
        assert eng.last_ld_variant() == 2 and eng.ld_layout() == 1, what
        assert eng.last_count_unit() == unit, (what, eng.last_count_unit())
        return [eng.window_ll(i) for i in range(len(targets))]


@pytest.mark.parametrize("placement", list(RING_PLACEMENTS))
@pytest.mark.parametrize("form", list(RING_FORMS))
def test_every_counting_form_at_every_ring_depth(oracle, form, placement):
    """ring_slots 2, 3, 4, 8 in all four counting forms (both guard policies of the tile ring: the vector forms stop at the
    run's last pair, the matrix-core forms request it again), with the power tables in LDS and in global memory.  Depth 2
    goes through run_form -- the oracle and the hp_ref bound --, the other depths must give its bits.  Before anything is
    compared: the longest run spans three laps of the deepest ring."""
    N, L, W, in_lds = RING_PLACEMENTS[placement]
    alle, nr, na = ring_case(placement)
    eps, M = 0.02, 20
    assert tab_in_lds(nr, na, W) == in_lds, placement                 # the precondition: where the tables sit
    pairs = ring_runs(nr, na, W)
    assert all(max(pairs) >= 3 * ring for ring in RING_DEPTHS), pairs  # ... and every depth wraps at least three times
    name, more, T, unit_lds, unit_mem = RING_FORMS[form]
    unit = unit_lds if in_lds else unit_mem
    opts = dict(FORMS[name]["opts"], **more, **RING_RUN_OPTS)
    first = {}
    run_form(oracle, name, alle, nr, na, W, eps, M, seed=5, spec=dict(FORMS[name], T=T, unit=unit, opts=dict(opts, ring_slots=2)),
             keep=first)
    targets, ref = first["targets"], first["windows"]
    for ring in RING_DEPTHS[1:]:
        got = ring_run(opts, ring, alle, nr, na, W, eps, M, targets, unit, (form, placement, ring))
        for i, want in ref.items():
            assert_bits(got[i], want, f"{form}, {placement}: ring_slots {ring} vs 2, individual {i}")
    if T > 4:           # the group alone: no single launch is left, and its individuals' tables are the same bits
        for ring in RING_DEPTHS:
            got = ring_run(opts, ring, alle, nr, na, W, eps, M, targets[:4], 0, (form, placement, ring, "T = 4"))
            for i, want in ref.items():
                if i < 4:
                    assert_bits(got[i], want, f"{form}, {placement}: ring_slots {ring}, the group alone, individual {i}")


@pytest.mark.parametrize("dispatch_events", [0, 1])
def test_queued_runs_with_an_end_event_of_their_own(dispatch_events):
    """end_in_dispatch 0 (an event packet behind the --LD kernel instead of its completion signal): six queued runs over two
    individuals in turn end with the bits of the synchronous runs, and every run has its times."""
    N, L = 300, 5000
    alle, nr, na = synth(4321, L, N)
    people = [3, 299, 3, 299, 3, 299]
    with E.Engine() as eng:
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        eng.upload_sites(np.arange(L), nr, na, 100)
        want = {}
        for t in set(people):
            eng.run([t], ld=True)
            want[t] = eng.window_ll(0)
        assert not (want[3].tobytes() == want[299].tobytes())
        eng.set_option("end_in_dispatch", 0)
        eng.set_option("dispatch_events", dispatch_events)
        eng.set_option("async", 1)
        for n in (5, 6):
            for t in people[:n]:
                eng.run([t], ld=True)
            assert eng.last_ld_variant() == 2
            assert_bits(eng.window_ll(0), want[people[n - 1]], f"{n} queued runs")
        for back in range(6):
            ms = eng.run_ms(back)
            assert ms["total"] > 0 and ms["ld"] > 0 and ms["total"] >= ms["ld"], (back, ms)
        eng.sync()
        eng.set_option("async", 0)
        eng.run([3], ld=True)
        assert_bits(eng.window_ll(0), want[3], "back to synchronous")


def test_compacted_tiles_without_the_reserved_buffer(oracle):
    """reserve_compact 0 (set before the panel goes up): the buffer of the compacted tiles is allocated by the first site list
    that wants it and again by a longer one; the results are those of a context that reserved it."""
    N, Lp = 130, 6000
    alle, nr, na = synth(97, Lp, N)
    short = np.sort(np.random.default_rng(98).choice(Lp, size=1500, replace=False)).astype(np.uint32)
    lists = [short, np.arange(Lp, dtype=np.uint32)]
    out = {}
    for reserve in (0, 1):
        with E.Engine() as eng:
            eng.set_option("reserve_compact", reserve)
            eng.upload_panel(E.pack_alleles_fast(alle), N)
            eng.set_option("compact_tiles", 1)
            for k, rows in enumerate(lists):
                eng.upload_sites(rows, nr[rows], na[rows], 100)
                assert eng.ld_layout() == 2
                eng.run([5, 77], ld=True)
                assert eng.last_ld_variant() == 2 and eng.ld_layout() == 2
                out[reserve, k] = [(eng.site_ll(i), eng.window_ll(i)) for i in range(2)]
    for k, rows in enumerate(lists):
        for i, t in enumerate((5, 77)):
            assert_bits(out[0, k][i][0], out[1, k][i][0], f"list {k} individual {t}: per-site values")
            assert_bits(out[0, k][i][1], out[1, k][i][1], f"list {k} individual {t}: windows")
        res = oracle.compare(alle[rows], nr[rows], na[rows], 77, window=100, ld=True)
        assert_bits(out[0, k][1][0], res["site"], f"list {k}: per-site values vs oracle")
        assert_bits(out[0, k][1][1][:, 2], res["win"][:, 2], f"list {k}: LIBD2 vs oracle")
        assert_ld_close(out[0, k][1][1][:, :2], res["win"][:, :2], f"list {k}: --LD windows vs oracle")


@pytest.mark.parametrize("density", [2, 4, 16])
def test_compact_density_decides_the_layout(oracle, density):
    """compact_tiles 0: the compacted tiles when fewer than one panel row in compact_density between the first and the last
    site carries reads (sparse_sites: n_cov * density < rows spanned), the panel's own otherwise -- one covered row in d for d
    below, at and above the option's value; and the same bits from either layout."""
    N, L = 70, 4000
    alle, nr0, na0 = synth(400 + density, L, N)
    seen = set()
    for d in sorted({max(1, density - 1), density, density + 1}):
        nr, na = nr0.copy(), na0.copy()
        nr[(nr.astype(int) + na) == 0] = 1
        off = np.arange(L) % d != 0
        nr[off] = na[off] = 0                                           # reads on rows 0, d, 2d, ...: one row in d
        n_cov = int(((nr.astype(int) + na) > 0).sum())
        assert n_cov == cdiv(L, d)
        span = (L - 1) - 0 + 1                                          # panel rows from the first site's to the last site's
        layout = 2 if n_cov * density < span else 1
        assert layout == (2 if d > density else 1)
        seen.add(layout)
        got = {}
        for tiles in (0, -1, 1):
            with E.Engine() as eng:
                eng.set_option("compact_density", density)
                eng.set_option("compact_tiles", tiles)
                eng.set_option("ld_variant", 2)      # (a sparse list on the panel's own tiles would take the strict kernel)
                eng.upload_panel(E.pack_alleles_fast(alle), N)
                eng.upload_sites(None, nr, na, 100)
                eng.run([9], ld=True)
                assert eng.last_ld_variant() == 2
                assert eng.ld_layout() == {0: layout, -1: 1, 1: 2}[tiles], (density, d, tiles)
                got[tiles] = (eng.site_ll(0), eng.window_ll(0))
        for tiles in (-1, 1):
            assert_bits(got[0][0], got[tiles][0], f"density {density}, one row in {d}: per-site values, compact_tiles {tiles}")
            assert_bits(got[0][1], got[tiles][1], f"density {density}, one row in {d}: windows, compact_tiles {tiles}")
        res = oracle.compare(alle, nr, na, 9, window=100, ld=True)
        assert_bits(got[0][0], res["site"], "per-site values vs oracle")
        assert_bits(got[0][1][:, 2], res["win"][:, 2], "LIBD2 vs oracle")
        assert_ld_close(got[0][1][:, :2], res["win"][:, :2], f"density {density}, one row in {d} vs oracle")
    assert seen == {1, 2}


@pytest.mark.parametrize("workers", [1, 3])
def test_staging_team_of_fewer_threads(tmp_path, workers):
    """stage_workers: ibdg_upload_panel_fd stages five pieces of 8 MB with one thread and with three (a thread's two buffers
    in turn, threads with one and with two pieces): the rows on the device are those of an upload from host memory."""
    N, L = 2504, 60_000                       # 640-byte rows: 13 107 rows per piece, five pieces
    assert cdiv(L, (8 << 20) // 640) == 5
    words = random_words(workers, L, N)
    want = popcounts(words)
    nr, na = np.ones(L, np.uint8), (np.arange(L) % 3).astype(np.uint8)
    fn = tmp_path / "rows.bin"
    with open(fn, "wb") as fh:
        fh.write(b"\x5a" * 4096)
        fh.write(words.tobytes())
    with E.Engine() as eng:
        eng.upload_panel(words, N)
        eng.upload_sites(None, nr, na, 100)
        eng.run([2500], ld=True)
        ref = eng.window_ll(0)
        eng.set_option("stage_workers", workers)
        with open(fn, "rb") as fh:
            eng.upload_panel_fd(fh.fileno(), 4096, L, N)
            got = eng.alt_counts(0, L)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, f"{len(bad)} rows, first {bad[0]} (piece {bad[0] // 13107})"
            eng.upload_sites(None, nr, na, 100)
            eng.run([2500], ld=True)
            assert_bits(eng.window_ll(0), ref, f"panel staged by {workers} threads")
        with pytest.raises(E.EngineError, match="stage_workers must be"):
            eng.set_option("stage_workers", 0)


# --------------------------------------------------------------------------- 6. one context through every change of input
LIFE_N, LIFE_L = 130, 3000                    # three chunks of 64 individuals, the last one partial
LIFE_N2 = 70


def life_case():
    """synth at a mean depth of 0.7: about half of the rows carry reads.  (Checked with the oracle when the test was
    written: at every (panel, window) used below the --LD columns of all windows are finite and non-zero.)"""
    alle, nr, na = synth(7001, LIFE_L, LIFE_N, cov_mean=0.7)
    alle2 = synth(7002, LIFE_L, LIFE_N2)[0]
    n_cov = int(((nr.astype(int) + na) > 0).sum())
    assert 0.4 * LIFE_L < n_cov < 0.6 * LIFE_L and cdiv(LIFE_N, 64) == 3 and LIFE_N % 64 != 0
    bg = np.ones(LIFE_N, dtype=np.uint8)
    bg[::3] = 2
    bg[5] = 0
    return dict(alle=alle, alle2=alle2, nr=nr, na=na, bg=bg, rows=np.arange(LIFE_L, dtype=np.uint32))


def life_results(eng, T, site_of=()):
    win = [eng.window_ll(i) for i in range(T)]
    for w in win:
        assert np.isfinite(w).all() and (w != 0).all()              # (a comparison of zeros would prove nothing)
    return dict(win=win, site={i: eng.site_ll(i) for i in site_of}, variant=eng.last_ld_variant(),
                unit=eng.last_count_unit(), layout=eng.ld_layout())


def life_fresh(c, panel, N, W, opts, targets, ld, bg, site_of):
    """A context of its own given only one step's inputs: the options in force, the panel, the sites, the run."""
    with E.Engine(0, 0.02, 20) as ref:
        for k, v in opts.items():
            ref.set_option(k, v)
        ref.upload_panel(panel, N)
        ref.upload_sites(c["rows"], c["nr"], c["na"], W)
        ref.run(targets, ld=ld, bg_count=bg)
        return life_results(ref, len(targets), site_of)


def test_one_context_lives_through_every_change_of_input():
    """Panel, sites, layout, background and comparison individuals change under ONE context, in the order in which the cached
    products (row table, IBD0 pass, fragment base, images, the count towards ibd0_after) are made, kept and dropped; after every
    step the tables are those of a fresh context given only that step's inputs, bit for bit.  Single steps have tests of their
    own -- the kept pass: test_gpu_parity.test_ibd0_from_one_pass_over_the_site_list; the re-layout in the middle of a series:
    the test around test_gpu_parity.py's `compact_targets`; a second panel: test_staging_team_of_fewer_threads -- the point
    here is the sequence.  --LD variant and count unit are compared with the fresh context's where that has made as many runs
    (step 1); the count units named otherwise are what plan_run's rules give for this history."""
    c = life_case()
    panel, panel2 = E.pack_alleles_fast(c["alle"]), E.pack_alleles_fast(c["alle2"])
    opts = {"async": 1}
    # (what, options set before it, upload of sites with this window or None, targets, ld, background, per-site tables of,
    #  the count unit expected of the long-lived context, its layout after the run)
    steps = [
        ("1: --LD, one individual", {}, 50, [7], True, None, (0,), 2, 1),
        ("2: again (images reused)", {}, None, [7], True, None, (), 2, 1),
        ("3: another individual", {}, None, [129], True, None, (0,), 2, 1),
        ("4: five through the matrix cores (IBD0 pass)", {}, None, [3, 64, 7, 128, 90], True, None, (), 0, 1),
        ("5: one again (IBD1 form from the kept pass)", {}, None, [129], True, None, (), 3, 1),
        ("6: another background", {}, None, [129], True, c["bg"], (), 2, 1),
        ("7: re-layout in the middle of the series", {"compact_targets": 1}, None, [129], True, c["bg"], (0,), 2, 2),
        ("8: the same sites with window 32", {}, 32, [129], True, c["bg"], (), 2, 2),
        ("9+10: twenty individuals, per-site tables of two", {"site_results": 1}, None, list(range(40, 60)), True, c["bg"],
         (0, 19), 0, 2),
        ("11: non-LD (a pending finalising step is flushed)", {}, None, [61], False, c["bg"], (0,), 0, 2),
    ]
    with E.Engine(0, 0.02, 20) as eng:
        eng.set_option("async", 1)
        eng.upload_panel(panel, LIFE_N)
        W = None
        for n, (what, more, new_w, targets, ld, bg, site_of, unit, layout) in enumerate(steps):
            for k, v in more.items():
                eng.set_option(k, v)
            opts.update(more)
            if new_w is not None:
                W = new_w
                eng.upload_sites(c["rows"], c["nr"], c["na"], W)
            if what.startswith("11"):
                eng.run([61], ld=True, bg_count=bg)                     # (leaves its finalising step to a successor)
            eng.run(targets, ld=ld, bg_count=bg)
            got = life_results(eng, len(targets), site_of)
            want = life_fresh(c, panel, LIFE_N, W, opts, targets, ld, bg, site_of)
            for i in range(len(targets)):
                assert_bits(got["win"][i], want["win"][i], f"step {what}: windows of #{i}")
            for i in site_of:
                assert_bits(got["site"][i], want["site"][i], f"step {what}: per-site values of #{i}")
            assert got["variant"] == want["variant"] == (2 if ld else 0), what
            assert got["unit"] == unit and got["layout"] == layout, (what, got["unit"], got["layout"])
            if n == 0:
                assert got["unit"] == want["unit"] and got["layout"] == want["layout"], what
        # 12: a second panel, then sites and one individual
        eng.upload_panel(panel2, LIFE_N2)
        with pytest.raises(E.EngineError, match="no sites"):
            eng.run([69], ld=True)
        eng.upload_sites(c["rows"], c["nr"], c["na"], 50)
        eng.run([69], ld=True)
        got = life_results(eng, 1, (0,))
        want = life_fresh(c, panel2, LIFE_N2, 50, opts, [69], True, None, (0,))
        assert_bits(got["win"][0], want["win"][0], "step 12: windows on the second panel")
        assert_bits(got["site"][0], want["site"][0], "step 12: per-site values on the second panel")
        assert got["variant"] == want["variant"] == 2


# --------------------------------------------------------------------------- 7. ibdg_set_option, option by option
# Written from the chain of comparisons ibdg_set_option was before it became a table: name -> (accepted values at both ends,
# refused values on either side).  Nothing refused: the option takes any value (stored as value != 0, clamped, or as it is).
OPTION_CASES = {
    "count_in_run": ((0, 1, -5, 1 << 40), ()), "multi_target": ((0, 1, -5, 1 << 40), ()),
    "mfma_targets": ((0, 1, -5, 1 << 40), ()), "mfma_plain_tau": ((0, 1, -5, 1 << 40), ()),
    "mfma_wg_sum": ((0, 1, -5, 1 << 40), ()), "end_in_dispatch": ((0, 1, -5, 1 << 40), ()),
    "prep_ahead": ((0, 1, -5, 1 << 40), ()), "dispatch_events": ((0, 1, -5, 1 << 40), ()),
    "async": ((0, 1, -5, 1 << 40), ()), "dev_inputs_ready": ((0, 1, -5, 1 << 40), ()),
    "staged_upload": ((0, 1, -5, 1 << 40), ()),
    "guided_runs": ((0, 4, -3, 1 << 40), ()),                            # unchecked
    "mfma_batch_groups": ((1, 64, -7, 0, 65, 1 << 40), ()),              # clamped to 1..64
    "ibd0_after": ((0, 1 << 40, -1, -(1 << 40)), ()),                    # clamped to >= 0
    "mfma_min": ((1, 15), (0, 16)), "stage_workers": ((1, 8), (0, 9)), "compact_tiles": ((-1, 1), (-2, 2)),
    "finalize_in_next": ((0, 1), (-1, 2)), "sum_dpp": ((0, 1), (-1, 2)), "mx_counts": ((0, 1), (-1, 2)),
    "reserve_compact": ((0, 1), (-1, 2)), "site_results": ((0, 1), (-1, 2)),
    "compact_density": ((1, 1000000), (0, 1000001)), "compact_targets": ((1, 65536), (0, 65537)),
    "rows_blocks_per_cu": ((0, 128), (-1, 129)), "site_blocks_per_cu": ((0, 128), (-1, 129)),
    "recount_blocks_per_cu": ((0, 128), (-1, 129)), "chunks_per_wave": ((0, 5), (-1, 6)),
    "waves_per_block": ((1, 8), (0, 9)), "ld_variant": ((0, 3), (-1, 4)),
    "record_lds_bytes": ((1024, 98304), (1023, 98305)), "windows_per_wave": ((1, 65536), (0, 65537)),
    "compact_align": ((1, 2, 4, 8, 16, 32), (0, -1, 3, 24, 33, 64, 1 << 40)),
    "ring_slots": ((2, 3, 4, 8), (1, 0, -2, 5, 6, 7, 9, 64, 1 << 40)),
}


def test_every_option_accepts_and_refuses_what_it_did():
    with E.Engine() as eng:
        for name, (good, bad) in OPTION_CASES.items():
            for v in bad:
                with pytest.raises(E.EngineError, match=rf"ERROR in ibdg_set_option: {name} must be "):
                    eng.set_option(name, v)
            for v in good:
                assert eng.lib.ibdg_set_option(eng.ctx, name.encode(), v) == 0, (name, v)
        with pytest.raises(E.EngineError, match="unknown option 'no_such_option'"):
            eng.set_option("no_such_option", 1)
        with pytest.raises(E.EngineError, match="mfma_min must be 1..15"):
            eng.set_option("mfma_min", 99)
        with pytest.raises(E.EngineError, match=r"compact_tiles must be -1 \(never\), 0 \(auto\) or 1 \(always\)"):
            eng.set_option("compact_tiles", 7)
        with pytest.raises(E.EngineError, match="ring_slots must be 2, 3, 4 or 8"):
            eng.set_option("ring_slots", 5)
