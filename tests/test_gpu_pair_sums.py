"""The IBD1 form's paired window end (option "pair_sums", ibdg_last_window_end): two consecutive windows of a run summed in
one tree through the wave's LDS scratch -- lane 31 stores the first window's sum, lane 63 the second's --, a run's odd last
window by DPP moves alone as before.  The additions are those of the single end in its order, so every window table must be
the BITS of pair_sums 0 and of the form that counts everything (ibd0_after 0); one individual per shape is held to the
oracle's bar and the extended-precision bound as well (test_gpu_precision.run_form).

  1. bits: the smallest shapes at which the pairing can go wrong, with runs of 1 window (every window unpaired), 2 (every
     window paired), 3 (a pair, then a single one) and 16 (the default), uniform runs and guided ones (short runs at the end
     of the grid);
  2. fallback: an LDS configuration in which the scratch would cost a workgroup per CU takes the single end;
  3. queue: the finalising step riding in the next launch reads what lanes 31 and 63 stored.
"""
import numpy as np
import pytest

import depth_cases as DC
import gap_cases as GC
from ibdgem_amd import engine as E
from test_gpu_parity import assert_bits, assert_ld_close, synth
from test_gpu_precision import FORMS, run_form

pytestmark = pytest.mark.gpu

EPS = 0.02
# the second run on an upload (the first one here: ibd0_after 1) takes the IBD1 form, one individual per workgroup
IBD1_OPTS = dict(ld_variant=2, mfma_targets=0, multi_target=0, ibd0_after=1, compact_tiles=-1)

# N, L, W, max_cov, rows given nine reads (the rare-plane flag: a fourth weight plane; max_cov 40 as in the depth-edge tests)
SHAPES = [
    (70, 900, 100, 20, ()),                 # a second chunk of 6 live lanes
    (131, 400, 7, 40, (5, 77, 78, 301)),    # many windows per tile
    (520, 640, 64, 20, ()),                 # 9 chunks: a second chunk group with one live wave, seven that leave in the prologue
    (3, 60, 2, 20, ()),                     # smallest panel and window
]
RUN_LENGTHS = (1, 2, 3, 16)
GUIDED = (0, 4)


def shape_inputs(N, L, W, M, deep):
    alle, nr, na = synth(7000 + N, L, N)
    for row in deep:
        nr[row], na[row] = 4, 5
    return alle, nr, na


def n_windows(nr, na, W):
    return -(-int(((nr.astype(int) + na) > 0).sum()) // W)


def ibd1_run(eng, t, pair, what):
    """One synchronous run of individual t in the IBD1 form with pair_sums = pair: count unit 3 and the window end asked for."""
    eng.set_option("pair_sums", pair)
    eng.run([t], ld=True)
    assert eng.last_ld_variant() == 2 and eng.last_count_unit() == 3, (what, eng.last_count_unit())
    assert eng.last_window_end() == (2 if pair else 1), (what, pair, eng.last_window_end())
    return eng.window_ll(0)


@pytest.mark.parametrize("N,L,W,M,deep", SHAPES)
def test_paired_window_ends_give_the_bits_of_single_ones(oracle, N, L, W, M, deep):
    alle, nr, na = shape_inputs(N, L, W, M, deep)
    n_win = n_windows(nr, na, W)
    if deep:
        assert (nr.astype(int) + na).max() == 9
    if N == 520:
        assert n_win % 2 == 1 and n_win < 16      # runs of 2: the last run is a single window; of 16: one run, its last window unpaired
    t = N // 2
    # the oracle's bar and the extended-precision bound, once per shape, every window of a pair (runs of 2)
    spec = dict(FORMS["popcount IBD1 form"], opts=dict(IBD1_OPTS, pair_sums=1, windows_per_wave=2, guided_runs=0))
    seed = next(s for s in range(100000) if int(np.random.default_rng(s).choice(np.arange(N), size=1, replace=False)[0]) == t)    # (run_form draws its individual)
    keep = {}
    run_form(oracle, "popcount IBD1 form", alle, nr, na, W, EPS, M, seed=seed, spec=spec, keep=keep)
    assert keep["targets"] == [t]
    checked = keep["windows"][0]
    assert checked.shape == (n_win, 3)
    ref = oracle.compare(alle, nr, na, t, window=W, eps=EPS, max_cov=M)
    with E.Engine(0, EPS, M) as eng:
        for k, v in IBD1_OPTS.items():
            eng.set_option(k, v)
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        for wpw in RUN_LENGTHS:
            for guided in GUIDED:
                what = f"N={N} W={W} windows_per_wave={wpw} guided_runs={guided}"
                eng.set_option("windows_per_wave", wpw)
                eng.set_option("guided_runs", guided)
                eng.set_option("ibd0_after", 1)
                eng.upload_sites(np.arange(L), nr, na, W)
                paired = ibd1_run(eng, t, 1, what)
                single = ibd1_run(eng, t, 0, what)
                eng.set_option("ibd0_after", 0)             # the form that counts everything
                eng.run([t], ld=True)
                assert eng.last_count_unit() == 2 and eng.last_window_end() == 1, what
                everything = eng.window_ll(0)
                assert_bits(paired, single, f"{what}: pair_sums 1 vs 0")
                assert_bits(paired, everything, f"{what}: pair_sums 1 vs ibd0_after 0")
                assert_bits(paired, checked, f"{what}: vs the run held to the bound")
                assert_ld_close(paired[:, :2], ref["win"][:, :2], f"{what}: vs oracle")


def ibd1_lds_bytes(max_seg, win_per_group, tab_len, ring_slots, scratch):
    """ld_popcount_lds_bytes(.., multi_target = 3 / 4) through ld_lds_layout (ibdg_ld_layout.h): records of 32 words, window
    constants of 8, tables of plain doubles in LDS, 8 waves, the rings, 1 KiB of scratch per wave with the paired end."""
    head = (max_seg * 32 + win_per_group * 8) * 4 + 15
    ring = (head + tab_len * 2 * 8 + 1023) & ~1023
    return ring + 8 * ring_slots * 1024 + (8 * 1024 if scratch else 0)


def test_single_end_where_the_scratch_would_cost_a_workgroup():
    """Rings of 8 slots and runs of 12 windows of 100 rows: 76 KiB of LDS without the scratch (two workgroups on a CU's 160 KiB),
    84 KiB with it (one).  The host keeps the single end whatever pair_sums says, and the bits are those of pair_sums 0."""
    N, L, W, wpw, ring = 70, 2600, 100, 12, 8
    alle, nr, na = synth(7070, L, N)
    opts = dict(IBD1_OPTS, ring_slots=ring, record_lds_bytes=96 * 1024, windows_per_wave=wpw, guided_runs=0)
    max_seg = int(GC.run_structure(nr, na, W, wpw, opts["record_lds_bytes"])["n_seg"].max())
    tab_len = DC.ct_max(nr, na, W) + 1
    assert DC.tab_in_lds(nr, na, W)
    without, with_scratch = (ibd1_lds_bytes(max_seg, wpw, tab_len, ring, s) for s in (False, True))
    print("segments", max_seg, "table entries", tab_len, "LDS bytes", without, with_scratch)
    assert 160 * 1024 // without == 2 and 160 * 1024 // with_scratch == 1
    got = {}
    with E.Engine(0, EPS, 20) as eng:
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        eng.upload_sites(np.arange(L), nr, na, W)
        for pair in (1, 0):
            eng.set_option("pair_sums", pair)
            eng.run([33], ld=True)
            assert eng.ld_layout() == 1 and eng.last_count_unit() == 3
            assert eng.last_window_end() == 1, pair
            got[pair] = eng.window_ll(0)
        # the same runs with rings of 2: the scratch fits, the paired end runs, the bits stay
        eng.set_option("ring_slots", 2)
        eng.upload_sites(np.arange(L), nr, na, W)
        got[2] = ibd1_run(eng, 33, 1, "rings of 2")
    assert_bits(got[1], got[0], "pair_sums 1 (refused) vs 0")
    assert_bits(got[2], got[0], "rings of 2, paired, vs rings of 8, single")


def test_queued_runs_finalise_what_lanes_31_and_63_stored():
    """async 1: the finalising step of a run rides in the next run's launch and reads the partial sums the paired end stored
    from lanes 31 and 63.  Three queued runs of three individuals: the last one's table is that of its lone synchronous run."""
    N, L, W, M, deep = SHAPES[1]
    alle, nr, na = shape_inputs(N, L, W, M, deep)
    people = [5, 130, 64]
    with E.Engine(0, EPS, M) as eng:
        for k, v in IBD1_OPTS.items():
            eng.set_option(k, v)
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        eng.upload_sites(np.arange(L), nr, na, W)
        alone = ibd1_run(eng, people[-1], 1, "synchronous")
        single = ibd1_run(eng, people[-1], 0, "synchronous")
        assert_bits(alone, single, "synchronous: pair_sums 1 vs 0")
        eng.set_option("pair_sums", 1)
        eng.set_option("async", 1)
        for t in people:
            eng.run([t], ld=True)
        assert eng.last_count_unit() == 3 and eng.last_window_end() == 2
        assert_bits(eng.window_ll(0), alone, "three queued runs")
