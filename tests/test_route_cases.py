"""The model of tests/route_cases.py, asserted from the arrays alone (CPU tier): which of the 40 constructed cases a default
context compacts at the upload, which ever reach the IBD1 form, what the 24 runs of tests/test_gpu_default_route.py must report,
and that the assertions made there can tell the host's thresholds from their neighbours."""
import numpy as np
import pytest

import bg_cases as BC
import depth_cases as DC
import gap_cases as GC
import route_cases as RC

DENSE = [case for case in RC.CASES if not RC.sparse(RC.make_case(*case))]
SPARSE = [case for case in RC.CASES if RC.sparse(RC.make_case(*case))]


def test_there_are_forty_cases():
    assert len(RC.CASES) == 40 == len(DC.NAMES) + len(GC.NAMES) + len(BC.NAMES)
    assert (len(DC.NAMES), len(GC.NAMES), len(BC.NAMES)) == (12, 7, 21)
    assert len(set(RC.CASES)) == 40


def test_which_cases_are_sparse():
    """Every gap case (ladder: 272 covered rows over 85 288) and the two full-depth cases (one row in five) are compacted at
    the upload; the other ten depth cases and the 21 backgrounds of 116 rows are not."""
    assert SPARSE == [("depth", "full-depth-15"), ("depth", "full-depth-16")] + [("gap", n) for n in GC.NAMES]
    assert DENSE == [("depth", n) for n in DC.NAMES[:10]] + [("bg", n) for n in BC.NAMES]
    c = RC.make_case("gap", "ladder")
    assert len(RC.covered(c)) == 272 and len(c["nr"]) == 85288
    for name in BC.NAMES:
        c = RC.make_case("bg", name)
        assert len(c["nr"]) == 116 == len(RC.covered(c)), name
    for name in ("full-depth-15", "full-depth-16"):
        c = RC.make_case("depth", name)
        assert len(RC.covered(c)) * 5 == len(c["nr"]), name
    # the rule itself, at its edge: 1 covered row in 4 exactly is dense, one row more of span is sparse
    for L, sparse in ((8, False), (9, True)):
        nr = np.zeros(L, dtype=np.uint8)
        nr[[0, 4]] = 1
        assert RC.sparse(dict(nr=nr, na=0 * nr)) == sparse


def test_only_full_depth_16_keeps_its_tables_outside_lds():
    for kind, name in RC.CASES:
        c = RC.make_case(kind, name)
        assert DC.tab_in_lds(c["nr"], c["na"], c["W"]) == ((kind, name) != ("depth", "full-depth-16")), (kind, name)
    assert all(t == (2, 2, 1) for t in RC.expected(("depth", "full-depth-16"), RC.N_RUNS))


@pytest.mark.parametrize("case", RC.CASES, ids=["-".join(c) for c in RC.CASES])
def test_the_triples_of_24_runs(case):
    got = RC.expected(case, RC.N_RUNS)
    if case == ("depth", "full-depth-16"):
        want = [(2, 2, 1)] * 24
    elif case in SPARSE:
        want = [(2, 2, 1)] * 7 + [(2, 3, 2)] * 17
    else:
        want = [(1, 2, 1)] * 7 + [(1, 3, 2)] * 14 + [(2, 3, 2)] * 3
    assert case not in RC.UNSURE_END
    assert got == want
    # a second upload of the same list starts over
    assert RC.expected(case, 1) == want[:1]


def test_every_module_has_a_case_that_ends_on_the_benchmarks_form():
    """(layout 2, count unit 3, paired end): what bench.py times."""
    for kind in RC.MODULES:
        assert any(RC.expected(case, RC.N_RUNS)[-1] == (2, 3, 2) for case in RC.CASES if case[0] == kind), kind


def test_pattern_b_leaves_the_pass_run_and_the_relayout_run_unread():
    assert RC.N_RUNS == 24 and RC.READS_A == tuple(range(1, 25))
    assert RC.READS_B == (3, 6, 9, 12, 15, 18, 21, 24)
    assert 8 not in RC.READS_B and 22 not in RC.READS_B and 8 in RC.READS_A and 22 in RC.READS_A
    # consecutive runs are other individuals, and every one of the six is read in pattern B
    people = list("abcdef")
    order = RC.cycle(people)
    assert len(order) == 24 and all(a != b for a, b in zip(order, order[1:]))
    assert {order[k - 1] for k in RC.READS_B} == {"c", "f"} and {order[7], order[21]} == {"b", "d"}


def test_the_neighbouring_thresholds_predict_other_triples():
    """The pass at the 7th or 9th run, the relayout in the 21st or 23rd: each gives some dense case another sequence of triples than
    the host's 8 and 22 -- at the run in question --, so the assertion after every run tells them apart."""
    for ibd0_after, run in ((7, 7), (9, 8)):
        differs = [case for case in DENSE if RC.expected(case, 24, ibd0_after=ibd0_after) != RC.expected(case, 24)]
        assert differs, ibd0_after
        a, b = RC.expected(differs[0], 24, ibd0_after=ibd0_after), RC.expected(differs[0], 24)
        assert [k + 1 for k in range(24) if a[k] != b[k]] == [run]
    for relayout_run in (21, 23):
        targets = RC.CREDIT_PER_RUN * relayout_run
        differs = [case for case in DENSE if RC.expected(case, 24, compact_targets=targets) != RC.expected(case, 24)]
        assert differs == DENSE, relayout_run
        a, b = RC.expected(DENSE[0], 24, compact_targets=targets), RC.expected(DENSE[0], 24)
        assert [k + 1 for k in range(24) if a[k] != b[k]] == [min(relayout_run, 22)]
    # the host's own numbers: 21 runs leave the credit at 252, the 22nd reaches 264 >= 256
    assert 21 * RC.CREDIT_PER_RUN < RC.COMPACT_TARGETS <= 22 * RC.CREDIT_PER_RUN
    # a sparse case cannot tell the relayout's threshold
    assert all(RC.expected(case, 24, compact_targets=12) == RC.expected(case, 24) for case in SPARSE)


def test_guided_runs_are_make_runs():
    # fewer windows than workgroups in flight: one window per run
    assert RC.guided_run_begins(5, 16, 3).tolist() == [0, 1, 2, 3, 4, 5]
    # three chunks, one chunk group of three waves: 256 * (16 // 3) = 1280 in flight
    b = RC.guided_run_begins(40000, 16, 3)
    d = np.diff(b)
    assert d[0] == 16 and d[-1] == 1 and (np.diff(d) <= 0).all() and b[-1] == 40000
    first_short = int(b[np.flatnonzero(d < 16)[0]])
    assert -(-(40000 - first_short) // 1280) < 16 <= -(-(40000 - first_short + 16) // 1280)
    # nine chunks: two chunk groups of five waves: 256 * 3 // 2 = 384
    assert np.diff(RC.guided_run_begins(384 * 2 + 1, 16, 9))[0] == 3


def test_the_lds_bytes_are_those_of_the_pair_sums_test():
    import test_gpu_pair_sums as pair_sums          # (no device is touched by importing it)
    for args in ((1, 16, 4, 2), (56, 16, 751, 2), (139, 8, 151, 2), (40, 12, 300, 8)):
        for scratch in (False, True):
            assert RC.ibd1_lds_bytes(*args, scratch) == pair_sums.ibd1_lds_bytes(*args, scratch)


@pytest.mark.parametrize("case", RC.CASES, ids=["-".join(c) for c in RC.CASES])
def test_the_window_end_does_not_hang_on_the_run_lengths(case):
    """Every run of a case is one window on an MI355X; with uniform runs of 1..16 windows (fewer compute units, another
    guided_runs) the layouts of the case's route would still give the same window end -- else the case belongs in UNSURE_END."""
    c = RC.make_case(*case)
    n_win, n_chunks = RC.n_windows(c), (c["n_ids"] + 63) // 64
    begins = RC.guided_run_begins(n_win, RC.WINDOWS_PER_WAVE, n_chunks)
    assert np.array_equal(begins, np.arange(n_win + 1)), case
    assert len(RC.UNSURE_END) <= 4 and set(RC.UNSURE_END) <= set(RC.CASES)
    layouts = sorted({t[0] for t in RC.expected(case, RC.N_RUNS)})
    for layout in layouts:
        ends = {RC.paired_end(c, layout, run_len) for run_len in range(1, 17)} | {RC.paired_end(c, layout)}
        assert (len(ends) == 1) != (case in RC.UNSURE_END), (case, layout, ends)
    # layout 1: the segments of a run of one window are gap_cases.run_structure's
    if 1 in layouts:
        rs = GC.run_structure(c["nr"], c["na"], c["W"], 1, RC.RECORD_LDS_BYTES)
        assert int(rs["n_seg"].max()) == RC.max_seg(c, 1, begins)
    # the compacted tiles hold a window's rows back to back: ceil(W / 32) tiles, one more where it straddles
    assert RC.max_seg(c, 2, begins) <= -(-c["W"] // 32) + 1


def test_one_context_through_the_small_panel_backgrounds():
    """Part (c) of the GPU module: nine runs per background of panel A in one context.  The count towards the pass restarts with
    every background, the relayout's credit does not: the 22nd run is the fourth on the third background."""
    seq, credit = [], 0
    for name in BC.A_NAMES:
        seq += RC.expected(("bg", name), 9, first_credit=credit)
        credit += 9 * RC.CREDIT_PER_RUN
    assert len(seq) == 9 * len(BC.A_NAMES) and [t[0] for t in seq] == [1] * 21 + [2] * (len(seq) - 21)
    assert all([t[1] for t in seq[i:i + 9]] == [2] * 7 + [3] * 2 for i in range(0, len(seq), 9))
    assert seq[18:27] == [(1, 2, 1)] * 3 + [(2, 2, 1)] * 4 + [(2, 3, 2)] * 2
    # no two neighbours in the table share a background: the count restarts every time (but not at the turn of the way back, where
    # the last background runs eighteen times in a row: the GPU test counts per background as the host does)
    keys = [(RC.make_case("bg", n)["mult"].tobytes(), RC.make_case("bg", n)["pu"]) for n in BC.A_NAMES]
    assert all(a != b for a, b in zip(keys, keys[1:]))
