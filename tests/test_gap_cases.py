"""The preconditions of tests/test_gpu_tile_gaps.py, asserted from the arrays of tests/gap_cases.py alone (CPU tier): the advances,
halves and ring slots the cases were made for follow from the site lists through the restated run structure and control words,
so a later edit of the cases cannot quietly lose them."""
import numpy as np
import pytest

import depth_cases as DC
import gap_cases as GC
import hp_ref as H

LD = H.LD


def words(name, ring=2, wpw=None):
    c = GC.make_case(name)
    rs = GC.run_structure(c["nr"], c["na"], c["W"], wpw or c["wpw"])
    return rs, GC.control_words(rs, ring)


def test_the_cases_are_what_their_names_say():
    for name in GC.NAMES:
        c = GC.make_case(name)
        cov = c["nr"].astype(int) + c["na"]
        assert c["alle"].shape == (len(cov), 2 * c["n_ids"]) and c["n_ids"] in (70, 130), name
        assert c["eps"] == 0.02 and c["M"] == 20 and 8 <= c["W"] <= 33 and c["refids"] is None and c["pu"] == -1, name
        assert cov.max() == 20 and cov[c["rows"]].min() >= 1 and (np.delete(cov, c["rows"]) == 0).all(), name
        assert (cov == 0).sum() > 10 * len(c["rows"]), name                        # mostly gaps
        assert set(np.unique(cov[c["rows"]]).tolist()) >= {1, 2, 3, 4, 7, 8, 15, 16, 20}, name
        # reads of the source's genotype on the target's first haplotype
        assert (c["alle"][c["rows"], 2 * GC.TARGET] == c["alle"][c["rows"], 2 * GC.SOURCE]).all() and c["target"] == GC.TARGET
        # rare planes among the segments, and segments without them (flags bit 12)
        seg = DC.segments(c["nr"], c["na"], c["W"])
        rare = (seg["nc"] > 3) | (seg["na"] > 2)
        assert rare.any() and (~rare).any(), name


def test_the_run_model_is_the_hosts():
    """run_begins against make_runs' loop (ibdg_api.cpp, guided_runs 0), and the control words of a dense list."""
    for n_win, g in ((1, 16), (16, 16), (17, 16), (40, 4), (5, 7)):
        runs, w = [], 0
        while w < n_win:
            runs.append(w)
            w = min(w + g, n_win)
        runs.append(n_win)
        assert GC.run_begins(n_win, g).tolist() == runs
    nr = np.ones(64 * 5 + 3, dtype=np.uint8)
    rs = GC.run_structure(nr, 0 * nr, 16, 4)                   # runs of 64 rows: one pair each
    assert rs["pairs"] == [1] * 5 + [1] and rs["n_seg"].tolist() == [4] * 5 + [1]
    adv, nhalf, nslot, in_run = GC.control_words(rs, 3)
    assert adv.max() == 0 and nslot.max() == 0 and in_run.sum() == 3 * 5 and nhalf[in_run].tolist() == [0, 1, 1] * 5
    rs = GC.run_structure(nr, 0 * nr, 16, 16)
    adv, nhalf, nslot, in_run = GC.control_words(rs, 3)
    assert adv[:15].tolist() == ([0, 0, 0, 1] * 4)[:15] and nslot[:15].tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 0, 0, 0, 0]
    assert not in_run[15] and adv[16:].tolist() == [0, 0, 0, 1, 0] and nslot[16:].tolist() == [0, 0, 0, 1, 0]


def test_ladder_meets_every_advance_in_both_halves():
    c = GC.make_case("ladder")
    rs, (adv, nhalf, nslot, in_run) = words("ladder")
    assert len(rs["begin"]) - 1 >= 2                                                # more than one run
    met = {(int(a), int(h)) for a, h in zip(adv[in_run], nhalf[in_run])}
    want = {(a, h) for a in GC.LADDER_ADV for h in (0, 1)}
    assert want <= met, sorted(want - met)
    assert adv[in_run].max() == 255                                                 # no overflow
    win = rs["seg"]["win"]
    big = in_run & (adv >= 2)
    nxt = np.flatnonzero(big) + 1
    between = win[nxt] != win[np.flatnonzero(big)]
    # gaps between windows (a window ends just before one) and inside a window (it straddles one)
    assert between.any() and (~between).any()
    # ... and windows that end inside a cluster: the next segment is the same tile again (advance 0, the same half)
    assert ((adv == 0) & in_run & (np.r_[win[1:], -1] != win)).any()
    per_win = np.bincount(win)
    assert per_win.max() >= 3 and len(c["rows"]) > c["W"] * c["wpw"]
    assert max(rs["pairs"]) >= 3 * 8                                                # three laps of the deepest ring in one run


@pytest.mark.parametrize("ring", GC.RING_DEPTHS)
def test_ladder_advances_below_at_and_above_every_ring_depth(ring):
    rs, (adv, nhalf, nslot, in_run) = words("ladder", ring)
    a = set(adv[in_run].tolist())
    assert {ring - 1, ring, ring + 1} <= a, (ring, sorted(a))
    # every slot of the ring is the next segment's at some point, and the slot follows the pair: (pair - first pair) % ring
    assert set(nslot[in_run].tolist()) == set(range(ring))
    q = rs["seg"]["tile"] >> 1
    for s0, s1 in zip(rs["seg_begin"][:-1], rs["seg_begin"][1:]):
        assert (nslot[s0:s1 - 1] == (q[s0 + 1:s1] - q[s0]) % ring).all()
    # advances that are multiples of the depth (the same slot again) and not
    assert any(x and x % ring == 0 for x in a) and any(x % ring for x in a)


@pytest.mark.parametrize("rerequest", [False, True])
@pytest.mark.parametrize("ring", GC.RING_DEPTHS)
def test_the_control_words_lead_the_ring_to_every_segments_own_tile(ring, rerequest):
    """The restated control words walked by the restated tile ring (gap_cases.ring_walk; both guard policies): every segment
    of every case reads its own pair and half.  And what the GPU test relies on: a slot off by one where the advance reaches
    the ring depth, a wrong half behind a skipped pair, an advance one short of 255 each lead some segment of `ladder` to
    another pair or half -- tile words of other panel rows under this segment's masks."""
    for name in GC.LAYOUT1_NAMES:
        c = GC.make_case(name)
        for wpw in {c["wpw"], c.get("alt_wpw", c["wpw"])}:
            rs, (adv, nhalf, nslot, in_run) = words(name, ring, wpw)
            pair, half = GC.ring_walk(rs, adv, nhalf, nslot, ring, rerequest)
            tile = rs["seg"]["tile"]
            assert np.array_equal(pair, tile >> 1) and np.array_equal(half, tile & 1), (name, wpw)
    rs, (adv, nhalf, nslot, in_run) = words("ladder", ring)
    tile = rs["seg"]["tile"]
    wrong = {"slot": (adv, nhalf, np.where(adv >= ring, (nslot + 1) % ring, nslot)),
             "half": (adv, np.where(adv >= 2, nhalf ^ 1, nhalf), nslot),
             "advance": (np.where(adv == 255, 254, adv), nhalf, nslot)}
    for what, (a, h, s) in wrong.items():
        pair, half = GC.ring_walk(rs, a, h, s, ring, rerequest)
        assert not (np.array_equal(pair, tile >> 1) and np.array_equal(half, tile & 1)), what


def test_upper_start_runs_begin_in_upper_halves_and_end_behind_a_skip():
    c = GC.make_case("upper-start")
    rs, (adv, nhalf, nslot, in_run) = words("upper-start")
    tile = rs["seg"]["tile"]
    assert len(rs["begin"]) - 1 == len(GC.UPPER_LAST)
    assert (tile[rs["seg_begin"][:-1]] & 1 == 1).all()                              # x_off0 = 8 in every run
    before_last = rs["seg_begin"][1:] - 2
    assert adv[before_last].tolist() == list(GC.UPPER_LAST) and in_run[before_last].all()
    assert min(GC.UPPER_LAST) > max(GC.RING_DEPTHS) and max(GC.UPPER_LAST) == 255
    assert set(nhalf[before_last].tolist()) == {0, 1}
    # the second run structure: every run but the first begins in a lower half, and no run ends where one of the first ends
    rs2, (adv2, _, _, in_run2) = words("upper-start", wpw=c["alt_wpw"])
    first = rs2["seg"]["tile"][rs2["seg_begin"][:-1]] & 1
    assert len(first) >= 4 and first[0] == 1 and (first[1:] == 0).all()
    assert set(rs2["begin"][1:-1].tolist()).isdisjoint(rs["begin"].tolist())
    assert adv2[in_run2].max() == 255 and sorted(adv2[in_run2 & (adv2 > 8)].tolist())[-3:] == [70, 130, 255]


def test_boundary_gap_lies_between_two_runs_and_in_a_run_of_the_twin():
    c, t = GC.make_case("boundary"), GC.make_case("boundary-shifted")
    rs, (adv, _, _, in_run) = words("boundary")
    assert adv[in_run].max() <= 255 and adv[in_run].max() < 8
    q = rs["seg"]["tile"] >> 1
    jump = q[rs["seg_begin"][1:-1]] - q[rs["seg_begin"][1:-1] - 1]                  # from a run's last pair to the next run's first
    assert GC.BOUNDARY_GAP >= 256 and sorted(jump.tolist())[-2:] == [GC.BOUNDARY_GAP, GC.BOUNDARY_GAP + 1]
    # the twin: one window of sites more in front, every other site as it was
    assert len(t["rows"]) == len(c["rows"]) + c["W"] and np.array_equal(t["rows"][c["W"]:], c["rows"])
    assert np.array_equal(t["alle"], c["alle"]) and np.array_equal(t["nr"][c["W"]:], c["nr"][c["W"]:])
    rs, (adv, _, _, in_run) = words("boundary-shifted")
    assert sorted(adv[in_run].tolist())[-2:] == [GC.BOUNDARY_GAP, GC.BOUNDARY_GAP + 1]


def test_the_edges_differ_by_one_pair_in_one_gap():
    a, b = GC.make_case("edge-255"), GC.make_case("edge-256")
    for c, top in ((a, 255), (b, 256)):
        rs, (adv, _, _, in_run) = words(f"edge-{top}")
        assert adv[in_run].max() == top and (adv[in_run] == top).sum() == 1
        assert np.sort(adv[in_run])[-2] < 8
    ra, rb = a["rows"], b["rows"]
    assert len(ra) == len(rb)
    d = rb - ra
    k = int(np.flatnonzero(d)[0])
    assert (d[:k] == 0).all() and (d[k:] == 64).all() and 0 < k < len(ra) - 1
    assert np.array_equal(a["alle"][ra], b["alle"][rb]) and np.array_equal(a["nr"][ra], b["nr"][rb])
    assert np.array_equal(a["na"][ra], b["na"][rb])


def test_one_row_tiles_has_a_segment_per_row():
    c = GC.make_case("one-row-tiles")
    rs, (adv, nhalf, _, in_run) = words("one-row-tiles")
    rows = c["rows"]
    assert len(rs["seg"]["tile"]) == len(rows) and len(set((rows // 32).tolist())) == len(rows)
    assert rows[0] == 31 and rows[-1] == len(c["nr"]) - 1 and len(c["nr"]) % 256 != 0 and len(c["nr"]) % 32 != 0
    # inside a run: 0 into the upper half of the same pair, 2 into the lower half of the next pair but one, in turn
    for s0, s1 in zip(rs["seg_begin"][:-1], rs["seg_begin"][1:]):
        n = s1 - 1 - s0
        assert adv[s0:s1 - 1].tolist() == ([0, 2] * n)[:n] and nhalf[s0:s1 - 1].tolist() == ([1, 0] * n)[:n]
    assert rs["n_seg"].tolist() == [128, 128, 69] and c["wpw"] * c["W"] == 128


@pytest.mark.parametrize("name", GC.NAMES)
def test_every_window_truth_is_a_normal_double(name):
    """As test_depth_cases: both columns of every window of the case's target are at least 2^-1022."""
    c = GC.make_case(name)
    tr = H.ld_truth(c["alle"], c["nr"], c["na"], c["target"], c["W"], H.binomial_factors(c["eps"], c["M"]), c["refids"], c["pu"])
    lo = min(tr["ibd0"].min(), tr["ibd1"].min())
    print(f"{name}: {len(tr['rows'])} windows, smallest truth 2^{float(np.log2(lo)):.0f}")
    assert lo >= LD(2.0) ** -1022 and np.isfinite(tr["ibd0"]).all() and np.isfinite(tr["ibd1"]).all()


def test_the_matrix_core_groups_take_every_case():
    for name in GC.NAMES:
        c = GC.make_case(name)
        assert DC.tab_in_lds(c["nr"], c["na"], c["W"]), name
        assert DC.mfma_takes(c["nr"], c["na"], c["W"]) is True, name
        assert c["wpw"] <= 16                                  # (mfma_takes covers runs of 1..16 windows)


@pytest.mark.parametrize("name", GC.NAMES)
def test_the_two_renderings_select_the_same_panel_rows(name):
    c = GC.make_case(name)
    rows, nr, na = GC.row_index_rendering(c)
    cov = c["nr"].astype(int) + c["na"]
    assert rows.dtype == np.uint32 and np.array_equal(rows, np.flatnonzero(cov > 0)) and (np.diff(rows.astype(int)) > 0).all()
    assert np.array_equal(nr, c["nr"][cov > 0]) and np.array_equal(na, c["na"][cov > 0]) and (nr.astype(int) + na >= 1).all()
    # the same windows over the same panel rows
    a = H.windows(c["nr"], c["na"], c["W"])
    b = H.windows(nr, na, c["W"])
    assert len(a) == len(b) and all(np.array_equal(x, rows[y]) for x, y in zip(a, b))


def test_run_seed_draws_the_target_first():
    for name in ("ladder", "boundary"):
        c = GC.make_case(name)
        for T in (1, 4, 15):
            rng = np.random.default_rng(GC.run_seed(name, T))
            assert int(rng.choice(np.arange(c["n_ids"]), size=T, replace=False)[0]) == c["target"]
