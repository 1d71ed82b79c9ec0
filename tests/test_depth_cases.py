"""The preconditions of tests/test_gpu_depth_edges.py, asserted from the arrays of tests/depth_cases.py alone (CPU tier): a later
edit of the cases cannot quietly lose the coverage they were made for."""
import numpy as np
import pytest

import depth_cases as DC
import hp_ref as H

LD = H.LD


@pytest.fixture(scope="module")
def segs():
    """name -> segments of the case on the panel's own rows (the layout of every form but "popcount compacted")."""
    out = {}
    for name in DC.NAMES:
        c = DC.make_case(name)
        out[name] = DC.segments(c["nr"], c["na"], c["W"])
    return out


def test_the_cases_are_what_their_names_say():
    for name in DC.NAMES:
        c = DC.make_case(name)
        cov = c["nr"].astype(int) + c["na"]
        assert c["alle"].shape == (len(cov), 2 * 130) and c["eps"] == 0.02 and cov.max() <= c["M"], name
        assert c["refids"] is None and c["pu"] == -1 and 0 <= c["target"] < 130
    lattice = {(r, a) for r in range(51) for a in range(51) if 1 <= r + a <= 50}
    for name in ("lattice", "ladder"):
        c = DC.make_case(name)
        rows = list(zip(c["nr"].tolist(), c["na"].tolist()))
        assert len(rows) == 1325 and set(rows) == lattice and c["W"] == 3 and c["M"] == 50, name
    c = DC.make_case("ladder")
    key = [(r + a, a) for r, a in zip(c["nr"].tolist(), c["na"].tolist())]
    assert key == sorted(key)
    c = DC.make_case("lattice")
    key = [(r + a, a) for r, a in zip(c["nr"].tolist(), c["na"].tolist())]
    assert key != sorted(key)
    for m in (1, 7, 8, 15, 16, 31, 32):
        c = DC.make_case(f"lattice-M{m}")
        rows = list(zip(c["nr"].tolist(), c["na"].tolist()))
        full = {(r, a) for r in range(m + 1) for a in range(m + 1) if 1 <= r + a <= m}
        assert c["M"] == m and c["W"] == 3 and set(rows) == full and len(rows) >= 96, m       # three tiles or more
        assert len(rows) % len(full) == 0 and all(rows.count(p) == len(rows) // len(full) for p in full), m
    for W in (15, 16):
        c = DC.make_case(f"full-depth-{W}")
        cov = c["nr"].astype(int) + c["na"]
        assert c["W"] == W and c["M"] == 50 and set(cov.tolist()) == {0, 50} and 5 * int((cov == 50).sum()) == len(cov)
        assert len(H.windows(c["nr"], c["na"], W)) == 8
        assert all(r[-1] // 32 - r[0] // 32 >= 2 for r in H.windows(c["nr"], c["na"], W))     # three or more tiles a window
        assert (c["alle"][:, 2 * c["target"]] == c["alle"][:, 2 * DC.FULL_SOURCE]).all() and c["target"] != DC.FULL_SOURCE
        g = c["alle"][:, 14].astype(int) + c["alle"][:, 15]
        assert all(int((g[cov == 50] == k).sum()) >= 5 for k in range(3)), "every genotype class among the read rows"


def test_every_plane_count_and_both_rare_triggers_occur(segs):
    nc = np.concatenate([s["nc"] for s in segs.values()])
    na = np.concatenate([s["na"] for s in segs.values()])
    assert set(nc.tolist()) == {1, 2, 3, 4, 5, 6}, sorted(set(nc.tolist()))       # (depth <= 50: plane 5 is the top one)
    assert set(na.tolist()) == {0, 1, 2, 3, 4, 5, 6}, sorted(set(na.tolist()))
    # flags bit 12 of k_prep_seg_walk: nc > 3 || na > 2 -- each side alone
    assert ((na > 2) & (nc <= 3)).any() and ((nc > 3) & (na <= 2)).any()
    assert ((nc <= 3) & (na <= 2)).any()                                           # ... and segments that stay on the fast path
    # the compacted layout's segments (virtual rows back to back) reach the same planes
    c = DC.make_case("ladder")
    v = DC.segments(c["nr"], c["na"], c["W"], win_rows=c["W"])
    assert set(v["nc"].tolist()) >= {2, 3, 4, 5, 6} and set(v["na"].tolist()) >= {1, 2, 3, 4, 5, 6}


def test_ladder_steps_from_deep_to_wide_in_consecutive_segments(segs):
    """k_win_target_g's regimes (ibdg_ld_mfma.hip): deep = nc > 3, wide = nc > 4 || na > 4."""
    s = segs["ladder"]
    nc, na = s["nc"], s["na"]
    wide = (nc > 4) | (na > 4)
    step = [i for i in range(len(nc) - 1) if nc[i] == 4 and not wide[i] and nc[i + 1] == 5 and wide[i + 1]]
    assert step, "no segment with nc == 4 next to one with nc == 5"
    # consecutive segments walk through every regime, in order
    assert [int(x) for x in nc] == sorted(int(x) for x in nc)
    assert {(int(c) > 3, bool(w)) for c, w in zip(nc, wide)} == {(False, False), (True, False), (True, True)}


def test_spike_places_every_depth_at_every_position_once():
    c = DC.make_case("spike")
    cov = c["nr"].astype(int) + c["na"]
    alt = c["na"].astype(int)
    assert len(cov) == 54 * 32 == 1728 and c["W"] == 15
    assert (cov == 0).any()
    spikes = np.flatnonzero(cov > 3)
    assert len(spikes) == 54
    placed = sorted((int(cov[r]), int(r % 32)) for r in spikes)
    assert placed == sorted((d, p) for d in DC.SPIKE_DEPTHS for p in DC.SPIKE_POSITIONS)
    assert [int(r // 32) for r in spikes] == list(range(54))                       # one a tile
    assert (cov[np.setdiff1d(np.arange(len(cov)), spikes)] <= 3).all()
    for d in DC.SPIKE_DEPTHS:
        assert {int(alt[r]) for r in spikes if cov[r] == d} == set(DC.spike_alts(d)), d
    # the borrow across planes 2 / 3 in the IBD1 form: the low three bits of alt above those of the depth.  No alt count can do
    # that at depth 15 or 31 (low bits 7); every other depth from 8 on has such a row.
    b = DC.borrows(cov, alt)
    for d in DC.SPIKE_DEPTHS:
        if d >= 8 and (d & 7) != 7:
            assert b[spikes[cov[spikes] == d]].any(), d
        else:
            assert not any(DC.borrows(d, a) for a in range(d + 1)), d
    assert int(b.sum()) >= 5


def test_spike_has_deep_rows_in_tiles_shared_by_two_windows(segs):
    c = DC.make_case("spike")
    cov = c["nr"].astype(int) + c["na"]
    s = segs["spike"]
    shared = {int(t) for t in s["tile"] if int((s["tile"] == t).sum()) > 1}
    deep_alone = 0
    for i in range(len(s["nc"])):
        if int(s["tile"][i]) not in shared or s["nc"][i] <= 3:
            continue
        others = [k for k in range(len(s["nc"])) if s["tile"][k] == s["tile"][i] and k != i]
        # the deep row belongs to this window's part of the tile; the neighbouring window's segment of the same tile has none
        if all(s["nc"][k] <= 3 and s["na"][k] <= 2 for k in others) and int((cov[s["rows"][i]] >= 8).sum()) == 1:
            deep_alone += 1
    assert deep_alone >= 1
    # ... at both ends of a tile: a deep row at position 0 or 31 of a shared tile
    ends = {int(r % 32) for i in range(len(s["nc"])) if int(s["tile"][i]) in shared for r in s["rows"][i] if cov[r] >= 8}
    assert ends & {0, 31}, ends


def test_where_the_power_tables_sit():
    for name in DC.NAMES:
        c = DC.make_case(name)
        assert DC.tab_in_lds(c["nr"], c["na"], c["W"]) == (name != "full-depth-16"), name
    c = DC.make_case("full-depth-15")
    assert DC.ct_max(c["nr"], c["na"], 15) == 750 and (750 + 1) * 32 <= 24 * 1024 < (800 + 1) * 32
    c = DC.make_case("full-depth-16")
    assert DC.ct_max(c["nr"], c["na"], 16) == 800


def test_which_cases_the_matrix_core_groups_take():
    """k_ld_mfma keeps tables of 56 bytes an entry beside 36 KiB of strips, and the host gives it a run only within 64 KiB
    (ibdg_api.cpp): windows of up to about 500 reads.  full-depth-15 (750) lies beyond that whatever the run length, so its
    "mfma" forms are counted by k_ld_popcount_mt and the single-individual kernels; every other case with the tables in
    LDS goes to k_ld_mfma."""
    for name in DC.NAMES:
        c = DC.make_case(name)
        assert DC.mfma_takes(c["nr"], c["na"], c["W"]) == (name not in ("full-depth-15", "full-depth-16")), name


@pytest.mark.parametrize("name", DC.NAMES)
def test_every_window_truth_is_a_normal_double(name):
    """Both columns of every window of the case's target are at least 2^-1022: the absolute term A 2^-1074 of the bounds
    excuses nothing there, and a wrong exponent cannot hide in an underflow."""
    c = DC.make_case(name)
    tr = H.ld_truth(c["alle"], c["nr"], c["na"], c["target"], c["W"], H.binomial_factors(c["eps"], c["M"]), c["refids"], c["pu"])
    lo = min(tr["ibd0"].min(), tr["ibd1"].min())
    print(f"{name}: {len(tr['rows'])} windows, smallest truth 2^{float(np.log2(lo)):.0f}")
    assert lo >= LD(2.0) ** -1022 and np.isfinite(tr["ibd0"]).all() and np.isfinite(tr["ibd1"]).all()
    if c["W"] == 3:
        assert float(np.log2(LD(c["eps"]))) * 50 > -283                           # eps^50 a row: three rows stay above 2^-849


def test_run_seed_draws_the_target_first():
    for name in ("lattice", "full-depth-15"):
        c = DC.make_case(name)
        for T in (1, 4, 31):
            rng = np.random.default_rng(DC.run_seed(name, T))
            assert int(rng.choice(np.arange(130), size=T, replace=False)[0]) == c["target"]


def test_a_miscounted_plane_shows_in_the_window_value():
    """What the GPU test relies on: a spike row counted without its top plane (in the depth, or in the alt count) moves its
    window's truths far beyond the fast forms' bound, and no other window's."""
    c = DC.make_case("spike")
    fac = H.binomial_factors(c["eps"], c["M"])
    cov = c["nr"].astype(int) + c["na"]
    want = H.ld_truth(c["alle"], c["nr"], c["na"], c["target"], c["W"], fac)
    B = H.fast_B("popcount", 130)
    for row in np.flatnonzero(cov >= 8)[[0, 5, 17, 29, 35, 41]]:
        for plane_of in ("depth", "alt"):
            nr, na = c["nr"].astype(int), c["na"].astype(int)
            if plane_of == "depth":
                top = 1 << (int(cov[row]).bit_length() - 1)
                drop_alt = max(0, top - nr[row])                       # the reads that go: reference reads first
                nr[row], na[row] = nr[row] - (top - drop_alt), na[row] - drop_alt
            elif na[row] >= 4:
                top = 1 << (int(na[row]).bit_length() - 1)
                na[row], nr[row] = na[row] - top, nr[row] + top         # an alt plane lost: the depth stands
            else:
                continue
            got = H.ld_truth(c["alle"], nr, na, c["target"], c["W"], fac)
            k = [i for i, rows in enumerate(want["rows"]) if row in rows][0]
            for key in ("ibd0", "ibd1"):
                r = H.excess(got[key].astype(np.float64), want[key], B, H.FAST_A)
                assert r[k] > 1e6, (int(row), plane_of, key, float(r[k]))
                # (a depth of exactly 8 loses every read with its plane: the row leaves the windows, the later ones shift)
                assert ((np.delete(r, k) if nr[row] + na[row] else r[:k]) <= 1.0).all()
