"""ibdg_log2_segments_host: the segments of an IBD-state path on the host, no device.

The twin against a restatement in plain Python integers: itertools.groupby over ibdg_log2_states_host's path, the emissions
recomputed with numpy fp64 and Python's round (half to even) of the exact product, post_q from ibdg_log2_posteriors_host's
gammas the same way.  Records and summary equal exactly, on every table."""
import ctypes as C
import itertools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from ibdgem_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 255, 256, 257, 601]
DEFAULT = (1e-3, 1e-6, 1e-3)
PENS = [DEFAULT, (0.5, 0.25, 0.5), (1.0, 1.0, 1.0)]


@pytest.fixture(scope="module", autouse=True)
def library():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)


def random_table(n, seed=0, spread=3.0):
    """Logs far outside what a product of likelihoods could hold in a double; the columns close enough for every state to win."""
    rng = np.random.default_rng(77 * n + seed)
    return rng.normal(-3000.0, 400.0, (n, 1)) + rng.uniform(-spread, spread, (n, 3))


def positions(n, seed=0):
    """First and last position of n windows along a chromosome: increasing, a window of one site among them."""
    rng = np.random.default_rng(seed + n)
    gaps = rng.integers(0, 5000, 2 * n).astype(np.uint64)
    gaps[::7] = 0
    p = np.cumsum(gaps) + np.uint64(10_000)
    return p[0::2].copy(), p[1::2].copy()


def emissions(tab):
    """e_w[s] as Python integers: one fp64 subtraction, the clamp, then the exact product rounded half to even."""
    out = []
    for row in np.asarray(tab, dtype=np.float64).reshape(-1, 3):
        m = row.max() if not np.isnan(row).any() else np.nan
        if np.isnan(row).any() or not np.isfinite(m):
            out.append((0, 0, 0))
            continue
        d = np.maximum(row - m, -16777216.0)
        out.append(tuple(round(Fraction(float(x)) * 65536) for x in d))
    return out


def restated(tab, pen, with_post=False, pos=None):
    """(records as tuples (first, n_win, state, e0, e1, e2, post_q, post_min), summary as 12 Python integers)"""
    tab = np.asarray(tab, dtype=np.float64).reshape(-1, 3)
    path, _, count = E.log2_states_host(tab, *pen, want_score=False)
    e = emissions(tab)
    post = E.log2_posteriors_host(tab, *pen)[0] if with_post else None
    recs, summ, f = [], [0] * 12, 0
    for s, run in itertools.groupby(path.tolist()):
        n = len(list(run))
        ws = range(f, f + n)
        q = sum(round(Fraction(float(post[w, s])) * 2 ** 32) for w in ws) if with_post else 0
        mn = min(float(post[w, s]) for w in ws) if with_post else 0.0
        recs.append((f, n, s, *(sum(e[w][k] for w in ws) for k in range(3)), q, mn))
        summ[s] += 1
        summ[3 + s] = max(summ[3 + s], n)
        if pos is not None:
            span = (int(pos[1][f + n - 1]) - int(pos[0][f]) + 1) % 2 ** 64
            summ[6 + s] = (summ[6 + s] + span) % 2 ** 64
            summ[9 + s] = max(summ[9 + s], span)
        f += n
    return recs, summ, count


def as_tuples(seg):
    return [(int(r["first"]), int(r["n_win"]), int(r["state"]), *(int(x) for x in r["e"]), int(r["post_q"]), float(r["post_min"]))
            for r in seg]


def twin_checked(tab, pen, with_post=False, pos=None):
    tab = np.asarray(tab, dtype=np.float64).reshape(-1, 3)
    n = len(tab)
    pf, pl = pos if pos is not None else (None, None)
    seg, n_seg, summary = E.log2_segments_host(tab, *pen, with_post=with_post, pos_first=pf, pos_last=pl)
    recs, summ, count = restated(tab, pen, with_post, pos)
    assert n_seg == len(recs) == len(seg)
    assert as_tuples(seg) == recs
    assert [int(x) for x in summary] == summ
    assert (seg["reserved"] == 0).all()
    # the records tile the windows
    assert int(seg["n_win"].sum()) == n
    assert (seg["first"] == np.concatenate([[0], np.cumsum(seg["n_win"])[:-1]])).all()
    assert (seg["state"][1:] != seg["state"][:-1]).all()
    # the summary against the path's own counts
    for s in range(3):
        mine = seg[seg["state"] == s]
        assert int(mine["n_win"].sum()) == int(count[s])
        assert int(summary[s]) == len(mine) and int(summary[3 + s]) == (int(mine["n_win"].max()) if len(mine) else 0)
    # count and summary alone are the same
    s2, n2, sum2 = E.log2_segments_host(tab, *pen, with_post=with_post, pos_first=pf, pos_last=pl, want_seg=False)
    assert s2 is None and n2 == n_seg and sum2.tobytes() == summary.tobytes()
    return seg, n_seg, summary


def test_the_record_is_56_bytes():
    assert E.SEGMENT_DTYPE.itemsize == 56
    assert [E.SEGMENT_DTYPE.fields[k][1] for k in ("first", "n_win", "state", "reserved", "e", "post_q", "post_min")] == \
        [0, 4, 8, 12, 16, 40, 48]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pen", PENS)
def test_random_tables(n, pen):
    tab = random_table(n)
    twin_checked(tab, pen)
    twin_checked(tab, pen, pos=positions(n))
    seg, n_seg, summary = twin_checked(tab, pen, with_post=True, pos=positions(n))
    assert (seg["post_min"] > 0).all() and (seg["post_min"] <= 1).all()
    assert (seg["post_q"] <= seg["n_win"].astype(np.uint64) << np.uint64(32)).all()
    # without positions the bp groups are 0; without posteriors the support is 0
    seg0, _, sum0 = twin_checked(tab, pen)
    assert (sum0[6:] == 0).all() and (seg0["post_q"] == 0).all() and (seg0["post_min"] == 0.0).all()
    assert sum0[:6].tobytes() == summary[:6].tobytes()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pen", PENS)
def test_the_three_twins_agree(n, pen):
    """ibdg_log2_segments_host runs the same recurrence and the same sum-product pass as its two neighbours: its records and
    summary with posteriors, assembled from THEIR path and gammas (restated), and the bytes of its post_min against the gammas'."""
    tab, pos = random_table(n), positions(n)
    seg, n_seg, summary = E.log2_segments_host(tab, *pen, with_post=True, pos_first=pos[0], pos_last=pos[1])
    recs, summ, count = restated(tab, pen, with_post=True, pos=pos)
    assert n_seg == len(recs) and as_tuples(seg) == recs and [int(x) for x in summary] == summ
    path, _, count2 = E.log2_states_host(tab, *pen, want_score=False)
    post = E.log2_posteriors_host(tab, *pen)[0]
    assert count2.tobytes() == count.tobytes()
    assert np.repeat(seg["state"], seg["n_win"]).astype(np.uint8).tobytes() == path.astype(np.uint8).tobytes()
    mins = np.array([post[int(r["first"]):int(r["first"]) + int(r["n_win"]), int(r["state"])].min() for r in seg])
    assert seg["post_min"].tobytes() == mins.astype(np.float64).tobytes()


def test_random_tables_show_every_case():
    """What the random tables are there for: at 601 windows the small penalties give many segments of all three states."""
    seg, n_seg, _ = twin_checked(random_table(601), (0.5, 0.25, 0.5))
    assert n_seg > 20 and set(seg["state"].tolist()) == {0, 1, 2} and seg["n_win"].max() > 1
    seg, n_seg, _ = twin_checked(random_table(601), DEFAULT)
    assert n_seg < 601


def test_no_windows():
    seg, n_seg, summary = E.log2_segments_host(np.zeros((0, 3)), *DEFAULT, with_post=True)
    assert len(seg) == 0 and n_seg == 0 and (summary == 0).all()
    e = np.zeros(0, dtype=np.uint64)
    seg, n_seg, summary = E.log2_segments_host(np.zeros((0, 3)), *DEFAULT, pos_first=e, pos_last=e)
    assert len(seg) == 0 and n_seg == 0 and (summary == 0).all()


def test_windows_that_say_nothing():
    """A NaN column, a maximum of -inf or +inf: emission (0, 0, 0), which adds nothing to a sum and breaks no segment by itself."""
    tab = random_table(300, 1)
    tab[5, 1] = np.nan
    tab[17] = -np.inf
    tab[18, 2] = np.inf
    tab[100:140, 0] = np.nan
    tab[299] = np.nan
    tab[200, 1] = -np.inf                       # a -inf column beside finite ones: clamped, not silent
    for pen in PENS:
        seg, _, _ = twin_checked(tab, pen, with_post=True, pos=positions(300))
    e = emissions(tab)
    assert e[5] == e[17] == e[18] == e[120] == e[299] == (0, 0, 0) and min(e[200]) == -(1 << 40)
    quiet = np.full((40, 3), np.nan)
    seg, n_seg, summary = twin_checked(quiet, DEFAULT, with_post=True)
    assert n_seg == 1 and as_tuples(seg)[0][:6] == (0, 40, 0, 0, 0, 0)


def test_one_state_throughout():
    for s in range(3):
        tab = np.full((700, 3), -5000.0)
        tab[:, s] = -4990.0
        seg, n_seg, summary = twin_checked(tab, DEFAULT, with_post=True, pos=positions(700))
        assert n_seg == 1 and (int(seg[0]["first"]), int(seg[0]["n_win"]), int(seg[0]["state"])) == (0, 700, s)
        assert [int(x) for x in seg[0]["e"]] == [0 if k == s else -700 * 10 * 65536 for k in range(3)]
        pf, pl = positions(700)
        assert int(summary[6 + s]) == int(summary[9 + s]) == int(pl[-1]) - int(pf[0]) + 1


def test_a_change_at_every_window():
    n = 515
    tab = np.full((n, 3), -900.0)
    tab[np.arange(n), np.arange(n) % 3] = -890.0
    seg, n_seg, summary = twin_checked(tab, (1.0, 1.0, 1.0), with_post=True, pos=positions(n))
    assert n_seg == n and (seg["n_win"] == 1).all() and (seg["state"] == np.arange(n) % 3).all()
    assert [int(x) for x in summary[:6]] == [172, 172, 171, 1, 1, 1]


def test_differences_below_the_clamp():
    tab = random_table(64, 3)
    tab[::2, 0] -= 2.0 ** 25
    tab[1::4, 2] -= 1e300
    tab[10:20, 1] += 2.0 ** 30                   # the other two clamped at once
    for pen in PENS:
        seg, _, _ = twin_checked(tab, pen, with_post=True)
        assert min(int(x) for r in seg for x in r["e"]) <= -(1 << 40)


def test_a_sum_of_2_to_the_61_does_not_wrap():
    """2^21 windows with column 2 clamped in every one: e[2] = -2^21 * 2^40 = -2^61 in the one segment."""
    n = 1 << 21
    tab = np.zeros((n, 3))
    tab[:, 0] = -7.0
    tab[:, 1] = -7.5
    tab[:, 2] = -1e9
    seg, n_seg, summary = E.log2_segments_host(tab, *DEFAULT)
    assert n_seg == 1 and [int(x) for x in summary[:6]] == [1, 0, 0, n, 0, 0]
    assert as_tuples(seg) == [(0, n, 0, 0, -n * 32768, -(1 << 61), 0, 0.0)]
    with pytest.raises(E.EngineError, match=r"ibdg_log2_states_host: \d+ windows, more than"):
        E.log2_segments_host(np.zeros((n + 1, 3)), *DEFAULT)


def test_a_cap_below_the_count():
    tab = random_table(601)
    pen = (0.5, 0.25, 0.5)
    full, n_seg, summary = E.log2_segments_host(tab, *pen, with_post=True)
    assert n_seg > 20
    for cap in (0, 1, 7, n_seg - 1, n_seg, n_seg + 3):
        # (engine.log2_segments_host keeps a sentinel record behind the cap and raises if it is touched)
        seg, n2, sum2 = E.log2_segments_host(tab, *pen, with_post=True, seg_cap=cap)
        assert n2 == n_seg and sum2.tobytes() == summary.tobytes()
        assert seg.tobytes() == full[:cap].tobytes()


def test_positions_wrap_like_any_unsigned_sum():
    tab = np.full((4, 3), -100.0)
    tab[:, 1] = -90.0
    pf = np.array([0, 5, 6, 7], dtype=np.uint64)
    pl = np.array([2, 5, 6, 2 ** 64 - 1], dtype=np.uint64)
    _, _, summary = twin_checked(tab, DEFAULT, pos=(pf, pl))
    assert int(summary[7]) == 0 and int(summary[10]) == 0          # 2^64 - 1 - 0 + 1 wraps to 0


def test_errors():
    lib = E.load_library()
    tab = random_table(10)
    for pen in ((0.0, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, float("nan")), (-1.0, 0.5, 0.5)):
        with pytest.raises(E.EngineError, match=r"ibdg_log2_states_host: p\d\d = .* is not in \(0, 1\]"):
            E.log2_segments_host(tab, *pen)
        with pytest.raises(E.EngineError, match=r"p\d\d = .* is not in \(0, 1\]"):
            E.log2_segments_host(tab, *pen, with_post=True)
    pf, pl = positions(10)
    with pytest.raises(E.EngineError, match="ibdg_log2_segments_host: pos_first without pos_last"):
        E.log2_segments_host(tab, *DEFAULT, pos_first=pf)
    with pytest.raises(E.EngineError, match="ibdg_log2_segments_host: pos_last without pos_first"):
        E.log2_segments_host(tab, *DEFAULT, pos_last=pl)
    bad = pl.copy()
    bad[4] = pf[4] - np.uint64(1)
    with pytest.raises(E.EngineError, match="ibdg_log2_segments_host: window 4 ends at"):
        E.log2_segments_host(tab, *DEFAULT, pos_first=pf, pos_last=bad)
    n_seg, summary = C.c_uint64(0), np.zeros(12, dtype=np.uint64)
    args = (tab.ctypes.data, 10, 0.5, 0.5, 0.5, 0, None, None, None, 0)
    assert lib.ibdg_log2_segments_host(*args, None, summary.ctypes.data) != 0
    assert b"NULL n_seg" in lib.ibdg_last_error(None)
    assert lib.ibdg_log2_segments_host(*args, C.addressof(n_seg), None) != 0
    assert b"NULL summary" in lib.ibdg_last_error(None)
    assert lib.ibdg_log2_segments_host(None, 10, 0.5, 0.5, 0.5, 0, None, None, None, 0, C.addressof(n_seg), summary.ctypes.data) != 0
    assert b"NULL table" in lib.ibdg_last_error(None)
    assert lib.ibdg_log2_segments_host(*args, C.addressof(n_seg), summary.ctypes.data) == 0 and n_seg.value >= 1
