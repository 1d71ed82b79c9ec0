"""Window chains on the host: ibdg_log2_states_chains_host, ibdg_log2_posteriors_chains_host and
ibdg_log2_segments_chains_host, no device.

A chain start is a window treated the way window 0 is: uniform entry, no penalty into it.  The chains are then independent, which
gives a truth that does not come from the code under test: the path, the counts and the segments of a chained call are those of
separate calls on the slices (bytes), the scores are the slices' plus a running constant (exactly), and the posteriors are the
exact truth of tests/hp_post_ref.py on each slice within that module's bar at the whole table's length (the joint pass carries
its roundings across the borders; the count per window, R = 14, is unchanged: a start multiplies by 1.0, which is exact).
Beside that: no chains give today's bytes, a Python restatement of the chained recurrence, tables on which the chains change
the answer, and the refusals."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hp_post_ref as H
from ibdgem_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 5, 100, 257, 601]
DEFAULT = (1e-3, 1e-6, 1e-3)
PENS = [DEFAULT, (0.5, 0.25, 0.5)]
U = 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def library():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)


def table(n, seed=0):
    """Small random logs, the columns within +-8 bits (so that paths switch), with NaN, +-inf and all-equal rows mixed in."""
    rng = np.random.default_rng(977 * n + seed)
    tab = rng.normal(-300.0, 40.0, (n, 1)) + rng.uniform(-8.0, 8.0, (n, 3))
    for w in range(n):
        k = rng.integers(0, 24)
        if k == 0:
            tab[w, rng.integers(0, 3)] = math.nan
        elif k == 1:
            tab[w, rng.integers(0, 3)] = -math.inf
        elif k == 2:
            tab[w, rng.integers(0, 3)] = math.inf
        elif k == 3:
            tab[w] = tab[w, 0]
        elif k == 4:
            tab[w] = -math.inf
    return tab


def positions(n, seed=0):
    rng = np.random.default_rng(31 * n + seed)
    first = np.cumsum(rng.integers(1, 5000, n)).astype(np.uint64) * 2
    return first, first + rng.integers(0, 2, n).astype(np.uint64)


def start_sets(n):
    """{name: sorted starts}: window 1, the last window, every window, two consecutive windows, every block border k C -- and
    k C - 1, k C + 1 where C > 1 --, a seeded random set."""
    Cb = H.blocking(n)[0]
    rng = np.random.default_rng(n)
    sets = {"first": [1], "last": [n - 1], "every": list(range(1, n)), "two": [n // 2, n // 2 + 1],
            "borders": list(range(Cb, n, Cb)),
            "random": sorted(set(rng.integers(1, n, max(1, n // 9)).tolist()))}
    if Cb > 1:
        sets["borders-1"] = [w - 1 for w in range(Cb, n, Cb)]
        sets["borders+1"] = [w + 1 for w in range(Cb, n, Cb)]
    return {k: sorted(set(w for w in v if 1 <= w < n)) for k, v in sets.items()}


CASES = [(n, name) for n in SIZES for name in start_sets(n)]


def chains_of(n, starts):
    cuts = [0] + list(starts) + [n]
    return list(zip(cuts[:-1], cuts[1:]))


def join_summaries(parts):
    out = [0] * 12
    for p in parts:
        for i in range(12):
            out[i] = max(out[i], int(p[i])) if (i // 3) & 1 else out[i] + int(p[i])
    return out


# ---- a. no chains ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1] + SIZES)
@pytest.mark.parametrize("pen", PENS)
def test_no_starts_give_the_bytes_of_the_three_twins(n, pen):
    tab = table(n) if n else np.zeros((0, 3))
    pf, pl = positions(n) if n else (np.zeros(0, np.uint64),) * 2
    for a, b in zip(E.log2_states_host(tab, *pen), E.log2_states_host(tab, *pen, starts=[])):
        assert a.tobytes() == b.tobytes()
    a, b = E.log2_posteriors_host(tab, *pen), E.log2_posteriors_host(tab, *pen, starts=[])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    for kw in (dict(), dict(with_post=True), dict(pos_first=pf, pos_last=pl), dict(with_post=True, pos_first=pf, pos_last=pl)):
        a, b = E.log2_segments_host(tab, *pen, **kw), E.log2_segments_host(tab, *pen, starts=[], **kw)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()


# ---- b. the definition, restated ------------------------------------------------------------------------------------------

def restated(tab, pen, starts):
    """The chained integer recurrence of ibdg_states.h in Python integers: (path, scores, counts)."""
    P01, P02, P12 = (H.penalty(p) for p in pen)
    penm = [[0, P01, P02], [P01, 0, P12], [P02, P12, 0]]
    zero = [[0] * 3] * 3
    starts = set(starts)
    n = len(tab)
    score, frm = [], []
    for w in range(n):
        e = H.emission(tab[w])
        if w == 0:
            v, f = list(e), [0, 1, 2]
        else:
            m = zero if w in starts else penm
            prev, v, f = score[-1], [], []
            for s in range(3):
                best, arg = prev[0] + m[0][s], 0
                for q in (1, 2):
                    if prev[q] + m[q][s] > best:                      # strict: the lowest state wins a tie
                        best, arg = prev[q] + m[q][s], q
                v.append(best + e[s])
                f.append(arg)
        score.append(v)
        frm.append(f)
    st = 0
    for s in (1, 2):
        if score[-1][s] > score[-1][st]:
            st = s
    path = [0] * n
    for w in range(n - 1, -1, -1):
        path[w] = st
        st = frm[w][st]
    return path, score, [path.count(s) for s in range(3)]


@pytest.mark.parametrize("n,name", CASES)
@pytest.mark.parametrize("pen", PENS)
def test_the_restated_recurrence(n, name, pen):
    tab, starts = table(n), start_sets(n)[name]
    path, score, count = E.log2_states_host(tab, *pen, starts=starts)
    rp, rs, rc = restated(tab, pen, starts)
    assert path.tolist() == rp and count.tolist() == rc
    assert score.tolist() == rs
    for w in starts:                                                     # at a start `from` is the same for every state: the score
        assert len({int(score[w, s]) - H.emission(tab[w])[s] for s in range(3)}) == 1     # is one maximum plus the emission


# ---- c. independence: path, counts, scores, segments ----------------------------------------------------------------------

@pytest.mark.parametrize("n,name", CASES)
@pytest.mark.parametrize("pen", PENS)
def test_chains_are_separate_calls_on_the_slices(n, name, pen):
    tab, starts = table(n), start_sets(n)[name]
    pf, pl = positions(n)
    path, score, count = E.log2_states_host(tab, *pen, starts=starts)
    post, _, _ = E.log2_posteriors_host(tab, *pen, starts=starts)
    parts, K = [], 0
    for c0, c1 in chains_of(n, starts):
        p, s, c = E.log2_states_host(tab[c0:c1], *pen)
        assert path[c0:c1].tobytes() == p.tobytes(), (c0, c1)
        assert (score[c0:c1] == s + K).all(), (c0, c1)                    # exactly: integers
        K = int(score[c1 - 1].max())
        parts.append(c)
    assert count.tolist() == np.sum(parts, axis=0).tolist()
    for with_pos in (False, True):
        kw = dict(pos_first=pf, pos_last=pl) if with_pos else {}
        for with_post in (False, True):
            seg, n_seg, summary = E.log2_segments_host(tab, *pen, with_post=with_post, starts=starts, **kw)
            want, sums = [], []
            for c0, c1 in chains_of(n, starts):
                kws = dict(pos_first=pf[c0:c1], pos_last=pl[c0:c1]) if with_pos else {}
                s, k, sm = E.log2_segments_host(tab[c0:c1], *pen, **kws)
                s = s.copy()
                s["first"] += c0
                want.append(s)
                sums.append(sm)
            want = np.concatenate(want)
            assert n_seg == len(want) == len(seg)
            assert summary.tolist() == join_summaries(sums)
            assert (seg["reserved"] == 0).all()
            for f in ("first", "n_win", "state", "e"):
                assert seg[f].tobytes() == want[f].tobytes(), f
            if not with_post:
                assert seg.tobytes() == want.tobytes()                    # every byte: the slices' records, `first` shifted
            else:
                # the support is that of the chained posteriors (the joint pass: the slices' own gammas only within the bar)
                for r in seg:
                    g = post[r["first"]:r["first"] + r["n_win"], r["state"]]
                    assert int(r["post_q"]) == sum(int(np.rint(x * 2.0 ** 32)) for x in g) and r["post_min"] == g.min()
    # no record crosses a border
    seg, _, _ = E.log2_segments_host(tab, *pen, starts=starts)
    firsts = set(seg["first"].tolist())
    assert set(starts) <= firsts
    for r in seg:
        assert not any(r["first"] < w < r["first"] + r["n_win"] for w in starts)


# ---- d. posteriors against the exact truth of every chain ------------------------------------------------------------------

_truths = {}


def truth_of(n, c0, c1, pen):
    key = (n, c0, c1, pen)
    if key not in _truths:
        _truths[key] = H.Truth(table(n)[c0:c1], *pen)
    return _truths[key]


def test_the_bar_holds_at_these_sizes():
    assert H.R == 14
    for n in SIZES:
        assert H.Rn(n) * U <= 1e-10 and n <= H.EXACT_WINDOWS


@pytest.mark.parametrize("n,name", CASES)
@pytest.mark.parametrize("pen", PENS)
def test_posteriors_are_each_chains_own(n, name, pen):
    tab, starts = table(n), start_sets(n)[name]
    post, expect, log2_z = E.log2_posteriors_host(tab, *pen, starts=starts)
    assert np.isfinite(post).all()
    want = [Fraction(0)] * 3
    Z, ez = 1, 0
    for c0, c1 in chains_of(n, starts):
        t = truth_of(n, c0, c1, pen)
        for w in range(c0, c1):
            for s in range(3):
                err, bar = H.gamma_err_and_bar(float(post[w, s]), t.P[w - c0][s], t.Z, n)       # the whole table's n
                assert err <= bar, f"gamma[{w}][{s}] = {post[w, s]!r}: {H._ratio(err, bar):.3g} bars from its chain's ({c0}, {c1})"
        for s in range(3):
            want[s] += Fraction(t.S[s][0], t.Z)
        Z, ez = Z * t.Z, ez + t.ez
    for s in range(3):
        err, bar = H.expect_err_and_bar(float(expect[s]), want[s].numerator, want[s].denominator, n)
        assert err <= bar, f"expect[{s}] = {expect[s]!r}: {H._ratio(err, bar):.3g} bars from {float(want[s])!r}"
    bl = Z.bit_length()
    top = Z >> (bl - 64) if bl > 64 else Z << (64 - bl)
    truth = math.log2(top / 2.0 ** 64) + (bl + ez)
    r = H.log2_z_err_over_bar(log2_z, truth, n)
    assert r <= 1.0, f"log2_z = {log2_z!r}: {r:.3g} bars from {truth!r}"
    p2, e2, z2 = E.log2_posteriors_host(tab, *pen, want_post=False, starts=starts)
    assert p2 is None and e2.tobytes() == expect.tobytes() and z2 == log2_z


# ---- e. the tests can fail: tables on which the chains change the answer --------------------------------------------------

def test_one_window_against_the_rest():
    """IBD0 by 5 bits everywhere but in one window, which favours IBD1 by 5: one chain pays two switches (2 x 9.97 bits) for 10
    bits and stays in IBD0; with starts at that window and the next it is a chain of its own and takes IBD1."""
    n, w = 40, 17
    tab = np.full((n, 3), -100.0)
    tab[:, 0] += 5.0
    tab[w] = [-100.0, -95.0, -100.0]
    path, _, count = E.log2_states_host(tab, *DEFAULT)
    assert path.tolist() == [0] * n
    path, _, count = E.log2_states_host(tab, *DEFAULT, starts=[w, w + 1])
    assert path.tolist() == [0] * w + [1] + [0] * (n - w - 1) and count.tolist() == [n - 1, 1, 0]
    seg, n_seg, summary = E.log2_segments_host(tab, *DEFAULT, starts=[w, w + 1])
    assert seg["first"].tolist() == [0, w, w + 1] and seg["state"].tolist() == [0, 1, 0] and summary[:3].tolist() == [2, 1, 0]
    seg, n_seg, _ = E.log2_segments_host(tab, *DEFAULT, starts=[w + 5])   # a start inside a run of one state cuts it
    assert seg["first"].tolist() == [0, w + 5] and seg["state"].tolist() == [0, 0]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pen", PENS)
def test_one_chain_lies_a_thousand_bars_from_the_chains(n, pen):
    """Chains that favour different states by 20 bits: the truth of the table as ONE chain (the model without starts) lies at
    least 1000 bars from the chains' own truth in some window -- what the bars of test_posteriors_are_each_chains_own can
    tell apart."""
    for name, starts in start_sets(n).items():
        tab = np.full((n, 3), -200.0)
        for k, (c0, c1) in enumerate(chains_of(n, starts)):
            tab[c0:c1, (2 * k) % 3] += 20.0
        one = H.Truth(tab, *pen)
        found = False
        for c0, c1 in chains_of(n, starts):
            t = H.Truth(tab[c0:c1], *pen)
            for w in (c0, c1 - 1):
                for s in range(3):
                    err, bar = H.control_err_and_bar(one.P[w][s], one.Z, t.P[w - c0][s], t.Z, n)
                    found = found or err >= 1000 * bar
            if found:
                break
        assert found, (n, name)


# ---- f. refusals ----------------------------------------------------------------------------------------------------------

BAD = [([0], r"starts\[0\] = 0 \(window 0 always starts a chain"),
       ([3, 0], r"starts\[1\] = 0 "),
       ([10], r"starts\[0\] = 10 is not below the 10 windows"),
       ([2, 4000000000], r"starts\[1\] = 4000000000 is not below the 10 windows"),
       ([5, 3], r"starts\[1\] = 3 does not lie above starts\[0\] = 5 \(strictly increasing\)"),
       ([4, 4], r"starts\[1\] = 4 does not lie above starts\[0\] = 4 \(strictly increasing\)")]


@pytest.mark.parametrize("starts,msg", BAD)
def test_bad_starts_are_refused_by_all_three(starts, msg):
    tab = table(10)
    for fn, call in (("ibdg_log2_states_chains_host", E.log2_states_host), ("ibdg_log2_posteriors_chains_host", E.log2_posteriors_host),
                     ("ibdg_log2_segments_chains_host", E.log2_segments_host)):
        with pytest.raises(E.EngineError, match=fn + ": " + msg):
            call(tab, *DEFAULT, starts=starts)


def test_null_starts_and_the_namesakes_refusals():
    lib = E.load_library()
    tab = table(10)
    count, expect, z = np.zeros(3, np.uint64), np.zeros(3), C.c_double(0.0)
    n_seg, summary = C.c_uint64(0), np.zeros(12, np.uint64)
    assert lib.ibdg_log2_states_chains_host(tab.ctypes.data, 10, *DEFAULT, None, None, count.ctypes.data, None, 2) != 0
    assert "ibdg_log2_states_chains_host: NULL starts with n_starts = 2" in lib.ibdg_last_error(None).decode()
    assert lib.ibdg_log2_posteriors_chains_host(tab.ctypes.data, 10, *DEFAULT, None, expect.ctypes.data, C.addressof(z), None, 1) != 0
    assert "ibdg_log2_posteriors_chains_host: NULL starts with n_starts = 1" in lib.ibdg_last_error(None).decode()
    assert lib.ibdg_log2_segments_chains_host(tab.ctypes.data, 10, *DEFAULT, 0, None, None, None, 0, C.addressof(n_seg),
                                              summary.ctypes.data, None, 3) != 0
    assert "ibdg_log2_segments_chains_host: NULL starts with n_starts = 3" in lib.ibdg_last_error(None).decode()
    # NULL with no starts is no chains
    assert lib.ibdg_log2_states_chains_host(tab.ctypes.data, 10, *DEFAULT, None, None, count.ctypes.data, None, 0) == 0
    assert count.tolist() == E.log2_states_host(tab, *DEFAULT)[2].tolist()
    # the namesakes' refusals, under the new names
    with pytest.raises(E.EngineError, match=r"ibdg_log2_states_chains_host: p01 = 0 is not in \(0, 1\]"):
        E.log2_states_host(tab, 0.0, 0.5, 0.5, starts=[1])
    with pytest.raises(E.EngineError, match=r"ibdg_log2_posteriors_chains_host: p12 = 2 is not in \(0, 1\]"):
        E.log2_posteriors_host(tab, 0.5, 0.5, 2.0, starts=[1])
    assert lib.ibdg_log2_states_chains_host(tab.ctypes.data, (1 << 21) + 1, *DEFAULT, None, None, count.ctypes.data, None, 0) != 0
    assert "2^21" in lib.ibdg_last_error(None).decode()
    # no windows: every start is outside
    with pytest.raises(E.EngineError, match=r"starts\[0\] = 1 is not below the 0 windows"):
        E.log2_states_host(np.zeros((0, 3)), *DEFAULT, starts=[1])
