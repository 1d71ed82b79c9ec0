"""CPU tier of the hard log tables (tests/hard_tables.py): no device.

  1. The cases are what they claim: assertions on the integers of states_emission restated in Python (hp_post_ref.emission), for
     the dead-shift family on the shifted switch weight, for dead-underflow on the product that underflows.
  2. The six finite families at every size: the host twin gives no NaN, rows of gamma that sum to 1 within 4 u, a finite log2_z.
  3. The twin against references that share no code with it, on every family: the path against the integer recurrence of
     hp_steps_ref, the posteriors byte for byte against the definition's fixed order restated in Python floats (restated_posteriors
     below -- the tables of this file put an entry at 0, at a subnormal or 2^-1000 below its vector's largest at most windows, which
     is where post_rescale and post_weight have branches), the records against sums formed from those, the draws byte for byte
     against hp_sample_ref; and, at the sizes an exact truth can afford, the posteriors within the counted bar of hp_steps_ref.Truth.
  4. The dead families: gamma = 0 in every row, expect = (0, 0, 0), log2_z = -inf, records with post_q = 0 and post_min = 0.0, the
     path untouched (the integer recurrence's), the draws the restatement's; for dead-shift the exact truth has Z == 0 as well.
  5. The negative control: the restatement without the rule (0 / 0 as IEEE has it) is NaN in every dead row, differs from the
     twin there and equals it everywhere else: without the rule the twin would fail 4.
  6. The host program on 200 sites of real input that reach a dead chain (hard_tables.write_dead_chain_input), on its route
     without a device."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hard_tables as HT
import hp_post_ref as H
import hp_sample_ref as R
import hp_steps_ref as S
from ibdgem_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
TRUTH_SIZES = [1, 2, 3, 256, 257]                # what an exact truth of every family can afford (edge1000 at 257: a second each)


@pytest.fixture(scope="module", autouse=True)
def library():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)


# ---- the definition's posteriors in its fixed order, in Python floats -------------------------------------------------------

def _mat_vec(M, v):
    return [(M[3 * q] * v[0] + M[3 * q + 1] * v[1]) + M[3 * q + 2] * v[2] for q in range(3)]


def restated_posteriors(tab, pen, shift=None, starts=(), rule=True, model=None):
    """(post [n][3], expect [3], log2_z) by steps 1 .. 5 of ibdg_states.h, on the weights of hp_sample_ref.Model.  rule: the
    dead-chain rule; without it a window with D == 0 gets IEEE's 0 / 0.  model: that Model, where the caller has it already."""
    m = model or R.Model(tab, pen, None if shift is None else [int(x) for x in shift], starts)
    n = m.n
    _, nbk, blocks = H.blocking(n)
    mat, mexp = [], []
    for w0, w1 in blocks:                                       # 1
        B = m.b[0] * 3 if w0 == 0 else m._matrix(w0)
        e = 0
        for w in range(w0 + 1, w1):
            M = m._matrix(w)
            B = R._vec_mat(B[0:3], M) + R._vec_mat(B[3:6], M) + R._vec_mat(B[6:9], M)
            B, e = R._rescale(B, e)
        mat.append(B)
        mexp.append(e)
    fin, fexp = [None] * nbk, [0] * nbk                         # 2
    v, e = mat[0][0:3], mexp[0]
    for k in range(1, nbk):
        fin[k], fexp[k] = list(v), e
        if k + 1 < nbk:
            v, e = R._rescale(R._vec_mat(v, mat[k]), e + mexp[k])
    gout, g = [None] * nbk, [1.0, 1.0, 1.0]
    for k in range(nbk - 1, -1, -1):
        gout[k] = list(g)
        if k > 0:
            g, _ = R._rescale(_mat_vec(mat[k], g), 0)
    post, part = [None] * n, [[0.0, 0.0, 0.0] for _ in range(256)]
    D, De = 1.0, 0
    for b, (w0, w1) in enumerate(blocks):
        be = list(gout[b])                                      # 3
        for w in range(w1 - 1, w0 - 1, -1):
            post[w] = list(be)
            if w > w0:
                be, _ = R._rescale(_mat_vec(m._matrix(w), be), 0)
        v, e = (fin[b], fexp[b]) if b else (None, 0)            # 4
        acc = [0.0, 0.0, 0.0]
        for w in range(w0, w1):
            if w == 0:
                v, e = list(m.b[0]), 0
            else:
                v, e = R._rescale(R._vec_mat(v, m._matrix(w)), e)
            p = [v[s] * post[w][s] for s in range(3)]
            D, De = (p[0] + p[1]) + p[2], e
            if D == 0.0:
                assert p == [0.0, 0.0, 0.0]
                g3 = [0.0] * 3 if rule else [math.nan] * 3
            else:
                g3 = [x / D for x in p]
            post[w] = g3
            acc = [acc[s] + g3[s] for s in range(3)]
        part[b] = acc
    d = 128                                                     # 5
    while d:
        for b in range(d):
            part[b] = [part[b][s] + part[b + d][s] for s in range(3)]
        d //= 2
    return post, part[0], (math.log2(D) if D > 0.0 else -math.inf) + float(De)


def restated_records(tab, path, post, starts=()):
    """[(first, n_win, state, e0, e1, e2, post_q, post_min)] from a path and gammas (None: no support), in Python integers."""
    e, starts, out, f, n = [H.emission(row) for row in tab], set(starts), [], 0, len(path)
    while f < n:
        w = f + 1
        while w < n and path[w] == path[f] and w not in starts:
            w += 1
        s = path[f]
        q = sum(round(Fraction(post[x][s]) * 2 ** 32) for x in range(f, w)) if post is not None else 0
        mn = min(post[x][s] for x in range(f, w)) if post is not None else 0.0
        out.append((f, w - f, s, *(sum(e[x][k] for x in range(f, w)) for k in range(3)), q, mn))
        f = w
    return out


def as_tuples(seg):
    return [(int(r["first"]), int(r["n_win"]), int(r["state"]), *(int(x) for x in r["e"]), int(r["post_q"]), float(r["post_min"]))
            for r in seg]


def bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def forms(c):
    """(penalties, starts, shift) a case is run with: a dead family under its own penalties and shift, with chain starts that keep
    away from its pair; a finite one under both penalty sets, plain, with chains, with shifts drawn from +-3 bits, with both."""
    n = c.n
    if c.family in HT.DEAD:
        keep = [w for w in HT.chain_starts(n) if c.marks.get(w) is None]
        return [(c.pen, (), c.shift), (c.pen, keep, c.shift)]
    sh = HT.shifts(n, 9) if n >= 2 else None
    out = []
    for pen in HT.PENS:
        out += [(pen, (), None), (pen, HT.chain_starts(n), None)]
        if n >= 2:
            out += [(pen, (), sh), (pen, HT.chain_starts(n), sh)]
    return out


def kw(starts, shift):
    return dict(starts=list(starts) if len(starts) else None, shift=shift)


def variants(family):
    return range(2) if family in HT.DEAD else range(5)


# ---- 1. the cases are what they claim ---------------------------------------------------------------------------------------

def test_sizes_and_edge_windows():
    assert [HT.blocking(n)[0] for n in HT.SIZES] == [1, 1, 1, 1, 1, 2, 3, 5]
    assert HT.edge_windows(1) == [0] and HT.edge_windows(2) == [0, 1] and HT.edge_windows(3) == [0, 1, 2]
    assert HT.edge_windows(257) == [0, 1, 2, 3, 4, 128, 255, 256]               # C = 2: 0, 1, C, 2 C - 1, 2 C, n / 2, n - 2, n - 1
    assert HT.edge_windows(1279) == [0, 1, 4, 5, 9, 10, 639, 1275, 1277, 1278]  # C = 5, the last block begins at 1275
    for n in HT.SIZES:
        assert [H.blocking(n)[0], H.blocking(n)[1]] == list(HT.blocking(n))


@pytest.mark.parametrize("n", HT.SIZES)
def test_naninf_windows_say_nothing_or_meet_the_clamp(n):
    seen = set()
    for v in range(5):
        c = HT.case("naninf", n, v)
        assert sorted(c.marks) == HT.edge_windows(n)
        for w, (kind, col) in c.marks.items():
            e = H.emission(c.tab[w])
            seen.add(kind)
            if kind == "-inf":                       # two finite columns beside it: the difference is -inf, the clamp's
                assert e[col] == -(1 << 40) and max(e) == 0 and np.isfinite(np.delete(c.tab[w], col)).all()
            else:
                assert e == [0, 0, 0], (w, kind)
        for w in set(range(n)) - set(c.marks):
            assert np.isfinite(c.tab[w]).all()
    assert seen == set(HT.NANINF_KINDS)              # every kind at every size, over the five variants


@pytest.mark.parametrize("n", HT.SIZES)
def test_deep_and_alternating_have_one_live_state(n):
    for fam in ("deep", "alternating"):
        for v in range(5):
            c = HT.case(fam, n, v)
            assert sorted(c.marks) == (HT.edge_windows(n) if fam == "deep" else list(range(n)))
            for w, live in c.marks.items():
                b = [H.weight(x) for x in H.emission(c.tab[w])]
                assert b[live] == 1.0 and sum(b) == 1.0                     # the others weigh exactly 0
            ws = sorted(c.marks)
            changes = [w for a, w in zip(ws, ws[1:]) if c.marks[a] != c.marks[w]]
            assert changes or n == 1
            if fam == "alternating" and HT.blocking(n)[0] > 1:             # inside blocks and across their borders
                C = HT.blocking(n)[0]
                assert any(w % C for w in changes)
                # (7 w // 3 takes the same value mod 3 at 3 k - 1 and 3 k: at C = 3 the borders are the windows without a change)
                assert any(w % C == 0 for w in changes) == (C != 3)
    # large block and walk exponents: log2 Z under the default penalties
    assert E.log2_posteriors_host(HT.case("alternating", 255).tab, *HT.PENS[1])[2] < -2000
    assert E.log2_posteriors_host(HT.case("alternating", 1279).tab, *HT.PENS[1])[2] < -11000


@pytest.mark.parametrize("n", HT.SIZES)
def test_edge1000_lies_on_both_sides_of_the_cut(n):
    ks = set()
    for v in range(5):
        c = HT.case("edge1000", n, v)
        for w, (best, o1, o2) in c.marks.items():
            e = H.emission(c.tab[w])
            assert e[best] == 0 and e[(best + 1) % 3] == round(Fraction(o1) * 65536) and e[(best + 2) % 3] == round(Fraction(o2) * 65536)
            ks |= {x >> 16 for x in e}
    assert ks == {0, -1000, -1001, -1022, -1023, -1074, -1075}       # -1000: the last weight that is kept, -1001: the first that is 0
    assert H.weight(-1000 * 65536) == 2.0 ** -1000 and H.weight(-1000 * 65536 - 1) == 0.0


@pytest.mark.parametrize("n", HT.SIZES)
def test_clamp_reaches_the_clamp_and_the_halves(n):
    es, halves = set(), set()
    for v in range(5):
        c = HT.case("clamp", n, v)
        for w, (best, o1, o2) in c.marks.items():
            e = H.emission(c.tab[w])
            for col, o in (((best + 1) % 3, o1), ((best + 2) % 3, o2)):
                d = float(c.tab[w, col]) - float(c.tab[w, best])
                assert d == o                                                 # the subtraction gives the offset back
                prod = Fraction(max(d, -16777216.0)) * 65536
                assert e[col] == round(prod)
                es.add(e[col])
                if prod.denominator == 2:
                    halves.add((math.floor(prod) % 2, e[col]))
    assert es == {-(1 << 40), 0, -2}
    # -0.5 -> 0, -1.5 -> -2, -2.5 -> -2 and -2^40 + 0.5 -> -2^40: ties to even from both parities, at both ends of the range
    assert halves == {(1, 0), (0, -2), (1, -2), (0, -(1 << 40))}


@pytest.mark.parametrize("n", HT.SIZES)
def test_ties_are_exact(n):
    for v in range(3):
        c = HT.case("ties", n, v)
        for w in range(n):
            e = H.emission(c.tab[w])
            assert e == ([0, 0, -2 * 65536] if w in c.marks else [0, 0, 0])
        path, score, _ = E.log2_states_host(c.tab, *HT.PENS[0])
        assert (score[:, 0] == score[:, 1]).all() and (path == 0).all()      # equal maxima at every window: the lowest state


@pytest.mark.parametrize("n", HT.SIZES[1:])
def test_the_dead_families_have_a_zero_where_they_say(n):
    C = HT.blocking(n)[0]
    firsts = set()
    for v in range(2):
        c = HT.case("dead-shift", n, v)
        (p, s0), (p1, s1) = sorted(c.marks.items())
        firsts.add(p)
        assert p1 == p + 1 and (s0, s1) == (0, 1) and int(c.shift[p1]) == -(1 << 30) and not c.shift[np.arange(n) != p1].any()
        assert [H.weight(x) for x in H.emission(c.tab[p])] == [1.0, 0.0, 0.0]
        assert [H.weight(x) for x in H.emission(c.tab[p1])] == [0.0, 1.0, 0.0]
        Pw = S.window_penalties(c.pen, c.shift, (), p1)
        assert all(x >> 16 < -1000 for x in Pw) and [H.weight(x) for x in Pw] == [0.0, 0.0, 0.0]    # exactly 0, all three
        c = HT.case("dead-underflow", n, v)
        a = H.weight(H.penalty(1e-300), is_emission=False)
        assert a > 0.0 and a * a == 0.0 and H.penalty(1e-300) >> 16 == -997                        # a is kept, a * a underflows
        ws = sorted(c.marks)
        assert ws == list(range(ws[0], ws[-1] + 1)) and all(c.marks[x] != c.marks[y] for x, y in zip(ws, ws[1:]))
        for w in ws:
            b = [H.weight(x) for x in H.emission(c.tab[w])]
            assert b[c.marks[w]] == 1.0 and sum(b) == 1.0
        if C >= 2:                                   # two whole blocks of the stretch in a row, and the window before them
            whole = [b for b in range(HT.blocking(n)[1]) if b * C - 1 >= ws[0] and min((b + 1) * C, n) - 1 <= ws[-1] and b > 0]
            assert any(b + 1 in whole for b in whole)
    if C >= 2:
        assert len(firsts) == 2 and any(p % C == C - 1 for p in firsts) and any(p % C != C - 1 for p in firsts)


# ---- 2., 3. the finite families ---------------------------------------------------------------------------------------------

def twin_equals_the_restatements(c, pen, starts, shift, K=2):
    """Every product of the four twins against Python.  Returns (post, expect, log2_z) of the twin."""
    tab, n, k = c.tab, c.n, kw(starts, shift)
    what = f"{c.family}, {n} windows, penalties {pen}, starts {list(starts)}, shifts {shift is not None}"
    path, score, count = E.log2_states_host(tab, *pen, **k)
    wpath, wscore, wcount = S.restated(tab.tolist(), pen, shift, starts)
    assert path.tolist() == wpath and score.tolist() == wscore and count.tolist() == wcount, what + ": the path"
    post, expect, log2_z = E.log2_posteriors_host(tab, *pen, **k)
    wpost, wexpect, wz = restated_posteriors(tab, pen, shift, starts)
    assert bits(post) == bits(wpost), what + ": gamma"
    assert bits(expect) == bits(wexpect) and bits(log2_z) == bits(wz), what + ": expect, log2_z"
    p2, e2, z2 = E.log2_posteriors_host(tab, *pen, want_post=False, **k)
    assert p2 is None and bits(e2) == bits(expect) and bits(z2) == bits(log2_z)
    for with_post in (False, True):
        seg, n_seg, _ = E.log2_segments_host(tab, *pen, with_post=with_post, **k)
        assert n_seg == len(seg) and as_tuples(seg) == restated_records(tab, wpath, wpost if with_post else None, starts), \
            what + f": the records (posteriors {with_post})"
    m = R.Model(tab, pen, None if shift is None else shift.tolist(), starts)
    paths, out = E.log2_samples_host(tab, *pen, K, 77, 5, **k)
    for d in range(K):
        want = R.draw(m, 77, 5, d)
        assert paths[d].tolist() == want and out[d].tolist() == R.record(want, starts), what + f": draw {d}"
    return post, expect, log2_z


@pytest.mark.parametrize("family", HT.FINITE)
@pytest.mark.parametrize("n", HT.SIZES)
def test_finite_families_no_nan_and_the_restatements(n, family):
    for v in variants(family):
        c = HT.case(family, n, v)
        for pen, starts, shift in forms(c):
            if v < 2:
                post, expect, log2_z = twin_equals_the_restatements(c, pen, starts, shift)
            else:
                post, expect, log2_z = E.log2_posteriors_host(c.tab, *pen, **kw(starts, shift))
            assert np.isfinite(post).all() and np.isfinite(expect).all() and math.isfinite(log2_z)
            assert (np.abs(post.sum(axis=1) - 1.0) <= 4 * U).all()
            assert (post >= 0.0).all()


@pytest.mark.parametrize("family", HT.FINITE)
@pytest.mark.parametrize("n", TRUTH_SIZES)
def test_finite_families_within_the_bar_of_the_exact_truth(n, family):
    assert H.Rn(max(TRUTH_SIZES)) * U <= 1e-10
    c = HT.case(family, n, 1)
    for pen, starts, shift in forms(c)[0::3]:        # each penalty set plain, and with chains and shifts
        post, expect, log2_z = E.log2_posteriors_host(c.tab, *pen, **kw(starts, shift))
        t = S.Truth(c.tab, *pen, shift, starts)
        assert not t.dead
        H.check(c.tab, pen, post.tolist(), expect.tolist(), log2_z, t)


# ---- 4., 5. the dead families -----------------------------------------------------------------------------------------------

def dead_rows(c):
    """The windows whose gamma the rule sets to 0.  All of them, except for dead-underflow at C = 1: no block matrix multiplies two
    switch weights there, the individual has a Z, and what underflows is single entries of beta in front of the stretch."""
    return None if c.family == "dead-shift" or HT.UNDERFLOW_DEAD(c.n) else "some"


@pytest.mark.parametrize("family", HT.DEAD)
@pytest.mark.parametrize("n", HT.SIZES[1:])
def test_dead_families(n, family):
    for v in variants(family):
        c = HT.case(family, n, v)
        for pen, starts, shift in forms(c):
            post, expect, log2_z = twin_equals_the_restatements(c, pen, starts, shift, K=3)
            assert not np.isnan(post).any() and not np.isnan(expect).any() and not math.isnan(log2_z)
            sums = post.sum(axis=1)
            assert ((sums == 0.0) | (np.abs(sums - 1.0) <= 4 * U)).all()
            seg, _, _ = E.log2_segments_host(c.tab, *pen, with_post=True, **kw(starts, shift))
            if dead_rows(c) is None:
                assert not post.any() and not expect.any() and log2_z == -math.inf
                assert not seg["post_q"].any() and bits(seg["post_min"]) == bits(np.zeros(len(seg)))
            else:
                assert (sums == 0.0).any() == (n >= 3) and math.isfinite(log2_z)      # (two windows: one product, no underflow)
                dead = [not post[r["first"]:r["first"] + r["n_win"]].any() for r in seg]
                assert all(r["post_q"] == 0 and r["post_min"] == 0.0 for r, d in zip(seg, dead) if d)
            # the negative control: without the rule these rows are NaN, and nothing else moves
            npost, nexpect, nz = restated_posteriors(c.tab, pen, shift, starts, rule=False)
            npost = np.array(npost)
            hit = bool((sums == 0.0).any())
            assert (np.isnan(npost).all(axis=1) == (sums == 0.0)).all() and bool(np.isnan(nexpect).all()) == hit
            assert bits(npost[sums != 0.0]) == bits(post[sums != 0.0]) and (bits(npost) != bits(post)) == hit
            assert bits(nz) == bits(log2_z)
        if family == "dead-shift":
            # the exact truth has Z == 0 too; its check asks for exactly the rule's answers and takes nothing else
            post, expect, log2_z = E.log2_posteriors_host(c.tab, *c.pen, shift=c.shift)
            t = S.Truth(c.tab, *c.pen, c.shift)
            assert t.dead and t.log2_z() == -math.inf and t.as_fraction(0, 0) == 0
            H.check(c.tab, c.pen, post.tolist(), expect.tolist(), log2_z, t)
            nan = np.full_like(post, np.nan)
            for bad in ((nan.tolist(), expect.tolist(), log2_z), (post.tolist(), [0.0, math.nan, 0.0], log2_z),
                        (post.tolist(), expect.tolist(), math.nan), (post.tolist(), expect.tolist(), -1e308)):
                with pytest.raises(AssertionError, match="dead chain"):
                    H.check(c.tab, c.pen, *bad, t)
            # without its shift the same table has paths
            live = E.log2_posteriors_host(c.tab, *c.pen)
            assert np.isfinite(live[0]).all() and (np.abs(live[0].sum(axis=1) - 1.0) <= 4 * U).all() and math.isfinite(live[2])
        else:
            # the exact truth of an underflow has a Z: this kind is held to the definition's order alone
            assert n > 257 or S.Truth(c.tab, *c.pen, None).Z > 0


def test_the_rule_never_fires_on_a_finite_family():
    for family in HT.FINITE:
        c = HT.case(family, 257, 0)
        for pen, starts, shift in forms(c):
            a, b = restated_posteriors(c.tab, pen, shift, starts), restated_posteriors(c.tab, pen, shift, starts, rule=False)
            assert bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1]) and a[2] == b[2]


def test_the_sampler_on_a_dead_chain():
    """D = 0 gives state 2 from the window at which alpha dies to the end, and at the window before it, whose candidates are
    alpha times the zero switch weights; the usual rule in front of those; the distribution of a dead table does not exist."""
    c = HT.case("dead-shift", 513, 0)
    p, p1 = sorted(c.marks)
    m = R.Model(c.tab, c.pen, c.shift.tolist())
    assert all(a == [0.0, 0.0, 0.0] for a in m.alpha[p1:]) and all(max(a) >= 1.0 for a in m.alpha[:p1])
    assert m.a[p1] == (0.0, 0.0, 0.0) and m.alpha[p][1:] == [0.0, 0.0]
    paths, out = E.log2_samples_host(c.tab, *c.pen, 4, 1, 2, shift=c.shift)
    assert (paths[:, p:] == 2).all() and len({q[:p].tobytes() for q in paths}) > 1
    assert all(m.alpha[w][q[w]] > 0.0 for q in paths for w in range(p))
    small = HT.case("dead-shift", 3, 0)
    assert R.path_distribution(R.Model(small.tab, small.pen, small.shift.tolist())) == {}
    assert len(R.path_distribution(R.Model(small.tab, small.pen))) == 27


# ---- the host program reaches a dead chain from real inputs (no device: the twin's route) --------------------------------------

def test_the_host_program_reaches_a_dead_chain(tmp_path):
    exe = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    args = HT.write_dead_chain_input(str(tmp_path))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", IBDGEM_KEEP_TEARDOWN="1")
    out = tmp_path / "out"
    out.mkdir()
    res = subprocess.run([exe] + args + ["--summary-only", "-O", str(out)], cwd=tmp_path, capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    files = {fn: (out / fn).read_bytes() for fn in os.listdir(out)}
    HT.read_dead_chain_run(files)
    rows = [l.split("\t") for l in files["pu.ind0.logposteriors.txt"].decode().splitlines()[1:]]
    assert rows == [["1", "0.000000", "0.000000", "0.000000", "0"], ["2", "0.000000", "0.000000", "0.000000", "0"]]
    recs = [l.split("\t") for l in files["pu.ind0.logsegments.txt"].decode().splitlines()[1:]]
    assert [r[1] for r in recs] == ["0", "2"] and all(r[-2:] == ["0.000000", "0.000000"] for r in recs)
    # the table behind it: in window 1 IBD0 alone is alive, in window 2 it is more than 1000 bits below IBD2
    sc = [l.split("\t") for l in files["pu.ind0.loghiddengem.txt"].decode().splitlines()[1:3]]
    assert float(sc[0][2]) < -1000 and float(sc[0][3]) < -1000 and float(recs[1][9]) < -1000
