"""CPU tier of the long blocks (hard_tables.LONG_SIZES): no device.  tests/test_gpu_log_long_blocks.py holds the kernels of the
log-domain state family to the host twin at many windows a thread; here the twin is held to references that share no code with
it at the same sizes, so that "device == twin" means something there.

  1. The generators are what they claim: the (C, owners, last) table of LONG_SIZES by the formula of blocking(), the trip counts
     of the lattice, the coverage of dense_chain_starts, the windows edge_shifts touches, the stretches of the plateaus family.
  2. Up to 40000 windows, every family of LONG_FAMILIES, plain, with dense chain starts, with edge shifts and with both: the
     twin's path, scores and counts against the integer recurrence of hp_steps_ref, its posteriors byte for byte against the
     definition's fixed order in Python floats (test_hard_tables.restated_posteriors), its records against sums formed from
     those, its draws byte for byte against hp_sample_ref.  A table that edge_shifts kills (hard_tables.chain_alive: a step whose
     switch weights are all 0 between windows that share no live state) carries the rule's mark; every other one of a finite
     family is finite.
  3. At 8193 and 40000 windows an exact truth is unaffordable (integers of millions of bits): a plain forward-backward in
     numpy.longdouble over the same weights, rescaled by exact powers of two, and hp_post_ref's bar widened by the reference's
     own rounding.
  4. At 2^21 windows nothing walks the table in Python: with chain starts at every multiple of 40000 the twin's path is the
     concatenation of its paths over the slices alone (exact in integers), each slice a size held to the integer
     recurrence by 2.; no NaN, rows of gamma that sum to 1 or are 0, the dead families' mark.
  5. Negative controls: a restatement for which the last window of every block says nothing, and one whose chain starts lie a
     window late, differ from the twin in what the comparisons of 2. compare, at every size."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import hard_tables as HT
import hp_post_ref as H
import hp_sample_ref as R
import hp_steps_ref as S
from ibdgem_amd import engine as E
from test_hard_tables import as_tuples, bits, kw, library, restated_posteriors, restated_records  # noqa: F401 (library: the fixture)

U = 2.0 ** -53
UP_TO_40000 = [n for n in HT.LONG_SIZES if n <= 40000]
LATTICE = [256 * C - 5 for C in range(6, 17)]
TOP = 1 << 21
SLICE = 40000
LD_SIZES = [8193, 40000]


@pytest.fixture(autouse=True)
def pure_functions_once(monkeypatch):
    """hp_post_ref's emission, penalty and weight are pure functions of a row, a probability and an integer, and the restatements
    ask for each of them several times per window and form: the same answers, kept for the length of a test."""
    emission = H.emission
    kept = functools.lru_cache(maxsize=None)(lambda row: tuple(emission(row)))
    monkeypatch.setattr(H, "emission", lambda l: list(kept(tuple(float(x) for x in l))))
    monkeypatch.setattr(H, "penalty", functools.lru_cache(maxsize=None)(H.penalty))
    monkeypatch.setattr(H, "weight", functools.lru_cache(maxsize=None)(H.weight))


# ---- 1. the generators are what they claim -------------------------------------------------------------------------------------

def test_long_sizes_and_their_shapes():
    assert HT.LONG_SIZES == [1531, 1787, 2043, 2299, 2555, 2811, 3067, 3323, 3579, 3835, 4091, 1793, 2048, 8192, 8193, 40000, TOP]
    assert sorted(HT.LONG_SHAPES) == sorted(HT.LONG_SIZES)
    for n in HT.LONG_SIZES:
        C, nbk = HT.blocking(n)
        assert (C, nbk, n - (nbk - 1) * C) == HT.LONG_SHAPES[n], n
        assert (C, nbk) == tuple(H.blocking(n)[:2])
        assert nbk <= 256 and 1 <= n - (nbk - 1) * C <= C
    assert [HT.LONG_SHAPES[n] for n in (1793, 2048, 8192, 8193, 40000, TOP)] == \
        [(8, 225, 1), (8, 256, 8), (32, 256, 32), (33, 249, 9), (157, 255, 122), (8192, 256, 8192)]
    # the lattice: two trip counts a launch, C and C - 5; over it every remainder mod 4 and mod 8, with the unrolled body run
    # 0 times, once, and twice or more
    trips = sorted({t for n in LATTICE for t in (HT.LONG_SHAPES[n][0], HT.LONG_SHAPES[n][2])})
    assert trips == list(range(1, 17))
    for unroll, most in ((4, 2), (8, 1)):           # (a remainder r != 0 behind two 8-way bodies would take 16 + r trips)
        for r in range(unroll):
            runs = {min(t // unroll, 2) for t in trips if t % unroll == r}
            assert runs == (set(range(most + 1)) if r else {1, 2}), (unroll, r)
    assert {b * HT.blocking(8192)[0] % 32 for b in range(256)} == {0}                        # 8192: a block is a mask word
    assert {b * 33 % 32 for b in range(249)} == set(range(32))                               # 8193: every offset into a word


@pytest.mark.parametrize("n", HT.LONG_SIZES)
def test_dense_chain_starts_cover_what_they_claim(n):
    C, nbk = HT.blocking(n)
    st = HT.dense_chain_starts(n)
    assert st == sorted(set(st)) and st[0] >= 1 and st[-1] == n - 1
    have = set(st)
    assert all(w in have for w in range(5, n, 37))
    assert all(b * C in have for b in range(3, nbk, 3))
    assert all(min(n, (b + 1) * C) - 1 in have for b in range(0, nbk, 5))
    for b in HT.DENSE_WORD_BLOCKS(nbk):
        assert all(w in have for w in range(b * C, min(n, (b + 1) * C)) if w % 32 == 0 and w >= 1)
    if C >= 8:              # a start at every position of the 8-way unrolled backward walks, counted from the block's end
        assert {(HT.block_end(n, w) - 1 - w) % 8 for w in st} == set(range(8))
    if C >= 16:             # (asked for from C = 33; it holds from the largest lattice size on)
        per = np.bincount(np.array(st) // C, minlength=nbk)
        assert {w % 32 for w in st} == set(range(32))
        assert per.max() >= 2
        # a block without a start: only below C = 37, where the starts at w % 37 == 5 can miss a block.  From there on every
        # thread has a start, and what is empty is whole mask words inside a thread's block
        words = np.bincount(np.array(st) // 32, minlength=(n + 31) // 32)
        assert per.min() == 0 if C < 37 else per.min() >= 1 and words.min() == 0 and words.max() >= 2


@pytest.mark.parametrize("n", HT.LONG_SIZES)
def test_edge_shifts_touch_the_look_ahead(n):
    C, nbk = HT.blocking(n)
    sh, plain = HT.edge_shifts(n, 9), HT.shifts(n, 9)
    assert sh.dtype == np.int32 and len(sh) == n and np.abs(sh.astype(np.int64)).max() <= HT.SHIFT_MAX
    touched, seen = [], {"first": set(), "second": set(), "last": set()}
    for b in range(0, nbk, 7):
        w0, w1 = b * C, min(n, (b + 1) * C)
        for w in sorted({w0, min(w0 + 1, w1 - 1), w1 - 1}):
            touched.append(w)
        for name, w in (("first", w0), ("second", w0 + 1), ("last", w1 - 1)):
            if w1 - w0 >= 3:
                seen[name].add(int(sh[w]))
    rest = np.setdiff1d(np.arange(n), touched)
    assert (sh[rest] == plain[rest]).all() and (np.abs(plain) <= 3 * HT.BIT).all()
    assert [int(x) for x in sh[touched[:4]]] == HT.EDGE_SHIFT_VALUES                         # in turn, from the first one on
    if nbk > 7 * 4 and C >= 3:                                                               # every value at every position
        assert all(v == set(HT.EDGE_SHIFT_VALUES) for v in seen.values()), seen


@pytest.mark.parametrize("n", HT.LONG_SIZES)
def test_plateaus_are_stretches_of_one_best_state(n):
    C = HT.blocking(n)[0]
    lengths = [max(1, x) for x in (1, C - 1, C, C + 1, 3 * C + 2, 20 * C)]
    at = set()
    for v in range(2):
        c = HT.case("plateaus", n, v)
        first = sorted(c.marks)
        assert first[0] == 0
        ends = first[1:] + [n]
        for i, (f, e) in enumerate(zip(first, ends)):
            assert e - f == lengths[(i + v) % 6] or e == n
            assert c.marks[f] == (i + v) % 3
        best = np.repeat([c.marks[f] for f in first], np.diff(first + [n]))
        rows = np.arange(n)
        assert (c.tab.argmax(axis=1) == best).all()
        for k in (1, 2):                                                                     # best by 40 bits in the integers
            assert (np.rint((c.tab[rows, (best + k) % 3] - c.tab[rows, best]) * 65536.0) == -40 * 65536).all()
        assert H.emission(c.tab[n // 2]) == [0 if s == best[n // 2] else -40 * 65536 for s in range(3)]
        # under both penalty sets the path follows the stretches: segments that end at every position of a block, and segments
        # that cover whole blocks
        if n <= 40000:
            path = E.log2_states_host(c.tab, *HT.PENS[1])[0]
            assert (path == best).all()
            assert any(f // C + 2 <= (e - 1) // C for f, e in zip(first, ends))               # a whole block inside
        at |= {e % C for e in ends}
    # over the two variants the stretches end at every position of a block, as long as a table has C or so stretches
    assert at == set(range(C)) if C <= 32 else 0 in at and len(at) >= 32


def test_records_of_is_restated_records():
    c = HT.case("naninf", 1793, 1)
    starts = HT.dense_chain_starts(c.n)
    path = S.restated(c.tab.tolist(), HT.PENS[0], None, starts)[0]
    post = restated_posteriors(c.tab, HT.PENS[0], None, starts)[0]
    assert records_of(c.tab, path, post, starts) == (restated_records(c.tab, path, None, starts),
                                                     restated_records(c.tab, path, post, starts))
    assert all(round(Fraction(x) * 2 ** 32) == round(x * 4294967296.0) for x in (0.5 ** 33, 1.5 * 0.5 ** 32, 2.5 * 0.5 ** 32, 1.0))


def test_chain_alive_on_the_dead_shift_family():
    """hard_tables.chain_alive against the exact truth of hp_steps_ref where that is affordable: dead exactly where Z == 0."""
    for n in (3, 257):
        for v in range(2):
            c = HT.case("dead-shift", n, v)
            assert not HT.chain_alive(c.tab, c.pen, c.shift) and S.Truth(c.tab, *c.pen, c.shift).dead
            assert HT.chain_alive(c.tab, c.pen, None) and HT.chain_alive(c.tab, c.pen, c.shift, [sorted(c.marks)[1]])
        for fam in HT.LONG_FINITE:
            c = HT.case(fam, n, 0)
            sh = HT.edge_shifts(n, 9)
            sh[n // 2] = -HT.SHIFT_MAX
            assert HT.chain_alive(c.tab, c.pen, sh) == (not S.Truth(c.tab, *c.pen, sh).dead), (fam, n)


# ---- 2. the twin against the restatements, up to 40000 windows -----------------------------------------------------------------

def forms(c):
    """(penalties, starts, shift): a finite family under both penalty sets, plain, with dense chain starts, with edge shifts, with
    both; a dead family under its own penalties and shift, plain and with the dense starts that keep away from its windows."""
    n = c.n
    dense = HT.dense_chain_starts(n)
    if c.family in HT.DEAD:
        keep = [w for w in dense if c.marks.get(w) is None and c.marks.get(w - 1) is None]
        return [(c.pen, (), c.shift), (c.pen, keep, c.shift)]
    sh = HT.edge_shifts(n, 9)
    return [(pen, starts, shift) for pen in HT.PENS for starts in ((), dense) for shift in (None, sh)]


def twin_products(tab, pen, starts, shift, K=2):
    k = kw(starts, shift)
    out = {}
    out["path"], out["score"], out["count"] = (x.tolist() for x in E.log2_states_host(tab, *pen, **k))
    post, expect, log2_z = E.log2_posteriors_host(tab, *pen, **k)
    out["post"], out["expect"], out["log2_z"] = bits(post), bits(expect), bits(log2_z)
    p2, e2, z2 = E.log2_posteriors_host(tab, *pen, want_post=False, **k)
    assert p2 is None and bits(e2) == bits(expect) and bits(z2) == bits(log2_z)
    for with_post in (False, True):
        seg, n_seg, _ = E.log2_segments_host(tab, *pen, with_post=with_post, **k)
        assert n_seg == len(seg)
        out[f"records{int(with_post)}"] = as_tuples(seg)
    paths, rec = E.log2_samples_host(tab, *pen, K, 77, 5, **k)
    out["draws"], out["draw records"] = paths.tolist(), rec.tolist()
    return out, post, expect, log2_z


def restated_products(tab, pen, starts, shift, K=2):
    """The same products from Python alone: integers, floats in the definition's order, Fractions."""
    sh = None if shift is None else [int(x) for x in shift]
    out = {}
    out["path"], out["score"], out["count"] = S.restated(tab.tolist(), pen, sh, starts)
    m = R.Model(tab, pen, sh, starts)
    post, expect, log2_z = restated_posteriors(tab, pen, sh, starts, model=m)
    out["post"], out["expect"], out["log2_z"] = bits(post), bits(expect), bits(log2_z)
    out["records0"], out["records1"] = records_of(tab, out["path"], post, starts)
    out["draws"] = [R.draw(m, 77, 5, d) for d in range(K)]
    out["draw records"] = [R.record(p, starts) for p in out["draws"]]
    return out


def records_of(tab, path, post, starts):
    """test_hard_tables.restated_records without and with gammas in one walk over the segments.  round(g 2^32) is taken on the
    float: the product with a power of two is exact, and Python rounds a float to the nearest integer, ties to even."""
    tab = tab.tolist()
    starts, plain, full, f, n = set(starts), [], [], 0, len(path)
    while f < n:
        w = f + 1
        while w < n and path[w] == path[f] and w not in starts:
            w += 1
        s = path[f]
        e = [H.emission(tab[x]) for x in range(f, w)]
        head = (f, w - f, s, *(sum(r[k] for r in e) for k in range(3)))
        g = [post[x][s] for x in range(f, w)]
        plain.append(head + (0, 0.0))
        full.append(head + (sum(round(x * 4294967296.0) for x in g), min(g)))
        f = w
    return plain, full


def differences(a, b):
    return sorted(k for k in a if a[k] != b[k])


def variants_at(n, family):
    """Variants 0 and 1; at 40000 windows, where a table in its eight forms costs half a minute of Python, one of them, the two
    in turn over the families.  (Thinned there alone, and never the families.)"""
    return (HT.LONG_FAMILIES.index(family) % 2,) if n >= 40000 else (0, 1)


@pytest.mark.parametrize("family", HT.LONG_FAMILIES)
@pytest.mark.parametrize("n", UP_TO_40000)
def test_the_twin_equals_the_restatements(n, family):
    for v in variants_at(n, family):
        c = HT.case(family, n, v)
        for pen, starts, shift in forms(c):
            what = f"{family} {v}, {n} windows, penalties {pen}, {len(starts)} starts, shifts {shift is not None}"
            got, post, expect, log2_z = twin_products(c.tab, pen, starts, shift)
            assert differences(got, restated_products(c.tab, pen, starts, shift)) == [], what
            assert not np.isnan(post).any() and not np.isnan(expect).any() and not math.isnan(log2_z), what
            sums = post.sum(axis=1)
            if family in HT.DEAD:
                assert not post.any() and not expect.any() and log2_z == -math.inf, what + ": the rule's mark"
            elif HT.chain_alive(c.tab, pen, shift, starts):
                assert ((sums == 0.0) | (np.abs(sums - 1.0) <= 4 * U)).all() and (post >= 0.0).all(), what
                if shift is None or family not in HT.TINY_WEIGHTS:
                    assert (sums != 0.0).all() and math.isfinite(log2_z), what
            else:                                   # an edge shift of -2^30 between windows that share no live state
                assert shift is not None and not post.any() and not expect.any() and log2_z == -math.inf, what + ": killed"


# ---- 3. a truth at higher precision --------------------------------------------------------------------------------------------

def longdouble_gamma(m):
    """gamma [n][3] by a plain forward-backward in numpy.longdouble over the weights of the hp_sample_ref.Model m, the vector
    rescaled by an exact power of two after every step; None for a table without a path (Z == 0: the zeros are exact)."""
    LD = np.longdouble
    n = m.n
    b = np.array(m.b, dtype=LD)
    M = np.ones((n, 3, 3), dtype=LD)
    if n > 1:
        a = np.array(m.a[1:], dtype=LD)
        M[1:, 0, 1] = M[1:, 1, 0] = a[:, 0]
        M[1:, 0, 2] = M[1:, 2, 0] = a[:, 1]
        M[1:, 1, 2] = M[1:, 2, 1] = a[:, 2]
    M *= b[:, None, :]                               # M_w[q][s] = a_w[q][s] b_w[s]

    def rescaled(v):
        mx = v.max()
        return np.ldexp(v, -int(np.frexp(mx)[1])) if mx > 0 else v

    alpha, beta = np.empty((n, 3), dtype=LD), np.empty((n, 3), dtype=LD)
    v = b[0].copy()
    for w in range(n):
        if w:
            v = rescaled(v @ M[w])
        alpha[w] = v
    g = np.ones(3, dtype=LD)
    for w in range(n - 1, -1, -1):
        beta[w] = g
        if w:
            g = rescaled(M[w] @ g)
    P = alpha * beta
    D = P.sum(axis=1, keepdims=True)
    if (D == 0).any():
        assert (D == 0).all()
        return None
    return P / D


@pytest.mark.parametrize("n", LD_SIZES)
def test_finite_families_within_the_bar_of_a_longdouble_truth(n):
    """hp_post_ref's bar R n u t + 2^-1000, widened by 1 + 2^-11 for the reference's own rounding: the same count R n of roundings
    at 2^-64 instead of 2^-53.  Prints the worst error / bar (DESIGN 4.9 records it)."""
    LD = np.longdouble
    assert np.finfo(LD).eps == LD(2.0) ** -63 and np.finfo(LD).minexp < -16000            # x87 extended: 64 bits, 15 of exponent
    assert H.Rn(max(LD_SIZES)) * U <= 1e-10
    wide = LD(1) + LD(2.0) ** -11
    worst = 0.0
    for family in HT.LONG_FINITE:
        c = HT.case(family, n, 1)
        both = (HT.PENS[1], HT.dense_chain_starts(n), HT.edge_shifts(n, 9))
        for pen, starts, shift in ((HT.PENS[0], (), None), both):
            post = E.log2_posteriors_host(c.tab, *pen, **kw(starts, shift))[0]
            t = longdouble_gamma(R.Model(c.tab, pen, None if shift is None else shift.tolist(), starts))
            assert (t is not None) == HT.chain_alive(c.tab, pen, shift, starts), family
            if t is None:
                assert not post.any(), f"{family}, {n} windows: a dead chain"
                continue
            err = np.abs(post.astype(LD) - t)
            bar = (LD(H.Rn(n)) * LD(U) * t + np.ldexp(LD(1), -H.ABS_BITS)) * wide
            ratio = float((err / bar).max())
            worst = max(worst, ratio)
            assert (err <= bar).all(), f"{family}, {n} windows, penalties {pen}: {ratio:.3g} bars from the long-double truth"
    print(f"{n} windows: the twin's worst gamma error is {worst:.3g} of the bar")
    assert 0.0 < worst


def _ld_ratio(num, den):
    """num / den of two huge non-negative integers as a long double, from the leading 64 bits of each (2^-62 of the quotient)."""
    LD = np.longdouble
    if num == 0:
        return LD(0)

    def top(x):
        sh = max(x.bit_length() - 64, 0)
        y = x >> sh
        return LD(y >> 32) * LD(2.0) ** 32 + LD(y & 0xffffffff), sh
    (a, sa), (b, sb) = top(num), top(den)
    return np.ldexp(a / b, max(sa - sb, -16300))


def test_the_longdouble_truth_against_the_exact_one():
    """The reference of the test above, held to hp_steps_ref.Truth where that can be afforded: within its own rounding, R n at
    2^-64, of the exact gamma."""
    LD = np.longdouble
    n = 257
    for family in HT.LONG_FINITE:
        c = HT.case(family, n, 1)
        starts, shift = HT.dense_chain_starts(n), HT.edge_shifts(n, 9)
        if not HT.chain_alive(c.tab, HT.PENS[1], shift, starts):
            shift = HT.shifts(n, 9)
        t = S.Truth(c.tab, *HT.PENS[1], shift, starts)
        g = longdouble_gamma(R.Model(c.tab, HT.PENS[1], shift.tolist(), starts))
        assert not t.dead
        for w in range(0, n, 7):
            for s in range(3):
                x = _ld_ratio(t.P[w][s], t.Z)
                assert abs(g[w, s] - x) <= LD(H.Rn(n)) * LD(2.0) ** -64 * x + np.ldexp(LD(1), -H.ABS_BITS), (family, w, s)


# ---- 4. 2^21 windows -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", HT.LONG_FAMILIES)
def test_the_limit_in_slices(family):
    n = TOP
    c = HT.case(family, n, 0)
    pen = c.pen
    starts = list(range(SLICE, n, SLICE))
    assert len(starts) == 52 and n - starts[-1] == 17152
    keep = [w for w in starts if c.marks.get(w) is None and c.marks.get(w - 1) is None] if family in HT.DEAD else starts
    shifts = [c.shift] if family in HT.DEAD else [None, HT.edge_shifts(n, 9)]
    for shift in shifts:
        path, score, count = E.log2_states_host(c.tab, *pen, **kw(starts, shift))
        parts, cnt = [], np.zeros(3, dtype=np.uint64)
        for f, e in zip([0] + starts, starts + [n]):
            p, _, k = E.log2_states_host(c.tab[f:e], *pen, want_score=False, shift=None if shift is None else shift[f:e])
            parts.append(p)
            cnt += k
        assert np.concatenate(parts).tobytes() == path.tobytes() and cnt.tolist() == count.tolist(), family
        assert int(count.sum()) == n
    C = HT.blocking(n)[0]
    for st, shift in (((), shifts[0]), (keep, shifts[-1])):
        post, expect, log2_z = E.log2_posteriors_host(c.tab, *pen, **kw(st, shift))
        assert not np.isnan(post).any() and not np.isnan(expect).any() and not math.isnan(log2_z), family
        sums = post.sum(axis=1)
        assert ((sums == 0.0) | (np.abs(sums - 1.0) <= 4 * U)).all() and (post >= 0.0).all(), family
        if family in HT.DEAD:
            assert not post.any() and not expect.any() and log2_z == -math.inf, family + ": the rule's mark"
        elif HT.chain_alive(c.tab, pen, shift, st) and (shift is None or family not in HT.TINY_WEIGHTS):
            assert (sums != 0.0).all() and math.isfinite(log2_z) and abs(float(expect.sum()) - n) <= n * (4 + C + 8) * U, family
        elif HT.chain_alive(c.tab, pen, shift, st):
            pass                                    # (a product of two weights near 2^-1000 may underflow: 0 or 1, as asserted)
        else:
            assert not post.any() and log2_z == -math.inf, family + ": killed"


# ---- 5. negative controls ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", UP_TO_40000)
def test_wrong_restatements_are_caught(n):
    c = HT.case("plateaus" if n % 2 else "naninf", n, 0)
    pen, starts, shift = HT.PENS[0], HT.dense_chain_starts(n), HT.shifts(n, 9)
    got = twin_products(c.tab, pen, starts, shift)[0]
    assert differences(got, restated_products(c.tab, pen, starts, shift)) == []
    # the last window of every block says nothing
    C, nbk, blocks = H.blocking(n)
    wrong = c.tab.copy()
    wrong[[w1 - 1 for _, w1 in blocks]] = np.nan
    d = differences(got, restated_products(wrong, pen, starts, shift))
    assert {"score", "post", "expect", "log2_z", "records0", "records1"} <= set(d), d
    # the chain starts a window late
    late = sorted({w + 1 for w in starts if w + 1 < n})
    d = differences(got, restated_products(c.tab, pen, late, shift))
    assert {"score", "post", "log2_z", "records0", "records1"} <= set(d) and {"draws", "draw records"} & set(d), d
