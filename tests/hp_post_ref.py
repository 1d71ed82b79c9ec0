"""Truth and bar for the IBD-state posteriors (ibdgem_amd/csrc/ibdg_states.h).

Truth.  The weights of the definition are restated here as Python floats (the split x = 65536 k + 256 j + i, the two tables
from libm's exp2, ldexp), then forward-backward runs over them with no rounding at all.  Every weight is a dyadic rational, so
alpha, beta and Z are held as Python integers over a common power of two -- fractions.Fraction with the gcd left out, which
at 1279 windows (numerators of 2 x 10^5 bits) is what keeps a case under a second.  At a window all of alpha_w[s] beta_w[s]
and Z share one power of two: gamma_w[s] = P[w][s] / Z as a quotient of two integers, and every comparison below is an
integer comparison.  as_fraction() gives fractions.Fraction where a caller wants one.
Past EXACT_WINDOWS = 601 windows the 3 n products alpha_w[s] beta_w[s] of 10^5-bit factors are what a truth costs (9 s at 1279
windows), so there each is enclosed instead: both factors cut to their leading KEEP = 4096 bits give integers lo <= P <= hi,
hi / lo - 1 < 2^-4094, and an output passes only if it is within the bar of lo and of hi -- |got Z - P| is convex in P and the
bar is linear in it, so it is then within the bar of every value between them, the exact P among them.  Nothing is rounded;
the forward and backward vectors and Z are exact at every size, and the negative controls use exact products.

Bar.  |got - truth| <= R n_win u truth + 2^-1000 for gamma, u = 2^-53.  R counts the roundings on the way to one gamma per
window step of the sequence written in ibdg_states.h, the way hp_log_ref.log_B counts: all terms are non-negative, so sums
do not cancel and the relative error of a sum is at most that of its worst term plus one per addition.
  weights                 0: the truth uses the same floats
  M_w[q][s] = a b         1
  a vector or matrix step v M_w: the product 1, the two additions 2, with M_w's: 4 per window; rescales are exact
  a block matrix B_b      <= 4 C_b (C_b windows)
  the walks               F_{k+1} = F_k B_k: B_k's count + 3; likewise G
  alpha_w, w in block b   <= 4 (w + 1) + 3 b;  beta_w <= 4 (n - 1 - w) + 3 (nbk - 1 - b);  together <= 4 n + 3 (nbk - 1) <= 7 n - 3
                          (a block owns at least one window: nbk <= n)
  p_s = alpha beta        + 1;  D = (p_0 + p_1) + p_2: + 2 more;  gamma = p_s / D: the counts of p_s and D and 1
                          = 2 (7 n - 3 + 1) + 2 + 1 = 14 n - 1
so R = 14.  (1 + u)^k - 1 <= k u (1 + k u) and k u <= 1e-10 at every shape tested (asserted by the tests): the slack of the
count (the -1, and 3 (nbk - 1) < 3 n wherever C > 1) covers it.  An entry that falls 2^-1022 below the largest of its vector
is rounded as a subnormal, an absolute error below 2^-1022 of a quantity that is at most 6: the 2^-1000.
expect[s]: the gammas' bars summed, plus the C - 1 additions of a block and the 8 of the tree on the sum: (R n + C + 8) u truth
+ n 2^-1000.  log2_z: Z's count is below gamma's, an error e of Z moves log2 Z by e / ln 2 < 2 e; the library's log2 and the
addition of the exponent are an ulp of the result each, and the truth's own float evaluation two more: 2 R n u + 4 u |truth| + 4 u.

The dead-chain rule (ibdg_states.h).  Where a weight is exactly 0 -- a shifted switch weight below 2^-1000
(hp_steps_ref.Truth; the constant penalties' weights are never 0) -- every path can have weight 0: Z == 0 here too, exactly.
Then there is no quotient and the definition's answer is the truth: gamma_w = (0, 0, 0) at every window, expect = (0, 0, 0),
log2_z = -inf, and check() asks for exactly these, no bar.  (The definition's other way to D = 0, a product of two tiny
weights that underflows, is a rounding: the exact Z of such a table is not 0, and this truth has nothing to say about it.)
"""
import ctypes
import ctypes.util
import math
from fractions import Fraction

R = 14
EXACT_WINDOWS = 601
KEEP = 4096
U_BITS = 53
ABS_BITS = 1000
THREADS = 256

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.exp2.restype = ctypes.c_double
_libm.exp2.argtypes = [ctypes.c_double]
T1 = [_libm.exp2(j / 256.0) for j in range(256)]
T2 = [_libm.exp2(i / 65536.0) for i in range(256)]


# ---- the definition's integers and weights, restated ---------------------------------------------------------------------

def emission(l):
    l = [float(x) for x in l]
    if any(math.isnan(x) for x in l) or not math.isfinite(max(l)):
        return [0, 0, 0]
    m = max(l)
    return [round(max(x - m, -16777216.0) * 65536.0) for x in l]          # round() on a float: ties to even


def penalty(p):
    assert 0.0 < p <= 1.0
    return max(round(math.log2(p) * 65536.0), -(1 << 40))


def weight(x, is_emission=True):
    assert x <= 0
    k, j, i = x >> 16, x >> 8 & 255, x & 255
    assert 65536 * k + 256 * j + i == x
    if is_emission and k < -1000:
        return 0.0
    return math.ldexp(T1[j] * T2[i], k)


def blocking(n_win):
    """C, nbk and the blocks' [w0, w1) of ibdg_states.h."""
    C = (n_win + THREADS - 1) // THREADS
    nbk = (n_win + C - 1) // C
    return C, nbk, [(b * C, min((b + 1) * C, n_win)) for b in range(nbk)]


def _ints(ws):
    """Floats (dyadic, >= 0) as integers over one power of two: ([m_i], e) with w_i = m_i 2^e."""
    parts = [w.as_integer_ratio() for w in ws]
    sh = max(d.bit_length() - 1 for _, d in parts)
    return [n << (sh - (d.bit_length() - 1)) for n, d in parts], -sh


# ---- exact forward-backward ----------------------------------------------------------------------------------------------

class _Products:
    """P[w][s] = alpha_w[s] beta_w[s], formed when first asked for (the products are most of a long truth's cost)."""

    def __init__(self, alpha, beta):
        self.alpha, self.beta, self.have = alpha, beta, {}

    def __getitem__(self, w):
        if w not in self.have:
            self.have[w] = [self.alpha[w][s] * self.beta[w][s] for s in range(3)]
        return self.have[w]

    def enclosure(self, w, s):
        """(lo, hi), lo <= P[w][s] <= hi, from the leading KEEP bits of the two factors."""
        a, b = self.alpha[w][s], self.beta[w][s]
        sa, sb = max(a.bit_length() - KEEP, 0), max(b.bit_length() - KEEP, 0)
        ta, tb = a >> sa, b >> sb
        return ta * tb << (sa + sb), (ta + (sa > 0)) * (tb + (sb > 0)) << (sa + sb)


class Truth:
    """alpha[w], beta[w]: integer triples (their powers of two add up to Z's at every window); P[w][s] = alpha beta; Z.
    gamma_w[s] = P[w][s] / Z exactly; S[s] = sum_w P[w][s]: expect[s] = S[s] / Z; log2_z as a float."""

    def __init__(self, tab, p01, p02, p12):
        tab = [[float(x) for x in row] for row in tab]
        self.n = n = len(tab)
        self.pen = (p01, p02, p12)
        a01, a02, a12 = (weight(penalty(p), is_emission=False) for p in (p01, p02, p12))
        assert min(a01, a02, a12) > 0.0
        A, self.ea = _ints([1.0, a01, a02, a01, 1.0, a12, a02, a12, 1.0])
        self.A = [A[0:3], A[3:6], A[6:9]]
        self.b = [[weight(e) for e in emission(row)] for row in tab]
        assert all(max(b) == 1.0 for b in self.b)                          # the best state weighs exactly 1
        self.B, self.eb = zip(*(_ints(b) for b in self.b)) if n else ((), ())
        self.alpha = self._forward()
        self.beta = self.backward_from(n - 1, [1, 1, 1]) if n else {}
        self.Z = sum(self.alpha[-1]) if n else 1
        self.ez = self.eb[0] + sum(self.ea + e for e in self.eb[1:]) if n else 0
        self.P = _Products(self.alpha, self.beta)
        self._S = None

    def bounds(self, w, s):
        """(lo, hi) around P[w][s]: the product itself twice up to EXACT_WINDOWS windows, its enclosure beyond."""
        if self.n <= EXACT_WINDOWS:
            return self.P[w][s], self.P[w][s]
        return self.P.enclosure(w, s)

    @property
    def S(self):
        """(lo, hi) around sum_w P[w][s], s = 0, 1, 2."""
        if self._S is None:
            b = [[self.bounds(w, s) for w in range(self.n)] for s in range(3)]
            self._S = [(sum(x[0] for x in col), sum(x[1] for x in col)) for col in b]
        return self._S

    def _forward(self):
        out = []
        for w in range(self.n):
            if w == 0:
                v = list(self.B[0])
            else:
                v = [sum(v[q] * self.A[q][s] for q in range(3)) * self.B[w][s] for s in range(3)]
            out.append(v)
        return out

    def backward_from(self, w_last, vec):
        """{w: beta_w} for w <= w_last with beta at w_last set to `vec` (the truth: n - 1 and (1, 1, 1))."""
        out, v = {w_last: list(vec)}, list(vec)
        for w in range(w_last, 0, -1):
            t = [self.B[w][s] * v[s] for s in range(3)]
            v = [sum(self.A[q][s] * t[s] for s in range(3)) for q in range(3)]
            out[w - 1] = v
        return out

    @property
    def dead(self):
        """No path has weight (the dead-chain rule): gamma is (0, 0, 0) everywhere, expect (0, 0, 0), log2_z -inf."""
        return self.n > 0 and self.Z == 0

    def as_fraction(self, w, s):
        return Fraction(0) if self.dead else Fraction(self.P[w][s], self.Z)

    def expect(self, s):
        """The lower end of expect[s]'s enclosure (expect[s] itself up to EXACT_WINDOWS windows)."""
        return Fraction(0) if self.dead else Fraction(self.S[s][0], self.Z)

    def log2_z(self):
        if self.dead:
            return -math.inf
        bl = self.Z.bit_length()
        top = self.Z >> (bl - 64) if bl > 64 else self.Z << (64 - bl)
        return math.log2(top / 2.0 ** 64) + (bl + self.ez)


def Rn(n_win):
    return R * n_win


def _float_ratio(got):
    gn, gd = float(got).as_integer_ratio()
    return gn, gd


def _ratio(err, bar):
    """err / bar of two (huge) integers as a float, for reports: both cut to the bar's leading 128 bits first."""
    sh = max(bar.bit_length() - 128, 0)
    return (err >> sh) / (bar >> sh)


def gamma_err_and_bar(got, P, Z, n_win):
    """|got - P / Z| and R n u P / Z + 2^-1000, both times Z gd 2^53 2^1000 (gd: got's denominator): two integers."""
    gn, gd = _float_ratio(got)
    return abs(gn * Z - P * gd) << (U_BITS + ABS_BITS), (Rn(n_win) * P * gd << ABS_BITS) + (Z * gd << U_BITS)


def gamma_within_bar(got, P, Z, n_win):
    err, bar = gamma_err_and_bar(got, P, Z, n_win)
    return err <= bar


def gamma_err_over_bar(got, P, Z, n_win):
    return _ratio(*gamma_err_and_bar(got, P, Z, n_win))


def control_err_and_bar(Pc, Dc, P, Z, n_win):
    """|Pc / Dc - P / Z| and the bar of P / Z, both times Z Dc 2^53 2^1000: how far a wrong model's gamma lies from the truth."""
    return abs(Pc * Z - P * Dc) << (U_BITS + ABS_BITS), (Rn(n_win) * P * Dc << ABS_BITS) + (Z * Dc << U_BITS)


def expect_err_and_bar(got, S, Z, n_win):
    C = blocking(n_win)[0]
    gn, gd = _float_ratio(got)
    return abs(gn * Z - S * gd) << (U_BITS + ABS_BITS), ((Rn(n_win) + C + 8) * S * gd << ABS_BITS) + (n_win * Z * gd << U_BITS)


def log2_z_err_over_bar(got, truth, n_win):
    u = 2.0 ** -U_BITS
    return abs(got - truth) / (2 * Rn(n_win) * u + 4 * u * abs(truth) + 4 * u)


def check(tab, pen, post, expect, log2_z, truth=None):
    """Every output against the truth within its bar.  Returns (truth, the largest error / bar seen)."""
    t = truth or Truth(tab, *pen)
    n = t.n
    worst = 0.0
    if t.dead:                                       # the dead-chain rule: exact answers, no bar
        for w in range(n):
            assert [float(x) for x in post[w]] == [0.0, 0.0, 0.0], f"gamma[{w}] = {list(post[w])!r} of a dead chain (Z == 0)"
        assert [float(x) for x in expect] == [0.0, 0.0, 0.0], f"expect = {list(expect)!r} of a dead chain"
        assert log2_z == -math.inf, f"log2_z = {log2_z!r} of a dead chain"
        return t, 0.0
    for w in range(n):
        for s in range(3):
            for P in set(t.bounds(w, s)):
                err, bar = gamma_err_and_bar(post[w][s], P, t.Z, n)
                worst = max(worst, _ratio(err, bar))
                assert err <= bar, (f"gamma[{w}][{s}] = {post[w][s]!r}: {_ratio(err, bar):.3g} bars from {P / t.Z!r} "
                                    f"(n_win {n}, penalties {pen})")
    for s in range(3):
        for S in set(t.S[s]):
            err, bar = expect_err_and_bar(expect[s], S, t.Z, n)
            worst = max(worst, _ratio(err, bar))
            assert err <= bar, f"expect[{s}] = {expect[s]!r}: {_ratio(err, bar):.3g} bars from {S / t.Z!r}"
    r = log2_z_err_over_bar(log2_z, t.log2_z(), n)
    assert r <= 1.0, f"log2_z = {log2_z!r}: {r:.3g} bars from {t.log2_z()!r}"
    return t, max(worst, r)


# ---- negative controls: wrong models a blocked forward-backward can turn into, in the same exact arithmetic ----------------
# A control is (f, windows): f(w) = (P'[0..2], D') with the wrong gamma_w[s] = P'[s] / D', and the windows to look at, those
# where it is most wrong first.

def control_swapped(t, tab):
    """p01 and p12 exchanged."""
    p01, p02, p12 = t.pen
    c = Truth(tab, p12, p02, p01)
    return (lambda w: (c.P[w], c.Z)), range(t.n)


def control_last_block_left_out(t):
    """The backward walk starts one block early: G of the last block but one is (1, 1, 1), as if the last block's matrix had
    not been applied.  The last block's own windows are right, the ones just before it the most wrong."""
    w0 = blocking(t.n)[2][-1][0]
    assert w0 > 0
    beta = t.backward_from(w0 - 1, [1, 1, 1])

    def f(w):
        P = [t.alpha[w][s] * beta[w][s] for s in range(3)]
        return P, sum(P)
    return f, range(w0 - 1, -1, -1)


def control_backward_late(t):
    """gamma_w from alpha_w and beta_{w+1}."""
    def f(w):
        P = [t.alpha[w][s] * t.beta[w + 1][s] for s in range(3)]
        return P, sum(P)
    return f, range(t.n - 1)


def control_exceeds(t, control, factor=1000):
    """The first (window, state) at which a control lies at least `factor` bars from the truth, or None."""
    f, windows = control
    for w in windows:
        Pc, Dc = f(w)
        for s in range(3):
            err, bar = control_err_and_bar(Pc[s], Dc, t.P[w][s], t.Z, t.n)
            if err >= factor * bar:
                return w, s
    return None
