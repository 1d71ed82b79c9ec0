"""The sampled paths of ibdgem_amd/csrc/ibdg_states.h, restated in plain Python on top of tests/hp_post_ref.py.

alpha.  Python floats are the definition's fp64, so the forward vectors are formed here in the definition's fixed order: the block
matrices (step 1), the forward walk (step 2) and the forward half of step 4, each with its rescale, over the blocking of 256.
The weights are hp_post_ref's (the same floats on either side); a window's switch weights are (1, 1, 1) at a chain start, the
shifted penalties' weights by the emissions' rule where there are shifts, else the penalties' own.

A draw.  sm64, the key of (seed, stream, k), one U per window, the rule of sample_pick; walked once from the back (draw) and as
6-bit maps composed per block and scanned (draw_by_maps): the two are the same path because maps compose associatively.
u_of and variant are the tests' handles: u_of(k, w) replaces U (its largest value, for the x < D fact), variant makes one of
three wrong samplers that the statistical bars must catch.

Exact.  For a table of at most 6 windows path_distribution gives P(path) of all 3^n paths as Fractions of the same weights.

The dead-chain rule (ibdg_states.h).  Where a switch weight is exactly 0, every path can have weight 0.
alpha is then (0, 0, 0) from some window on, every candidate there is 0, D = 0 and pick() answers state 2 -- the sampler's
arithmetic as it is, the same integer on either side; in front of that window the usual rule holds.  Such draws are defined
bytes, not samples: there is no distribution, and path_distribution gives {} (Z == 0).
"""
import math
from fractions import Fraction
from itertools import product

import hp_post_ref as H
import hp_steps_ref as S

MASK = (1 << 64) - 1
U_MAX = 1.0 - 2.0 ** -53
MAP_ID = 0 | 1 << 2 | 2 << 4


# ---- the numbers ---------------------------------------------------------------------------------------------------------

def sm64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ z >> 30) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ z >> 27) * 0x94D049BB133111EB) & MASK
    return z ^ z >> 31


def key(seed, stream, k):
    return sm64(sm64(sm64(seed) ^ stream) ^ k)


def uniform(ky, w):
    return float(sm64(ky ^ w) >> 11) * 2.0 ** -53


# ---- the weights ---------------------------------------------------------------------------------------------------------

def switch_weights(pen, shift, starts, w):
    """(a01, a02, a12) of the step into window w >= 1."""
    if w in starts:
        return (1.0, 1.0, 1.0)
    if shift is None:
        return tuple(H.weight(H.penalty(p), is_emission=False) for p in pen)
    return tuple(H.weight(P) for P in S.window_penalties(pen, shift, starts, w))


def emission_weights(row):
    return [H.weight(e) for e in H.emission(row)]


# ---- alpha, in the definition's order --------------------------------------------------------------------------------------

def _rescale(v, e):
    mx = max(v)
    E = (math.frexp(mx)[1] - 1) if mx >= 2.0 ** -1022 else -1023       # the exponent field less 1023; 0 and subnormals: -1023
    if E == 0 or E < -1022 or E > 1022:
        return v, e
    sc = math.ldexp(1.0, -E)
    return [x * sc for x in v], e + E


def _step_matrix(a, b):
    return [b[0], a[0] * b[1], a[1] * b[2],
            a[0] * b[0], b[1], a[2] * b[2],
            a[1] * b[0], a[2] * b[1], b[2]]


def _vec_mat(v, M):
    return [(v[0] * M[s] + v[1] * M[3 + s]) + v[2] * M[6 + s] for s in range(3)]


class Model:
    """The table's weights and alpha [n][3] (mantissas) as the definition forms them."""

    def __init__(self, tab, pen, shift=None, starts=()):
        self.tab = [[float(x) for x in row] for row in tab]
        self.n = n = len(self.tab)
        self.pen, self.shift, self.starts = pen, shift, set(int(s) for s in starts)
        self.b = [emission_weights(row) for row in self.tab]
        self.a = [None] + [switch_weights(pen, shift, self.starts, w) for w in range(1, n)]
        self.alpha = self._alpha() if n else []

    def _matrix(self, w):
        return _step_matrix(self.a[w], self.b[w])

    def _alpha(self):
        n = self.n
        _, nbk, blocks = H.blocking(n)
        mat, mexp = [], []
        for w0, w1 in blocks:                                   # step 1
            R = self.b[0] * 3 if w0 == 0 else self._matrix(w0)
            e = 0
            for w in range(w0 + 1, w1):
                M = self._matrix(w)
                R = _vec_mat(R[0:3], M) + _vec_mat(R[3:6], M) + _vec_mat(R[6:9], M)
                R, e = _rescale(R, e)
            mat.append(R)
            mexp.append(e)
        fin, fexp = [None] * nbk, [0] * nbk                     # step 2, the forward walk
        v, e = mat[0][0:3], mexp[0]
        for k in range(1, nbk):
            fin[k], fexp[k] = list(v), e
            if k + 1 < nbk:
                v = _vec_mat(v, mat[k])
                e += mexp[k]
                v, e = _rescale(v, e)
        alpha = [None] * n                                      # step 4, the forward half
        for b, (w0, w1) in enumerate(blocks):
            v, e = (fin[b], fexp[b]) if b else (None, 0)
            for w in range(w0, w1):
                if w == 0:
                    v, e = list(self.b[0]), 0
                else:
                    v, e = _rescale(_vec_mat(v, self._matrix(w)), e)
                alpha[w] = list(v)
        return alpha


# ---- a draw ----------------------------------------------------------------------------------------------------------------

def pick(c, U):
    c01 = c[0] + c[1]
    x = U * (c01 + c[2])
    return 0 if x < c[0] else 1 if x < c01 else 2


def weights_into(a, sp):
    """a[q][sp] for q = 0, 1, 2 from a = (a01, a02, a12)."""
    return ((1.0, a[0], a[1]), (a[0], 1.0, a[2]), (a[1], a[2], 1.0))[sp]


def candidates(m, w, sp, variant=None):
    """c_0..2 of window w given the state sp drawn at w + 1 (ignored at the last window)."""
    al = m.alpha[w]
    if w + 1 == m.n or variant == "no_a":
        return list(al)
    a = m.a[w + 1]
    if variant == "a_of_w":                         # the step into w, not into w + 1 (window 0 has none: no penalty)
        a = m.a[w] if w >= 1 else (1.0, 1.0, 1.0)
    col = weights_into(a, sp)
    return [al[q] * col[q] for q in range(3)]


def _u(ky, k, w, u_of):
    return uniform(ky, w) if u_of is None else u_of(k, w)


def draw(m, seed, stream, k, u_of=None, variant=None):
    """The path of draw k, walked once from the back."""
    ky = key(seed, stream, 0 if variant == "shared_u" else k)
    path, st = [0] * m.n, 0
    for w in range(m.n - 1, -1, -1):
        st = pick(candidates(m, w, st, variant), _u(ky, k, w, u_of))
        path[w] = st
    return path


def map_at(a, s):
    return a >> (2 * s) & 3


def map_after(a, b):
    return map_at(a, map_at(b, 0)) | map_at(a, map_at(b, 1)) << 2 | map_at(a, map_at(b, 2)) << 4


def window_map(m, w, U):
    """Window w's map in the form of `from`: the state at w + 1 -> the state at w (constant at the last window)."""
    return sum(pick(candidates(m, w, sp), U) << (2 * sp) for sp in range(3))


def draw_by_maps(m, seed, stream, k, blocks=None):
    """The same path the kernel's way: the maps composed per block, a suffix scan over the blocks, every block resolved from
    the state the blocks behind it give.  blocks: [(w0, w1)], default the blocking of 256."""
    ky = key(seed, stream, k)
    blocks = blocks or H.blocking(m.n)[2]
    maps = [window_map(m, w, uniform(ky, w)) for w in range(m.n)]
    blk = []
    for w0, w1 in blocks:
        f = MAP_ID
        for w in range(w1 - 1, w0 - 1, -1):
            f = map_after(maps[w], f)
        blk.append(f)
    suffix = [MAP_ID] * (len(blocks) + 1)
    for j in range(len(blocks) - 1, -1, -1):
        suffix[j] = map_after(blk[j], suffix[j + 1])
    path = [0] * m.n
    for j, (w0, w1) in enumerate(blocks):
        st = map_at(suffix[j + 1], 0)
        for w in range(w1 - 1, w0 - 1, -1):
            st = map_at(maps[w], st)
            path[w] = st
    return path


# ---- the record ------------------------------------------------------------------------------------------------------------

def record(path, starts=(), pos_first=None, pos_last=None):
    """uint64[15]: the windows per state, then n_seg[3], longest_win[3], bp[3], longest_bp[3] of the path's segments."""
    starts = set(starts)
    rec = [0] * 15
    n, f = len(path), 0
    while f < n:
        w = f + 1
        while w < n and path[w] == path[f] and w not in starts:
            w += 1
        s = path[f]
        span = (int(pos_last[w - 1]) - int(pos_first[f]) + 1) & MASK if pos_first is not None else 0
        rec[s] += w - f
        rec[3 + s] += 1
        rec[6 + s] = max(rec[6 + s], w - f)
        rec[9 + s] = (rec[9 + s] + span) & MASK
        rec[12 + s] = max(rec[12 + s], span)
        f = w
    return rec


# ---- the exact distribution of a small table -------------------------------------------------------------------------------

def path_distribution(m):
    """{path: P(path)} over all 3^n paths, n <= 6, in Fractions of the model's weights."""
    assert 1 <= m.n <= 6
    wt = {}
    for p in product(range(3), repeat=m.n):
        x = Fraction(m.b[0][p[0]])
        for w in range(1, m.n):
            x *= Fraction(weights_into(m.a[w], p[w])[p[w - 1]]) * Fraction(m.b[w][p[w]])
        wt[p] = x
    Z = sum(wt.values())
    if Z == 0:                                      # a dead chain: no path has weight, no distribution
        return {}
    return {p: x / Z for p, x in wt.items()}


def bar(p, K):
    """6 standard deviations of a binomial frequency and 2 / K, as a float (p a Fraction or float)."""
    p = float(p)
    return 6.0 * math.sqrt(max(p * (1.0 - p), 0.0) / K) + 2.0 / K
