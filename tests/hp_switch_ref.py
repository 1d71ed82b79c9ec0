"""Truth and bar for the switches (ibdgem_amd/csrc/ibdg_states.h), on top of tests/hp_steps_ref.py.

Truth.  Over hp_steps_ref.Truth's integers -- alpha[w], beta[w], the step's weights Aw[w] and the emission weights B[w], each
over its own power of two -- x_w[q][s] = alpha_{w-1}[q] Aw[w][q][s] B[w][s] beta_w[s] is an integer over the power of two that Z
has (alpha_w[s] = sum_q alpha_{w-1}[q] Aw[w][q][s] B[w][s], so the nine add up to sum_s alpha_w[s] beta_w[s] = Z at every
window).  sw_w[k] = y_w[k] / Z with y_01 = x[0][1] + x[1][0], y_02 = x[0][2] + x[2][0], y_12 = x[1][2] + x[2][1], and n[k] = (sum
of y_w[k] over the counted steps) / Z: exact quotients of integers, compared as integers.  brute_force() sums the weights of
all 3^n paths of a small table instead and must give the same integers.

The counted rule, restated: step w >= 1 is counted for pair k iff w starts no chain and there are no shifts or P_k + shift[w]
<= 0 (counted()).

Bar.  Roundings on the way to one sw_w[k] in the order ibdg_states.h writes, counted the way hp_post_ref counts R = 14 (all
terms non-negative: a sum's relative error is at most its worst term's plus one per addition):
  alpha_{w-1} and beta_w together      <= 7 n - 3   (hp_post_ref: 4 n + 3 (nbk - 1), a block owns at least one window)
  M_w[q][s] = a b                      1
  x = (v M) beta                       2 products:            x  <= 7 n
  y_k = x + x                          1 addition:            y  <= 7 n + 1
  X = (r_0 + r_1) + r_2, r_q of 3      8 additions:           X  <= 7 n + 8
  sw = y / X                           y's, X's and 1:        14 n + 10
so |got - truth| <= (14 n + Q) u truth + 2^-1000 with Q = 10, u = 2^-53; (1 + u)^k - 1 <= k u (1 + k u) is covered by the slack
of the count as in hp_post_ref (k u <= 1e-10 at every shape tested).  n[k]: the quotients' bars summed, plus the C - 1 additions
of a block and the 8 of the tree on the sum: (14 n + Q + C + 8) u truth + n 2^-1000.  The bars are this count, not a measured
number; the tests print the worst error over the bar.

Dead chains (Z == 0 exactly, a shifted weight that is 0): sw = (0, 0, 0) at every window and n = (0, 0, 0), no bar.
"""
import hp_post_ref as H
import hp_steps_ref as HS

R = H.R
Q = 10
PAIRS = ((0, 1), (0, 2), (1, 2))


def counted(pen, shift, starts, w, k):
    """Whether the step into window w >= 1 is counted for pair k."""
    if w in starts:
        return False
    return shift is None or H.penalty(pen[k]) + int(shift[w]) <= 0


class Truth:
    """x(w): the nine integers of step w >= 1; y(w): the three of the pairs; Z; N[k] = the counted sums."""

    def __init__(self, tab, p01, p02, p12, shift=None, starts=()):
        self.t = t = HS.Truth(tab, p01, p02, p12, shift, starts)
        self.n, self.pen, self.shift, self.starts = t.n, (p01, p02, p12), shift, set(starts)
        self.Z = t.Z
        self.dead = t.dead
        self._y = {}
        self._x = (None, None)
        self._N = None

    def x(self, w):
        if self._x[0] != w:                                         # (the last one asked for is kept: its callers go window by window)
            t = self.t
            self._x = (w, [[t.alpha[w - 1][q] * t.Aw[w][q][s] * t.B[w][s] * t.beta[w][s] for s in range(3)] for q in range(3)])
        return self._x[1]

    def y(self, w):
        if w not in self._y:
            x = self.x(w)
            assert sum(map(sum, x)) == self.Z, f"the nine of step {w} do not add up to Z"
            self._y[w] = [x[q][s] + x[s][q] for q, s in PAIRS]
        return self._y[w]

    def stay(self, w):
        """sum_s x_w[s][s]: Z - stay = the three y."""
        x = self.x(w)
        return x[0][0] + x[1][1] + x[2][2]

    def column(self, w, s):
        """sum_q x_w[q][s] = alpha_w[s] beta_w[s], the numerator of gamma_w[s]."""
        x = self.x(w)
        return x[0][s] + x[1][s] + x[2][s]

    def is_counted(self, w, k):
        return counted(self.pen, self.shift, self.starts, w, k)

    @property
    def N(self):
        if self._N is None:
            self._N = [sum(self.y(w)[k] for w in range(1, self.n) if self.is_counted(w, k)) for k in range(3)]
        return self._N

    def counted_steps(self):
        return [sum(self.is_counted(w, k) for w in range(1, self.n)) for k in range(3)]


def _mat_vec(M, v):
    return [(M[3 * q] * v[0] + M[3 * q + 1] * v[1]) + M[3 * q + 2] * v[2] for q in range(3)]


def restated(tab, pen, shift=None, starts=(), counted_rule=True, wrong_X=False):
    """(sw [n][3], n[3]) by the definition's fixed order in Python floats, on the weights of hp_sample_ref.Model: steps 1 to 3 of
    the posteriors, the switches' forward pass, step 5's tree.  The two negative controls: counted_rule=False adds every step
    w >= 1 to the sums; wrong_X=True divides by the posteriors' D of window w - 1, (v[0] beta_{w-1}[0] + v[1] beta_{w-1}[1]) +
    v[2] beta_{w-1}[2], in the place of X."""
    import hp_sample_ref as SR
    sh = None if shift is None else [int(x) for x in shift]
    m = SR.Model(tab, pen, sh, starts)
    n = m.n
    if n == 0:
        return [], [0.0, 0.0, 0.0]
    _, nbk, blocks = H.blocking(n)
    mat, mexp = [], []
    for w0, w1 in blocks:                                       # 1
        B = m.b[0] * 3 if w0 == 0 else m._matrix(w0)
        e = 0
        for w in range(w0 + 1, w1):
            M = m._matrix(w)
            B = SR._vec_mat(B[0:3], M) + SR._vec_mat(B[3:6], M) + SR._vec_mat(B[6:9], M)
            B, e = SR._rescale(B, e)
        mat.append(B)
        mexp.append(e)
    fin, fexp = [None] * nbk, [0] * nbk                         # 2
    v, e = mat[0][0:3], mexp[0]
    for k in range(1, nbk):
        fin[k], fexp[k] = list(v), e
        if k + 1 < nbk:
            v, e = SR._rescale(SR._vec_mat(v, mat[k]), e + mexp[k])
    gout, g = [None] * nbk, [1.0, 1.0, 1.0]
    for k in range(nbk - 1, -1, -1):
        gout[k] = list(g)
        if k > 0:
            g, _ = SR._rescale(_mat_vec(mat[k], g), 0)
    beta = [None] * n
    for b, (w0, w1) in enumerate(blocks):                       # 3
        be = list(gout[b])
        for w in range(w1 - 1, w0 - 1, -1):
            beta[w] = list(be)
            if w > w0:
                be, _ = SR._rescale(_mat_vec(m._matrix(w), be), 0)
    sw, part = [None] * n, [[0.0, 0.0, 0.0] for _ in range(256)]
    st = set(int(s) for s in starts)
    for b, (w0, w1) in enumerate(blocks):                       # forward
        v, e = (fin[b], fexp[b]) if b else (None, 0)
        acc = [0.0, 0.0, 0.0]
        for w in range(w0, w1):
            if w == 0:
                v, e = list(m.b[0]), 0
                sw[0] = [0.0, 0.0, 0.0]
                continue
            M = m._matrix(w)
            x = [[(v[q] * M[3 * q + s]) * beta[w][s] for s in range(3)] for q in range(3)]
            r = [(x[q][0] + x[q][1]) + x[q][2] for q in range(3)]
            X = (r[0] + r[1]) + r[2]
            if wrong_X:
                X = (v[0] * beta[w - 1][0] + v[1] * beta[w - 1][1]) + v[2] * beta[w - 1][2]
            y = [x[0][1] + x[1][0], x[0][2] + x[2][0], x[1][2] + x[2][1]]
            sw[w] = [0.0, 0.0, 0.0] if X == 0.0 else [yk / X for yk in y]
            for k in range(3):
                if not counted_rule or counted(pen, sh, st, w, k):
                    acc[k] = acc[k] + sw[w][k]
            v, e = SR._rescale(SR._vec_mat(v, M), e)
        part[b] = acc
    d = 128                                                     # 5
    while d:
        for b in range(d):
            part[b] = [part[b][k] + part[b + d][k] for k in range(3)]
        d //= 2
    return sw, part[0]


def brute_force(tab, pen, shift=None, starts=()):
    """(y[w][k] for w = 0 .. n - 1 (y[0] = zeros), Z) from all 3^n paths, in the integers of hp_steps_ref.Truth."""
    t = HS.Truth(tab, *pen, shift, starts)
    n = t.n
    assert n <= 7
    y = [[0, 0, 0] for _ in range(n)]
    Z = 0

    def walk(path, wgt):
        nonlocal Z
        w = len(path)
        if w == n:
            Z += wgt
            for i in range(1, n):
                a, b = path[i - 1], path[i]
                if a != b:
                    y[i][PAIRS.index((min(a, b), max(a, b)))] += wgt
            return
        for s in range(3):
            walk(path + (s,), wgt * t.B[w][s] * (t.Aw[w][path[-1]][s] if w else 1))

    walk((), 1)
    return y, Z


def sw_err_and_bar(got, Y, Z, n_win):
    """|got - Y / Z| and (14 n + Q) u Y / Z + 2^-1000, both times Z gd 2^53 2^1000: two integers."""
    gn, gd = float(got).as_integer_ratio()
    return abs(gn * Z - Y * gd) << (H.U_BITS + H.ABS_BITS), ((H.Rn(n_win) + Q) * Y * gd << H.ABS_BITS) + (Z * gd << H.U_BITS)


def n_err_and_bar(got, N, Z, n_win):
    C = H.blocking(n_win)[0]
    gn, gd = float(got).as_integer_ratio()
    return (abs(gn * Z - N * gd) << (H.U_BITS + H.ABS_BITS),
            ((H.Rn(n_win) + Q + C + 8) * N * gd << H.ABS_BITS) + (n_win * Z * gd << H.U_BITS))


def control_err_and_bar(Yc, Dc, Y, Z, n_win):
    """|Yc / Dc - Y / Z| and the bar of Y / Z, both times Z Dc 2^53 2^1000: how far a wrong model's sw lies from the truth."""
    return abs(Yc * Z - Y * Dc) << (H.U_BITS + H.ABS_BITS), ((H.Rn(n_win) + Q) * Y * Dc << H.ABS_BITS) + (Z * Dc << H.U_BITS)


def check(truth, sw, expect):
    """sw [n][3] (or None) and expect [3] against the truth within their bars.  Returns the largest error / bar seen."""
    t, n, worst = truth, truth.n, 0.0
    if t.dead:
        if sw is not None:
            for w in range(n):
                assert [float(v) for v in sw[w]] == [0.0, 0.0, 0.0], f"sw[{w}] = {list(sw[w])!r} of a dead chain (Z == 0)"
        assert [float(v) for v in expect] == [0.0, 0.0, 0.0], f"expect = {list(expect)!r} of a dead chain"
        return 0.0
    if sw is not None and n:
        assert [float(v) for v in sw[0]] == [0.0, 0.0, 0.0]
        for w in range(1, n):
            for k in range(3):
                err, bar = sw_err_and_bar(sw[w][k], t.y(w)[k], t.Z, n)
                worst = max(worst, H._ratio(err, bar))
                assert err <= bar, f"sw[{w}][{k}] = {sw[w][k]!r}: {H._ratio(err, bar):.3g} bars from {t.y(w)[k] / t.Z!r} (n_win {n})"
    for k in range(3):
        err, bar = n_err_and_bar(expect[k], t.N[k], t.Z, n)
        worst = max(worst, H._ratio(err, bar))
        assert err <= bar, f"expect[{k}] = {expect[k]!r}: {H._ratio(err, bar):.3g} bars from {t.N[k] / t.Z!r} (n_win {n})"
    return worst
