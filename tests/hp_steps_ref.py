"""Truth for the step shifts (ibdgem_amd/csrc/ibdg_states.h): the definition restated in Python integers, on top of
tests/hp_post_ref.py.

Path.  window_penalties() is P_xy(w) = min(0, max(-2^40, P_xy + shift[w])), 0 at a chain start; brute_force() walks all 3^n
paths of a small table, restated() is the recurrence with the window's own matrix.  Both take the lowest state on a tie, the way
the definition does: the final state is the lowest of the best, and `from` the lowest state of a maximum.

Posteriors.  Truth is hp_post_ref.Truth with a matrix per window: a_xy(w) is the weight of P_xy(w) by the emissions' rule (below
2^-1000 it is 0), the same float on either side, so the weights stay inputs, the count of roundings per window stays R = 14 and
the module's bars hold as they are.  Every weight is a dyadic rational or 0: alpha, beta and Z are integers over powers of two
that add up to the same total at every window, as in hp_post_ref.
"""
import hp_post_ref as H

PEN_MIN = -(1 << 40)
SHIFT_MAX = 1 << 30


def shift_penalty(P, sh):
    return min(0, max(PEN_MIN, P + int(sh)))


def window_penalties(pen, shift, starts, w):
    """(P_01(w), P_02(w), P_12(w)) of the step into window w >= 1."""
    if w in starts:
        return (0, 0, 0)
    return tuple(shift_penalty(H.penalty(p), 0 if shift is None else shift[w]) for p in pen)


def _matrix(P):
    return [[0, P[0], P[1]], [P[0], 0, P[2]], [P[1], P[2], 0]]


# ---- the path ---------------------------------------------------------------------------------------------------------

def brute_force(tab, pen, shift, starts=()):
    """(path, scores, counts) from all 3^n paths: score[w][s] is the best sum over the paths of windows 0 .. w that end in s; the
    path is the best whole path that is smallest read from its end (the traceback's choice among equals)."""
    n = len(tab)
    starts = set(starts)
    e = [H.emission(row) for row in tab]
    m = [None] + [_matrix(window_penalties(pen, shift, starts, w)) for w in range(1, n)]

    def total(path):
        return sum(e[w][path[w]] for w in range(len(path))) + sum(m[w][path[w - 1]][path[w]] for w in range(1, len(path)))

    def paths(k):
        if k == 0:
            yield ()
            return
        for p in paths(k - 1):
            for s in range(3):
                yield p + (s,)

    score = []
    for w in range(n):
        best = [None] * 3
        for p in paths(w + 1):
            t = total(p)
            if best[p[-1]] is None or t > best[p[-1]]:
                best[p[-1]] = t
        score.append(best)
    top = max(score[-1])
    winners = [p for p in paths(n) if total(p) == top]
    path = list(min(winners, key=lambda p: p[::-1]))
    return path, score, [path.count(s) for s in range(3)]


def restated(tab, pen, shift, starts=()):
    """The recurrence of ibdg_states.h with the window's own penalties, in Python integers: (path, scores, counts)."""
    starts = set(starts)
    n = len(tab)
    score, frm = [], []
    for w in range(n):
        e = H.emission(tab[w])
        if w == 0:
            v, f = list(e), [0, 1, 2]
        else:
            m = _matrix(window_penalties(pen, shift, starts, w))
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


# ---- the posteriors -----------------------------------------------------------------------------------------------------

class Truth(H.Truth):
    """hp_post_ref.Truth with a matrix per window: A[w], over 2^ea[w], for the step into window w >= 1."""

    def __init__(self, tab, p01, p02, p12, shift, starts=()):
        tab = [[float(x) for x in row] for row in tab]
        self.n = n = len(tab)
        self.pen = (p01, p02, p12)
        starts = set(starts)
        self.Aw, self.eaw = [None], [0]
        for w in range(1, n):
            a01, a02, a12 = (H.weight(P) for P in window_penalties(self.pen, shift, starts, w))     # (the emissions' rule)
            A, ea = H._ints([1.0, a01, a02, a01, 1.0, a12, a02, a12, 1.0])
            self.Aw.append([A[0:3], A[3:6], A[6:9]])
            self.eaw.append(ea)
        self.b = [[H.weight(e) for e in H.emission(row)] for row in tab]
        assert all(max(b) == 1.0 for b in self.b)
        self.B, self.eb = zip(*(H._ints(b) for b in self.b)) if n else ((), ())
        self.alpha = self._forward()
        self.beta = self.backward_from(n - 1, [1, 1, 1]) if n else {}
        self.Z = sum(self.alpha[-1]) if n else 1
        self.ez = self.eb[0] + sum(self.eaw[w] + self.eb[w] for w in range(1, n)) if n else 0
        self.P = H._Products(self.alpha, self.beta)
        self._S = None

    def _forward(self):
        out = []
        for w in range(self.n):
            if w == 0:
                v = list(self.B[0])
            else:
                A = self.Aw[w]
                v = [sum(v[q] * A[q][s] for q in range(3)) * self.B[w][s] for s in range(3)]
            out.append(v)
        return out

    def backward_from(self, w_last, vec):
        out, v = {w_last: list(vec)}, list(vec)
        for w in range(w_last, 0, -1):
            A = self.Aw[w]
            t = [self.B[w][s] * v[s] for s in range(3)]
            v = [sum(A[q][s] * t[s] for s in range(3)) for q in range(3)]
            out[w - 1] = v
        return out
