"""Hard log2 window tables for the log-domain IBD-state family (ibdgem_amd/csrc/ibdg_states.h): the case generators that
tests/test_hard_tables.py (host twin against the restatements, no device) and tests/test_gpu_log_hard_tables.py (kernels against
the twin, through ibdg_set_window_log2) share.  A run of the engine never writes such a table: no NaN or infinite column, no
emission below 2^-1000, no difference near the -2^24 clamp, a block exponent that barely moves.

case(family, n_win, variant) gives a Case: the table [n_win][3], the penalties the family is meant for, its own step shifts or
None, and what the family claims about itself (the windows it touched), which the CPU tier asserts on the integers.
Families (FINITE: the twin's posteriors are finite and sum to 1; DEAD: no path has weight, the dead-chain rule):
  naninf          at the edge windows in turn: a NaN in one column, an all-NaN row, -inf in one column, +inf in one column, an
                  all -inf row.  Four of the five say nothing (emission (0, 0, 0)); -inf in one column beside two finite ones
                  is a difference of -inf, which the clamp takes: e = -2^40 there
  deep            at the edge windows one live state, the other two 5000 bits below (weight 0), the live state changing from
                  edge to edge
  alternating     every window has one live state, (7 w // 3) % 3, the others 4990 bits below: the state changes inside blocks
                  and across their borders, and Z falls by a switch weight at most windows (large block and walk exponents)
  edge1000        the two other columns at offsets from EDGE_OFFSETS below the best, rotated over windows and states: both sides
                  of POST_K_MIN, and of the subnormal range
  clamp           offsets from CLAMP_OFFSETS: the -2^24 clamp and its edge, and products d * 65536 that end in .5 after an even
                  and after an odd integer
  ties            an all-zero table with every third row (-7, -7, -9): exact ties for the strict > of states_step and argmax3
  dead-shift      a window with state 0 alone alive, then one with state 1 alone alive and a shift of -2^30 on the step between
                  them: the shifted switch weight is exactly 0.  variant 0: the pair inside a block (where C >= 2), variant 1:
                  across a block border (windows C - 1 and C)
  dead-underflow  penalties 1e-300 (a switch weighs 2^-996.6: not 0) and a stretch of windows whose only live state alternates:
                  a block matrix of C >= 2 windows multiplies two switch weights, 2^-1993 is 0 in fp64, and the rows the
                  forward walk needs are gone.  Dead for C >= 2 only: at C = 1 no such product is ever formed (UNDERFLOW_DEAD)
  plateaus        (LONG_FAMILIES only) one state best by 40 bits over stretches of 1, C - 1, C, C + 1, 3 C + 2, 20 C windows in
                  turn (at least 1 each), the best state advancing by one per stretch; marks: a stretch's first window -> its
                  state.  Segments that end at every position of a block, and segments that cover many whole blocks
The edge1000 and clamp tables sit on a base cut to multiples of 2^-20, so that l_s - max(l) gives back the offset exactly.
"""
import math

import numpy as np

SIZES = [1, 2, 3, 255, 256, 257, 513, 1279]           # C = 1, 1, 1, 1, 1, 2, 3, 5
FINITE = ["naninf", "deep", "alternating", "edge1000", "clamp", "ties"]
DEAD = ["dead-shift", "dead-underflow"]
FAMILIES = FINITE + DEAD
PENS = [(0.05, 0.01, 0.05), (1e-3, 1e-6, 1e-3)]
UNDERFLOW_PEN = (1e-300, 1e-300, 1e-300)
EDGE_OFFSETS = [-999.5, -1000.0, -1000.0 - 2.0 ** -16, -1000.5, -1022.0, -1023.0, -1074.0, -1075.0]
CLAMP_OFFSETS = [-2.0 ** 24, -2.0 ** 24 - 1.0, -2.0 ** 24 + 2.0 ** -17, -2.0 ** 30, -1e300, -2.0 ** -17, -3 * 2.0 ** -17,
                 -5 * 2.0 ** -17]
NANINF_KINDS = ["nan", "nanrow", "-inf", "+inf", "-infrow"]
SHIFT_MAX = 1 << 30
BIT = 65536


def blocking(n):
    C = (n + 255) // 256
    return C, (n + C - 1) // C


def UNDERFLOW_DEAD(n):
    return blocking(n)[0] >= 2


def edge_windows(n):
    """0, 1, C - 1, C, 2 C - 1, 2 C, n / 2, the last block's first window, n - 2, n - 1, as far as they exist."""
    C, nbk = blocking(n)
    return sorted({w for w in (0, 1, C - 1, C, 2 * C - 1, 2 * C, n // 2, (nbk - 1) * C, n - 2, n - 1) if 0 <= w < n})


def base(n, seed):
    """normal(-3000, 400) per window + uniform(-3, 3) per column."""
    rng = np.random.default_rng([seed, n])
    return rng.normal(-3000.0, 400.0, (n, 1)) + rng.uniform(-3.0, 3.0, (n, 3))


def shifts(n, seed):
    """Step shifts drawn from +-3 bits (shift[0] is ignored)."""
    return np.random.default_rng([seed, n, 1]).integers(-3 * BIT, 3 * BIT + 1, n).astype(np.int32)


def chain_starts(n):
    """A start at window 1, at a block border (or window 2) and at the last window, as far as they exist."""
    C = blocking(n)[0]
    return sorted({w for w in (1, C if C > 1 else 2, n - 1) if 1 <= w < n})


class Case:
    def __init__(self, family, tab, pen=PENS[0], shift=None, marks=None):
        self.family, self.tab, self.pen, self.shift = family, np.ascontiguousarray(tab, dtype=np.float64), pen, shift
        self.marks = marks or {}        # window -> what the family did there
        self.n = len(self.tab)


def _one_live(row, live, below):
    out = np.full(3, row[live] - below)
    out[live] = row[live]
    return out


def _dead_pair(n, variant):
    """The first window of the pair: inside a block (variant 0, where a block has two windows) or its last window (variant 1)."""
    C, nbk = blocking(n)
    if n == 2:
        return 0
    if variant == 0 and C >= 2:
        return (nbk // 2) * C                  # windows b C and b C + 1 of block b
    return C - 1 if C >= 2 else n // 2         # windows C - 1 and C; at C = 1 every pair crosses a border


def case(family, n, variant=0):
    seed = 1000 * LONG_FAMILIES.index(family) + variant
    tab, marks = base(n, seed), {}
    edges = edge_windows(n)
    if family == "naninf":
        for i, w in enumerate(edges):
            kind, col = NANINF_KINDS[(i + variant) % 5], (i + 2 * variant) % 3
            if kind == "nan":
                tab[w, col] = np.nan
            elif kind == "nanrow":
                tab[w] = np.nan
            elif kind == "-inf":
                tab[w, col] = -np.inf
            elif kind == "+inf":
                tab[w, col] = np.inf
            else:
                tab[w] = -np.inf
            marks[w] = (kind, col)
        return Case(family, tab, marks=marks)
    if family == "deep":
        for i, w in enumerate(edges):
            live = (i + variant) % 3
            tab[w] = _one_live(tab[w], live, 5000.0)
            marks[w] = live
        return Case(family, tab, marks=marks)
    if family == "alternating":
        rows = np.arange(n)
        live = (7 * rows // 3 + variant) % 3
        top = tab[rows, live]
        tab[:] = (top - 4990.0)[:, None]               # (_one_live for every row at once: the same subtraction)
        tab[rows, live] = top
        return Case(family, tab, marks=dict(zip(rows.tolist(), live.tolist())))
    if family in ("edge1000", "clamp"):
        offs = EDGE_OFFSETS if family == "edge1000" else CLAMP_OFFSETS
        tab = np.round(tab * 2.0 ** 20) / 2.0 ** 20
        for w in range(n):
            best = (w + variant) % 3
            o1, o2 = offs[(w + variant) % 8], offs[(3 * w + 5 + variant) % 8]
            m = tab[w, best]
            tab[w, (best + 1) % 3], tab[w, (best + 2) % 3] = m + o1, m + o2
            marks[w] = (best, o1, o2)
        return Case(family, tab, marks=marks)
    if family == "ties":
        tab = np.zeros((n, 3))
        for w in range(variant % 3, n, 3):
            tab[w] = (-7.0, -7.0, -9.0)
            marks[w] = "tie"
        return Case(family, tab, marks=marks)
    if family == "dead-shift":
        assert n >= 2
        p = _dead_pair(n, variant)
        tab[p], tab[p + 1] = (-10.0, -5000.0, -5000.0), (-5000.0, -10.0, -5000.0)
        shift = np.zeros(n, dtype=np.int32)
        shift[p + 1] = -SHIFT_MAX
        return Case(family, tab, pen=PENS[0], shift=shift, marks={p: 0, p + 1: 1})
    if family == "dead-underflow":
        assert n >= 2
        p = _dead_pair(n, variant)
        C = blocking(n)[0]
        lo, hi = max(0, p - 2 * C), min(n, p + 2 + 2 * C)          # the pair and two blocks' worth of windows on either side
        for w in range(lo, hi):
            live = (w - p) % 2
            tab[w] = _one_live(np.full(3, -10.0), live, 4990.0)
            marks[w] = live
        return Case(family, tab, pen=UNDERFLOW_PEN, marks=marks)
    if family == "plateaus":
        C = blocking(n)[0]
        lengths = [max(1, x) for x in (1, C - 1, C, C + 1, 3 * C + 2, 20 * C)]
        w, i = 0, variant
        while w < n:
            live, end = i % 3, min(n, w + lengths[i % 6])
            for other in ((live + 1) % 3, (live + 2) % 3):
                tab[w:end, other] = tab[w:end, live] - 40.0
            marks[w] = live
            w, i = end, i + 1
        return Case(family, tab, marks=marks)
    raise KeyError(family)


# ---- long blocks: many windows a thread (tests/test_hard_tables_long.py, tests/test_gpu_log_long_blocks.py) ----------------------
# A thread of the kernels walks the C windows of its block in loops that the compiler may unroll or pipeline (two of them are
# unrolled by hand, 4 and 8 ways), and reads the chain mask a word of 32 windows at a time.  The lattice 256 C - 5 puts the trip
# counts C and C - 5 into one launch for C = 6 .. 16: every remainder mod 4 and mod 8, an unrolled body run not at all, once and
# more often.  8192: every block is one aligned mask word; 8193: blocks straddle the words at every offset, 7 idle threads;
# 40000: a chromosome's windows; 2^21: the most the calls take.

LONG_SIZES = [256 * C - 5 for C in range(6, 17)] + [1793, 2048, 8192, 8193, 40000, 1 << 21]
# n_win -> (C, owning blocks, windows of the last block), written out: the CPU tier asserts blocking()'s formula gives them
LONG_SHAPES = dict([(256 * C - 5, (C, 256, C - 5)) for C in range(6, 17)]
                   + [(1793, (8, 225, 1)), (2048, (8, 256, 8)), (8192, (32, 256, 32)), (8193, (33, 249, 9)),
                      (40000, (157, 255, 122)), (1 << 21, (8192, 256, 8192))])
LONG_FINITE = FINITE + ["plateaus"]
TINY_WEIGHTS = ["edge1000"]                            # the families that keep emission weights near 2^-1000
LONG_FAMILIES = FAMILIES + ["plateaus"]                # (behind the others: the seeds of FAMILIES stay what they are)
EDGE_SHIFT_VALUES = [-SHIFT_MAX, SHIFT_MAX, 0, -3 * BIT]


def DENSE_WORD_BLOCKS(nbk):
    """The two blocks with a start at every multiple of 32."""
    return 1, nbk // 2


def block_end(n, w):
    """The end (exclusive) of the block that owns window w."""
    C = blocking(n)[0]
    return min(n, (w // C + 1) * C)


def dense_chain_starts(n):
    """Starts that no thread escapes: every window with w % 37 == 5, the first window of every third block, the last window of
    every fifth block, every multiple of 32 in two blocks (DENSE_WORD_BLOCKS), and n - 1.  Strictly increasing, in [1, n)."""
    C, nbk = blocking(n)
    ws = set(range(5, n, 37))
    ws |= {b * C for b in range(0, nbk, 3)}
    ws |= {min(n, (b + 1) * C) - 1 for b in range(0, nbk, 5)}
    for b in DENSE_WORD_BLOCKS(nbk):
        ws |= {w for w in range(b * C, min(n, (b + 1) * C)) if w % 32 == 0}
    ws.add(n - 1)
    return sorted(w for w in ws if 1 <= w < n)


def edge_shifts(n, seed):
    """shifts(n, seed) with -2^30, +2^30, 0 and -3 bits in turn on the first, the second and the last window of every seventh
    block: where the one-window look-ahead of the kernels' shift_at begins, is one window in, and stands still at the block's end.
    (A shift of -2^30 makes every switch weight of its step 0: a table whose live states differ across that step has no path, the
    dead-chain rule -- chain_alive below says which.)"""
    C, nbk = blocking(n)
    sh, i = shifts(n, seed), 0
    for b in range(0, nbk, 7):
        w0, w1 = b * C, min(n, (b + 1) * C)
        for w in sorted({w0, min(w0 + 1, w1 - 1), w1 - 1}):
            sh[w] = EDGE_SHIFT_VALUES[i % 4]
            i += 1
    return sh


def chain_alive(tab, pen, shift=None, starts=()):
    """Whether some path through the table has a weight other than 0 (the exact Z is not 0), from the supports alone: which
    emission and switch weights are exactly 0 (below 2^-1000), walked as sets of states.  Only the windows with a zero switch
    weight are walked: behind any other step every state with an emission is alive.
    False: the dead-chain rule's mark on every row.  True: rows of gamma that sum to 1 -- unless a product of kept weights
    underflows, the other way to D = 0.  Across a step without switch weights alpha_w[s] = alpha_{w-1}[s] b_w[s]:
    alpha_{w-1}[s] is at least a switch weight times an emission weight below the vector's largest entry, so with kept weights
    of 2^-46 and more (every family but TINY_WEIGHTS, at the penalties of PENS) nothing comes near 2^-1022; with emissions kept at
    2^-999.5 the product of two of them is 0 in fp64, and such a table may have rows of 0 although it has paths."""
    import hp_post_ref as H
    import hp_steps_ref as S
    tab = np.asarray(tab, dtype=np.float64)
    n = len(tab)
    if shift is None or n < 2:
        return True
    sh = np.asarray(shift, dtype=np.int64)
    Pmin = min(H.penalty(p) for p in pen)
    cut = -1000 * BIT
    special = np.nonzero(Pmin + sh < cut)[0]
    starts = set(int(s) for s in starts)
    support = lambda w: {s for s, e in enumerate(H.emission(tab[w])) if e >= cut}
    alive, at = None, -1                                   # the states alive at window `at`
    for w in (int(x) for x in special if x >= 1 and int(x) not in starts):
        prev = alive if at == w - 1 else support(w - 1)
        P = S.window_penalties(pen, {w: int(sh[w])}, starts, w)
        ok = [[True, P[0] >= cut, P[1] >= cut], [P[0] >= cut, True, P[2] >= cut], [P[1] >= cut, P[2] >= cut, True]]
        alive, at = {s for s in support(w) if any(ok[q][s] for q in prev)}, w
        if not alive:
            return False
    return True


# ---- a dead chain from real inputs: the host program's files -----------------------------------------------------------------

DEAD_INPUT_IDS, DEAD_INPUT_WINDOW = 60, 100
DEAD_INPUT_SCALE = "1e308"       # --switch-scale: two windows 100 kb apart get a shift of log2(1e5 / 1e308) = -1006.6 bits


def write_dead_chain_input(directory):
    """Panel, legend, individuals and pileup of 200 sites (two windows of 100) under `directory`; returns the host program's
    arguments for them.  Every site has 20 reads, all of the alternative allele.  The first individual is homozygous reference
    over the first window, where the panel's frequency is a half: the reads contradict IBD1 by 20 bits a site and IBD2 by 113, so
    IBD0 alone is alive.  Over the second window it alone carries the alternative allele, twice: the reads agree with it, and IBD0
    lies log2(1 / 60^2) = 11.8 bits a site below IBD2 -- 1180 bits in all, weight 0.  The two windows' live states are disjoint,
    and with --switch-scale 1e308 every switch weight is exactly 0: no path has weight.  Every other individual is alive."""
    N, W = DEAD_INPUT_IDS, DEAD_INPUT_WINDOW
    L = 2 * W
    rng = np.random.default_rng(5)
    alle = np.zeros((L, 2 * N), dtype=np.uint8)
    alle[:W] = rng.random((W, 2 * N)) < 0.5
    alle[:W, 0:2] = 0
    alle[W:, 0:2] = 1
    pos = [1000 * (i + 1) for i in range(L)]
    with open(f"{directory}/dead.hap", "w") as fh:
        fh.write("".join(" ".join(map(str, r)) + "\n" for r in alle))
    with open(f"{directory}/dead.legend", "w") as fh:
        fh.write("ID pos allele0 allele1\n" + "".join(f"SNP{i + 1} {p} A C\n" for i, p in enumerate(pos)))
    with open(f"{directory}/dead.indv", "w") as fh:
        fh.write("".join(f"ind{i}\n" for i in range(N)))
    with open(f"{directory}/dead.pileup", "w") as fh:
        fh.write("".join(f"1\t{p}\tN\t20\t{'C' * 20}\t{'I' * 20}\t{']' * 20}\n" for p in pos))
    return ["-H", "dead.hap", "-L", "dead.legend", "-I", "dead.indv", "-P", "dead.pileup", "-N", "pu", "-w", str(W),
            "--log-stats", "--states", "--posteriors", "--segments", "--sample-paths", "5", "--seed", "7",
            "--switch-scale", DEAD_INPUT_SCALE]


def read_dead_chain_run(files):
    """What the run of hard_tables.write_dead_chain_input must show, from {file name: bytes}: the first individual dead, the others
    alive."""
    post = [l.split("\t") for l in files["pu.logibdposteriors.txt"].decode().splitlines() if not l.startswith("#")]
    ids = [f"ind{i}" for i in range(DEAD_INPUT_IDS)]
    assert [r[0] for r in post[:len(ids)]] == ids
    assert post[0][1:] == ["2", "0.000", "0.000", "0.000", "0.000000", "0.000000", "0.000000", "-inf"]
    for r in post[1:len(ids)]:
        assert r[1] == "2" and abs(sum(float(x) for x in r[2:5]) - 2.0) <= 0.002 and math.isfinite(float(r[8]))
    seg = [l.split("\t") for l in files["pu.logibdsegments.txt"].decode().splitlines() if not l.startswith("#")]
    assert seg[0][0] == "ind0" and [seg[0][1], seg[0][5], seg[0][9]] == ["1", "0", "1"]      # its path: IBD0, then IBD2
    smp = [l.split("\t") for l in files["pu.logibdsamples.txt"].decode().splitlines() if not l.startswith("#")]
    assert smp[0][:3] == ["ind0", "2", "5"] and smp[0][3 + 24] == "2.000"                    # every draw: state 2 in both windows
