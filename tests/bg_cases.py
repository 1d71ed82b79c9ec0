"""Backgrounds at every chunk and lane edge of the --LD kernels, by construction.

A run's background is a -B list (individuals with multiplicities 0..255, the C ABI's bg_count bytes), the -N individual
(pu), and what the two exclusions of src/ibdgem.c:714 and :742-750 leave of them for each comparison individual.  The kernels
lay the individuals out in chunks of 64 lanes (one wave of the counting kernels), half chunks of 32 (one wave of k_ld_mfma,
eight of which mfma_wg_sum adds up) and chunk groups of eight (one workgroup of k_ld_popcount); random multiplicities 0..2
leave none of these empty and none with a single weighted lane.  The cases here do, in named, seeded inputs (numpy only:
importable without a device).

make_case(name) -> dict(alle, nr, na, W, eps, M, target, refids, pu, n_ids, mult, targets, interesting).  refids is the list
as the reference reads it (every individual mult[i] times, in order), targets(T) the fixed comparison individuals of a form
with T of them: the case's `interesting` ones first (the target first of all), then a seeded draw of the others -- never
pu except where the case says so, and never somebody whose own exclusion would empty a background the case calls non-empty.
eps = 0.02, max_cov 20, W = 33, 3 * 33 + 17 rows with min(max(Poisson(2), 1), 20) reads each: four windows, the last one
short, windows that straddle the 32-row tiles.

Panel A: 130 individuals -- three chunks, the last with two lanes; five half chunks.
Panel B: 520 individuals -- nine chunks: a second chunk group of k_ld_popcount with one live wave; 18 half chunks: groups of
8, 8 and 2 in mfma_wg_sum.

  chunk-empty                 64..127 with multiplicity 0; the target is 64 (lane 0 of the empty chunk), the others outside it
  own-chunk-otherwise-empty   of chunk 1 only the target (70, multiplicity 2): its masked sum over the chunk is 63 zeros
  half-chunks-empty           lanes 32..63 of chunk 0 and 0..31 of chunk 1 with multiplicity 0
  one-lane-per-chunk          only 0, 127 and 129 listed; the target is elsewhere
  tail-only                   only 128 and 129 listed
  single-first, single-last   one background individual (0, 129), the target elsewhere: a background of 1
  empty                       only the target listed
  empty-by-pu                 only the target and pu listed: both exclusions are needed to reach 0
  mult-255                    255 on every seventh individual (the target and pu among them), 0 on every eleventh that is no seventh, else 1
  mult-edges                  0, 1, 2, 3, 128, 255 in turn at lanes 0, 31, 32, 63 of every chunk
  pu-next-to-target           pu = target + 1, same half chunk
  pu-lane63-other-chunk       pu = 127, the target in chunk 0
  pu-in-tail                  pu = 129
  pu-unlisted                 pu has multiplicity 0
  pu-is-target                pu is the first comparison individual
  targets-unlisted            every comparison individual has multiplicity 0: nothing of theirs is excluded
  group-in-one-half           targets(T) starts with 64..78 (multiplicities 1..3): a group of 15 inside one wave of k_ld_mfma
  B-first-group-empty         panel B, chunks 0..7 with multiplicity 0: only 512..519 listed
  B-second-group-empty        panel B, chunk 8 with multiplicity 0
  B-mult-255                  as mult-255, across nine chunks
"""
import functools

import numpy as np

N_A, N_B = 130, 520
EPS = 0.02
MAX_COV = 20
W = 33
N_ROWS = 3 * W + 17
T_MAX = 31
MULT_EDGE_VALUES = (0, 1, 2, 3, 128, 255)
EDGE_LANES = (0, 31, 32, 63)

NAMES = ["chunk-empty", "own-chunk-otherwise-empty", "half-chunks-empty", "one-lane-per-chunk", "tail-only", "single-first",
         "single-last", "empty", "empty-by-pu", "mult-255", "mult-edges", "pu-next-to-target", "pu-lane63-other-chunk",
         "pu-in-tail", "pu-unlisted", "pu-is-target", "targets-unlisted", "group-in-one-half", "B-first-group-empty",
         "B-second-group-empty", "B-mult-255"]
A_NAMES = [n for n in NAMES if not n.startswith("B-")]
EMPTY = ("empty", "empty-by-pu")


@functools.lru_cache(maxsize=None)
def inputs(n_ids):
    """The panel and the reads of every case on it (shared: leave them unchanged).  Alleles and depths as
    test_gpu_parity.synth draws them, with a read on every row."""
    rng = np.random.default_rng(8100 + n_ids)
    f = np.clip(rng.beta(0.3, 1.0, size=N_ROWS), 1e-3, 0.999)
    alle = (rng.random((N_ROWS, 2 * n_ids)) < f[:, None]).astype(np.uint8)
    cov = np.clip(rng.poisson(2.0, size=N_ROWS), 1, MAX_COV)
    na = rng.binomial(cov, f)
    out = alle, (cov - na).astype(np.uint8), na.astype(np.uint8)
    for x in out:
        x.setflags(write=False)
    return out


def mult_255(n_ids):
    m = np.ones(n_ids, dtype=np.int64)
    m[::11] = 0
    m[::7] = 255
    return m


def mult_edges(n_ids):
    m = np.ones(n_ids, dtype=np.int64)
    at = [64 * c + lane for c in range((n_ids + 63) // 64) for lane in EDGE_LANES if 64 * c + lane < n_ids]
    for k, i in enumerate(at):
        m[i] = MULT_EDGE_VALUES[k % len(MULT_EDGE_VALUES)]
    return m


def _background(name):
    """(n_ids, mult, pu, interesting comparison individuals -- the target first --, who else may be drawn as one)."""
    n = N_B if name.startswith("B-") else N_A
    m = np.ones(n, dtype=np.int64)
    everybody = np.arange(n)
    pu, others = -1, everybody
    if name == "chunk-empty":
        m[64:128] = 0
        who, others = [64, 0, 129], np.r_[0:64, 128:130]
    elif name == "own-chunk-otherwise-empty":
        m[64:128] = 0
        m[70] = 2
        who = [70, 5, 129]
    elif name == "half-chunks-empty":
        m[32:96] = 0
        who = [5, 40, 100]
    elif name == "one-lane-per-chunk":
        m[:] = 0
        m[[0, 127, 129]] = 1
        who, others = [70, 1, 128], np.setdiff1d(everybody, [0, 127, 129])
    elif name == "tail-only":
        m[:128] = 0
        who = [3, 128, 64]
    elif name in ("single-first", "single-last"):
        only = 0 if name == "single-first" else n - 1
        m[:] = 0
        m[only] = 1
        who, others = [77, n - 1 - only, 64], np.setdiff1d(everybody, [only])
    elif name == "empty":
        m[:] = 0
        m[70] = 1
        who = [70, 0, 129]
    elif name == "empty-by-pu":
        m[:] = 0
        m[[5, 6]] = 1
        pu, who = 6, [5, 64, 129]
    elif name in ("mult-255", "B-mult-255"):
        m = mult_255(n)
        pu, who = 63, [70, 11, 1] if n == N_A else [70, 518, 11]
    elif name == "mult-edges":
        m = mult_edges(n)
        who = [95, 64, 0]
    elif name == "pu-next-to-target":
        pu, who = 41, [40, 42, 104]
    elif name == "pu-lane63-other-chunk":
        pu, who = 127, [5, 126, 128]
    elif name == "pu-in-tail":
        pu, who = 129, [5, 128, 64]
    elif name == "pu-unlisted":
        pu, who = 20, [5, 21, 129]
        m[pu] = 0
    elif name == "pu-is-target":
        pu, who = 5, [5, 6, 127]
    elif name == "targets-unlisted":
        who = [64, 0, 129]
        edges = who + [31, 32, 63, 127, 128]
        drawn = [int(x) for x in np.random.default_rng(77).permutation(n) if int(x) not in edges]
        others = np.array((edges + drawn)[:T_MAX])          # the comparison individuals of every form, and nobody else
        m[1::9] = 2
        m[others] = 0
    elif name == "group-in-one-half":
        who, others = list(range(64, 79)), np.r_[0:64, 96:130]
        m[64:79] = 1 + np.arange(15) % 3
    elif name == "B-first-group-empty":
        m[:512] = 0
        who = [3, 515, 511]
    elif name == "B-second-group-empty":
        m[512:] = 0
        who = [515, 0, 300]
    else:
        raise ValueError(name)
    if pu >= 0 and name != "pu-is-target":
        others = np.setdiff1d(others, [pu])
    return n, m, pu, who, others


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The case's inputs (shared: leave them unchanged)."""
    n, m, pu, who, others = _background(name)
    alle, nr, na = inputs(n)
    rng = np.random.default_rng(8200 + NAMES.index(name))
    rest = [int(x) for x in rng.permutation(np.asarray(others)) if int(x) not in who]
    order = (list(who) + rest)[:max(T_MAX, len(who))]
    assert len(order) >= T_MAX and len(set(order)) == len(order), name
    refids = np.repeat(np.arange(n), m)
    mult = m.astype(np.uint8)
    assert (mult == m).all()
    for x in (refids, mult):
        x.setflags(write=False)

    def targets(T):
        assert 1 <= T <= len(order)
        return order[:T]

    return dict(alle=alle, nr=nr, na=na, W=W, eps=EPS, M=MAX_COV, target=order[0], refids=refids, pu=pu, n_ids=n, mult=mult,
                targets=targets, interesting=min(len(who), 3))


def checked(name, T):
    """The positions in targets(T) a run of T individuals is checked at: the interesting ones (three at the most: in
    group-in-one-half the group's first, middle and last), and the last of the drawn ones; of four or fewer, all."""
    c = make_case(name)
    if T <= 4:
        return list(range(T))
    if name == "group-in-one-half":
        first = [0, 7, 14]
    else:
        first = list(range(c["interesting"]))
    return sorted({i for i in first if i < T} | {T - 1})


def full_background(name):
    """refids, pu of a run of the case's panel with everybody listed once."""
    return np.arange(make_case(name)["n_ids"]), -1
