"""Site lists with gaps on the panel's own 32-row tiles (ibdg_ld_layout 1), by construction, and what the host and k_prep_* make of
them.

On that layout the counting kernels walk a run of windows segment by segment (one record per window x tile), and each record's
control word tells the tile ring (TileRing, ibdg_ld_popcount.hip) how to reach the NEXT segment of the run: `adv`, the 64-row
tile pairs to advance (8 bits), `nhalf`, the half of the pair it reads, and `nslot` = (pair - the run's first pair) % ring depth
(k_prep_seg_walk / k_prep_seg_flags, ibdg_prep.hip).  Dense site lists only ever advance by 0 or 1.  The cases here are clusters
of covered rows with empty stretches between them, written as ZERO-COVERAGE ROWS of an np.arange(L) site list (n_ref = n_alt =
0), so that depth_cases.segments / ct_max / tab_in_lds / mfma_takes and test_gpu_precision.run_form apply unchanged;
row_index_rendering() gives the same sites as a row_index list that simply omits those rows.  numpy only: importable without a
device.

make_case(name) -> dict(alle, nr, na, W, eps, M, target, refids, pu, n_ids) as depth_cases.make_case, plus rows (the panel row
of every site with reads), wpw (the option windows_per_wave the case is made for: runs of wpw windows), and per case alt_wpw,
twin, gap.  eps = 0.02, M = 20, every covered row has 1..20 reads, drawn from the genotype of background individual SOURCE,
whose first haplotype the target carries as its own first (both --LD columns of the target stay normal doubles).

  ladder         N = 70, W = 11, runs of 16 windows.  Consecutive segments of a run advance by every value of LADDER_ADV, each
                 once into a lower and once into an upper half; cluster sizes of LADDER_SIZES rows: windows that straddle a gap,
                 windows that end just before one, gaps inside a window and between windows.
  upper-start    N = 130, W = 8, runs of 4 windows.  Every run's first segment lies in the upper half of its pair (x_off0);
                 with alt_wpw = 7 every run but the first starts in a lower half.  The run's last segment is preceded by an
                 advance of UPPER_LAST pairs: both guard policies past the run's last pair are taken right after a skip.
  boundary       N = 130, W = 8, runs of 4 windows; BOUNDARY_GAP = 300 pairs exactly between two runs (legal: no control word
                 crosses a run's end).  twin "boundary-shifted": one window of sites more in front, so the gap lies inside a run.
  edge-255       N = 130, W = 8, runs of 4 windows; two site lists, the same sites row for row, whose one large in-run gap is
  edge-256       255 pairs (the largest the control word holds) and 256 (adv_overflow: the strict kernel or the compacted tiles).
  one-row-tiles  N = 130, W = 8, runs of 16 windows; every covered row in a tile of its own (as many segments as rows),
                 advances 0 (lower to upper half of one pair) and 2 in turn; the first site is panel row 31, the last the
                 panel's last row, and the panel's row count is no multiple of 256 (nor of 32).
"""
import functools

import numpy as np

import depth_cases as DC

EPS = 0.02
MAX_COV = 20
SOURCE = 7
TARGET = 5
RECORD_LDS_BYTES = 96 * 1024        # a record budget that never halves a run of these cases
SEG_BYTES = 80 + 8                  # sizeof(ibdg::Seg) + 8: what build_segments (ibdg_api.cpp) charges a segment
RING_DEPTHS = (2, 3, 4, 8)

LADDER_ADV = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 64, 254, 255)
LADDER_SIZES = (5, 6, 9, 2, 11, 4, 7, 13, 3, 8)
UPPER_LAST = (9, 17, 40, 70, 255, 130)
BOUNDARY_GAP = 300

NAMES = ["ladder", "upper-start", "boundary", "boundary-shifted", "edge-255", "edge-256", "one-row-tiles"]
# what runs on the panel's own tiles: edge-256 and the shifted boundary overflow the control word
LAYOUT1_NAMES = [n for n in NAMES if n not in ("edge-256", "boundary-shifted")]


# --------------------------------------------------------------------------- the run structure and the control words
def run_begins(n_win, wpw):
    """make_runs (ibdg_api.cpp) with guided_runs 0: runs of windows_per_wave windows, the last one shorter; the first window of
    every run and, last, the window count."""
    return np.r_[np.arange(0, n_win, wpw), n_win].astype(np.int64)


def run_structure(nr, na, W, wpw, record_lds_bytes=RECORD_LDS_BYTES):
    """The runs of a site list uploaded as np.arange(L) on the panel's own tiles (layout 1: row = position in the list), for
    windows_per_wave = wpw, guided_runs 0.  The run length stands while a run's records fit the budget, max_seg * (sizeof(Seg) + 8)
    <= record_lds_bytes (build_segments halves it otherwise): asserted.  dict(seg = depth_cases.segments, begin = run_begins,
    seg_begin [n_runs + 1] first segment of every run, pairs [n_runs] tile pairs spanned, n_seg [n_runs])."""
    seg = DC.segments(nr, na, W)
    n_win = int(seg["win"][-1]) + 1
    begin = run_begins(n_win, wpw)
    seg_begin = np.searchsorted(seg["win"], begin, side="left")
    n_seg = np.diff(seg_begin)
    assert int(n_seg.max()) * SEG_BYTES <= record_lds_bytes, n_seg
    q = seg["tile"] >> 1
    pairs = [int(q[b - 1] - q[a] + 1) for a, b in zip(seg_begin[:-1], seg_begin[1:])]
    return dict(seg=seg, begin=begin, seg_begin=seg_begin, pairs=pairs, n_seg=n_seg)


def control_words(rs, ring):
    """(adv, nhalf, nslot, in_run) per segment, as k_prep_seg_flags computes them for ring depth `ring`: for segment s of the run
    [s0, s1) with a successor in the run (in_run: s + 1 < s1), adv = pair(s + 1) - pair(s) -- NOT clamped here; above 255 the
    device sets adv_overflow --, nhalf = tile(s + 1) & 1, nslot = (pair(s + 1) - pair(s0)) % ring; 0 for a run's last segment."""
    tile = rs["seg"]["tile"].astype(np.int64)
    q = tile >> 1
    n = len(tile)
    adv, nhalf, nslot, in_run = (np.zeros(n, dtype=np.int64) for _ in range(4))
    for s0, s1 in zip(rs["seg_begin"][:-1], rs["seg_begin"][1:]):
        s = np.arange(s0, s1 - 1)
        adv[s] = q[s + 1] - q[s]
        nhalf[s] = tile[s + 1] & 1
        nslot[s] = (q[s + 1] - q[s0]) % ring
        in_run[s] = 1
    return adv, nhalf, nslot, in_run.astype(bool)


def ring_walk(rs, adv, nhalf, nslot, ring, rerequest):
    """TileRing and the segment walkers (ibdg_ld_popcount.hip) on pair NUMBERS instead of tile words: per run, prime() requests
    the pairs q0 .. q0 + ring - 1 into the slots (q - q0) % ring; a segment reads its words from the slot and half the control
    word of the segment BEFORE it named (the run's first: slot 0, half tile0 & 1 = x_off0), then advance(adv) makes adv
    requests.  Past the run's last pair the vector forms request nothing (rerequest False), the matrix-core forms that pair
    again.  adv is the 8-bit field: min(adv, 255).  A load reaches its slot only through a wait, in issue order, and the counted
    wait (wait_first: before the run's first segment and behind every advance of one pair or more) leaves the newest ring - 1
    in flight -- none once the nominal requests have passed the run's last pair in the vector forms.  Returns (pair, half) as
    read per segment; -1 where the slot holds nothing yet."""
    tile = rs["seg"]["tile"].astype(np.int64)
    pair, half = np.full(len(tile), -1, dtype=np.int64), np.zeros(len(tile), dtype=np.int64)
    for s0, s1 in zip(rs["seg_begin"][:-1], rs["seg_begin"][1:]):
        q0, q_last = int(tile[s0] >> 1), int(tile[s1 - 1] >> 1)
        slots, flight, q_issue = [-1] * ring, [], q0
        for s in range(s0, s1):
            n_req = ring if s == s0 else min(int(adv[s - 1]), 255)
            for _ in range(n_req):
                if rerequest or q_issue <= q_last:
                    flight.append(((q_issue - q0) % ring, min(q_issue, q_last)))
                q_issue += 1
            if n_req:
                keep = ring - 1 if rerequest or q_issue - 1 <= q_last else 0
                landed = max(0, len(flight) - keep)
                for slot, q in flight[:landed]:
                    slots[slot] = q
                del flight[:landed]
            slot, h = (0, int(tile[s0] & 1)) if s == s0 else (int(nslot[s - 1]), int(nhalf[s - 1]))
            pair[s], half[s] = slots[slot], h
    return pair, half


def run_opts(c, wpw=None):
    """The engine options that fix the run structure run_structure() models."""
    return {"windows_per_wave": wpw or c["wpw"], "guided_runs": 0, "record_lds_bytes": RECORD_LDS_BYTES}


# --------------------------------------------------------------------------- clusters of covered rows
class _Clusters:
    """Covered rows as clusters (tile, first position in the tile, rows), appended by the advance from the tile before."""

    def __init__(self, first_tile, pos, n):
        self.items = [(first_tile, pos, n)]
        self.n_cov = n

    @property
    def tile(self):
        return self.items[-1][0]

    def add(self, adv, half, n, pos=None):
        tile = 2 * ((self.tile >> 1) + adv) + half
        assert tile > self.tile and 1 <= n <= 32, (self.tile, adv, half, n)
        pos = (5 * len(self.items)) % (33 - n) if pos is None else pos
        assert pos + n <= 32
        self.items.append((tile, pos, n))
        self.n_cov += n

    def rows(self):
        return np.concatenate([32 * t + p + np.arange(n) for t, p, n in self.items]).astype(np.int64)


def _ladder(W, wpw):
    rng = np.random.default_rng(77)
    steps = [(a, h) for a in LADDER_ADV for h in (0, 1) if (a, h) != (0, 0)]     # (0, lower): a window's end inside a cluster
    steps = [steps[i] for i in rng.permutation(len(steps))]
    steps += [(1, i & 1) for i in range(10)]                  # ... and ten pairs in a row: every slot of the deepest ring in turn
    cl = _Clusters(2, 3, LADDER_SIZES[0])
    k = 1
    for adv, half in steps:
        # a control word exists only inside a run: a step that would fall between two runs gets a cluster in front of it
        # (and a step to the upper half of the same pair one that ends in a lower half)
        if cl.n_cov % (W * wpw) == 0 or (adv == 0 and cl.tile & 1):
            cl.add(1, 0, 4)
        cl.add(adv, half, LADDER_SIZES[k % len(LADDER_SIZES)])
        k += 1
    return cl.rows(), 32 * (cl.tile + 1) + 40


def _run_template(cl, first, steps, sizes):
    """One run of sum(sizes) covered rows: `first` = (adv, half) from the cluster before (None: the list's first cluster is the
    run's first), then `steps` between its clusters."""
    assert len(steps) == len(sizes) - 1
    if first is not None:
        cl.add(first[0], first[1], sizes[0])
    for (adv, half), n in zip(steps, sizes[1:]):
        cl.add(adv, half, n)


def _upper_start():
    # 32 covered rows a run (W = 8, four windows): clusters of 6 (upper) 10 8 5 (lower) rows, then 3 rows behind a long advance.
    # Offsets 8, 16 and 24 of the run -- where runs of seven windows begin -- lie in lower halves.
    sizes = (6, 10, 8, 5, 3)
    cl = _Clusters(3, 11, sizes[0])
    for r, last in enumerate(UPPER_LAST):
        _run_template(cl, None if r == 0 else (1 + r % 3, 1), [(1, 0), (3, 0), (5, 0), (last, r & 1)], sizes)
    return cl.rows(), 32 * (cl.tile + 1) + 7


def _boundary():
    sizes = (6, 10, 8, 5, 3)
    cl = _Clusters(2, 20, sizes[0])                   # (tile 0 stays free for the shifted twin's extra window)
    for r, between in enumerate((None, (3, 1), (BOUNDARY_GAP, 0), (2, 1), (BOUNDARY_GAP + 1, 1))):
        _run_template(cl, between, [(1, 0), (0, 1), (2, 0), (1, 1)], sizes)
    return cl.rows(), 32 * (cl.tile + 1) + 13


def _edge(gap):
    sizes = (6, 10, 8, 5, 3)
    cl = _Clusters(1, 0, sizes[0])
    for r, between in enumerate((None, (2, 0), (1, 1), (4, 1))):
        mid = (gap, 1) if r == 1 else (2, 0)
        _run_template(cl, between, [(1, 0), (0, 1), mid, (1, 1)], sizes)
    return cl.rows(), 32 * (cl.tile + 1) + 21


def _one_row_tiles(n_rows):
    # tiles 0 1 | 8 9 | 16 17 ...: pair 4j, lower then upper half (advance 0), then two pairs on (advance 2)
    k = np.arange(n_rows)
    tile = 4 * (k // 2) + (k & 1)
    pos = (7 * k + 3) % 32
    pos[0], pos[-1] = 31, 17
    rows = 32 * tile + pos
    return rows.astype(np.int64), int(rows[-1]) + 1


def _inputs(seed, rows, L, n_ids, lead=0):
    """The panel and the reads: the alleles and depths of the covered rows come from a stream of their own (two site lists with
    the same clusters in other places share them), the rows between them from a second one.  `lead` further rows at the panel's
    start get reads as well (the shifted twin's extra window); the caller takes them out of the base case."""
    rng, fill = np.random.default_rng(seed), np.random.default_rng(seed + 1000)
    n = len(rows)
    cov_alle, _ = DC.panel(rng, n + lead, n_ids)
    cov_alle[:, 2 * TARGET] = cov_alle[:, 2 * SOURCE]
    depth = 1 + np.minimum(rng.poisson(1.0, size=n + lead), 4)
    rare = np.arange(n + lead) % 7 == 3
    depth[rare] = np.array([8, 20, 15, 4, 16, 7])[(np.arange(n + lead) // 7) % 6][rare]      # the planes beyond cov 0-2 / alt 0-1
    g = cov_alle[:, 2 * SOURCE].astype(np.int64) + cov_alle[:, 2 * SOURCE + 1]
    alt = rng.binomial(depth, np.array([EPS, 0.5, 1 - EPS])[g])
    alle, _ = DC.panel(fill, L, n_ids)
    where = np.r_[np.arange(lead), rows]
    assert len(np.unique(where)) == len(where) and (np.diff(rows) > 0).all() and rows[-1] < L
    alle[where] = cov_alle[np.r_[n + np.arange(lead), np.arange(n)]]
    nr, na = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    nr[where] = (depth - alt)[np.r_[n + np.arange(lead), np.arange(n)]]
    na[where] = alt[np.r_[n + np.arange(lead), np.arange(n)]]
    return alle, nr, na


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The case's inputs (shared: leave them unchanged)."""
    n_ids, W, wpw, extra, lead = 130, 8, 4, {}, 0
    if name == "ladder":
        n_ids, W, wpw = 70, 11, 16
        rows, L = _ladder(W, wpw)
        seed = 9100
    elif name == "upper-start":
        rows, L = _upper_start()
        seed, extra = 9101, dict(alt_wpw=7)
    elif name in ("boundary", "boundary-shifted"):
        rows, L = _boundary()
        seed, lead = 9102, W
        extra = dict(twin="boundary-shifted" if name == "boundary" else "boundary", gap=BOUNDARY_GAP)
    elif name in ("edge-255", "edge-256"):
        gap = int(name[len("edge-"):])
        rows, L = _edge(gap)
        seed, extra = 9103, dict(twin="edge-256" if gap == 255 else "edge-255", gap=gap)
    elif name == "one-row-tiles":
        wpw = 16
        rows, L = _one_row_tiles(8 * 40 + 5)
        seed = 9104
    else:
        raise ValueError(name)
    alle, nr, na = _inputs(seed, rows, L, n_ids, lead)
    if name == "boundary":
        nr[:lead] = na[:lead] = 0
    elif name == "boundary-shifted":
        rows = np.r_[np.arange(lead), rows]
    cov = nr + na
    assert np.array_equal(np.flatnonzero(cov > 0), rows) and 1 <= cov[rows].min() and cov.max() == MAX_COV
    nr, na = nr.astype(np.uint8), na.astype(np.uint8)
    for x in (alle, nr, na, rows):
        x.setflags(write=False)
    return dict(alle=alle, nr=nr, na=na, W=W, eps=EPS, M=MAX_COV, target=TARGET, refids=None, pu=-1, n_ids=n_ids, rows=rows,
                wpw=wpw, **extra)


def row_index_rendering(c):
    """The case as a row_index list that omits the rows without reads: (row_index, n_ref, n_alt) of its sites."""
    rows = c["rows"]
    return rows.astype(np.uint32), c["nr"][rows], c["na"][rows]


@functools.lru_cache(maxsize=None)
def run_seed(name, T):
    """As depth_cases.run_seed: a seed with which test_gpu_precision.run_form, drawing T comparison individuals, draws the
    case's target first."""
    c = make_case(name)
    cand = np.arange(c["n_ids"])
    for seed in range(100000):
        if int(np.random.default_rng(seed).choice(cand, size=T, replace=False)[0]) == c["target"]:
            return seed
    raise AssertionError((name, T))
