"""Inputs that put every read depth 1..50 and every edge of the weight planes through the --LD kernels, by construction.

The fast --LD kernels count reads from bit-planes of the depths (ibdg::Seg::cov[8], alt[8], one record per (window,
32-row tile) segment, k_prep_seg_walk in ibdg_prep.hip), and every counting form switches code by the bit length of the
largest depth (nc) and alt count (na) of a segment.  Poisson depths reach the upper planes by chance; the cases here
reach them in every segment regime, in named, seeded inputs (numpy only: importable without a device).

make_case(name) -> dict(alle, nr, na, W, eps, M, target, refids, pu, n_ids).  eps = 0.02, 130 individuals (three chunks,
the last partial), everybody in the background, and a panel drawn as test_gpu_precision.synth draws its alleles:

  lattice         every (n_ref, n_alt) with 1 <= n_ref + n_alt <= 50 once (1325 rows), shuffled; W = 3
  ladder          the same rows sorted by depth, then n_alt: tiles of one depth, consecutive segments through every
                  regime; W = 3
  lattice-M<m>    the full lattice of max_cov m in (1, 7, 8, 15, 16, 31, 32), repeated to three tiles or more, shuffled,
                  for an engine made with that max_cov (the row decode idx / d of k_prep_* and the P(D|G) table's stride
                  on both sides of every power of two); W = 3
  spike           54 tiles of min(Poisson(1), 3) reads (rows without reads among them); tile k has one row of depth
                  SPIKE_DEPTHS[k // 6] at position SPIKE_POSITIONS[k % 6], its n_alt one of spike_alts(depth) in turn;
                  W = 15: windows straddle tiles
  full-depth-15   one row in five with exactly 50 reads, the others none; n_alt ~ Binomial(50, [eps, 1/2, 1 - eps][g])
  full-depth-16   from the genotype g of background individual 7, whose first haplotype the target carries as its own
                  first: both columns stay large.  8 windows of 15 rows (750 reads: the last length whose power tables stay
                  in LDS) and of 16 (800: in global memory)

Also what the tests need to know about a case without a device: segments(), tab_in_lds(), mfma_lds_bytes().
"""
import functools

import numpy as np

N_IDS = 130
EPS = 0.02
MAX_COV = 50
LATTICE_M = (1, 7, 8, 15, 16, 31, 32)
SPIKE_DEPTHS = (4, 7, 8, 15, 16, 31, 32, 49, 50)
SPIKE_POSITIONS = (0, 1, 15, 16, 30, 31)
SPIKE_W = 15
FULL_SOURCE = 7             # the background individual whose genotype the full-depth reads are drawn from
FULL_WINDOWS = 8

NAMES = ["lattice", "ladder"] + [f"lattice-M{m}" for m in LATTICE_M] + ["spike", "full-depth-15", "full-depth-16"]


def panel(rng, n_rows, n_ids=N_IDS, eps_f=1e-3):
    """Alleles [n_rows][2 n_ids] and their frequencies, as test_gpu_precision.synth draws them."""
    f = np.clip(rng.beta(0.4, 1.0, size=n_rows), eps_f, 0.999)
    return (rng.random((n_rows, 2 * n_ids)) < f[:, None]).astype(np.uint8), f


def lattice_rows(max_cov):
    """(n_ref, n_alt) of every pair with 1 <= n_ref + n_alt <= max_cov, by depth, then by n_alt."""
    pairs = [(d - a, a) for d in range(1, max_cov + 1) for a in range(d + 1)]
    return np.array(pairs, dtype=np.int64)


def spike_alts(depth):
    """n_alt of the spike rows of one depth, in turn.  From depth 8 on the last one has 7 in its low three bits: more than
    the depth's unless those are 7 as well (15, 31), so that the three-bit subtraction cov - alt of the IBD1 form
    (sliced_diff, ibdg_ld_images.hip) borrows out of plane 2 and the higher planes have to make it up."""
    alts = [0, depth, 1, depth - 1, depth // 2]
    if depth >= 8:
        alts.append((depth & ~7) - 1)
    return alts


def borrows(cov, alt):
    """Rows whose low three bits of n_alt exceed those of the depth, with planes above them: sliced_diff's borrow out of bit 2
    where the true difference is not negative."""
    cov, alt = np.asarray(cov, dtype=np.int64), np.asarray(alt, dtype=np.int64)
    return (cov >= 8) & ((alt & 7) > (cov & 7))


def _lattice(seed, max_cov, shuffle, min_rows=0):
    rng = np.random.default_rng(seed)
    rows = lattice_rows(max_cov)
    rows = np.tile(rows, (max(1, -(-min_rows // len(rows))), 1))
    if shuffle:
        rows = rows[rng.permutation(len(rows))]
    alle, _ = panel(rng, len(rows))
    return alle, rows[:, 0], rows[:, 1]


def _spike(seed):
    rng = np.random.default_rng(seed)
    n_tiles = len(SPIKE_DEPTHS) * len(SPIKE_POSITIONS)
    alle, f = panel(rng, 32 * n_tiles)
    cov = np.minimum(rng.poisson(1.0, size=32 * n_tiles), 3)
    na = rng.binomial(cov, f)
    for k in range(n_tiles):
        d = SPIKE_DEPTHS[k // 6]
        alts = spike_alts(d)
        row = 32 * k + SPIKE_POSITIONS[k % 6]
        cov[row], na[row] = d, alts[(k // 6 + k % 6) % len(alts)]
    return alle, cov - na, na


def _full_depth(seed, W, target):
    rng = np.random.default_rng(seed)
    n_rows = 5 * W * FULL_WINDOWS
    alle, _ = panel(rng, n_rows)
    alle[:, 2 * target] = alle[:, 2 * FULL_SOURCE]
    g = alle[:, 2 * FULL_SOURCE].astype(np.int64) + alle[:, 2 * FULL_SOURCE + 1]
    cov = np.where(np.arange(n_rows) % 5 == 2, MAX_COV, 0)
    na = rng.binomial(cov, np.array([EPS, 0.5, 1 - EPS])[g])
    return alle, cov - na, na


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The case's inputs (shared: leave them unchanged)."""
    seed = 9000 + NAMES.index(name)
    M, W, target = MAX_COV, 3, 5
    if name == "lattice":
        alle, nr, na = _lattice(seed, MAX_COV, True)
    elif name == "ladder":
        alle, nr, na = _lattice(seed, MAX_COV, False)
    elif name.startswith("lattice-M"):
        M = int(name[len("lattice-M"):])
        alle, nr, na = _lattice(seed, M, True, min_rows=96)
    elif name == "spike":
        W = SPIKE_W
        alle, nr, na = _spike(seed)
    elif name.startswith("full-depth-"):
        W, target = int(name[len("full-depth-"):]), 70
        alle, nr, na = _full_depth(seed, W, target)
    else:
        raise ValueError(name)
    assert int((nr + na).max()) <= M and int(nr.min()) >= 0
    nr, na = nr.astype(np.uint8), na.astype(np.uint8)
    for x in (alle, nr, na):
        x.setflags(write=False)
    return dict(alle=alle, nr=nr, na=na, W=W, eps=EPS, M=M, target=target, refids=None, pu=-1, n_ids=N_IDS)


# --------------------------------------------------------------------------- what the host and k_prep_* make of a case
def segments(nr, na, W, win_rows=0):
    """The (window, 32-row tile) segments as k_prep_seg_scatter / k_prep_seg_walk build them (ibdg_prep.hip): covered row j
    belongs to window j // W and to the tile of its row -- its own panel row (win_rows = 0: row = position in the site list,
    as every test here uploads them) or the compacted layout's virtual row (j // W) win_rows + j % W --, and a segment's nc /
    na are the bit lengths of its largest depth / alt count (the `if (cov[k]) nc = k + 1` loop over the eight planes).
    Returns dict(win, tile, nc, na, rows: the panel rows of each segment), in the kernels' order."""
    cov = np.asarray(nr, dtype=np.int64) + np.asarray(na, dtype=np.int64)
    alt = np.asarray(na, dtype=np.int64)
    rows = np.flatnonzero(cov > 0)
    j = np.arange(len(rows))
    win = j // W
    row = rows if win_rows == 0 else win * win_rows + j % W
    tile = row // 32
    start = np.flatnonzero(np.r_[True, (win[1:] != win[:-1]) | (tile[1:] != tile[:-1])])
    ends = np.r_[start[1:], len(rows)]
    bitlen = lambda x: int(x).bit_length()          # noqa: E731
    return dict(win=win[start], tile=tile[start], nc=np.array([bitlen(cov[rows[a:b]].max()) for a, b in zip(start, ends)]),
                na=np.array([bitlen(alt[rows[a:b]].max()) for a, b in zip(start, ends)]),
                rows=[rows[a:b] for a, b in zip(start, ends)])


def ct_max(nr, na, W):
    """Most reads in one window (PrepInfo::ct_max)."""
    cov = np.asarray(nr, dtype=np.int64) + np.asarray(na, dtype=np.int64)
    cov = cov[cov > 0]
    return max(int(cov[i:i + W].sum()) for i in range(0, len(cov), W))


def tab_in_lds(nr, na, W):
    """As test_gpu_precision.tab_in_lds (ibdg_api.cpp: (ct_max + 1) 32 <= 24 KiB), restated so that this module needs no
    device."""
    return (ct_max(nr, na, W) + 1) * 32 <= 24 * 1024


def mfma_lds_bytes(ct, win_per_group, max_seg):
    """ld_mfma_lds_bytes (ibdg_ld_mfma.hip) for a largest window of ct reads: the host hands groups of individuals to
    k_ld_mfma only where this is at most 64 KiB (ibdg_api.cpp, next to the tab_in_lds condition); otherwise the counting
    kernels take them.  8 waves, strips of 36 doubles."""
    return win_per_group * 33 * 16 + (ct + 1) * 56 + 16 + (max_seg + 1) * 32 + 8 * 16 * 36 * 8


def mfma_takes(nr, na, W):
    """True / False where the host's choice follows from the inputs alone: the tables in LDS and ld_mfma_lds_bytes within
    64 KiB for any run length the host may settle on (1..16 windows, their segments), or beyond it for all of them."""
    if not tab_in_lds(nr, na, W):
        return False
    ct = ct_max(nr, na, W)
    seg = segments(nr, na, W)
    per_win = int(np.bincount(seg["win"]).max())
    if mfma_lds_bytes(ct, 16, 16 * per_win) <= 64 * 1024:
        return True
    assert mfma_lds_bytes(ct, 1, 1) > 64 * 1024, "the host's choice depends on its run length here"
    return False


@functools.lru_cache(maxsize=None)
def run_seed(name, T):
    """A seed with which test_gpu_precision.run_form, drawing T comparison individuals, draws the case's target first: the one
    whose windows the preconditions of test_depth_cases.py are asserted for."""
    c = make_case(name)
    cand = np.array([x for x in range(c["n_ids"]) if x != c["pu"]])
    for seed in range(100000):
        if int(np.random.default_rng(seed).choice(cand, size=T, replace=False)[0]) == c["target"]:
            return seed
    raise AssertionError((name, T))
