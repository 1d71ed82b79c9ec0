"""Extended-precision reference of the --LD window columns, and the error bounds the kernels are held to.

What it computes is what oracle/ibd_oracle.c's orc_compare computes for the two --LD columns (src/ibdgem.c:669-759):
per window of `window` rows with reads, for every background individual the product over the window's rows of its own
genotype factor (IBD0) and of the four target-haplotype x own-haplotype factors (IBD1), then the means over the
background.  It does so in np.longdouble (a 64-bit mantissa on x86-64), multiplying PER-ROW FACTORS: none of the
kernels' algebra (rho, sigma, K', exponent counting) is used, so it cannot share their mistakes.

Two truths:
  * table truth     -- the factors are the reference's fp64 P(D|G) entries (orc_pDgG, DBL_MIN clamp included),
                       exactly; the error left is that of the products and sums;
  * binomial truth  -- every factor is C (1-e)^r e^a, C 2^-(r+a) or C (1-e)^a e^r in long double, from the doubles
                       `eps` and `(double)(1 - eps)` the engine and the reference both start from.

The truths' own error: a product of W factors is taken as a balanced tree inside blocks of 32 rows and serially over
the blocks (at most 5 + W/32 roundings of 2^-64), the sums by numpy's pairwise summation -- below 0.02 of a double's
unit roundoff for W <= 1024 and any background, which the bounds below do not need to count.
"""
import math

import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, \
    "hp_ref needs an 80-bit long double (64-bit mantissa); this platform's np.longdouble is narrower"

LD = np.longdouble
U = 2.0 ** -53                     # unit roundoff of a double (round to nearest)
TINY = LD(2.0) ** -1074            # smallest subnormal
ROW_BLOCK = 32


# --------------------------------------------------------------------------- per-row factors
def binomial_factors(eps, max_cov):
    """f[r, a, g] for r + a <= max_cov: the P(D|G) factors in long double (src/ibd-math.c:57-70), from the doubles the
    reference multiplies with: eps and (double)(1 - eps).  f[0, 0, :] = 1 (rows without reads are never multiplied)."""
    d = max_cov + 1
    e = LD(float(eps))
    q = LD(float(1 - eps))
    f = np.zeros((d, d, 3), dtype=LD)
    for r in range(d):
        for a in range(d - r):
            c = LD(math.comb(r + a, r))
            f[r, a, 0] = c * q ** r * e ** a
            f[r, a, 1] = np.ldexp(c, -(r + a))
            f[r, a, 2] = c * q ** a * e ** r
    f[0, 0, :] = 1
    return f


def table_factors(pdg, max_cov):
    """f[r, a, g] = the fp64 entries pdg(r, a) -> (p00, p01, p11), exactly, as long doubles (pdg: e.g. the oracle's
    orc_pDgG, clamp included)."""
    d = max_cov + 1
    f = np.ones((d, d, 3), dtype=LD)
    for r in range(d):
        for a in range(d - r):
            if r + a:
                f[r, a, :] = np.asarray(pdg(r, a), dtype=np.float64)
    return f


# --------------------------------------------------------------------------- windows
def windows(n_ref, n_alt, window):
    """Row indices of every window: rows with reads, `window` of them at a time, in order (src/ibdgem.c:572-730); the
    last window may be short."""
    cov = np.asarray(n_ref, dtype=np.int64) + np.asarray(n_alt, dtype=np.int64)
    rows = np.flatnonzero(cov > 0)
    return [rows[i:i + window] for i in range(0, len(rows), window)]


def _prod_rows(x):
    """Product over axis 0 of a long-double array: balanced trees over blocks of ROW_BLOCK rows, the blocks serially."""
    out = np.ones(x.shape[1:], dtype=LD)
    for b in range(0, x.shape[0], ROW_BLOCK):
        y = x[b:b + ROW_BLOCK]
        while y.shape[0] > 1:
            if y.shape[0] & 1:
                y = np.concatenate([y, np.ones((1,) + y.shape[1:], dtype=LD)])
            y = y[0::2] * y[1::2]
        out = out * y[0]
    return out


def background(n_ids, target, refids=None, pu_id=-1):
    """(individual ids, multiplicities) of the background after the exclusions of src/ibdgem.c:714 (the target and the
    -N individual); duplicates in `refids` count with their multiplicity (read_rf, src/ibd-parse.c:262-308)."""
    ids = np.arange(n_ids) if refids is None else np.asarray(refids, dtype=np.int64)
    ids = ids[(ids != target) & (ids != pu_id)]
    uniq, mult = np.unique(ids, return_counts=True)
    return uniq, mult


def ld_truth(alleles, n_ref, n_alt, target, window, factors, refids=None, pu_id=-1):
    """The two --LD columns per window in long double: dict(ibd0, ibd1 [n_win] long double, rows [list of row arrays],
    reads [n_win] total reads, n_bg = background size with multiplicity).  An empty background gives NaN, like the
    reference's 0/0."""
    alleles = np.asarray(alleles, dtype=np.uint8)
    nr = np.asarray(n_ref, dtype=np.int64)
    na = np.asarray(n_alt, dtype=np.int64)
    ids, mult = background(alleles.shape[1] // 2, target, refids, pu_id)
    n_bg = int(mult.sum())
    wins = windows(nr, na, window)
    ibd0 = np.empty(len(wins), dtype=LD)
    ibd1 = np.empty(len(wins), dtype=LD)
    w = mult.astype(LD)
    for k, rows in enumerate(wins):
        if n_bg == 0:
            ibd0[k] = ibd1[k] = LD(np.nan)
            continue
        fr = factors[nr[rows], na[rows]]                         # [rows][3]
        h0 = alleles[rows][:, 2 * ids].astype(np.int64)         # [rows][bg]
        h1 = alleles[rows][:, 2 * ids + 1].astype(np.int64)
        t0 = alleles[rows, 2 * target].astype(np.int64)[:, None]
        t1 = alleles[rows, 2 * target + 1].astype(np.int64)[:, None]
        pick = lambda g: np.take_along_axis(fr, g, axis=1)      # noqa: E731  factor of class g per row and individual
        own = _prod_rows(pick(h0 + h1))
        cross = sum(_prod_rows(pick(t + h)) for t in (t0, t1) for h in (h0, h1))
        ibd0[k] = np.sum(w * own) / n_bg
        ibd1[k] = np.sum(w * cross) / (4 * n_bg)
    reads = np.array([int((nr[r] + na[r]).sum()) for r in wins], dtype=np.int64)
    return dict(ibd0=ibd0, ibd1=ibd1, rows=wins, reads=reads, n_bg=n_bg)


# --------------------------------------------------------------------------- bounds
def chunks(n_ids):
    return (n_ids + 63) // 64


def sum_depth(n_ids):
    """Additions any one background term passes through on its way to a window's sum, in the fast kernels:
      3   the four IBD1 products of a lane (pairwise in the counting kernels, in turn where an individual's slots are
          added into the strip in k_ld_mfma: at most three);
      6   the fixed-order wave sum of 64 lanes (wave_sum_to_lane63 / wave_sum_lane63_only, ibdg_ld_dev.h: six dpp_add);
      3   the sums of up to eight waves or half chunks of a workgroup (k_ld_popcount_mt's waves, k_ld_mfma's
          mfma_wg_sum groups of eight half chunks, ibdg_ld_mfma.hip);
      6 + ceil(n_chunks / 64) - 1   the chunks' sums: one lane a chunk, in turn over every 64th chunk, then the same
          six-step wave tree (k_ld_finalize, k_ld_finalize_g; ibd0_from_pass, ibdg_ld_dev.h).
    Each addition of non-negative terms costs at most one unit roundoff of the sum."""
    return 3 + 6 + 3 + 6 + (chunks(n_ids) + 63) // 64


# product terms of one background individual's window value, in unit roundoffs (u = 2^-53), per fast form
PRODUCT_ROUNDINGS = {
    # rho^E2 and sigma^E3 as doubles rounded once from the long-double tables (grow_pow_tables, ibdg_api.cpp: 2), their
    # product (ld_value, ibdg_ld_dev.h: 1; the ldexp is exact above 2^-1022), K' kept in a 64-bit mantissa over the
    # window's coefficients (k_prep_win_raw: W roundings of 2^-64, <= 0.5 for W <= 1024) and rounded to a double once
    # (k_prep_win_kp: 1 + 2^-11), then mK' times the sum and the division by n_refpanel (k_ld_finalize: 2).  The
    # long-double tables themselves (me_powl: about 2 log2(n) roundings of 2^-64) add < 0.02.
    "popcount": 2 + 1 + 0.5 + 1 + 2 + 0.1,
    # k_ld_popcount_mt: the same tables and products (the counts differ in where they are taken, not in what is multiplied)
    "popcount_mt": 2 + 1 + 0.5 + 1 + 2 + 0.1,
    # k_ld_mfma: V_x and U_t as products of two table mantissas each (ds_read of r/s entries, ibdg_ld_mfma.hip: 2 entries
    # + 1 product), times the individual's multiplicity (wgt: 1), the tau^G entry and its product (2), the rescale to the
    # wave's eRef (an exact power of two above 2^-1022), then K' and the window end as above (0.5 + 1 + 2)
    "mfma": 2 + 1 + 1 + 2 + 0.5 + 1 + 2 + 0.1,
}

# absolute part, in units of 2^-1074: a term's ldexp into the subnormals rounds once (0.5, kept by the mean over the
# background), the multiplication by mK' (0.5) and the division by n_refpanel (0.5) once each
FAST_A = 1.5


def fast_B(form, n_ids):
    """B of the fast forms against the binomial truth: product roundings + summation depth (no W in it: the exponents
    are exact integers whatever the window's length)."""
    return PRODUCT_ROUNDINGS[form] + sum_depth(n_ids)


def strict_B(variant, n_rows, n_bg, n_ids):
    """B of the strict forms against the table truth.  Each background individual's product is a running product of
    fp64 factors in row order (n_rows - 1 roundings), then:
      variant 1 (tree): the fast forms' summation depth, and the final division (1);
      variant 3 (reference order, the oracle's own arithmetic): the IBD1 four-term sum (3), the serial background sum
                        (n_bg - 1) and the division (1)."""
    if variant == 1:
        return (n_rows - 1) + sum_depth(n_ids) + 1
    return (n_rows - 1) + 3 + (n_bg - 1) + 1


def strict_A(n_rows):
    """Absolute part of the strict forms, in units of 2^-1074: once a running product is subnormal every further
    multiplication rounds by up to half a subnormal step (n_rows), and the division (1)."""
    return n_rows + 1


def excess(got, truth, B, A):
    """|got - t| / (B u t + A 2^-1074) per element, in long double (NaN where both are NaN; inf where only one is)."""
    g = np.asarray(got, dtype=np.float64).astype(LD)
    t = np.asarray(truth, dtype=LD)
    bound = LD(B) * LD(U) * np.abs(t) + LD(A) * TINY
    both_nan = np.isnan(g) & np.isnan(t)
    with np.errstate(invalid="ignore"):
        r = np.abs(g - t) / bound
    r = np.where(both_nan, LD(0), r)
    r = np.where(np.isnan(g) != np.isnan(t), LD(np.inf), r)
    return r


def check(got, truth, B, A, what):
    """Assert every |got - t| <= B u t + A 2^-1074; return the largest ratio to the bound."""
    r = excess(got, truth, B, A)
    worst = float(np.max(r)) if r.size else 0.0
    if worst > 1.0:
        i = int(np.argmax(r))
        g = float(np.asarray(got, dtype=np.float64).ravel()[i])
        t = np.asarray(truth, dtype=LD).ravel()[i]
        raise AssertionError(f"{what}: {int((r > 1).sum())}/{r.size} beyond B={B:.1f} u, A={A} (worst ratio "
                             f"{worst:.3g} at {i}: got {g!r}, truth {t!r})")
    return worst


BANDS = {                            # the ranges of a window value where underflow behaviour shows
    "1e-300..1e-290": (LD("1e-300"), LD("1e-290")),
    "2^-1022..1e-300": (LD(2.0) ** -1022, LD("1e-300")),
    "subnormal": (TINY, LD(2.0) ** -1022),
    "below 2^-1075": (LD(0), LD(2.0) ** -1075),
}


def band_counts(truth):
    t = np.asarray(truth, dtype=LD)
    t = t[~np.isnan(t)]
    return {k: int(((t >= lo) & (t < hi)).sum()) for k, (lo, hi) in BANDS.items()}
