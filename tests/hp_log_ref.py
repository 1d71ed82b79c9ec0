"""Truths and bounds of the log-window table (option "log_windows"), on top of tests/hp_ref.py (unchanged).

Two truths, both in long double:
  * ld_log2_truth    --LD LIBD0 / LIBD1: log2 of hp_ref.ld_truth with the binomial factors -- the mean over the background
                     (multiplicities, the target and pu_id excluded, src/ibdgem.c:714) of the exact window products;
  * rows_log2_truth  every other column: the sum over a window's rows with reads of log2 of the fp64 per-site value.

The long double's exponent has 15 bits: a truth is valid down to 2^-16382.  test_log_ref.py asserts every truth of CASES
is above 2^-16000.

Also the cases the GPU test runs (CASES), so that the CPU tier can check their regimes without a device.
"""
import math

import numpy as np

import hp_ref as H

LD = H.LD
U = H.U
LN2 = math.log(2.0)


# --------------------------------------------------------------------------- bounds
def log_B(n_ids):
    """Roundings of k_ld_log (ibdg_ld_log.hip) on the mean of a window, counted like hp_ref.fast_B: product roundings plus
    summation depth.  A rescale by a power of two is exact (the terms it flushes lie 2^-1100 below the sum).
      products  the two table entries rounded once from long double (2), their product (1), K' (0.5 + 1 as in hp_ref), the
                multiplicity times the product (1), mK' times the sum and the division (2), the long-double tables (0.1);
      depth     the lane's four IBD1 products (3), the wave's fixed tree (6), the chunks one lane a chunk in turn over every
                64th (ceil(chunks / 64)) and the same tree again (6)."""
    return (2 + 1 + 0.5 + 1 + 1 + 2 + 0.1) + (3 + 6 + 6 + (H.chunks(n_ids) + 63) // 64)


def ld_bar(truth_log2, n_ids):
    """|got - truth| <= (B + 2) u / ln 2 + 2 u |truth|: B roundings of the mean, the library's log2 and the final addition."""
    B = log_B(n_ids)
    assert B <= 40
    return (B + 2) * U / LN2 + 2 * U * np.abs(np.asarray(truth_log2, dtype=LD))


def rows_bar(truth_log2, abs_sum):
    """|got - truth| <= 2 u sum |log2 s_i| + 2 u |truth|: a 1-ulp log2 per term with a factor of 2, a compensated sum."""
    return 2 * U * np.asarray(abs_sum, dtype=LD) + 2 * U * np.abs(np.asarray(truth_log2, dtype=LD))


# --------------------------------------------------------------------------- truths
def ld_log2_truth(alle, nr, na, target, window, eps, max_cov, refids=None, pu_id=-1):
    """dict(lin0, lin1: the linear truths of hp_ref.ld_truth; log0, log1: their log2 in long double [n_win])."""
    tr = H.ld_truth(alle, nr, na, target, window, H.binomial_factors(eps, max_cov), refids=refids, pu_id=pu_id)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(lin0=tr["ibd0"], lin1=tr["ibd1"], log0=np.log2(tr["ibd0"]), log1=np.log2(tr["ibd1"]), n_bg=tr["n_bg"])


def rows_log2_truth(site, nr, na, window):
    """site: fp64 [n_sites][k] per-site values.  (sum [n_win][k], sum of |log2| [n_win][k]) in long double."""
    wins = H.windows(nr, na, window)
    lg = np.log2(np.asarray(site, dtype=np.float64).astype(LD))
    s = np.array([lg[r].sum(axis=0) for r in wins], dtype=LD).reshape(len(wins), -1)
    a = np.array([np.abs(lg[r]).sum(axis=0) for r in wins], dtype=LD).reshape(len(wins), -1)
    return s, a


# --------------------------------------------------------------------------- inputs
def genotype_reads(seed, n_ids, n_rows, depth, max_cov, eps, related=True, target=0):
    """Uniform allele frequencies 0.05-0.95, Poisson(depth) reads per row (capped at max_cov) drawn from the genotype of
    individual `target` (related) or from an unrelated genotype of the same frequencies.  Returns alleles [rows][2 n_ids], n_ref, n_alt."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.95, size=n_rows)
    alle = (rng.random((n_rows, 2 * n_ids)) < f[:, None]).astype(np.uint8)
    g = alle[:, 2 * target] + alle[:, 2 * target + 1] if related else (rng.random((n_rows, 2)) < f[:, None]).sum(axis=1)
    cov = np.minimum(rng.poisson(depth, size=n_rows), max_cov)
    p_alt = np.array([eps, 0.5, 1 - eps])[g]
    na = rng.binomial(cov, p_alt).astype(np.uint8)
    return alle, (cov - na).astype(np.uint8), na


def issue_inputs(depth, related):
    """The inputs the regimes of this table were stated for: 130 individuals, 1500 rows, eps 0.02, -M 50, W 100, seed 1."""
    return genotype_reads(1, 130, 1500, depth, 50, 0.02, related)


def spread_inputs(n_ids, window, one_above):
    """Every individual homozygous alternative except (one_above) individual 70, homozygous reference; three reference reads
    on every row: 300 reads per window of 100, rho = eps / (1 - eps) = 2^-5.6 at eps 0.02 -- the one individual's products lie
    about 1680 binades above all the others'.  Without it all individuals are equal."""
    n_rows = 3 * window + window // 2
    alle = np.ones((n_rows, 2 * n_ids), dtype=np.uint8)
    if one_above:
        alle[:, 140:142] = 0
    return alle, np.full(n_rows, 3, dtype=np.uint8), np.zeros(n_rows, dtype=np.uint8)


N_ROWS = 1500
DEPTHS = {2: 20, 30: 50}            # mean depth -> -M


def _bg(kind, n_ids, target, rng):
    """refids (None: everybody) and pu_id of a background kind."""
    if kind == "all":
        return None, -1
    if kind == "mult":               # a -B list with multiplicities 0-3, the target inside
        m = rng.integers(0, 4, size=n_ids)
        m[target] = 2
        return np.repeat(np.arange(n_ids), m), -1
    if kind == "mult_out":           # ... the target outside, pu_id set
        m = rng.integers(0, 4, size=n_ids)
        m[target] = 0
        return np.repeat(np.arange(n_ids), m), (target + 1) % n_ids
    if kind == "pu":
        return None, (target + 3) % n_ids
    if kind == "one":
        return np.array([(target + 1) % n_ids]), -1
    if kind == "empty":
        return np.array([target]), -1
    if kind == "chunk0":             # a whole chunk (individuals 64-127) with weight 0
        return np.array([i for i in range(n_ids) if not 64 <= i < 128]), -1
    raise ValueError(kind)


def make_case(name):
    """name -> dict(alle, nr, na, W, eps, M, target, refids, pu, depth)."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    target = c.get("target", 0)
    if c.get("spread") is not None:
        alle, nr, na = spread_inputs(c["n_ids"], c["W"], c["spread"])
    else:
        alle, nr, na = genotype_reads(c["seed"], c["n_ids"], N_ROWS, c["depth"], DEPTHS[c["depth"]], c["eps"], c.get("related", True), target)
    refids, pu = _bg(c.get("bg", "all"), c["n_ids"], target, rng)
    return dict(alle=alle, nr=nr, na=na, W=c["W"], eps=c["eps"], M=DEPTHS[c["depth"]], target=target, refids=refids, pu=pu,
                depth=c["depth"], n_ids=c["n_ids"], spread=c.get("spread"))


CASES = {}
_combo = [(0.02, 2), (0.001, 30), (0.02, 30), (0.001, 2)]
_k = 0
for _n in (5, 64, 130, 700):        # a partial chunk, an exact one, three with a two-lane tail, more than a workgroup's waves
    for _w in (2, 33, 100):         # windows straddle the 32-row tiles; 1500 rows leave a short last one
        _e, _d = _combo[_k % 4]
        CASES[f"N{_n}-W{_w}-e{_e}-d{_d}"] = dict(n_ids=_n, W=_w, eps=_e, depth=_d, seed=100 + _k, target=_k % _n)
        _k += 1
for _i, _b in enumerate(("mult", "mult_out", "pu", "one", "empty", "chunk0")):
    for _d in (2, 30):
        CASES[f"bg-{_b}-d{_d}"] = dict(n_ids=130, W=100, eps=0.02, depth=_d, seed=200 + 2 * _i + (_d == 30), target=5 + 60 * (_i % 2), bg=_b)
CASES["N700-W100-e0.02-d30"] = dict(n_ids=700, W=100, eps=0.02, depth=30, seed=120, target=699)
CASES["spread-one-above"] = dict(n_ids=130, W=100, eps=0.02, depth=2, seed=300, target=3, spread=True)
CASES["spread-all-equal"] = dict(n_ids=130, W=100, eps=0.02, depth=2, seed=301, target=3, spread=False)
CASES["unrelated-d30"] = dict(n_ids=130, W=100, eps=0.02, depth=30, seed=302, target=0, related=False)
