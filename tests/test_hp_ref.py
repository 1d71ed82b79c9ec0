"""CPU tier of the extended-precision reference (tests/hp_ref.py): it computes the operation the oracle computes, its
two truths differ by what the table's roundings allow, and the fast kernels' bound is tight enough to catch what the
1e-10 parity bar lets through -- the oracle's own accumulated roundings, a premature 0, a few bounds' worth of ulps."""
import math

import numpy as np
import pytest

import hp_ref as H

LD = H.LD
EPSES = (0.001, 0.02, 0.2, 0.49)
# one fp64 P(D|G) entry (orc_pDgG): C exact (< 2^53 for M <= 50), two glibc pow calls (< 1 ulp = 2 u each), two products
ENTRY_U = 2 + 2 + 2


def test_long_double_has_a_64_bit_mantissa():
    assert np.finfo(np.longdouble).nmant >= 63
    assert LD(1) + LD(2.0) ** -63 != LD(1)


def _table(oracle, eps, M):
    return H.table_factors(lambda r, a: oracle.pdg(eps, M, r, a), M)


@pytest.mark.parametrize("eps", EPSES)
@pytest.mark.parametrize("M", [1, 20, 50])
def test_table_entries_are_within_a_few_ulps_of_the_binomial_values(oracle, eps, M):
    nck = oracle.nck(M)
    assert all(int(nck[n, k]) == math.comb(n, k) for n in range(M + 1) for k in range(n + 1))
    tab, bino = _table(oracle, eps, M), H.binomial_factors(eps, M)
    r, a = np.meshgrid(np.arange(M + 1), np.arange(M + 1), indexing="ij")
    ok = (r + a >= 1) & (r + a <= M)
    t, b = tab[ok], bino[ok]
    assert (t > 0).all() and (b >= LD(2.0) ** -1022).all()     # no entry of these is clamped or subnormal
    ulps = np.abs(t - b) / b / LD(H.U)
    print(f"eps={eps} M={M}: largest entry error {float(ulps.max()):.2f} u")
    assert float(ulps.max()) <= ENTRY_U


def _case(seed, N, L, cov, M, f_lo=1e-3):
    rng = np.random.default_rng(seed)
    f = np.clip(rng.beta(0.4, 1.0, size=L), f_lo, 0.999)
    alle = (rng.random((L, 2 * N)) < f[:, None]).astype(np.uint8)
    c = np.minimum(rng.poisson(cov, size=L), M)
    na = rng.binomial(c, f).astype(np.uint8)
    return alle, (c - na).astype(np.uint8), na


CASES = [  # seed, N, L, W, eps, M, cov, background
    (1, 2, 300, 33, 0.02, 20, 2.0, None),
    (2, 65, 700, 100, 0.02, 20, 3.0, "dup"),
    (3, 129, 600, 257, 0.001, 50, 14.0, None),
    (4, 300, 500, 2, 0.2, 7, 3.0, "dup"),
    (5, 2504, 260, 100, 0.49, 20, 2.0, None),
    (6, 64, 1100, 1024, 0.02, 20, 4.0, None),
]


def _refids(kind, N, seed):
    if kind is None:
        return None
    rng = np.random.default_rng(seed)
    return rng.permutation(np.repeat(np.arange(N), rng.integers(0, 3, size=N)))


@pytest.mark.parametrize("seed,N,L,W,eps,M,cov,bg", CASES)
def test_the_oracle_is_within_its_serial_bound_of_the_table_truth(oracle, seed, N, L, W, eps, M, cov, bg):
    """The oracle's windows lie within (W + n_bg + c) u of hp_ref's table truth (plus what a running product loses in the
    subnormals): hp_ref computes the oracle's operation, window bounds, exclusions and multiplicities included."""
    alle, nr, na = _case(seed, N, L, cov, M)
    refids = _refids(bg, N, seed)
    target, pu = N - 1, (0 if N > 2 else -1)
    res = oracle.compare(alle, nr, na, target, window=W, eps=eps, max_cov=M, refids=refids, pu_id=pu)
    tr = H.ld_truth(alle, nr, na, target, W, _table(oracle, eps, M), refids=refids, pu_id=pu)
    assert len(tr["rows"]) == len(res["win"])
    assert [int(r[0]) for r in tr["rows"]] == list(res["first"])
    assert [int(r[-1]) for r in tr["rows"]] == list(res["last"])
    worst = 0.0
    for k, rows in enumerate(tr["rows"]):
        B, A = H.strict_B(3, len(rows), tr["n_bg"], N), H.strict_A(len(rows))
        for col, key in ((0, "ibd0"), (1, "ibd1")):
            worst = max(worst, H.check(res["win"][k:k + 1, col], tr[key][k:k + 1], B, A, f"window {k} {key}"))
    print(f"N={N} W={W} eps={eps}: oracle / serial bound <= {worst:.3f}")


@pytest.mark.parametrize("seed,N,L,W,eps,M,cov,bg", CASES)
def test_table_and_binomial_truths_differ_by_the_entries_roundings(oracle, seed, N, L, W, eps, M, cov, bg):
    alle, nr, na = _case(seed, N, L, cov, M)
    refids = _refids(bg, N, seed)
    tt = H.ld_truth(alle, nr, na, 0, W, _table(oracle, eps, M), refids=refids)
    bt = H.ld_truth(alle, nr, na, 0, W, H.binomial_factors(eps, M), refids=refids)
    for key in ("ibd0", "ibd1"):
        for k, rows in enumerate(tt["rows"]):
            t, b = tt[key][k], bt[key][k]
            assert abs(t - b) <= (len(rows) * ENTRY_U + 1) * LD(H.U) * b, (key, k)


def test_the_bound_of_the_fast_forms(oracle):
    """Where the reference's roundings accumulate -- 1024 identical rows with four reference reads, a homozygous-reference
    panel of 2504 individuals: every product is p00^1024 taken in 1023 multiplications, then 2503 of them added in turn
    -- the oracle is hundreds of u from the truth: inside its own serial bound, outside the fast forms' one."""
    N, W, eps, M = 2504, 1024, 0.02, 20
    alle = np.zeros((W, 2 * N), dtype=np.uint8)
    nr, na = np.full(W, 4, np.uint8), np.zeros(W, np.uint8)
    res = oracle.compare(alle, nr, na, 0, window=W, eps=eps, max_cov=M)
    bt = H.ld_truth(alle, nr, na, 0, W, H.binomial_factors(eps, M))
    tt = H.ld_truth(alle, nr, na, 0, W, _table(oracle, eps, M))
    got, t = res["win"][:, 0], bt["ibd0"]
    B = H.fast_B("popcount", N)
    r = float(H.excess(got, t, B, H.FAST_A)[0])
    print(f"oracle vs binomial truth: {r:.1f} x the fast bound (B = {B:.1f} u)")
    with pytest.raises(AssertionError, match="beyond"):
        H.check(got, t, B, H.FAST_A, "oracle, identical rows")
    H.check(got, tt["ibd0"], H.strict_B(3, W, N - 1, N), H.strict_A(W), "oracle within its serial bound")

    # a 0 where the truth is 1e-300, a value in the subnormals off by a few steps, a value a few bounds off
    t = np.array([LD("1e-300")], dtype=LD)
    with pytest.raises(AssertionError):
        H.check([0.0], t, B, H.FAST_A, "premature 0")
    t = np.array([LD(2.0) ** -1070], dtype=LD)
    H.check([2.0 ** -1070], t, B, H.FAST_A, "subnormal exact")
    with pytest.raises(AssertionError):
        H.check([2.0 ** -1070 + 2 * 2.0 ** -1074], t, B, H.FAST_A, "subnormal two steps off")
    H.check([0.0], np.array([LD(2.0) ** -1075], dtype=LD), B, H.FAST_A, "below half the smallest subnormal: 0")
    t = np.array([LD("0.37") * LD(2.0) ** -200], dtype=LD)
    for k, fails in ((B - 0.5, False), (B + 1, True), (3 * B, True)):
        g = float(t[0] * (1 + LD(k) * LD(H.U)))
        if fails:
            with pytest.raises(AssertionError):
                H.check([g], t, B, H.FAST_A, f"{k} u off")
        else:
            H.check([g], t, B, H.FAST_A, f"{k} u off")
