"""Every --LD kernel form against the extended-precision reference (tests/hp_ref.py).

The parity bar of test_gpu_parity.py (1e-10 relative against the oracle, "both below 1e-290" equal) is the bar of the
reference's text.  Here each form is held to the bound its own arithmetic allows:
  * fast forms (k_ld_popcount and its forms, k_ld_popcount_mt, k_ld_mfma) against the BINOMIAL truth:
        |got - t| <= B u t + A 2^-1074,  B = hp_ref.fast_B(form, N) -- no W in it --, A = hp_ref.FAST_A;
  * strict forms (ld_variant 1, and 3 = the reference's order) against the TABLE truth with hp_ref.strict_B/strict_A.
Every case keeps the parity checks as well (per-row values and LIBD2 bit for bit, --LD within 1e-10 of the oracle; the
reference order bit for bit), shows through the C ABI which form ran, and the underflow cases assert the bands of
hp_ref.BANDS they reach, so the coverage cannot quietly vanish.
"""
import math

import numpy as np
import pytest

import hp_ref as H
from ibdgem_amd import engine as E
from test_gpu_parity import assert_bits, assert_ld_close, bg_counts

pytestmark = pytest.mark.gpu

_SINGLE = dict(ld_variant=2, mfma_targets=0, multi_target=0, ibd0_after=0, compact_tiles=-1)
# name -> options, comparison individuals, expected ibdg_last_ld_variant / ibdg_last_count_unit / ibdg_ld_layout (None:
# not asserted), bound
FORMS = {
    "popcount mx1": dict(opts=dict(_SINGLE, mx_counts=1), T=1, variant=2, unit=2, layout=1, hp="popcount"),
    "popcount mx0": dict(opts=dict(_SINGLE, mx_counts=0), T=1, variant=2, unit=1, layout=1, hp="popcount"),
    "popcount IBD1 form": dict(opts=dict(_SINGLE, ibd0_after=1), T=1, variant=2, unit=3, layout=1, hp="popcount"),
    "popcount compacted": dict(opts=dict(_SINGLE, compact_tiles=1), T=1, variant=2, unit=2, layout=2, hp="popcount"),
    # groups of four in one workgroup: no single-individual launch is left (count unit 0) at T = 4, one at T = 9
    "popcount_mt T4": dict(opts=dict(ld_variant=2, mfma_targets=0, multi_target=1, compact_tiles=-1), T=4, variant=2,
                           unit=0, layout=1, hp="popcount_mt"),
    "popcount_mt T9": dict(opts=dict(ld_variant=2, mfma_targets=0, multi_target=1, compact_tiles=-1), T=9, variant=2,
                           unit=(2, 3), layout=1, hp="popcount_mt"),
    "strict tree": dict(opts=dict(ld_variant=1), T=1, variant=1, unit=0, layout=None, hp=1),
    "strict reference order": dict(opts=dict(ld_variant=3), T=1, variant=3, unit=0, layout=None, hp=3),
}
# groups of 15 through the matrix cores (mfma_min 4): T = 5 and 15 leave nothing to the counting kernels (count unit 0),
# T = 16 and 31 one individual each (a single launch: count unit 2, or 3 where it takes the IBD1 form)
for _T in (5, 15, 16, 31):
    for _tau in (0, 1):
        FORMS[f"mfma T{_T} tau{_tau}"] = dict(opts=dict(ld_variant=2, mfma_targets=1, multi_target=1, mfma_plain_tau=_tau,
                                                        compact_tiles=-1),
                                              T=_T, variant=2, unit=0 if _T in (5, 15) else (2, 3), layout=1, hp="mfma")
SINGLE_FORMS = [f for f, s in FORMS.items() if s["T"] == 1]
GROUP_FORMS = [f for f, s in FORMS.items() if s["T"] > 1]
# The forms on the route a context takes when no option is set (tests/route_cases.py), for tests/test_gpu_default_route.py:
# the same schema, kept apart from FORMS, whose item lists stay as they are.  The first one is the instantiation bench.py times.
ROUTE_FORMS = {
    "popcount IBD1 compacted": dict(opts=dict(_SINGLE, ibd0_after=1, compact_tiles=1), T=1, variant=2, unit=3, layout=2,
                                    hp="popcount"),
    "popcount_mt compacted T9": dict(opts=dict(ld_variant=2, mfma_targets=0, multi_target=1, compact_tiles=1), T=9, variant=2,
                                     unit=(2, 3), layout=2, hp="popcount_mt"),
}
for _tau in (0, 1):
    ROUTE_FORMS[f"mfma compacted T16 tau{_tau}"] = dict(opts=dict(FORMS[f"mfma T16 tau{_tau}"]["opts"], compact_tiles=1), T=16,
                                                        variant=2, unit=(2, 3), layout=2, hp="mfma")
# no option at all: the layout is the upload's own choice (2 for a sparse list: the caller says which), the first run counts everything
ROUTE_FORMS["defaults T1"] = dict(opts={}, T=1, variant=2, unit=2, layout=(1, 2), hp="popcount")
ROUTE_FORMS["defaults T16"] = dict(opts={}, T=16, variant=2, unit=(2, 3), layout=(1, 2), hp="mfma")

WORST = {}          # (form, window value normal) -> largest |got - t| / bound
BANDS_HIT = {}      # form -> band -> windows


def _truth_factors(oracle, form, eps, M):
    if isinstance((FORMS.get(form) or ROUTE_FORMS[form])["hp"], str):
        return H.binomial_factors(eps, M)
    return H.table_factors(lambda r, a: oracle.pdg(eps, M, r, a), M)


def run_form(oracle, form, alle, nr, na, W, eps, M, *, refids=None, pu=-1, seed=0, expect=None, spec=None, keep=None, rows=None,
             targets=None, checked=None):
    """One run of `form`; the parity checks and the bound on three of its comparison individuals.  Returns the truths;
    `keep` (a dict) receives the comparison individuals and the window tables of the checked ones.  `rows`: the row_index to
    upload (nr, na per site of it) instead of np.arange(L); the oracle and hp_ref then get the panel rows alle[rows].
    `targets`: the form's T comparison individuals instead of a draw by `seed`; `checked`: the positions among them to check
    instead of the first, the middle and the last one."""
    spec = spec or FORMS[form]
    L, N = alle.shape[0], alle.shape[1] // 2
    T = spec["T"]
    if targets is None:
        rng = np.random.default_rng(seed)
        cand = np.array([x for x in range(N) if x != pu])
        targets = [int(x) for x in rng.choice(cand, size=T, replace=False)]
    targets = [int(x) for x in targets]
    assert len(targets) == T
    with E.Engine(0, eps, M) as eng:
        for k, v in spec["opts"].items():
            eng.set_option(k, v)
        eng.upload_panel(E.pack_alleles_fast(alle), N)
        eng.upload_sites(np.arange(L) if rows is None else rows, nr, na, W)
        if spec["variant"] == 3:
            eng.set_background_order(refids if refids is not None else np.arange(N))
        eng.run(targets, ld=True, bg_count=bg_counts(refids, N), pu_id=pu)
        got = dict(variant=eng.last_ld_variant(), unit=eng.last_count_unit(), layout=eng.ld_layout())
        want = {"variant": spec["variant"], "unit": spec["unit"], "layout": spec["layout"], **(expect or {})}
        for k, v in want.items():
            if v is not None:
                assert got[k] in (v if isinstance(v, tuple) else (v,)), f"{form}: {k} {got[k]}, expected {v}"
        checked = sorted({0, T // 2, T - 1}) if checked is None else sorted(checked)
        out = {i: (eng.site_ll(i), eng.window_ll(i)) for i in checked}
    if keep is not None:
        keep.update(targets=targets, windows={i: out[i][1] for i in checked})
    fac = _truth_factors(oracle, form, eps, M)
    if rows is not None:
        alle = alle[rows]
    truths = []
    for i in checked:
        t = targets[i]
        site, win = out[i]
        res = oracle.compare(alle, nr, na, t, window=W, eps=eps, max_cov=M, refids=refids, pu_id=pu)
        assert_bits(site, res["site"], f"{form} t={t} per-row values")
        assert_bits(win[:, 2], res["win"][:, 2], f"{form} t={t} LIBD2")
        if spec["variant"] == 3:
            assert_bits(win, res["win"], f"{form} t={t} reference order")
        else:
            assert_ld_close(win[:, :2], res["win"][:, :2], f"{form} t={t} LD vs oracle")
        tr = H.ld_truth(alle, nr, na, t, W, fac, refids=refids, pu_id=pu)
        assert len(tr["rows"]) == len(win)
        for k, rows in enumerate(tr["rows"]):
            if isinstance(spec["hp"], str):
                B, A = H.fast_B(spec["hp"], N), H.FAST_A
            else:
                B, A = H.strict_B(spec["hp"], len(rows), tr["n_bg"], N), H.strict_A(len(rows))
            for col, key in ((0, "ibd0"), (1, "ibd1")):
                r = H.check(win[k:k + 1, col], tr[key][k:k + 1], B, A, f"{form} N={N} W={W} eps={eps} t={t} "
                                                                        f"window {k} {key}")
                normal = tr[key][k] >= H.LD(2.0) ** -1022
                WORST[form, normal] = max(WORST.get((form, normal), 0.0), r)
        hit = BANDS_HIT.setdefault(form, {b: 0 for b in H.BANDS})
        for key in ("ibd0", "ibd1"):
            for b, n in H.band_counts(tr[key]).items():
                hit[b] += n
        truths.append(tr)
    return truths


# --------------------------------------------------------------------------- shapes
def synth(seed, N, L, cov, M, eps_f=1e-3):
    rng = np.random.default_rng(seed)
    f = np.clip(rng.beta(0.4, 1.0, size=L), eps_f, 0.999)
    alle = (rng.random((L, 2 * N)) < f[:, None]).astype(np.uint8)
    c = np.minimum(rng.poisson(cov, size=L), M)
    na = rng.binomial(c, f).astype(np.uint8)
    return alle, (c - na).astype(np.uint8), na


# N: chunks of 64 and half chunks of 32 on both sides of their edges; N = 2 leaves a background of one.  L: two whole
# windows and a short last one.
SHAPES = [  # N, W, eps, M, cov, background
    (2, 33, 0.02, 20, 2.0, None),
    (63, 3, 0.2, 7, 3.0, "dup"),
    (64, 32, 0.02, 20, 3.0, None),
    (65, 257, 0.001, 50, 14.0, "dup"),
    (129, 100, 0.49, 20, 2.0, None),
    (129, 2, 0.02, 20, 2.0, "dup"),
    (64, 1024, 0.02, 20, 2.0, None),
    (2504, 100, 0.02, 20, 2.0, "dup"),
]


def _shape_case(i):
    N, W, eps, M, cov, bg = SHAPES[i]
    L = 2 * W + W // 2 + 1
    alle, nr, na = synth(300 + i, N, L, cov, M)
    refids = pu = None
    if bg == "dup":
        rng = np.random.default_rng(400 + i)
        refids = rng.permutation(np.repeat(np.arange(N), rng.integers(0, 3, size=N)))
    pu = N - 1 if N > 2 else -1
    return alle, nr, na, W, eps, M, refids, pu


def tab_in_lds(nr, na, W):
    """The host keeps the power tables in LDS when the largest window's reads ct_max satisfy (ct_max + 1) 32 <= 24 KiB
    (ibdg_api.cpp, tab_in_lds); k_ld_mfma and the IBD1 form need that."""
    cov = (nr.astype(np.int64) + na)[(nr.astype(np.int64) + na) > 0]
    ct = max(int(cov[i:i + W].sum()) for i in range(0, len(cov), W))
    return (ct + 1) * 32 <= 24 * 1024


@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=[f"N{s[0]}-W{s[1]}-e{s[2]}" for s in SHAPES])
def test_single_individual_forms_at_every_shape(oracle, shape):
    alle, nr, na, W, eps, M, refids, pu = _shape_case(shape)
    for form in SINGLE_FORMS:
        spec = FORMS[form]
        expect = None
        if form == "popcount IBD1 form":
            # (the IBD1 form needs the tables in LDS)
            expect = dict(unit=3 if tab_in_lds(nr, na, W) else (2, 3))
        run_form(oracle, form, alle, nr, na, W, eps, M, refids=refids, pu=pu, seed=shape, expect=expect, spec=spec)


@pytest.mark.parametrize("shape", [1, 2, 3, 4, 7], ids=[f"N{SHAPES[i][0]}-W{SHAPES[i][1]}" for i in (1, 2, 3, 4, 7)])
def test_group_forms_at_every_shape(oracle, shape):
    alle, nr, na, W, eps, M, refids, pu = _shape_case(shape)
    for form in GROUP_FORMS:
        if FORMS[form]["T"] >= alle.shape[1] // 2 - 1:
            continue
        if FORMS[form]["hp"] == "mfma" and not tab_in_lds(nr, na, W):
            continue            # (k_ld_mfma reads its tables from LDS only: the counting kernels take such runs)
        run_form(oracle, form, alle, nr, na, W, eps, M, refids=refids, pu=pu, seed=shape)


def test_strict_fallbacks(oracle):
    """M = 51 (beyond the exact coefficients) and an epsilon whose table is clamped to DBL_MIN (src/ibd-math.c:77-79):
    the automatic choice takes the strict kernel -- no fast form ran (count unit 0) -- and it holds its bound."""
    auto = dict(opts={}, T=1, variant=1, unit=0, layout=None, hp=1)
    alle, nr, na = synth(61, 90, 260, 20.0, 51)
    run_form(oracle, "strict tree", alle, nr, na, 100, 0.02, 51, spec=auto)
    alle, nr, na = synth(62, 90, 260, 2.0, 20)
    run_form(oracle, "strict tree", alle, nr, na, 100, 1e-30, 20, spec=auto)


# --------------------------------------------------------------------------- exponent-range switches
def switches(eps, ct_max):
    """The host's choice for a run whose largest window has ct_max reads (ibdg_api.cpp, the shift8 / rho_shift /
    mx_counts lines of the --LD launch, and tab_in_lds where the preparation hands over)."""
    log2_rho, log2_sigma = math.log2(eps / (1 - eps)), math.log2(0.5 / (1 - eps))
    shift8 = (ct_max + 1) * max(abs(log2_rho + 8.0), abs(log2_sigma)) <= 1000.0
    rho_shift = 8 if shift8 else round(-log2_rho)
    per_read = max(abs(log2_rho + rho_shift), abs(log2_sigma))
    tab_in_lds = (ct_max + 1) * 32 <= 24 * 1024
    mx_dropped = tab_in_lds and (ct_max + 1) * per_read > 1000.0
    return shift8, mx_dropped


def threshold(eps):
    """Largest ct_max for which shift8 holds."""
    log2_rho, log2_sigma = math.log2(eps / (1 - eps)), math.log2(0.5 / (1 - eps))
    return int(1000.0 / max(abs(log2_rho + 8.0), abs(log2_sigma))) - 1


def reads_case(seed, N, W, totals, M):
    """A panel whose windows carry exactly the given numbers of reads."""
    rng = np.random.default_rng(seed)
    L = W * len(totals)
    f = np.clip(rng.beta(0.4, 1.0, size=L), 1e-3, 0.999)
    alle = (rng.random((L, 2 * N)) < f[:, None]).astype(np.uint8)
    cov = np.zeros(L, dtype=np.int64)
    for k, s in enumerate(totals):
        c = np.full(W, s // W)
        c[:s % W] += 1
        cov[k * W:(k + 1) * W] = rng.permutation(c)
    assert cov.max() <= M
    na = rng.binomial(cov, f).astype(np.uint8)
    return alle, (cov - na).astype(np.uint8), na


@pytest.mark.parametrize("eps", [0.02, 0.001])
def test_exponent_range_switches(oracle, eps):
    """k_ld_popcount's power tables take rho^n 2^(8n) while (ct_max+1) max(|log2 rho + 8|, |log2 sigma|) <= 1000, else
    rho^n 2^(s n) with s = lround(-log2 rho); mx_counts is dropped where the tables sit in LDS and (ct_max+1) per_read
    > 1000.  Runs with their largest window on each side of the first switch, windows on each side within them.  The
    second switch cannot trip for eps < 0.5 (per_read <= 1 once s is the nearest integer, and tables in LDS mean
    ct_max < 768): asserted, so that a change of the formula shows."""
    thr = threshold(eps)
    assert switches(eps, thr)[0] and not switches(eps, thr + 1)[0]
    W, M, N = 100, 20, 129
    for ct in range(0, 768):
        assert not switches(eps, ct)[1]
    for k, totals in enumerate(([thr - 60, thr - 1, thr], [thr - 60, thr, thr + 1, thr + 90])):
        alle, nr, na = reads_case(700 + k, N, W, totals, M)
        assert (switches(eps, max(totals))[0]) == (k == 0)
        for form in ("popcount mx1", "popcount mx0", "popcount IBD1 form", "popcount compacted", "popcount_mt T4"):
            truths = run_form(oracle, form, alle, nr, na, W, eps, M, seed=k)
            assert list(truths[0]["reads"]) == totals
        print(f"eps={eps}: shift8 up to ct_max={thr}; run with ct_max={max(totals)} shift8={k == 0}")


# --------------------------------------------------------------------------- underflow bands
BAND_LOG2 = [300, 970, 990, 1005, 1015, 1030, 1050, 1068, 1085, 1150]     # -log2 of the window values aimed at


def band_case(N, W, eps):
    """A homozygous-reference panel read with alt reads only: every product of every window is a product of the same
    factors, C (1-e)^r e^a, so each window's value is chosen exactly through its alt reads -- and rows (1, a) give the
    products other mantissas than powers of e.  Windows are aimed at the -log2 values of BAND_LOG2."""
    per = -math.log2(eps)
    L = W * len(BAND_LOG2)
    alle = np.zeros((L, 2 * N), dtype=np.uint8)
    nr = np.zeros(L, dtype=np.uint8)
    na = np.zeros(L, dtype=np.uint8)
    for k, b in enumerate(BAND_LOG2):
        s = int(round(b / per))
        a = np.full(W, s // W)
        a[:s % W] += 1
        na[k * W:(k + 1) * W] = a
        nr[k * W:k * W + 3] = 1
    nr[(nr == 0) & (na == 0)] = 1          # (a row without reads is not windowed)
    return alle, nr, na


def span_case(N, W, eps):
    """A quarter of the panel homozygous alternative, the rest reference; alt reads on a third of a window's rows, ref
    reads on the rest (no row has both: every coefficient is 1), about 1005 / -log2(eps) of the first kind and 1100 /
    -log2(eps) more of the second: the reference individuals' products near 2^-1010, the others' more than 1074 binades
    below them, so the small ones flush under the wave's largest exponent (eRef in k_ld_mfma) or in the final ldexp.
    (A small epsilon keeps the reads few: k_ld_mfma takes only runs whose tables fit its LDS.)"""
    per = -math.log2(eps)
    L = W * 3
    alle = np.zeros((L, 2 * N), dtype=np.uint8)
    alle[:, 2 * (3 * N // 4):] = 1
    nr = np.zeros(L, dtype=np.uint8)
    na = np.zeros(L, dtype=np.uint8)
    for k in range(3):
        sa = round(1005 / per) + k
        sr = sa + round(1100 / per) + k
        a = np.full(W // 3, sa // (W // 3))
        a[:sa % (W // 3)] += 1
        r = np.full(W - W // 3, sr // (W - W // 3))
        r[:sr % (W - W // 3)] += 1
        na[k * W:k * W + W // 3], nr[k * W + W // 3:(k + 1) * W] = a, r
    return alle, nr, na


def test_underflow_bands_in_every_form(oracle):
    eps, M, N, W = 0.02, 20, 64, 100
    alle, nr, na = band_case(N, W, eps)
    s_eps = 1e-5
    salle, snr, sna = span_case(N, W, s_eps)
    fac = H.binomial_factors(s_eps, M)
    for k in range(3):      # the span: log2 of a reference and an alternative individual's product
        rows = slice(k * W, (k + 1) * W)
        lo = sum(float(np.log2(fac[r, a, 2])) for r, a in zip(snr[rows], sna[rows]))
        hi = sum(float(np.log2(fac[r, a, 0])) for r, a in zip(snr[rows], sna[rows]))
        assert hi - lo > 1074 and hi < -990, (k, hi, lo)
    for form in FORMS:
        BANDS_HIT[form] = {b: 0 for b in H.BANDS}
        before = dict(BANDS_HIT[form])
        truths = run_form(oracle, form, alle, nr, na, W, eps, M, seed=1)
        for key in ("ibd0", "ibd1"):
            counts = H.band_counts(truths[0][key])
            assert all(n >= 1 for n in counts.values()), (form, key, counts)
        run_form(oracle, form, salle, snr, sna, W, s_eps, M, seed=2)
        assert all(BANDS_HIT[form][b] > before[b] for b in H.BANDS), (form, BANDS_HIT[form])


def test_report():
    """The largest ratio to the bound per form and the bands each form reached (printed with -s)."""
    for form in FORMS:
        s = FORMS[form]
        if isinstance(s["hp"], str):
            bound = f"B={H.fast_B(s['hp'], 64):.1f}..{H.fast_B(s['hp'], 2504):.1f} u A={H.FAST_A}"
        else:
            bound = "B,A=strict(W, n_bg)"
        print(f"{form:24s} {bound:32s} worst normal {WORST.get((form, True), float('nan')):.3f} "
              f"subnormal {WORST.get((form, False), float('nan')):.3f}  bands {BANDS_HIT.get(form)}")
    assert all(v <= 1.0 for v in WORST.values())
