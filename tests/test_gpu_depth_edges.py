"""Every read depth 1..50 and every edge of the weight planes through every --LD form (the cases of tests/depth_cases.py).

The counting kernels treat the low bit-planes of a segment's depths and the rare higher ones with different code, chosen by
the bit length of the segment's largest depth; Poisson depths meet the upper planes by chance.  Here every (case, form)
  (a) goes through test_gpu_precision.run_form: per-row values and LIBD2 bit for bit against the oracle, --LD within 1e-10
      of it (the reference order bit for bit), the hp_ref bound on three comparison individuals -- the first of them the
      case's target, whose window truths test_depth_cases.py shows to be normal doubles: the bound's absolute term excuses
      nothing --, and the C ABI's report of which form ran;
  (b) the window tables of the counting forms are equal bit for bit (include/ibdgem_hip.h, ibdg_last_count_unit: exact
      integer counts, the same additions in the same order): the check no rounding can excuse;
  (c) option "log_windows" on the same inputs against the truths and bars of tests/hp_log_ref.py.
No bar is new.  The largest ratios go to test_gpu_precision.WORST / test_gpu_log_windows.WORST as well and are printed by
test_report here (-s); DESIGN.md s2 records them.

k_ld_mfma takes a run only where its LDS image stays within 64 KiB (depth_cases.mfma_takes): windows of up to about 500
reads.  full-depth-15 (750 reads a window, tables still in LDS) lies beyond that, so its "mfma" forms are counted by
k_ld_popcount_mt and the single-individual kernels: they run with those kernels' tighter bound and the count unit that
split leaves, instead of being skipped.
"""
import time

import numpy as np
import pytest

import depth_cases as DC
import hp_log_ref as HL
import hp_ref as H
import test_gpu_log_windows as LW
import test_gpu_precision as P
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

LD = H.LD
WORST = {}          # (form, "normal" / "subnormal") or "log ld" / "log rows" -> largest ratio to its bound, this module's runs
SLOWEST = [0.0, None]
EQUAL_FORMS = ("popcount mx0", "popcount mx1", "popcount IBD1 form", "popcount compacted", "popcount_mt T4")


def _in_lds(name):
    c = DC.make_case(name)
    return DC.tab_in_lds(c["nr"], c["na"], c["W"])


# the mfma forms are left out only where the tables are not in LDS
ITEMS = [(name, form) for name in DC.NAMES for form in P.FORMS if not (P.FORMS[form]["hp"] == "mfma" and not _in_lds(name))]


def spec_for(name, form, T=None):
    """The FORMS entry as this case runs it: the IBD1 form must report count unit 3 wherever the tables are in LDS; groups
    that k_ld_mfma does not take (see above) are split by k_ld_popcount_mt's groups of four."""
    c = DC.make_case(name)
    spec = dict(P.FORMS[form])
    if T is not None:
        spec["T"] = T
    in_lds = _in_lds(name)
    assert in_lds == P.tab_in_lds(c["nr"], c["na"], c["W"])
    if form == "popcount IBD1 form":
        spec["unit"] = 3 if in_lds else (2, 3)
    if spec["hp"] == "mfma" and not DC.mfma_takes(c["nr"], c["na"], c["W"]):
        spec["hp"] = "popcount_mt"
        spec["unit"] = 0 if spec["T"] % 4 == 0 else (2, 3)
    return spec


def timed_run(oracle, name, form, T=None, keep=None):
    c = DC.make_case(name)
    spec = spec_for(name, form, T)
    # run_form keeps the session's largest ratios per form in P.WORST: this run's are taken apart from them, then merged
    session = dict(P.WORST)
    P.WORST.clear()
    t0 = time.perf_counter()
    try:
        truths = P.run_form(oracle, form, c["alle"], c["nr"], c["na"], c["W"], c["eps"], c["M"], refids=c["refids"],
                            pu=c["pu"], seed=DC.run_seed(name, spec["T"]), spec=spec, keep=keep)
    finally:
        for (f, normal), v in P.WORST.items():
            k = (f, "normal" if normal else "subnormal")
            WORST[k] = max(WORST.get(k, 0.0), v)
        for key, v in session.items():
            P.WORST[key] = max(P.WORST.get(key, 0.0), v)
    dt = time.perf_counter() - t0
    if dt > SLOWEST[0]:
        SLOWEST[:] = [dt, f"{name} / {form}" + (f" T={T}" if T else "")]
    # the first comparison individual is the case's target: every one of its truths is a normal double
    for key in ("ibd0", "ibd1"):
        assert (truths[0][key] >= LD(2.0) ** -1022).all(), (name, form, key)
    return truths


@pytest.mark.parametrize("name,form", ITEMS, ids=[f"{n}-{f.replace(' ', '_')}" for n, f in ITEMS])
def test_every_form_at_every_depth_edge(oracle, name, form):
    timed_run(oracle, name, form)


@pytest.mark.parametrize("name", DC.NAMES)
def test_counting_forms_give_equal_bits(oracle, name):
    """The same four comparison individuals through every counting form (single launches: four of them; the group of
    four: one launch of k_ld_popcount_mt, count unit 0): the window tables of the three that run_form checked are the
    same bits."""
    tables = {}
    t0 = time.perf_counter()
    for form in EQUAL_FORMS:
        keep = {}
        timed_run(oracle, name, form, T=4, keep=keep)
        tables[form] = keep
    first = tables[EQUAL_FORMS[0]]
    assert first["targets"][0] == DC.make_case(name)["target"] and sorted(first["windows"]) == [0, 2, 3]
    for form in EQUAL_FORMS[1:]:
        assert tables[form]["targets"] == first["targets"]
        for i, want in first["windows"].items():
            assert_bits(tables[form]["windows"][i], want, f"{name}: {form} vs {EQUAL_FORMS[0]}, individual {first['targets'][i]}")
    if time.perf_counter() - t0 > SLOWEST[0]:
        SLOWEST[:] = [time.perf_counter() - t0, f"{name} / equal bits, five forms"]


def _ratio(got, truth, bar, what, key):
    got = np.asarray(got, dtype=np.float64).astype(LD)
    assert np.isfinite(got).all() and np.isfinite(truth).all(), what
    worst = float((np.abs(got - truth) / bar).max())
    print(f"{what}: largest ratio to the bar {worst:.3f}")
    WORST[key] = max(WORST.get(key, 0.0), worst)
    LW.WORST[key[4:]] = max(LW.WORST[key[4:]], worst)
    assert worst <= 1.0, f"{what}: worst ratio {worst:.3g}"


@pytest.mark.parametrize("name", DC.NAMES)
def test_log_windows_at_every_depth_edge(oracle, name):
    c = DC.make_case(name)
    t0 = time.perf_counter()
    tr = HL.ld_log2_truth(c["alle"], c["nr"], c["na"], c["target"], c["W"], c["eps"], c["M"], c["refids"], c["pu"])
    site = oracle.compare(c["alle"], c["nr"], c["na"], c["target"], ld=True, window=c["W"], eps=c["eps"], max_cov=c["M"],
                          refids=c["refids"], pu_id=c["pu"])["site"]
    s, a = HL.rows_log2_truth(site[:, 2:3], c["nr"], c["na"], c["W"])
    with LW.engine_for(c, dict(log_windows=1)) as eng:
        LW.run(eng, c, [c["target"]])
        assert eng.last_ld_variant() == 2
        lg, win = eng.window_log2(0), eng.window_ll(0)
    assert lg.shape == (len(tr["log0"]), 3) and win.shape == lg.shape
    for col, key in ((0, "log0"), (1, "log1")):
        _ratio(lg[:, col], tr[key], HL.ld_bar(tr[key], c["n_ids"]), f"{name} log2 column {col}", "log ld")
    _ratio(lg[:, 2], s[:, 0], HL.rows_bar(s[:, 0], a[:, 0]), f"{name} log2 column 2", "log rows")
    # the two tables of one run: the --LD columns are normal doubles by the precondition, LIBD2 where its truth says so
    assert (tr["lin0"] >= LD(2.0) ** -1022).all() and (tr["lin1"] >= LD(2.0) ** -1022).all()
    ok = np.ones(lg.shape, dtype=bool)
    ok[:, 2] = s[:, 0] >= -1022
    rel = np.abs(np.exp2(lg[ok]) - win[ok]) / win[ok]
    print(f"{name}: exp2(window_log2) off window_ll by at most {rel.max():.3e}")
    assert (win[ok] > 0).all() and rel.max() <= 1e-10, f"{name}: exp2(window_log2) off window_ll by {rel.max():.3e}"
    dt = time.perf_counter() - t0
    if dt > SLOWEST[0]:
        SLOWEST[:] = [dt, f"{name} / log_windows"]


def test_report():
    """This module's largest ratios to the bounds, and its slowest item (printed with -s)."""
    for key in sorted(WORST, key=str):
        print(f"depth edges: {str(key):44s} worst ratio {WORST[key]:.3f}")
    print(f"depth edges: slowest item {SLOWEST[1]}: {SLOWEST[0]:.2f} s")
    assert all(v <= 1.0 for v in WORST.values())
