"""The truths of tests/hp_log_ref.py checked against themselves and against the regimes they were made for (CPU tier)."""
import numpy as np
import pytest

import hp_log_ref as HL
import hp_ref as H

LD = H.LD
_TRUTHS = {}


def truth(name):
    if name not in _TRUTHS:
        c = HL.make_case(name)
        _TRUTHS[name] = HL.ld_log2_truth(c["alle"], c["nr"], c["na"], c["target"], c["W"], c["eps"], c["M"], c["refids"], c["pu"])
    return _TRUTHS[name]


@pytest.mark.parametrize("name", sorted(HL.CASES))
def test_log_truth_is_the_log_of_the_linear_truth_and_has_not_underflowed(name):
    tr = truth(name)
    for lin, lg in ((tr["lin0"], tr["log0"]), (tr["lin1"], tr["log1"])):
        if tr["n_bg"] == 0:
            assert np.isnan(lg).all()
            continue
        assert np.isfinite(lg).all() and (lg > -16000).all(), (name, float(lg.min()))      # the long double itself holds it
        normal = lin >= LD(2.0) ** -1022
        back = np.exp2(lg[normal])
        assert (np.abs(back - lin[normal]) <= LD(1e-15) * lin[normal]).all(), name


def test_log_B_leaves_room_for_another_tree_and_no_more():
    for n in (1, 5, 64, 130, 700, 2504, 65536):      # (one more addition per 4096 individuals)
        assert H.fast_B("popcount", n) - 8 <= HL.log_B(n) <= 40, (n, HL.log_B(n))


@pytest.mark.parametrize("related", [True, False])
def test_regimes_of_the_generator(related):
    """At Poisson(30) at least half of the LIBD0 windows lie below 2^-1074, at Poisson(2) none do."""
    for depth, want in ((30, "half"), (2, "none")):
        alle, nr, na = HL.issue_inputs(depth, related)
        tr = HL.ld_log2_truth(alle, nr, na, 0, 100, 0.02, 50)
        below = int((tr["log0"] < -1074).sum())
        print(f"Poisson({depth}) related={related}: {below} of {len(tr['log0'])} LIBD0 windows below 2^-1074, "
              f"{int((tr['log1'] < -1074).sum())} LIBD1, smallest log2 LIBD0 {float(tr['log0'].min()):.0f}")
        assert len(tr["log0"]) in (13, 14, 15)
        if want == "half":
            assert 2 * below >= len(tr["log0"])
        else:
            assert below == 0


def test_the_gpu_cases_reach_the_underflowed_regime():
    """Every Poisson(30) case with 100 rows a window has at least half of its LIBD0 windows below 2^-1074 (where the linear
    column is exactly 0), every Poisson(2) case with 100 rows a window none."""
    for name, c in HL.CASES.items():
        if c.get("spread") is not None or c.get("bg") == "empty":
            continue
        lg = truth(name)["log0"]
        if c["depth"] == 30 and c["W"] == 100:
            assert 2 * int((lg < -1075).sum()) >= len(lg), name
        if c["depth"] == 2:
            assert int((lg < -1074).sum()) == 0, name


def test_rows_truth_sums_the_logs():
    site = np.array([[0.5, 0.25, 1.0], [1.0, 1.0, 1.0], [2.0 ** -1022, 0.125, 0.5]])
    s, a = HL.rows_log2_truth(site, [1, 0, 2], [0, 0, 0], 5)
    assert s.shape == (1, 3) and [float(x) for x in s[0]] == [-1023.0, -5.0, -1.0]
    assert [float(x) for x in a[0]] == [1023.0, 5.0, 1.0]
