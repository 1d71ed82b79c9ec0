"""ibdg_log2_posteriors_host: forward-backward IBD-state probabilities on the host, no device.

The twin against the exact truth of tests/hp_post_ref.py within that module's counted bar (R = 14 roundings per window), on
every blocking shape and penalty set; against the closed form where the penalties are 1; and the conditions that keep the
bar honest: R n u <= 1e-10 at every shape, and wrong models 1000 bars away on the same inputs."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hp_post_ref as H
from ibdgem_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 100, 255, 256, 257, 601, 1279]
DEFAULT = (1e-3, 1e-6, 1e-3)
PENS = [DEFAULT, (0.5, 0.25, 0.5), (1.0, 1.0, 1.0)]
UNEVEN = (1e-3, 1e-6, 1e-2)                       # p01 != p12: the set under which exchanging them is another model
U = 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def library():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)


def random_table(n, seed=0):
    """Logs far outside what a product of likelihoods could hold in a double, the three columns within +-30 bits."""
    rng = np.random.default_rng(1000 * n + seed)
    return rng.normal(-3000.0, 400.0, (n, 1)) + rng.uniform(-30.0, 30.0, (n, 3))


_truths = {}


def truth_of(n, pen, seed=0):
    """The exact truth of random_table(n, seed) under `pen`, computed once for the tests that share it."""
    key = (n, pen, seed)
    if key not in _truths:
        _truths[key] = H.Truth(random_table(n, seed), *pen)
    return _truths[key]


def twin_checked(tab, pen, truth=None):
    tab = np.asarray(tab, dtype=np.float64).reshape(-1, 3)
    post, expect, log2_z = E.log2_posteriors_host(tab, *pen)
    n = len(tab)
    assert post.shape == (n, 3) and expect.shape == (3,)
    t, worst = H.check(tab, pen, post.tolist(), expect.tolist(), log2_z, truth)
    # rows of gamma sum to 1 within 4 u: three quotients of one denominator (1/2 ulp each of values <= 1) and two additions
    assert (np.abs(post.sum(axis=1) - 1.0) <= 4 * U).all()
    # expect sums to n_win within the bar: the three bars, and two additions of the test's own
    bars = sum(Fraction((H.Rn(n) + H.blocking(n)[0] + 8) * t.S[s][1], t.Z << 53) + Fraction(n, 1 << 1000) for s in range(3))
    assert abs(Fraction(float(expect.sum())) - n) <= bars + Fraction(4 * n, 1 << 53)
    # the probabilities nobody asked for change nothing
    p2, e2, z2 = E.log2_posteriors_host(tab, *pen, want_post=False)
    assert p2 is None and e2.tobytes() == expect.tobytes() and z2 == log2_z
    return post, expect, log2_z, t, worst


# ---- the bar's own conditions ------------------------------------------------------------------------------------------

def test_the_bar_is_tight_at_every_shape():
    assert H.R == 14
    for n in SIZES:
        assert H.Rn(n) * U <= 1e-10
    assert [H.blocking(n)[:2] for n in SIZES] == [(1, 1), (1, 2), (1, 3), (1, 100), (1, 255), (1, 256), (2, 129), (3, 201), (5, 256)]
    assert H.blocking(257)[2][-1] == (256, 257) and H.blocking(601)[2][-1] == (600, 601) and H.blocking(1279)[2][-1] == (1275, 1279)


def test_the_restated_weights():
    assert H.T1[0] == 1.0 and H.T2[0] == 1.0 and H.weight(0) == 1.0
    assert H.weight(-65536) == 0.5 and H.weight(-1000 * 65536) == 2.0 ** -1000 and H.weight(-1000 * 65536 - 1) == 0.0
    assert H.weight(-1) == H.T1[255] * H.T2[255] / 2 < 1.0
    for x in (-1, -255, -256, -65535, -65537, -12345678):
        assert abs(H.weight(x) / 2.0 ** (x / 65536.0) - 1.0) <= 4 * U           # two table entries, their product, the power
    assert H.weight(H.penalty(5e-324), is_emission=False) > 0.0                # a penalty's weight is never 0


@pytest.mark.parametrize("n", [n for n in SIZES if n > 1])
@pytest.mark.parametrize("pen", [DEFAULT, (0.5, 0.25, 0.5), UNEVEN])
def test_wrong_models_lie_a_thousand_bars_away(n, pen):
    """Every case with more than one block (C = 1 below 257: n blocks).  The three controls are other models only where the
    penalties make them so: exchanging p01 and p12 needs p01 != p12 (UNEVEN); under (1, 1, 1) a window's gamma depends on no
    other window and all three controls are the truth itself, which is why that set is not here."""
    assert H.blocking(n)[1] > 1
    t = truth_of(n, pen)
    tab = random_table(n)
    assert H.control_exceeds(t, H.control_last_block_left_out(t)) is not None
    assert H.control_exceeds(t, H.control_backward_late(t)) is not None
    if pen[0] != pen[2]:
        assert H.control_exceeds(t, H.control_swapped(t, tab)) is not None


# ---- twin against the truth --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pen", PENS + [UNEVEN])
def test_sizes_and_penalties(n, pen):
    tab = random_table(n)
    post, expect, _, t, worst = twin_checked(tab, pen, truth_of(n, pen))
    print(f"n_win {n} penalties {pen}: largest error / bar {worst:.3g}")
    if pen == (1.0, 1.0, 1.0):
        # the closed form: gamma_w = b_w / sum(b_w), one window at a time; here it is 3 products by 1, 2 additions, 1 division
        for w in range(n):
            b = [Fraction(x) for x in t.b[w]]
            for s in range(3):
                want = b[s] / sum(b)
                assert abs(Fraction(float(post[w, s])) - want) <= Fraction(H.Rn(n), 1 << 53) * want + Fraction(1, 1 << 1000)


def special_table(kind, n=40):
    tab = random_table(n, seed=7)
    if kind == "nan":
        tab[0, 1] = tab[17] = tab[n - 1, 2] = math.nan
    elif kind == "minus_inf":
        tab[3, 0] = tab[20, 2] = -math.inf
        tab[21, 0] = tab[21, 1] = -math.inf
        tab[22] = -math.inf                                    # no finite maximum: the window says nothing
        tab[23, 1] = math.inf
    elif kind == "all_minus_5000":
        tab[5] = tab[30] = -5000.0
    elif kind == "2000_down":
        tab[8, 0] = tab[8, 2] - 2000.0
        tab[9, 1] = tab[9, 0] - 2000.0
        tab[9, 2] = tab[9, 0] - 1000.0                          # the last weight that is not 0 ...
        tab[10, 2] = tab[10, 0] - 1000.0 - 2.0 ** -16           # ... and the first that is
    return tab


@pytest.mark.parametrize("kind", ["nan", "minus_inf", "all_minus_5000", "2000_down"])
@pytest.mark.parametrize("pen", PENS)
def test_special_windows(kind, pen):
    tab = special_table(kind)
    post, _, _, t, _ = twin_checked(tab, pen)
    assert np.isfinite(post).all()
    if kind == "nan":
        assert t.b[0] == t.b[17] == t.b[39] == [1.0, 1.0, 1.0]
    if kind == "minus_inf":
        assert t.b[3][0] == 0.0 and t.b[21][:2] == [0.0, 0.0] and t.b[22] == t.b[23] == [1.0, 1.0, 1.0]
        assert post[3, 0] == 0.0 and post[21, 2] == 1.0
    if kind == "all_minus_5000":
        assert t.b[5] == [1.0, 1.0, 1.0]
    if kind == "2000_down":
        assert t.b[8][0] == 0.0 and t.b[9][1] == 0.0 and t.b[9][2] == 2.0 ** -1000 and t.b[10][2] == 0.0
        assert post[8, 0] == 0.0 and post[9, 1] == 0.0 and post[10, 2] == 0.0


def test_a_window_of_zeros_is_a_window_like_any_other():
    """The 30 windows of test_log_states_host.py: IBD2 by 20 bits everywhere, window 11's linear columns all 0 -- as -5000
    three times (it says nothing) and as its true logs."""
    n = 30
    logs = np.full((n, 3), -240.0)
    logs[:, 2] += 20.0
    for w11 in ([-5000.0] * 3, [-1500.0, -1500.0, -1480.0]):
        logs[10] = w11
        post, expect, log2_z, _, _ = twin_checked(logs, DEFAULT)
        others = np.delete(post, 10, axis=0)
        assert (others[:, 2] > 0.999).all()
        assert expect[2] > 0.999 * (n - 1) and math.isfinite(log2_z)
    assert post[10, 2] > 0.999


def test_no_windows():
    post, expect, log2_z = E.log2_posteriors_host(np.zeros((0, 3)), *DEFAULT)
    assert post.shape == (0, 3) and expect.tolist() == [0.0, 0.0, 0.0] and log2_z == 0.0


# ---- errors --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [(0.0, 0.5, 0.5), (0.5, -0.1, 0.5), (0.5, 0.5, 1.0000001), (math.nan, 0.5, 0.5),
                               (0.5, math.inf, 0.5)])
def test_penalties_out_of_range_are_refused(p):
    with pytest.raises(E.EngineError, match=r"ibdg_log2_posteriors_host: p\d\d = .* is not in \(0, 1\]"):
        E.log2_posteriors_host(np.zeros((4, 3)), *p)


def test_too_many_windows_and_null_outputs():
    lib = E.load_library()
    expect = np.zeros(3)
    z = C.c_double(7.0)
    tab = np.zeros(3)                               # never read: the count of windows is refused first
    assert lib.ibdg_log2_posteriors_host(tab.ctypes.data, (1 << 21) + 1, 0.5, 0.5, 0.5, None, expect.ctypes.data, C.addressof(z)) != 0
    assert "2^21" in lib.ibdg_last_error(None).decode()
    assert lib.ibdg_log2_posteriors_host(tab.ctypes.data, 1, 0.5, 0.5, 0.5, None, None, C.addressof(z)) != 0
    assert "NULL expect" in lib.ibdg_last_error(None).decode()
    assert lib.ibdg_log2_posteriors_host(tab.ctypes.data, 1, 0.5, 0.5, 0.5, None, expect.ctypes.data, None) != 0
    assert "NULL log2_z" in lib.ibdg_last_error(None).decode()
    assert z.value == 7.0
    assert lib.ibdg_log2_posteriors_host(tab.ctypes.data, 1, 0.5, 0.5, 0.5, None, expect.ctypes.data, C.addressof(z)) == 0
    assert expect.tolist() == [1 / 3, 1 / 3, 1 / 3] and z.value == math.log2(3.0)
