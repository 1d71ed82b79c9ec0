"""Step shifts on the host: ibdg_log2_states_steps_host, ibdg_log2_posteriors_steps_host and
ibdg_log2_segments_steps_host, no device.

The truth does not come from the code under test: all 3^n paths of small tables and a Python restatement of the recurrence for
the path (tests/hp_steps_ref.py), exact integer forward-backward with a matrix per window for the posteriors, within the bar of
tests/hp_post_ref.py (R = 14: the weights are inputs).  Beside that, identities against the twins that were there before -- all
shifts 0, +2^30 where a chain would start, a constant shift against other penalties -- on every byte, negative controls, and the
refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hp_post_ref as H
import hp_steps_ref as HS
from ibdgem_amd import engine as E
from steps_cases import BIG, finite_table, shift_sets
from test_log_chains_host import positions, start_sets, table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [100, 601, 1279]
DEFAULT = (1e-3, 1e-6, 1e-3)
SMALL = (0.5, 0.25, 0.5)
PENS = [DEFAULT, SMALL]
U = 2.0 ** -53
PATTERNS = ["random", "w0", "w0-1", "w0+1", "all-min"]


@pytest.fixture(scope="module", autouse=True)
def library():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)


def table_for(n, name):
    return finite_table(n) if name == "all-min" else table(n)


def same_bytes(a, b, what):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.tobytes() == y.tobytes(), what
        else:
            assert np.float64(x).tobytes() == np.float64(y).tobytes(), what


# ---- 1. the path against a truth that is not the code under test --------------------------------------------------------

@pytest.mark.parametrize("n", range(1, 8))
@pytest.mark.parametrize("pen", PENS)
def test_all_paths_by_brute_force(n, pen):
    """Tables in half bits within +-3 (so that sums tie) and shifts of whole and half bits, +-2^30 among them; with and without
    a chain start."""
    for seed in range(6):
        rng = np.random.default_rng(100 * n + seed)
        tab = -50.0 + rng.integers(-6, 7, (n, 3)) / 2.0
        shift = (rng.integers(-8, 9, n) * 32768).astype(np.int64)
        shift[rng.integers(0, n)] = BIG if seed % 2 else -BIG
        for starts in ([], [n // 2] if n // 2 >= 1 else []):
            path, score, count = E.log2_states_host(tab, *pen, starts=starts, shift=shift)
            bp, bs, bc = HS.brute_force(tab, pen, shift, starts)
            assert path.tolist() == bp and score.tolist() == bs and count.tolist() == bc, (n, seed, starts)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pen", PENS)
def test_the_restated_recurrence(n, pen):
    differs = 0
    plain = E.log2_states_host(table(n), *pen)[0]
    for name, shift in shift_sets(n).items():
        tab = table_for(n, name)
        for starts in ([], start_sets(n)["random"]):
            path, score, count = E.log2_states_host(tab, *pen, starts=starts, shift=shift)
            rp, rs, rc = HS.restated(tab, pen, shift, starts)
            assert path.tolist() == rp and count.tolist() == rc and score.tolist() == rs, (name, len(starts))
        if name != "all-min":
            differs += E.log2_states_host(tab, *pen, shift=shift)[0].tobytes() != plain.tobytes()
    assert differs > 0                                                    # (the shifts do change paths on these tables)
    tab = finite_table(n)
    path = E.log2_states_host(tab, *pen, shift=shift_sets(n)["all-min"])[0]
    assert len(set(path.tolist())) == 1                                   # no switch is possible: one state throughout


# ---- 2. identities against the twins that were there before ---------------------------------------------------------------

def all_products(tab, pen, pf, pl, **kw):
    out = list(E.log2_states_host(tab, *pen, **kw)) + list(E.log2_posteriors_host(tab, *pen, **kw))
    segs = []
    for skw in (dict(), dict(with_post=True), dict(pos_first=pf, pos_last=pl), dict(with_post=True, pos_first=pf, pos_last=pl)):
        seg, n_seg, summary = E.log2_segments_host(tab, *pen, **skw, **kw)
        segs += [seg, np.uint64(n_seg), summary]
    return out, segs


@pytest.mark.parametrize("n", [0, 1, 2, 5] + SIZES)
@pytest.mark.parametrize("pen", PENS)
def test_all_shifts_zero_are_the_plain_twins(n, pen):
    tab = table(n) if n else np.zeros((0, 3))
    pf, pl = positions(n) if n else (np.zeros(0, np.uint64),) * 2
    zero = np.zeros(n, dtype=np.int32)
    for starts in ([], start_sets(n)["random"] if n >= 2 else []):
        kw = dict(starts=starts) if starts else {}
        a, sa = all_products(tab, pen, pf, pl, **kw)
        b, sb = all_products(tab, pen, pf, pl, shift=zero, **kw)
        same_bytes(a, b, "states, posteriors")
        for x, y in zip(sa, sb):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pen", PENS)
def test_a_free_step_is_a_chain_start_but_for_the_segments(n, pen):
    tab = table(n)
    pf, pl = positions(n)
    for name, starts in start_sets(n).items():
        shift = np.zeros(n, dtype=np.int32)
        shift[starts] = BIG
        assert H.weight(HS.shift_penalty(H.penalty(pen[1]), BIG)) == 1.0  # (post_weight(0) is exactly 1)
        a, _ = all_products(tab, pen, pf, pl, starts=starts)
        b, _ = all_products(tab, pen, pf, pl, shift=shift)
        same_bytes(a, b, name)
        # a shift alone begins no segment: the records are those of the path's runs, no forced break
        seg, n_seg, _ = E.log2_segments_host(tab, *pen, shift=shift)
        path = b[0]
        runs = [0] + [w for w in range(1, n) if path[w] != path[w - 1]]
        assert seg["first"].tolist() == runs and n_seg == len(runs), name


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k,p,q", [(3, (2.0 ** -10, 2.0 ** -20, 2.0 ** -10), (2.0 ** -7, 2.0 ** -17, 2.0 ** -7)),
                                   (-3, (2.0 ** -10, 2.0 ** -20, 2.0 ** -10), (2.0 ** -13, 2.0 ** -23, 2.0 ** -13))])
def test_a_constant_shift_is_other_penalties(n, k, p, q):
    tab = table(n)
    pf, pl = positions(n)
    a, sa = all_products(tab, q, pf, pl)
    b, sb = all_products(tab, p, pf, pl, shift=np.full(n, k * 65536, dtype=np.int32))
    same_bytes(a, b, "states, posteriors")
    for x, y in zip(sa, sb):
        assert x.tobytes() == y.tobytes()


# ---- 3. posteriors against the exact truth ---------------------------------------------------------------------------------

_truths = {}


def truth_of(n, name, pen, late=False):
    key = (n, name, pen, late)
    if key not in _truths:
        shift = shift_sets(n)[name].astype(np.int64)
        if late:
            shift = np.concatenate(([0], shift[:-1]))
            shift[1] = 0                                                  # (shift[0] is not a step's: nothing to apply late)
        _truths[key] = HS.Truth(table_for(n, name), *pen, shift)
    return _truths[key]


def test_the_bar_holds_at_these_sizes():
    assert H.R == 14
    for n in SIZES:
        assert H.Rn(n) * U <= 1e-10


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pen", PENS)
def test_posteriors_within_the_bar_of_the_exact_truth(n, name, pen):
    tab, shift = table_for(n, name), shift_sets(n)[name]
    post, expect, log2_z = E.log2_posteriors_host(tab, *pen, shift=shift)
    assert np.isfinite(post).all()
    t, worst = H.check(tab, pen, post.tolist(), expect.tolist(), log2_z, truth=truth_of(n, name, pen))
    print(f"n_win {n}, shifts {name}, penalties {pen}: largest error / bar {worst:.3g}")
    p2, e2, z2 = E.log2_posteriors_host(tab, *pen, want_post=False, shift=shift)
    assert p2 is None and e2.tobytes() == expect.tobytes() and z2 == log2_z
    if name == "all-min":                                                 # every switch weight is 0: gamma is the same in every window
        assert np.abs(post - post[0]).max() <= 2 * H.Rn(n) * U


@pytest.mark.parametrize("name", ["random", "w0", "w0-1", "w0+1"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pen", PENS)
def test_shifts_a_window_late_lie_a_thousand_bars_away(n, name, pen):
    """The negative control: the same shifts applied to the step one window later are another model, which the bar of the test
    above tells from the truth in some window."""
    t, late = truth_of(n, name, pen), truth_of(n, name, pen, late=True)
    hot = [w for w in range(1, n) if shift_sets(n)[name][w] != 0]
    windows = [w for x in hot for w in (x, x - 1)]
    assert H.control_exceeds(t, (lambda w: (late.P[w], late.Z), windows)) is not None


@pytest.mark.parametrize("n", SIZES)
def test_shifts_ignored_lie_a_thousand_bars_away(n):
    t = truth_of(n, "all-min", SMALL)
    plain = H.Truth(finite_table(n), *SMALL)
    assert H.control_exceeds(t, (lambda w: (plain.P[w], plain.Z), range(n))) is not None


# ---- 4. the refusals ------------------------------------------------------------------------------------------------------

def test_bad_shifts_are_refused_by_all_three():
    tab = table(10)
    for fn, call in (("ibdg_log2_states_steps_host", E.log2_states_host), ("ibdg_log2_posteriors_steps_host", E.log2_posteriors_host),
                     ("ibdg_log2_segments_steps_host", E.log2_segments_host)):
        for w, v in ((1, BIG + 1), (9, -BIG - 1), (4, -2 ** 31)):
            shift = np.zeros(10, dtype=np.int32)
            shift[w] = v
            with pytest.raises(E.EngineError, match=fn + rf": shift\[{w}\] = {v} is not within \+-2\^30"):
                call(tab, *DEFAULT, shift=shift)
        shift = np.zeros(10, dtype=np.int32)
        shift[0] = 2 ** 31 - 1                                            # shift[0] is ignored, whatever it holds
        shift[3], shift[5] = BIG, -BIG                                    # ... and the bounds themselves are inside
        call(tab, *DEFAULT, shift=shift)
        # the chains' and the namesakes' refusals, under the new names
        with pytest.raises(E.EngineError, match=fn + r": starts\[0\] = 10 is not below the 10 windows"):
            call(tab, *DEFAULT, starts=[10], shift=np.zeros(10, dtype=np.int32))
        with pytest.raises(ValueError, match="shift: 9 entries, not the 10 windows"):
            call(tab, *DEFAULT, shift=np.zeros(9, dtype=np.int32))
    with pytest.raises(E.EngineError, match=r"ibdg_log2_states_steps_host: p01 = 0 is not in \(0, 1\]"):
        E.log2_states_host(tab, 0.0, 0.5, 0.5, shift=np.zeros(10, dtype=np.int32))
    with pytest.raises(E.EngineError, match=r"ibdg_log2_posteriors_steps_host: p12 = 2 is not in \(0, 1\]"):
        E.log2_posteriors_host(tab, 0.5, 0.5, 2.0, shift=np.zeros(10, dtype=np.int32))


def test_a_null_shift_is_the_chained_twin():
    lib = E.load_library()
    tab = table(10)
    count = np.zeros(3, np.uint64)
    starts = np.array([4], dtype=np.uint32)
    assert lib.ibdg_log2_states_steps_host(tab.ctypes.data, 10, *DEFAULT, None, None, count.ctypes.data, starts.ctypes.data, 1, None) == 0
    assert count.tolist() == E.log2_states_host(tab, *DEFAULT, starts=[4])[2].tolist()
    assert lib.ibdg_log2_states_steps_host(tab.ctypes.data, 10, *DEFAULT, None, None, count.ctypes.data, None, 0, None) == 0
    assert count.tolist() == E.log2_states_host(tab, *DEFAULT)[2].tolist()
    z = C.c_double(0.0)
    expect = np.zeros(3)
    assert lib.ibdg_log2_posteriors_steps_host(tab.ctypes.data, 10, *DEFAULT, None, expect.ctypes.data, C.addressof(z), None, 0, None) == 0
    assert expect.tobytes() == E.log2_posteriors_host(tab, *DEFAULT)[1].tobytes()
