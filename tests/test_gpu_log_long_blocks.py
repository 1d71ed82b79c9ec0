"""GPU tier of the long blocks (hard_tables.LONG_SIZES): the kernels of the log-domain state family -- k_log2_states,
k_log2_posteriors, k_log2_segments_count / _write, k_log2_alpha, k_log2_sample_paths -- against the host twin on every byte, at
the block lengths the code is used and allowed at.  Thread b of a workgroup walks the C = ceil(n_win / 256) windows of its block
in loops; the other GPU tests of the family stop at C = 5, so the 4- and 8-way unrolled bodies of k_log2_sample_paths, whatever
the compiler unrolls or pipelines in the other walks, a thread that owns whole words of the chain mask and several starts, and
the ABI's limit of 2^21 windows never ran.  tests/test_hard_tables_long.py holds the twin to independent references at the same
sizes and on the same tables.

  the lattice 256 C - 5 (C = 6 .. 16: trip counts C and C - 5 in one launch), 1793 and 2048: every family of LONG_FAMILIES, five
      individuals, plain, with dense chain starts, with edge shifts and with both, K = 3 draws
  8192 (a block is one aligned mask word), 8193 (blocks straddle the words at every offset, 7 idle threads) and 40000 (a
      chromosome's windows): every family, plain and with both
  2^21: two tables, plain and with both, K = 2; 2^21 + 1: a run succeeds, the four calls of the family refuse and change nothing
  one context through 40000 and then 2043 windows: nothing of the larger shape is left behind
The tables reach the device through ibdg_set_window_log2 behind an ordinary run, as in tests/test_gpu_log_hard_tables.py."""
import time

import numpy as np
import pytest

import hard_tables as HT
import log_states_util as U
from ibdgem_amd import engine as E
from test_gpu_log_hard_tables import N, T, every_product, forms, products, run_of, table_set
from test_gpu_log_states_trips import engine, states_launch

pytestmark = pytest.mark.gpu

SMALL_SIZES = [n for n in HT.LONG_SIZES if n <= 4091]
BIG_SIZES = [8192, 8193, 40000]
TOP = 1 << 21
FOUR, TWO = {8: [0, 5, 6, 3], 4: [0, 1, 2, 3]}, {8: [0, 7], 4: [0, 3]}      # of forms(): a finite family has both penalty sets


def asserted_shape(n_targets, n_win):
    C, owners, last = HT.LONG_SHAPES[n_win]
    shape = dict(C=C, owners=owners, last=last, trips=1)
    assert states_launch(n_targets, n_win) == shape
    print(f"{n_win} windows, {n_targets} individuals: states_launch {shape}")
    return shape


def long_forms(family, n, pen, own, pick):
    all_forms = forms(family, n, pen, own, starts=HT.dense_chain_starts(n), rnd=HT.edge_shifts(n, 9))
    return [all_forms[i] for i in pick[len(all_forms)]]


def change_residues(path, n):
    """(w1 - 1 - w) % 8 over the windows w at which a path changes state, w1 the end of w's block: where in an 8-way unrolled
    backward walk of the block the change lies."""
    C = HT.blocking(n)[0]
    w = np.unique(np.nonzero(path[:, 1:] != path[:, :-1])[1] + 1)
    w1 = np.minimum((w // C + 1) * C, n)
    return set(((w1 - 1 - w) % 8).tolist())


def family_device_equals_twin(eng, family, n_win, pick):
    """Every product of the family's table set in the forms picked; returns the residues of the device's own paths."""
    tabs, pen, own, mine = table_set(family, n_win)
    eng.set_window_log2_all(tabs)
    assert eng.window_log2_all(T).tobytes() == tabs.tobytes(), family
    seen = set()
    for i, (p, starts, shift) in enumerate(long_forms(family, n_win, pen, own, pick)):
        what = f"{family}, {n_win} windows, penalties {p}, {len(starts)} starts, shifts {shift is not None}"
        post, log2_z = every_product(eng, tabs, p, starts, shift, what)
        seen |= change_residues(eng.window_log2_states(*p, want_score=False)[0], n_win)
        sums = post.sum(axis=2)
        if family in HT.LONG_FINITE:
            # a finite family is finite, but for the tables an edge shift of -2^30 kills: those carry the rule's mark
            alive = np.array([HT.chain_alive(tabs[t], p, shift, starts) for t in range(T)])
            assert (alive | (shift is not None)).all(), what
            if shift is None or family not in HT.TINY_WEIGHTS:                  # (else a product near 2^-2000 may underflow)
                assert (sums[alive] != 0.0).all() and np.isfinite(log2_z[alive]).all(), what
            assert not post[~alive].any() and (log2_z[~alive] == -np.inf).all(), what + ": killed by a shift"
        elif family == "dead-shift" or i == 0:                                  # (shifts of their own may revive an underflow)
            assert not post[mine].any() and (log2_z[mine] == -np.inf).all(), what + ": the rule's mark"
            assert post[2:].any()
    eng.set_window_chains([])
    eng.set_window_steps(None)
    return seen


@pytest.mark.parametrize("n_win", SMALL_SIZES)
def test_the_lattice_device_equals_twin(n_win):
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        shape = asserted_shape(T, n_win)
        run_of(eng, n_win)
        seen = set()
        for family in HT.LONG_FAMILIES:
            seen |= family_device_equals_twin(eng, family, n_win, FOUR)
        # the paths the device wrote change state at every position of the unrolled bodies
        assert seen >= set(range(min(shape["C"], 8))), seen


@pytest.mark.parametrize("family", HT.LONG_FAMILIES)
@pytest.mark.parametrize("n_win", BIG_SIZES)
def test_big_sizes_device_equals_twin(n_win, family):
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        asserted_shape(T, n_win)
        run_of(eng, n_win)
        seen = family_device_equals_twin(eng, family, n_win, TWO)
        if family in ("alternating", "plateaus", "edge1000"):                  # (tables whose best state moves all the time)
            assert seen == set(range(8)), seen


def test_the_limit():
    """2^21 windows, the most the calls take: window 1 and four individuals in the panel, two comparison individuals.  Prints
    the seconds the device calls and their twins took together (DESIGN 4.8 records a run)."""
    n_win = TOP
    alle, nr, na = U.covered_reads(21, n_win, 4)
    tabs = np.stack([HT.case("alternating", n_win, 0).tab, HT.case("plateaus", n_win, 0).tab])
    starts, shift = HT.dense_chain_starts(n_win), HT.edge_shifts(n_win, 9)
    with engine(alle, nr, na, 1) as eng:
        assert states_launch(2, n_win) == dict(C=8192, owners=256, last=8192, trips=1)
        print(f"{n_win} windows, 2 individuals: states_launch {states_launch(2, n_win)}")
        run_of(eng, n_win, [1, 2])
        eng.set_window_log2_all(tabs)
        t0 = time.perf_counter()
        for pen, st, sh in ((HT.PENS[0], [], None), (HT.PENS[1], starts, shift)):
            what = f"2^21 windows, penalties {pen}, {len(st)} starts, shifts {sh is not None}"
            post, log2_z = every_product(eng, tabs, pen, st, sh, what, K=2)
            alive = np.array([HT.chain_alive(tabs[t], pen, sh, st) for t in range(2)])
            assert alive.all() or sh is not None
            assert (post[alive].sum(axis=2) != 0.0).all() and np.isfinite(log2_z[alive]).all(), what
            assert not post[~alive].any() and (log2_z[~alive] == -np.inf).all(), what
        print(f"2^21 windows: every product twice, device and twin: {time.perf_counter() - t0:.1f} s")
        # the device calls alone, under penalties that nothing kept is fresh for
        fresh = (0.03, 0.002, 0.03)
        eng.sync()
        t0 = time.perf_counter()
        eng.window_log2_states(*fresh)
        eng.window_log2_posteriors(*fresh)
        eng.window_log2_segments(*fresh, with_post=True)
        eng.window_log2_samples(*fresh, 2, 8, np.arange(2, dtype=np.uint64))
        print(f"2^21 windows: the four device calls, T = 2, K = 2, with their copies: {time.perf_counter() - t0:.2f} s")


def test_one_window_more_than_the_limit():
    """A site list of 2^21 + 1 windows and a run over it are fine; each call of the family refuses it and changes nothing."""
    n_win = TOP + 1
    alle, nr, na = U.covered_reads(22, n_win, 4)
    msg = r"%s: 2097153 windows, more than the 2097152 \(2\^21\)"
    streams = np.zeros(1, dtype=np.uint64)
    with engine(alle, nr, na, 1) as eng:
        run_of(eng, n_win, [2])
        before = eng.window_log2_all(1)
        assert np.isfinite(before).all() and before.shape == (1, n_win, 3)
        for _ in range(2):
            with pytest.raises(E.EngineError, match=msg % "ibdg_window_log2_states"):
                eng.window_log2_states(*HT.PENS[0])
            with pytest.raises(E.EngineError, match=msg % "ibdg_window_log2_posteriors"):
                eng.window_log2_posteriors(*HT.PENS[0])
            with pytest.raises(E.EngineError, match=msg % "ibdg_window_log2_segments"):
                eng.window_log2_segments(*HT.PENS[0], with_post=True)
            with pytest.raises(E.EngineError, match=msg % "ibdg_window_log2_samples"):
                eng.window_log2_samples(*HT.PENS[0], 2, 1, streams)
            with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
                eng.get_log2_segments(1)
            with pytest.raises(E.EngineError, match="ibdg_get_log2_sample_path: no ibdg_window_log2_samples call"):
                eng.get_log2_sample_path(0, 0)
            assert eng.window_log2_all(1).tobytes() == before.tobytes()
            eng.run([2], ld=False)                         # ... and the context still runs
        assert eng.window_log2_all(1).tobytes() == before.tobytes()


def test_one_context_through_a_long_shape_and_a_short_one():
    """40000 windows with chains and shifts, then 2043 by a new upload of sites: the LDS arrays, masks and scratch buffers of the
    larger shape leave nothing behind -- every product equals a fresh context's, and the twin's."""
    big, small = 40000, 2043
    alle, nr, na = U.covered_reads(big, 2 * big, N)
    pen = HT.PENS[1]

    def at(eng, n_win, family):
        run_of(eng, n_win)
        assert eng.n_window_chains == 1 and not eng.has_window_steps()          # (a new site list has neither)
        tabs = table_set(family, n_win)[0]
        eng.set_window_log2_all(tabs)
        starts, shift = HT.dense_chain_starts(n_win), HT.edge_shifts(n_win, 9)
        eng.set_window_chains(starts)
        eng.set_window_steps(shift)
        return tabs, starts, shift, products(eng, pen)

    with engine(alle, nr, na, 2) as eng:
        asserted_shape(T, big)
        at(eng, big, "alternating")
        eng.upload_sites(np.arange(2 * small), nr[:2 * small], na[:2 * small], 2)
        asserted_shape(T, small)
        tabs, starts, shift, after = at(eng, small, "plateaus")
        every_product(eng, tabs, pen, starts, shift, "2043 windows behind 40000")
    with engine(alle, nr[:2 * small], na[:2 * small], 2) as fresh:
        assert at(fresh, small, "plateaus")[3] == after
