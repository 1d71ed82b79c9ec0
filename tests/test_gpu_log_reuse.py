"""GPU tier: what ibdg_window_log2_states / _posteriors / _segments keep from call to call on one run (LogStates in
ibdg_ctx.h: a path or posteriors made for the same penalties on the same run are not made again).  Every sequence of calls
gives the bytes of a fresh context that made only the last call, and of the host twin on the run's own tables; the penalties
of each case give different records, so a product kept for the wrong penalties or the wrong run cannot pass."""
import functools

import numpy as np
import pytest

import log_states_util as U
from ibdgem_amd import engine as E
from test_gpu_log_states_trips import engine, states_launch

pytestmark = pytest.mark.gpu

SMALL = (0.5, 0.25, 0.5)
DENSE = (1.0, 1.0, 1.0)
WIDE = (30, 601)                      # N, n_win: paths of several segments, windows over more than one block
A, B = (4, 7, 11), (5, 8, 12)
CAP = (40, 5)                         # with 1100 individuals: past the block cap, a second trip of the grid
MANY = tuple(t % 40 for t in range(1100))


def context(shape):
    N, n_win = shape
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    eng = engine(alle, nr, na, 2)
    assert eng.n_windows == n_win
    return eng


def segments(eng, pen, with_post):
    """(counts, summaries, records) of one segments call and its records, as bytes"""
    n_seg, summary = eng.window_log2_segments(*pen, with_post=with_post)
    return n_seg.tobytes(), summary.tobytes(), eng.get_log2_segments().tobytes()


@functools.lru_cache(maxsize=None)
def tables(shape, targets):
    with context(shape) as eng:
        eng.run(list(targets), ld=False)
        return eng.window_log2_all(len(targets))


@functools.lru_cache(maxsize=None)
def fresh(shape, targets, pen, with_post):
    """A context that has made nothing but the run and this one call."""
    with context(shape) as eng:
        eng.run(list(targets), ld=False)
        return segments(eng, pen, with_post)


@functools.lru_cache(maxsize=None)
def twin(shape, targets, pen, with_post):
    out = [E.log2_segments_host(tab, *pen, with_post=with_post) for tab in tables(shape, targets)]
    return (np.array([n for _, n, _ in out], dtype=np.uint64).tobytes(), b"".join(s.tobytes() for _, _, s in out),
            b"".join(seg.tobytes() for seg, _, _ in out))


def expected(shape, targets, pen, with_post):
    """What a call must give, after the fresh context and the twin have agreed on it; the other penalties give something else."""
    want = fresh(shape, targets, pen, with_post)
    assert want == twin(shape, targets, pen, with_post)
    other = DENSE if pen == SMALL else SMALL
    assert all(a != b for a, b in zip(want, fresh(shape, targets, other, with_post)))
    return want


def states_equal_twin(shape, targets, pen, got):
    path, score, count = got
    for t, tab in enumerate(tables(shape, targets)):
        wp, ws, wc = E.log2_states_host(tab, *pen)
        assert path[t].tobytes() == wp.tobytes() and count[t].tobytes() == wc.tobytes(), f"path of individual {t}"
        assert score is None or score[t].tobytes() == ws.tobytes(), f"scores of individual {t}"


def posteriors_equal_twin(shape, targets, pen, got):
    post, expect, log2_z = got
    for t, tab in enumerate(tables(shape, targets)):
        wp, we, wz = E.log2_posteriors_host(tab, *pen)
        assert post[t].tobytes() == wp.tobytes() and expect[t].tobytes() == we.tobytes(), f"posteriors of individual {t}"
        assert np.float64(log2_z[t]).tobytes() == np.float64(wz).tobytes(), f"log2 Z of individual {t}"


def reuse(shape, targets):
    """states, posteriors, segments with the same penalties: every kernel once, and every output as if alone"""
    want = expected(shape, targets, SMALL, True)
    with context(shape) as eng:
        eng.run(list(targets), ld=False)
        states_equal_twin(shape, targets, SMALL, eng.window_log2_states(*SMALL, want_score=False))
        posteriors_equal_twin(shape, targets, SMALL, eng.window_log2_posteriors(*SMALL))
        assert segments(eng, SMALL, True) == want
        # and the two kept products are still what their own calls give
        states_equal_twin(shape, targets, SMALL, eng.window_log2_states(*SMALL))
        posteriors_equal_twin(shape, targets, SMALL, eng.window_log2_posteriors(*SMALL))


def test_reuse():
    reuse(WIDE, A)


def test_reuse_past_the_block_cap():
    assert states_launch(len(MANY), CAP[1]) == dict(C=1, owners=5, last=1, trips=2)
    reuse(CAP, MANY)


def test_other_penalties_make_a_new_path():
    want = expected(WIDE, A, DENSE, False)
    with context(WIDE) as eng:
        eng.run(list(A), ld=False)
        eng.window_log2_states(*SMALL)
        assert segments(eng, DENSE, False) == want


def test_other_penalties_make_new_posteriors_only():
    want = expected(WIDE, A, DENSE, True)
    with context(WIDE) as eng:
        eng.run(list(A), ld=False)
        eng.window_log2_states(*DENSE)
        eng.window_log2_posteriors(*SMALL)
        assert segments(eng, DENSE, True) == want


@pytest.mark.parametrize("queued", [False, True])
def test_a_run_in_between(queued):
    """The second run as the host program queues a batch ahead (option "async" around it), and waited for."""
    want = expected(WIDE, B, SMALL, False)
    assert all(a != b for a, b in zip(want[1:], fresh(WIDE, A, SMALL, False)[1:]))
    with context(WIDE) as eng:
        eng.run(list(A), ld=False)
        states_equal_twin(WIDE, A, SMALL, eng.window_log2_states(*SMALL))
        eng.set_option("async", int(queued))
        eng.run(list(B), ld=False)
        eng.set_option("async", 0)
        assert segments(eng, SMALL, False) == want


def test_scores_after_a_kept_path():
    with context(WIDE) as eng:
        eng.run(list(A), ld=False)
        states_equal_twin(WIDE, A, SMALL, eng.window_log2_states(*SMALL, want_score=False))
        got = eng.window_log2_states(*SMALL, want_score=True)
        assert got[1] is not None
        states_equal_twin(WIDE, A, SMALL, got)


@pytest.mark.parametrize("first", [False, True])
def test_posteriors_off_after_on_and_on_after_off(first):
    want = {w: expected(WIDE, A, SMALL, w) for w in (False, True)}
    with context(WIDE) as eng:
        eng.run(list(A), ld=False)
        for with_post in (first, not first, first):
            got = segments(eng, SMALL, with_post)
            assert got == want[with_post]
            seg = np.frombuffer(got[2], dtype=E.SEGMENT_DTYPE)
            if with_post:
                assert (seg["post_min"] > 0).all() and (seg["post_q"] > 0).any()
            else:
                assert (seg["post_min"] == 0).all() and (seg["post_q"] == 0).all()
