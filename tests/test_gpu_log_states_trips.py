"""GPU tier: the kernels of the log-domain statistics past the first trip of their grid-stride loops and on every shape of
their blocking, in the manner of tests/test_gpu_launch_trips.py: each test restates its wrapper's formula here, asserts
the trip count / shape the inputs give, then compares.

  1. k_log2_states past STATES_MAX_BLOCKS individuals (LDS reused by a workgroup's second individual);
  2. ... with several windows a thread and a partial last block; with fewer windows than threads;
  3. the log instantiation of k_llr_partial past LLR_MAX_BLOCKS items."""
import numpy as np
import pytest

import log_states_util as U
from ibdgem_amd import engine as E
from test_gpu_arm_stats import random_case
from test_gpu_launch_trips import cdiv, llr_launch, llr_ranges

pytestmark = pytest.mark.gpu


def states_launch(T, n_win):
    """ibdg_window_log2_states / launch_log2_states: a workgroup of STATES_THREADS = 256 per individual, min(T,
    STATES_MAX_BLOCKS = 1024) workgroups (`t += gridDim.x`); thread b owns windows [b C, (b + 1) C), C = ceil(n_win / 256)."""
    C = cdiv(n_win, 256)
    owners = cdiv(n_win, C)
    return dict(C=C, owners=owners, last=n_win - (owners - 1) * C, trips=cdiv(T, min(T, 1024)))


def engine(alle, nr, na, W):
    eng = E.Engine(0, 0.02, 20)
    eng.set_option("log_windows", 1)
    eng.upload_panel(E.pack_alleles_fast(alle), alle.shape[1] // 2)
    eng.upload_sites(np.arange(len(nr)), nr, na, W)
    return eng


def test_states_past_the_block_cap():
    """1100 individuals (of 40, repeated) for 1024 workgroups: 76 workgroups take a second individual.  Every individual's
    result equals the twin's, so those of the second trip do, and equal individuals have equal results."""
    N, T, n_win = 40, 1100, 5
    alle, nr, na = U.covered_reads(5, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win
        assert states_launch(T, n_win) == dict(C=1, owners=5, last=1, trips=2)
        eng.run([t % N for t in range(T)], ld=False)
        _, path, score, count = U.device_equals_twin(eng, T, what="past the block cap")
        assert path[1024:].tobytes() == path[1024 % N:1024 % N + 76].tobytes()
        assert score[1024:].tobytes() == score[1024 % N:1024 % N + 76].tobytes()
        assert len({p.tobytes() for p in path}) > 1


@pytest.mark.parametrize("n_win,shape", [(601, dict(C=3, owners=201, last=1, trips=1)),
                                         (1279, dict(C=5, owners=256, last=4, trips=1)),
                                         (100, dict(C=1, owners=100, last=1, trips=1))])
def test_states_block_shapes(n_win, shape):
    N, T = 30, 9
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and states_launch(T, n_win) == shape
        eng.run(list(range(3, 3 + T)), ld=False)
        U.device_equals_twin(eng, T, what=f"{n_win} windows")
        # with penalties of about a bit the paths switch state often: inside blocks and across their borders
        _, path, _, _ = U.device_equals_twin(eng, T, pen=(0.5, 0.25, 0.5), what=f"{n_win} windows, small penalties")
        sw = np.nonzero(path[:, 1:] != path[:, :-1])[1] + 1
        assert len(sw) > 0
        if shape["C"] > 1:
            assert (sw % shape["C"] == 0).any() and (sw % shape["C"] != 0).any()


@pytest.mark.parametrize("ld", [True, False])
def test_log_llr_sums_past_the_block_cap(ld):
    """The case of test_gpu_launch_trips.test_llr_sums_past_the_block_cap through the log instantiation: 61 x 50 x 3 = 9150
    items for 8192 blocks; the same ranges ten at a time (no launch on a second trip) return the same bytes."""
    N, T = 70, 61
    alle, nr, na = random_case(31, N=N, L=12000)
    targets = [int(t) for t in np.random.default_rng(61).choice(N, size=T, replace=False)]
    with engine(alle, nr, na, 2) as e:
        n = e.n_windows
        first, end = llr_ranges(n)
        k = llr_launch(T, first, end)
        assert len(first) == 50 and k == dict(nb=3, items=9150, trips=2), (n, k)
        e.run(targets, ld=ld)
        _, got = U.log_sums_match_model(e, T, first, end)
        assert (got[:, 0] == 0).all() and got[:, 1].any()
        beyond = got.reshape(-1, 4)[cdiv(8192, k["nb"]):]
        assert len(beyond) > 0 and np.count_nonzero(np.nan_to_num(beyond)) > len(beyond)
        parts = []
        for s in range(0, 50, 10):
            assert llr_launch(T, first[s:s + 10], end[s:s + 10])["trips"] == 1
            parts.append(e.window_log2_llr_sums(first[s:s + 10], end[s:s + 10]))
        assert np.concatenate(parts, axis=1).tobytes() == got.tobytes()
