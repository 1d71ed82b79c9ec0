"""What the GPU tests of the log-domain statistics share (test_gpu_log_states.py, test_gpu_log_states_trips.py)."""
import numpy as np

from ibdgem_amd import engine as E

PEN = (1e-3, 1e-6, 1e-3)            # the host program's default penalties


def covered_reads(seed, L, N, depth=2.0, max_cov=20):
    """A panel of N individuals over L rows and reads on EVERY row (so that n_win = ceil(L / window))."""
    rng = np.random.default_rng(seed)
    f = np.clip(rng.beta(0.3, 1.0, size=L), 1e-3, 0.999)
    alle = (rng.random((L, 2 * N)) < f[:, None]).astype(np.uint8)
    cov = np.clip(rng.poisson(depth, size=L), 1, max_cov)
    n_alt = rng.binomial(cov, f).astype(np.uint8)
    return alle, (cov - n_alt).astype(np.uint8), n_alt


def device_equals_twin(eng, T, pen=PEN, what=""):
    """ibdg_window_log2_states of the last run against ibdg_log2_states_host on the same run's tables: path, score and
    count bit for bit, and the same path / count when the scores (and the paths) are not asked for.  Returns
    (tables, path, score, count)."""
    tabs = eng.window_log2_all(T)
    path, score, count = eng.window_log2_states(*pen)
    n = eng.n_windows
    assert path.shape == (T, n) and score.shape == (T, n, 3) and count.shape == (T, 3)
    for t in range(T):
        wp, ws, wc = E.log2_states_host(tabs[t], *pen)
        assert path[t].tobytes() == wp.tobytes(), f"{what}: path of individual {t}"
        assert score[t].tobytes() == ws.tobytes(), f"{what}: scores of individual {t}"
        assert count[t].tobytes() == wc.tobytes(), f"{what}: counts of individual {t}"
    assert (count.sum(axis=1) == n).all() and (path <= 2).all()           # every window has a state
    p2, s2, c2 = eng.window_log2_states(*pen, want_score=False)
    assert s2 is None and p2.tobytes() == path.tobytes() and c2.tobytes() == count.tobytes()
    p3, s3, c3 = eng.window_log2_states(*pen, want_path=False, want_score=False)
    assert p3 is None and s3 is None and c3.tobytes() == count.tobytes()
    return tabs, path, score, count


def log_model(tabs, first, end):
    """The long-double model of ibdg_window_log2_llr_sums: the table's own entries summed, [T][n_seg][2], and the bound
    2^-50 * sum(|l2| + |l0|) (|l1| + |l0|) of tests/test_gpu_arm_stats.py."""
    lg = np.asarray(tabs, dtype=np.float64).astype(np.longdouble)
    a, b = lg[..., 2] - lg[..., 0], lg[..., 1] - lg[..., 0]
    ea, eb = np.abs(lg[..., 2]) + np.abs(lg[..., 0]), np.abs(lg[..., 1]) + np.abs(lg[..., 0])
    T = lg.shape[0]
    sums = np.zeros((T, len(first), 2), dtype=np.longdouble)
    bounds = np.zeros((T, len(first), 2))
    for s, (f, e) in enumerate(zip(first, end)):
        sums[:, s, 0], sums[:, s, 1] = a[:, f:e].sum(axis=1), b[:, f:e].sum(axis=1)
        with np.errstate(invalid="ignore"):
            bounds[:, s, 0] = ea[:, f:e].sum(axis=1).astype(np.float64) * 2.0 ** -50
            bounds[:, s, 1] = eb[:, f:e].sum(axis=1).astype(np.float64) * 2.0 ** -50
    return sums, bounds


def log_sums_match_model(eng, T, first, end):
    tabs = eng.window_log2_all(T)
    got = eng.window_log2_llr_sums(first, end)
    assert got.shape == (T, len(first), 4)
    want, bound = log_model(tabs, first, end)
    for k in range(2):
        hi = got[..., 2 * k]
        nan = np.isnan(np.float64(want[..., k]))
        assert (np.isnan(hi) == nan).all()
        err = np.abs(hi[~nan].astype(np.longdouble) - want[..., k][~nan]).astype(np.float64)
        assert (err <= bound[..., k][~nan]).all(), (k, err.max())
        assert (np.abs(got[..., 2 * k + 1][~nan]) <= np.abs(hi[~nan]) * 2.0 ** -52).all()     # a normalised double-double
    return tabs, got
