"""GPU tier: ibdg_window_llr_sums (segmented sums of the window log-likelihood ratios on the device) and the host
program's --arm-stats / --stats-only on a device.

Through the ABI the sums are checked against a numpy long-double model built from window_ll_all of the same run:
|hi - model| <= 2^-50 * sum(|log2 L2'| + |log2 L0'|) (and the same with L1' for the second sum), L' = L or 2^-1074."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import armstats_check as A                        # noqa: E402
from ibdgem_amd import engine as E                # noqa: E402
from test_gpu_precision import band_case, span_case   # noqa: E402

pytestmark = pytest.mark.gpu
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
LD_CASES = ["synA/ld_default", "synA/ld_bg_self_nan", "synA/ld_bg20_w64", "synA/ld_varsites", "synB/ld_w37"]
ALL_CASES = LD_CASES + ["synA/nonld_flags", "synA/nonld_all_targets_w2"]
RANGES = ["both", "p_nan", "p_zero", "c0_at_end", "c1_at_start"]


def model(wall, first, end):
    """[T][n_seg][2] long-double sums and their bounds."""
    L = np.where(wall == 0, 2.0 ** -1074, wall).astype(np.longdouble)
    with np.errstate(invalid="ignore"):
        lg = np.log2(L)
    a, b = lg[..., 2] - lg[..., 0], lg[..., 1] - lg[..., 0]
    ea, eb = np.abs(lg[..., 2]) + np.abs(lg[..., 0]), np.abs(lg[..., 1]) + np.abs(lg[..., 0])
    T = wall.shape[0]
    sums = np.zeros((T, len(first), 2), dtype=np.longdouble)
    bounds = np.zeros((T, len(first), 2))
    for s, (f, e) in enumerate(zip(first, end)):
        sums[:, s, 0], sums[:, s, 1] = a[:, f:e].sum(axis=1), b[:, f:e].sum(axis=1)
        with np.errstate(invalid="ignore"):
            bounds[:, s, 0] = ea[:, f:e].sum(axis=1).astype(np.float64) * 2.0 ** -50
            bounds[:, s, 1] = eb[:, f:e].sum(axis=1).astype(np.float64) * 2.0 ** -50
    return sums, bounds


def check_against_model(eng, T, first, end):
    wall = eng.window_ll_all(T)
    got = eng.window_llr_sums(first, end)
    assert got.shape == (T, len(first), 4)
    want, bound = model(wall, first, end)
    for k in range(2):
        hi = got[..., 2 * k]
        nan = np.isnan(np.float64(want[..., k]))
        assert (np.isnan(hi) == nan).all()
        err = np.abs(hi[~nan].astype(np.longdouble) - want[..., k][~nan]).astype(np.float64)
        assert (err <= bound[..., k][~nan]).all(), (k, err.max(), bound[..., k][~nan].min())
        assert (np.abs(got[..., 2 * k + 1][~nan]) <= np.abs(hi[~nan]) * 2.0 ** -52).all()     # a normalised double-double
    return wall, got


def segments(n):
    return [5, 3, 0, 2, 10, 0, n], [5, 4, n, 40, n, n - 1, n]     # empty, one window, all, overlapping ranges, ...


def random_case(seed, N=100, L=3000):
    rng = np.random.default_rng(seed)
    f = np.clip(rng.beta(0.3, 1.0, size=L), 1e-3, 0.999)
    alle = (rng.random((L, 2 * N)) < f[:, None]).astype(np.uint8)
    cov = np.minimum(rng.poisson(2.0, size=L), 20)
    n_alt = rng.binomial(cov, f).astype(np.uint8)
    return alle, (cov - n_alt).astype(np.uint8), n_alt


@pytest.fixture(scope="module")
def eng():
    alle, nr, na = random_case(11)
    with E.Engine(0, 0.02, 20) as e:
        e.upload_panel(E.pack_alleles_fast(alle), alle.shape[1] // 2)
        e.upload_sites(np.arange(len(nr)), nr, na, 50)
        yield e


@pytest.mark.parametrize("ld", [True, False])
def test_sums_match_the_long_double_model(eng, ld):
    n = eng.n_windows
    first, end = segments(n)
    rows = {}
    for T in (1, 2, 15, 16, 30, 61):
        targets = [(7 + 3 * i) % 100 for i in range(T)]
        eng.run(targets, ld=ld)
        wall, got = check_against_model(eng, T, first, end)
        assert (got[:, 0, :] == 0).all()                           # the empty range
        for t, tgt in enumerate(targets):                          # same window rows -> the same sums, bit for bit
            key = wall[t].tobytes()
            if key in rows:
                assert rows[key].tobytes() == got[t].tobytes(), (T, tgt)
            rows[key] = got[t].copy()
    if not ld:                                                     # (the non-LD tables of an individual never change)
        assert len(rows) < sum((1, 2, 15, 16, 30, 61))


def dd_add(x, hi, lo):
    """The host program's double-double addition (ibdgem.c dd_add), in Python floats (no fused multiply-add)."""
    s = x[0] + hi
    bb = s - x[0]
    e = (x[0] - (s - bb)) + (hi - bb)
    e += x[1] + lo
    h = s + e
    return [h, e - (h - s)]


@pytest.mark.parametrize("ld", [True, False])
def test_ranges_of_several_blocks_of_windows(ld):
    """Window 2 over ~10 000 covered rows: ~5 000 windows, so a range spans up to three blocks of 2048 (k_llr_partial's
    offsets, the empty tail blocks of the shorter ranges of a launch, k_llr_combine's ordered sum).  Ranges start and end
    off the block boundaries.  A range cut in two anywhere -- at, beside or away from a block boundary -- and its parts'
    double-doubles added as the host program adds its devices' gives the whole range's sum to the bit; so does the same
    individual in a run of another size."""
    alle, nr, na = random_case(21, N=40, L=12000)
    with E.Engine(0, 0.02, 20) as e:
        e.upload_panel(E.pack_alleles_fast(alle), 40)
        e.upload_sites(np.arange(len(nr)), nr, na, 2)
        n = e.n_windows
        assert n > 2 * 2048 + 600, n
        first = [0, 1, 2047, 100, 5, 3000, 2048, n - 2049, 10, 4095]
        end = [n, n - 1, 2049, 2148, 4101, 3001, 4096, n, 10, n - 3]
        targets = list(range(0, 30))
        e.run(targets, ld=ld)
        _, got = check_against_model(e, 30, first, end)
        assert got[:, 1].any() and (got[:, 8] == 0).all()
        a, b = 1, n - 1
        cuts = [2, 2047, 2048, 2049, 2050, 4095, 4096, 4097, n // 2, n - 2]
        parts = e.window_llr_sums([a] * len(cuts) + cuts, cuts + [b] * len(cuts))
        whole = e.window_llr_sums([a], [b])
        for t in range(30):
            for c in range(len(cuts)):
                for k in (0, 2):
                    acc = dd_add([0.0, 0.0], parts[t, c, k], parts[t, c, k + 1])
                    acc = dd_add(acc, parts[t, len(cuts) + c, k], parts[t, len(cuts) + c, k + 1])
                    assert acc[0] + acc[1] == whole[t, 0, k], (t, cuts[c], k)
        wall30 = e.window_ll_all(30)
        sums30 = e.window_llr_sums(first, end)
        e.run([7], ld=ld)
        if e.window_ll_all(1)[0].tobytes() == wall30[7].tobytes():
            assert e.window_llr_sums(first, end)[0].tobytes() == sums30[7].tobytes()
        elif not ld:
            raise AssertionError("a non-LD window table changed with the run's size")


def test_errors(eng):
    n = eng.n_windows
    eng.run([3], ld=True)
    for first, end in (([4], [3]), ([0], [n + 1]), ([n + 1], [n + 1])):
        with pytest.raises(E.EngineError, match="ibdg_window_llr_sums"):
            eng.window_llr_sums(first, end)
    assert eng.window_llr_sums([], []).shape == (1, 0, 4)
    assert eng.lib.ibdg_window_llr_sums(eng.ctx, None, None, 1, None) != 0
    alle, nr, na = random_case(12, N=20, L=300)
    with E.Engine(0, 0.02, 20) as fresh:
        fresh.upload_panel(E.pack_alleles_fast(alle), 20)
        fresh.upload_sites(np.arange(len(nr)), nr, na, 50)
        with pytest.raises(E.EngineError, match="no results"):
            fresh.window_llr_sums([0], [1])


def test_nan_windows_of_an_empty_background(eng):
    bg = np.zeros(100, dtype=np.uint8)
    bg[3] = 1                                                      # the only background individual is the compared one
    eng.run([3], ld=True, bg_count=bg)
    n = eng.n_windows
    wall, got = check_against_model(eng, 1, [0, 2, 7], [n, 3, 7])
    assert np.isnan(wall[0, :, 0]).all()
    assert np.isnan(got[0, :2, [0, 2]]).all() and (got[0, 2] == 0).all()


def test_windows_that_underflow():
    """The inputs of test_gpu_precision's underflow bands: L0 / L2 down to subnormals and zero (2^-1074 in the terms)."""
    eps, M, N, W = 0.02, 20, 64, 100
    seen_tiny = False
    for (alle, nr, na), e in ((band_case(N, W, eps), eps), (span_case(N, W, 1e-5), 1e-5)):
        with E.Engine(0, e, M) as eng:
            eng.upload_panel(E.pack_alleles_fast(alle), N)
            eng.upload_sites(np.arange(len(nr)), nr, na, W)
            n = eng.n_windows
            for ld in (True, False):
                targets = [0, 5, 17, 40, 50, 63]
                eng.run(targets, ld=ld)
                wall, _ = check_against_model(eng, len(targets), [0, 0, n // 2], [n, 1, n])
                seen_tiny |= bool(((wall == 0) | (np.abs(wall) < 2.0 ** -1022)).any())
    assert seen_tiny


def _run(args, cwd, out, extra_env=None):
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([EXE] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, **(extra_env or {})))
    assert res.returncode == 0, res.stderr
    return res


@pytest.mark.parametrize("key", ALL_CASES)
def test_cli_arm_stats_match_the_script(key, tmp_path):
    args, inp = A.run_args(key)
    g = A.golden()["cases"][key]["ranges"]
    near = 0
    for rname in RANGES:
        if rname not in g:
            continue
        c0, c1 = g[rname]["range"]
        _run(args + ["--arm-stats", f"{c0},{c1}", "--summary-only"], inp, tmp_path / rname)
        near += A.check(A.read_armstats(str(tmp_path / rname / "UNKWN.armstats.txt")), key, rname)
    print(f"{key}: {near} values at a %.3e rounding boundary")


@pytest.mark.parametrize("key", ["synA/ld_default", "synA/ld_varsites", "synA/nonld_all_targets_w2", "synB/ld_w37"])
def test_cli_arm_stats_identical_over_several_contexts(key, tmp_path):
    args, inp = A.run_args(key)
    c0, c1 = A.golden()["cases"][key]["ranges"]["c1_at_start"]["range"]
    files = []
    for devices in ("0", "0,0", "0,0,0"):
        out = tmp_path / devices.replace(",", "_")
        _run(args + ["--arm-stats", f"{c0},{c1}", "--stats-only", "--devices", devices], inp, out)
        files.append((out / "UNKWN.armstats.txt").read_bytes())
    assert files[0] == files[1] == files[2]


def test_cli_61_individuals_stats_only_equals_summary_only(tmp_path):
    """Three batches of the engine (30 + 30 + 1), the next one queued while the host goes through the last: the armstats
    file is the same whether the window tables come back (--summary-only) or not (--stats-only)."""
    args, inp = A.run_args("synA/ld_default")
    i = args.index("-s")
    args = args[:i] + ["-s", ",".join(f"ind{(3 + 11 * k) % 70}" for k in range(61))] + args[i + 2:]
    c0, c1 = A.golden()["cases"]["synA/ld_default"]["ranges"]["both"]["range"]
    _run(args + ["--arm-stats", f"{c0},{c1}", "--summary-only"], inp, tmp_path / "s")
    _run(args + ["--arm-stats", f"{c0},{c1}", "--stats-only"], inp, tmp_path / "o")
    a = (tmp_path / "s" / "UNKWN.armstats.txt").read_bytes()
    assert a == (tmp_path / "o" / "UNKWN.armstats.txt").read_bytes()
    assert len(a.splitlines()) == 62
    assert os.listdir(tmp_path / "o") == ["UNKWN.armstats.txt"]
    assert len([f for f in os.listdir(tmp_path / "s") if f.endswith(".summary.txt")]) == 61
