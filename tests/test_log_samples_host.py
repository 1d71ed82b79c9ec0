"""ibdg_log2_samples_host: IBD-state paths drawn from the posterior on the host, no device.

The twin against the restatement of tests/hp_sample_ref.py byte for byte; the two facts of the definition (a state of weight 0
is never drawn, x < D); the draws' distribution against the exact path distribution of small tables and against the twin's own
gamma at 1279 windows, within binomial bars, with three wrong samplers that the same bars catch; what a draw depends on; the
errors."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import hp_sample_ref as R
from ibdgem_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 255, 256, 257, 513, 1279]
DEFAULT = (1e-3, 1e-6, 1e-3)
SOFT = (0.05, 0.01, 0.05)
SEED = 20260131                                 # the constant of the statistical tests (the first one tried)
BIT = 65536


@pytest.fixture(scope="module", autouse=True)
def library():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)


def random_table(n, seed=0, spread=30.0):
    rng = np.random.default_rng(1000 * n + seed)
    return rng.normal(-3000.0, 400.0, (n, 1)) + rng.uniform(-spread, spread, (n, 3))


def positions(n, seed=3):
    rng = np.random.default_rng(seed)
    first = np.cumsum(rng.integers(1, 5000, n)).astype(np.uint64) * 2
    return first, first + rng.integers(0, 2000, n).astype(np.uint64)


def chain_starts(n):
    """1, a block's first window and n - 1 (what of them the table has)."""
    C_ = R.H.blocking(n)[0]
    return sorted({w for w in (1, C_ if C_ > 1 else 2, n - 1) if 1 <= w < n})


def hard_shifts(n, seed=5):
    """Moderate shifts, with switch weights driven to 0 (below 2^-1000) and up to the cap on the way."""
    rng = np.random.default_rng(seed)
    sh = rng.integers(-3 * BIT, 3 * BIT, n).astype(np.int32)
    sh[rng.random(n) < 0.1] = -(1 << 30)
    sh[rng.random(n) < 0.1] = 1 << 30
    return sh


def special_table(kind, n):
    tab = random_table(n, seed=7, spread=3.0)
    idx = sorted({0, n // 3, n // 2, n - 1})
    if kind == "nan":
        for i in idx:
            tab[i, i % 3] = math.nan
        tab[n // 2] = math.nan
    elif kind == "deep":                          # emissions below 2^-1000: a state of weight 0 in alpha
        for j, i in enumerate(idx):
            tab[i, j % 3] = tab[i].max() - 2000.0
        if n > 4:
            tab[n // 4, 0] = tab[n // 4, 1] = tab[n // 4, 2] - 1500.0
    return tab


def cases(n):
    """(name, table, penalties, starts, shift) for a size."""
    out = [("plain", random_table(n), DEFAULT, (), None), ("soft", random_table(n, 1, 3.0), SOFT, (), None)]
    if n >= 2:
        out.append(("chains", random_table(n, 2, 3.0), SOFT, chain_starts(n), None))
        out.append(("shifts", random_table(n, 3, 3.0), SOFT, (), hard_shifts(n)))
        out.append(("chains+shifts", random_table(n, 4, 3.0), DEFAULT, chain_starts(n), hard_shifts(n, 6)))
    out.append(("nan", special_table("nan", n), SOFT, (), None))
    out.append(("deep", special_table("deep", n), SOFT, (), hard_shifts(n, 8) if n >= 2 else None))
    return out


def twin(tab, pen, K, seed, stream, starts=(), shift=None, pos=None, want_paths=True):
    pf, pl = pos if pos is not None else (None, None)
    return E.log2_samples_host(tab, *pen, K, seed, stream, pos_first=pf, pos_last=pl, want_paths=want_paths,
                               starts=starts if len(starts) else None, shift=shift)


# ---- twin == restatement ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_twin_equals_restatement(n, K):
    assert [R.H.blocking(m)[0] for m in (256, 257, 1279)] == [1, 2, 5]
    pos = positions(n)
    for name, tab, pen, starts, shift in cases(n):
        m = R.Model(tab, pen, None if shift is None else shift.tolist(), starts)
        paths, out = twin(tab, pen, K, 77, 5, starts, shift, pos)
        _, bare = twin(tab, pen, K, 77, 5, starts, shift, None, want_paths=False)
        for k in range(K):
            want = R.draw(m, 77, 5, k)
            assert paths[k].tolist() == want, f"{name}: path of draw {k} at n_win {n}"
            assert out[k].tolist() == R.record(want, starts, *pos), f"{name}: record of draw {k} at n_win {n}"
            assert bare[k].tolist() == R.record(want, starts), f"{name}: record without positions"
            assert int(out[k, :3].sum()) == n and int(bare[k, 9:].sum()) == 0
        if name in ("chains+shifts", "deep"):
            # the kernel's way -- maps composed per block and scanned -- and any other blocking give the same path
            assert R.draw_by_maps(m, 77, 5, K - 1) == paths[K - 1].tolist()
            odd = [(w0, min(w0 + 7, n)) for w0 in range(0, n, 7)]
            assert R.draw_by_maps(m, 77, 5, K - 1, odd) == paths[K - 1].tolist()


def test_the_numbers():
    assert R.sm64(0) == 0xE220A8397B1DCDAF and R.sm64(1) == 0x910A2DEC89025CC1       # splitmix64's first outputs from 0 and 1
    assert 0.0 <= R.uniform(R.key(1, 2, 3), 4) < 1.0
    assert R.U_MAX == float((1 << 53) - 1) * 2.0 ** -53 < 1.0


def test_no_windows():
    paths, out = E.log2_samples_host(np.zeros((0, 3)), *DEFAULT, 4, 1, 0)
    out[:] = 7
    paths, out = E.log2_samples_host(np.zeros((0, 3)), *DEFAULT, 4, 1, 0)
    assert paths.shape == (4, 0) and out.shape == (4, 15) and not out.any()


# ---- the two facts -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_a_state_of_weight_zero_is_never_drawn(n):
    zeros = 0
    for name, tab, pen, starts, shift in cases(n):
        m = R.Model(tab, pen, None if shift is None else shift.tolist(), starts)
        paths, _ = twin(tab, pen, 3, 11, 2, starts, shift)
        for k in range(3):
            p = paths[k]
            for w in range(n):
                assert m.alpha[w][p[w]] > 0.0, f"{name}: draw {k} holds state {p[w]} at window {w}, where alpha is 0"
                if w:
                    assert R.weights_into(m.a[w], p[w])[p[w - 1]] > 0.0, f"{name}: draw {k} switches across a zero weight into {w}"
        # U at its largest: x < D, and what is picked has weight
        for w in range(n):
            for sp in range(3):
                c = R.candidates(m, w, sp)
                D = (c[0] + c[1]) + c[2]
                zeros += min(c) == 0.0
                if D >= 2.0 ** -1022:
                    assert R.U_MAX * D < D
                    assert c[R.pick(c, R.U_MAX)] > 0.0 and c[R.pick(c, 0.0)] > 0.0
                elif D == 0.0:
                    assert R.pick(c, R.U_MAX) == 2
        if name == "deep":
            worst = R.draw(m, 0, 0, 0, u_of=lambda k, w: R.U_MAX)
            assert all(m.alpha[w][worst[w]] > 0.0 for w in range(n))
    assert zeros > 0                                # the tables do hold weights of 0


# ---- the distribution --------------------------------------------------------------------------------------------------------

def small_tables():
    """Hand-built tables of 5 windows with their penalties and shifts: near-equal states; a state of weight 0; a chain start."""
    near = [[-100.0, -100.05, -99.95], [-200.0, -200.1, -200.0], [-50.0, -50.0, -50.0], [-10.2, -10.0, -10.1], [-7.0, -7.1, -7.05]]
    zero = [[-100.0, -101.0, -100.5], [-200.0, -199.0, -201.0], [-2300.0, -300.0, -301.0], [-10.0, -11.0, -10.5], [-7.0, -7.5, -8.0]]
    sh = [0, 2 * BIT, -2 * BIT, BIT, -3 * BIT]
    return [("near", near, (0.3, 0.1, 0.3), sh, ()), ("zero", zero, (0.3, 0.2, 0.1), sh, ()),
            ("chain", zero, (0.3, 0.2, 0.1), sh, (3,))]


def path_frequencies(paths):
    n = paths.shape[1]
    code = (paths.astype(np.int64) * 3 ** np.arange(n)).sum(axis=1)
    cnt = np.bincount(code, minlength=3 ** n)
    return {p: cnt[sum(s * 3 ** w for w, s in enumerate(p))] / len(paths) for p in R.product(range(3), repeat=n)}


def misses(freq, dist, K):
    return [p for p in dist if abs(freq[p] - float(dist[p])) > R.bar(dist[p], K)]


@pytest.mark.parametrize("case", small_tables(), ids=lambda c: c[0])
def test_exact_distribution_and_controls(case):
    name, tab, pen, sh, starts = case
    K = 20000
    m = R.Model(tab, pen, sh, starts)
    dist = R.path_distribution(m)
    assert len(dist) == 243 and sum(dist.values()) == 1
    paths, _ = twin(np.array(tab), pen, K, SEED, 0, starts, np.array(sh, dtype=np.int32))
    freq = path_frequencies(paths)
    assert misses(freq, dist, K) == []
    if name != "near":
        assert all(freq[p] == 0.0 for p in dist if dist[p] == 0) and any(dist[p] == 0 for p in dist)
    for variant in ("no_a", "shared_u", "a_of_w"):
        wrong = np.array([R.draw(m, SEED, 0, k, variant=variant) for k in range(K)], dtype=np.uint8)
        assert misses(path_frequencies(wrong), dist, K), f"{name}: the bars do not catch {variant}"


def test_marginals_at_1279_windows_and_controls():
    n, K = 1279, 2000
    tab = random_table(n, 9, 2.0)
    rng = np.random.default_rng(12)
    sh = rng.integers(-4 * BIT, 4 * BIT, n).astype(np.int32)
    post, _, _ = E.log2_posteriors_host(tab, *SOFT, shift=sh)
    paths, out = twin(tab, SOFT, K, SEED, 0, (), sh)
    freq = np.stack([(paths == s).mean(axis=0) for s in range(3)], axis=1)
    bars = 6.0 * np.sqrt(post * (1.0 - post) / K) + 2.0 / K
    assert (np.abs(freq - post) <= bars).all(), np.argwhere(np.abs(freq - post) > bars)[:5]
    assert (out[:, :3].sum(axis=0) == np.array([(paths == s).sum() for s in range(3)])).all()
    # the wrong samplers over the walk's first 64 windows (the table's last: a draw starts from the back)
    m = R.Model(tab, SOFT, sh.tolist())
    tail = range(n - 1, n - 65, -1)
    for variant in ("no_a", "shared_u", "a_of_w"):
        cnt = np.zeros((n, 3))
        for k in range(K):
            ky, st = R.key(SEED, 0, 0 if variant == "shared_u" else k), 0
            for w in tail:
                st = R.pick(R.candidates(m, w, st, variant), R.uniform(ky, w))
                cnt[w, st] += 1
        w = np.array(tail)
        assert (np.abs(cnt[w] / K - post[w]) > bars[w]).any(), f"the bars do not catch {variant}"


# ---- what a draw depends on --------------------------------------------------------------------------------------------------

def test_streams_and_prefixes():
    tab = random_table(257, 1, 2.0)
    p7, o7 = twin(tab, SOFT, 7, 9, 4)
    p3, o3 = twin(tab, SOFT, 3, 9, 4)
    assert p7[:3].tobytes() == p3.tobytes() and o7[:3].tobytes() == o3.tobytes()
    other, _ = twin(tab, SOFT, 3, 9, 5)
    reseeded, _ = twin(tab, SOFT, 3, 10, 4)
    assert other.tobytes() != p3.tobytes() and reseeded.tobytes() != p3.tobytes()
    assert len({p7[k].tobytes() for k in range(7)}) == 7
    big, _ = twin(tab, SOFT, 2, 2 ** 64 - 1, 2 ** 64 - 1)                       # the whole of both words counts
    m = R.Model(tab, SOFT)
    assert big[1].tolist() == R.draw(m, 2 ** 64 - 1, 2 ** 64 - 1, 1)


# ---- errors ------------------------------------------------------------------------------------------------------------------

def test_errors():
    tab = np.zeros((4, 3))
    fn = "ibdg_log2_samples_host"
    for p in [(0.0, 0.5, 0.5), (0.5, math.nan, 0.5), (0.5, 0.5, 1.5)]:
        with pytest.raises(E.EngineError, match=fn + r": p\d\d = .* is not in \(0, 1\]"):
            E.log2_samples_host(tab, *p, 1, 1, 0)
    for K in (0, 65537):
        with pytest.raises(E.EngineError, match=fn + f": n_samples = {K} is not in 1 .. 65536"):
            E.log2_samples_host(tab, *DEFAULT, K, 1, 0)
    with pytest.raises(E.EngineError, match=fn + r": starts\[0\] = 0"):
        E.log2_samples_host(tab, *DEFAULT, 1, 1, 0, starts=[0])
    with pytest.raises(E.EngineError, match=fn + r": starts\[1\] = 4 is not below the 4 windows"):
        E.log2_samples_host(tab, *DEFAULT, 1, 1, 0, starts=[1, 4])
    with pytest.raises(E.EngineError, match=fn + r": shift\[2\] = .* is not within"):
        E.log2_samples_host(tab, *DEFAULT, 1, 1, 0, shift=[0, 0, (1 << 30) + 1, 0])
    pos = np.arange(4, dtype=np.uint64)
    with pytest.raises(E.EngineError, match=fn + ": pos_first without pos_last"):
        E.log2_samples_host(tab, *DEFAULT, 1, 1, 0, pos_first=pos)
    with pytest.raises(E.EngineError, match=fn + ": pos_last without pos_first"):
        E.log2_samples_host(tab, *DEFAULT, 1, 1, 0, pos_last=pos)
    with pytest.raises(E.EngineError, match=fn + ": window 2 ends at 1, before its start 2"):
        E.log2_samples_host(tab, *DEFAULT, 1, 1, 0, pos_first=pos, pos_last=np.array([0, 1, 1, 3], dtype=np.uint64))
    lib = E.load_library()
    out = np.zeros(15, dtype=np.uint64)
    assert lib.ibdg_log2_samples_host(tab.ctypes.data, 4, 0.5, 0.5, 0.5, None, 0, None, 1, 1, 0, None, None, None, None) != 0
    assert "NULL out" in lib.ibdg_last_error(None).decode()
    assert lib.ibdg_log2_samples_host(None, 4, 0.5, 0.5, 0.5, None, 0, None, 1, 1, 0, None, None, None, out.ctypes.data) != 0
    assert "NULL table" in lib.ibdg_last_error(None).decode()
    assert lib.ibdg_log2_samples_host(tab.ctypes.data, (1 << 21) + 1, 0.5, 0.5, 0.5, None, 0, None, 1, 1, 0, None, None, None,
                                      out.ctypes.data) != 0
    assert "2^21" in lib.ibdg_last_error(None).decode()
    assert lib.ibdg_log2_samples_host(tab.ctypes.data, 4, 0.5, 0.5, 0.5, None, 0, None, 1, 1, 0, None, None, None, out.ctypes.data) == 0
    assert int(out[:3].sum()) == 4
