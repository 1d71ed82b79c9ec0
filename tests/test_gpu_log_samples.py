"""GPU tier: k_log2_alpha and k_log2_sample_paths (ibdg_window_log2_samples, ibdg_get_log2_sample_path) against the host twin
on every byte, on the run's own log tables: every blocking shape, the grid stride past its first trip, chains, shifts and
positions, more than one chunk of pairs; that a draw does not depend on the batch; that the kept alpha goes stale when it
must; and the host program's routes with --sample-paths."""
import os
import subprocess

import numpy as np
import pytest

import armstats_check as A
import log_states_util as U
from ibdgem_amd import engine as E
from test_gpu_log_states_trips import engine

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
SMALL = (0.5, 0.25, 0.5)
SIZES = [1, 2, 3, 255, 256, 257, 513, 1279]
BIT = 65536


def positions(n, seed=3):
    rng = np.random.default_rng(seed)
    first = np.cumsum(rng.integers(1, 5000, n)).astype(np.uint64) * 2
    return first, first + rng.integers(0, 2000, n).astype(np.uint64)


def chain_starts(n):
    C = (n + 255) // 256
    return sorted({w for w in (1, C if C > 1 else 2, n - 1) if 1 <= w < n})


def shifts(n, seed=5):
    rng = np.random.default_rng(seed)
    sh = rng.integers(-3 * BIT, 3 * BIT, n).astype(np.int32)
    sh[rng.random(n) < 0.1] = -(1 << 30)
    sh[rng.random(n) < 0.1] = 1 << 30
    return sh


def device_equals_twin(eng, T, K, pen, seed, streams, starts=(), shift=None, pos=(None, None), what=""):
    """Every byte of out against the twin on the run's tables, and three draws' paths drawn again.  Returns out."""
    tabs = eng.window_log2_all(T)
    out = eng.window_log2_samples(*pen, K, seed, streams, *pos)
    assert out.shape == (T, K, 15)
    again = sorted({(0, 0), (T - 1, K - 1), (T // 2, K // 2)})
    for t in range(T):
        paths, want = E.log2_samples_host(tabs[t], *pen, K, seed, int(streams[t]), pos_first=pos[0], pos_last=pos[1],
                                          starts=starts if len(starts) else None, shift=shift)
        assert out[t].tobytes() == want.tobytes(), f"{what}: records of individual {t}"
        for tt, k in again:
            if tt == t:
                assert eng.get_log2_sample_path(t, k).tobytes() == paths[k].tobytes(), f"{what}: path of draw {k} of individual {t}"
    assert (out[:, :, :3].sum(axis=2) == eng.n_windows).all()
    return out


@pytest.mark.parametrize("n_win", SIZES)
def test_sizes(n_win, monkeypatch):
    N, T = 30, 5
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    pos = positions(n_win)
    streams = np.arange(3, 3 + T, dtype=np.uint64)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win
        eng.run(list(range(3, 3 + T)), ld=False)
        # T K = 1500 pairs for 1024 workgroups: 476 take a second pair
        whole = device_equals_twin(eng, T, 300, SMALL, 7, streams, pos=pos, what=f"{n_win} windows, K = 300")
        assert len({whole[0, k].tobytes() for k in range(300)}) > 1 or n_win < 3
        device_equals_twin(eng, T, 1, U.PEN, 7, streams, what=f"{n_win} windows, K = 1")
        # chunks of 7 pairs: the host's loop runs 215 times and ends on a chunk of 2
        monkeypatch.setenv("IBDG_SAMPLE_SCRATCH_BYTES", str(7 * (n_win + 8 * 28)))
        chunked = eng.window_log2_samples(*SMALL, 300, 7, streams, *pos)
        monkeypatch.delenv("IBDG_SAMPLE_SCRATCH_BYTES")
        assert chunked.tobytes() == whole.tobytes()
        if n_win >= 2:
            st, sh = chain_starts(n_win), shifts(n_win)
            eng.set_window_chains(st)
            device_equals_twin(eng, T, 3, SMALL, 8, streams, starts=st, pos=pos, what=f"{n_win} windows, chains")
            eng.set_window_steps(sh)
            device_equals_twin(eng, T, 3, SMALL, 8, streams, starts=st, shift=sh, what=f"{n_win} windows, chains and shifts")
            eng.set_window_chains(())
            device_equals_twin(eng, T, 3, U.PEN, 8, streams, shift=sh, pos=pos, what=f"{n_win} windows, shifts")
            eng.set_window_steps(None)
        # one individual
        eng.run([11], ld=False)
        device_equals_twin(eng, 1, 300, SMALL, 9, np.array([11], dtype=np.uint64), what=f"{n_win} windows, T = 1")
        device_equals_twin(eng, 1, 3, SMALL, 9, np.array([11], dtype=np.uint64), pos=pos, what=f"{n_win} windows, T = 1, K = 3")


def test_a_draw_does_not_depend_on_the_batch():
    N, n_win, K = 40, 257, 50
    alle, nr, na = U.covered_reads(21, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        eng.run([9], ld=False)
        alone = eng.window_log2_samples(*SMALL, K, 5, np.array([9], dtype=np.uint64))
        batch = [20 + i for i in range(16)]
        batch[7] = 9
        eng.run(batch, ld=False)
        many = eng.window_log2_samples(*SMALL, K, 5, np.array(batch, dtype=np.uint64))
        assert many[7].tobytes() == alone[0].tobytes()
        assert many[6].tobytes() != alone[0].tobytes()
        other = eng.window_log2_samples(*SMALL, K, 5, np.array([b + 100 for b in batch], dtype=np.uint64))
        assert other[7].tobytes() != alone[0].tobytes()              # the stream, not the slot, is what a draw is keyed by


def test_staleness_and_the_posteriors_beside_it():
    N, n_win, T, K = 30, 513, 4, 5
    alle, nr, na = U.covered_reads(31, 2 * n_win, N)
    streams = np.arange(T, dtype=np.uint64)
    st, sh = chain_starts(n_win), shifts(n_win)

    def fresh(targets, pen, starts=(), shift=None):
        with engine(alle, nr, na, 2) as e2:
            if len(starts):
                e2.set_window_chains(starts)
            if shift is not None:
                e2.set_window_steps(shift)
            e2.run(targets, ld=False)
            return e2.window_log2_samples(*pen, K, 3, streams).tobytes()

    with engine(alle, nr, na, 2) as eng:
        a, b = [1, 2, 3, 4], [5, 6, 7, 8]
        eng.run(a, ld=False)
        before = [x.tobytes() for x in eng.window_log2_posteriors(*SMALL)]
        assert eng.window_log2_samples(*SMALL, K, 3, streams).tobytes() == fresh(a, SMALL)
        assert [x.tobytes() for x in eng.window_log2_posteriors(*SMALL)] == before
        assert eng.window_log2_samples(*U.PEN, K, 3, streams).tobytes() == fresh(a, U.PEN)                  # new penalties
        eng.set_window_chains(st)
        with pytest.raises(E.EngineError, match="ibdg_get_log2_sample_path: no ibdg_window_log2_samples call"):
            eng.get_log2_sample_path(0, 0)
        assert eng.window_log2_samples(*U.PEN, K, 3, streams).tobytes() == fresh(a, U.PEN, st)              # new chains
        eng.set_window_steps(sh)
        assert eng.window_log2_samples(*U.PEN, K, 3, streams).tobytes() == fresh(a, U.PEN, st, sh)          # new steps
        eng.run(b, ld=False)
        assert eng.window_log2_samples(*U.PEN, K, 3, streams).tobytes() == fresh(b, U.PEN, st, sh)          # a new run
        assert fresh(a, U.PEN) != fresh(b, U.PEN) != fresh(a, SMALL)


# ---- the host program --------------------------------------------------------------------------------------------------

def _run(args, cwd, out):
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([EXE] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))}


def _devices():
    import torch
    return torch.cuda.device_count()


@pytest.mark.parametrize("key,more", [("synA/ld_default", []), ("synA/nonld_all_targets_w2", ["--posteriors", "--segments"]),
                                      ("synB/ld_w37", ["--chain-gap", "20000", "--switch-scale", "5000"])])
def test_cli_every_route_gives_the_same_bytes(key, more, tmp_path):
    """The routes of test_gpu_log_posteriors.py with --sample-paths: one context and --stats-only draws on the device and 120 K
    bytes per individual leave it; two contexts, or files per individual, run the twin on the gathered tables."""
    args, inp = A.run_args(key)
    stats = ["--log-stats", "--states", "--p01", "0.05", "--p02", "0.01", "--p12", "0.05"] + more
    smp = stats + ["--sample-paths", "60", "--seed", "7"]
    full = _run(args + smp + ["--summary-only", "--devices", "0"], inp, tmp_path / "full")
    only = {d: _run(args + smp + ["--stats-only", "--devices", d], inp, tmp_path / f"only{len(d)}") for d in ("0", "0,0")}
    per = [fn for fn in full if fn.endswith(".logsamples.txt")]
    assert len(per) >= 2 and len(per) == len([fn for fn in full if fn.endswith(".loghiddengem.txt")])
    assert "UNKWN.logibdsamples.txt" in only["0"] and not [fn for fn in only["0"] if fn.endswith(".logsamples.txt")]
    assert sorted(only["0"]) == sorted(only["0,0"])
    for fn, data in only["0"].items():
        assert data == full[fn] == only["0,0"][fn], fn
    rows = [l.split("\t") for l in full["UNKWN.logibdsamples.txt"].decode().splitlines()]
    assert len(rows) == len(per) + 2 and all(r[2] == "60" for r in rows[1:])
    if _devices() >= 2:
        two = _run(args + smp + ["--stats-only", "--devices", "0,1"], inp, tmp_path / "two")
        assert two == only["0"]
    # every file the run writes without the option is unchanged
    plain = _run(args + stats + ["--summary-only", "--devices", "0"], inp, tmp_path / "plain")
    assert sorted(plain) == sorted(fn for fn in full if fn not in per and fn != "UNKWN.logibdsamples.txt")
    for fn, data in plain.items():
        assert full[fn] == data, fn


def test_errors():
    alle, nr, na = U.covered_reads(3, 40, 20)
    fn = "ibdg_window_log2_samples"
    with engine(alle, nr, na, 2) as eng:
        s = np.array([1, 2], dtype=np.uint64)
        with pytest.raises(E.EngineError, match=fn + ": no results"):
            eng.window_log2_samples(*U.PEN, 1, 1, np.zeros(0, dtype=np.uint64))
        eng.run([1, 2], ld=False)
        n = eng.n_windows
        with pytest.raises(E.EngineError, match=fn + r": p\d\d = .* is not in \(0, 1\]"):
            eng.window_log2_samples(0.0, 0.5, 0.5, 1, 1, s)
        for K in (0, 65537):
            with pytest.raises(E.EngineError, match=fn + f": n_samples = {K} is not in 1 .. 65536"):
                eng.window_log2_samples(*U.PEN, K, 1, s)
        pos = np.arange(n, dtype=np.uint64)
        with pytest.raises(E.EngineError, match=fn + ": pos_first without pos_last"):
            eng.window_log2_samples(*U.PEN, 1, 1, s, pos_first=pos)
        with pytest.raises(E.EngineError, match=fn + ": pos_last without pos_first"):
            eng.window_log2_samples(*U.PEN, 1, 1, s, pos_last=pos)
        with pytest.raises(E.EngineError, match=fn + ": window 0 ends at 0, before its start 1"):
            eng.window_log2_samples(*U.PEN, 1, 1, s, pos_first=pos + np.uint64(1), pos_last=pos)
        out = np.zeros((2, 1, 15), dtype=np.uint64)
        assert eng.lib.ibdg_window_log2_samples(eng.ctx, 0.5, 0.5, 0.5, 1, 1, s.ctypes.data, None, None, None) != 0
        assert "NULL out" in eng.lib.ibdg_last_error(eng.ctx).decode()
        assert eng.lib.ibdg_window_log2_samples(eng.ctx, 0.5, 0.5, 0.5, 1, 1, None, None, None, out.ctypes.data) != 0
        assert "NULL stream" in eng.lib.ibdg_last_error(eng.ctx).decode()
        with pytest.raises(E.EngineError, match="ibdg_get_log2_sample_path: no ibdg_window_log2_samples call"):
            eng.get_log2_sample_path(0, 0)
        eng.window_log2_samples(*U.PEN, 2, 1, s)
        with pytest.raises(E.EngineError, match="ibdg_get_log2_sample_path: individual 2 of 2"):
            eng.get_log2_sample_path(2, 0)
        with pytest.raises(E.EngineError, match="ibdg_get_log2_sample_path: draw 2 of 2"):
            eng.get_log2_sample_path(0, 2)
        eng.set_option("log_windows", 0)
        eng.run([1, 2], ld=False)
        with pytest.raises(E.EngineError, match="option log_windows"):
            eng.window_log2_samples(*U.PEN, 1, 1, s)
