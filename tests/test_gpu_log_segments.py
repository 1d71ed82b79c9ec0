"""GPU tier: k_log2_segments_count / k_log2_segments_write (ibdg_window_log2_segments, ibdg_get_log2_segments) against the
host twin on the run's own log tables, on the shapes of tests/test_gpu_log_states_trips.py -- with penalty sets under which the
device's own records show every case of the blocking (a segment inside a block, across a border, over whole blocks, a block
full of starts) --, past the block cap, with the posteriors, the errors, and the host program's routes with --segments."""
import os
import subprocess

import numpy as np
import pytest

import armstats_check as A
import log_states_util as U
import segments_check as S
from ibdgem_amd import engine as E
from test_gpu_log_states_trips import engine, states_launch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
SMALL = (0.5, 0.25, 0.5)
DENSE = (1.0, 1.0, 1.0)


def positions(n):
    """Increasing positions with a window of a single site every fifth window."""
    first = np.arange(n, dtype=np.uint64) * np.uint64(1000) + np.uint64(17)
    last = first + np.where(np.arange(n) % 5 == 0, 0, 700).astype(np.uint64)
    return first, last


def split(seg, n_seg):
    """The records of every individual, cut from the compact array by the counts."""
    off = np.concatenate([[0], np.cumsum(n_seg.astype(np.int64))])
    assert off[-1] == len(seg)
    return [seg[off[t]:off[t + 1]] for t in range(len(n_seg))]


def device_equals_twin(eng, T, pen, what=""):
    """Counts, summaries and records of the last run, device against twin on the same tables: with and without posteriors,
    with and without positions, and the same bytes from a second call.  Returns the records per individual, of the call with
    posteriors and positions."""
    tabs = eng.window_log2_all(T)
    n = eng.n_windows
    pos = positions(n)
    out = None
    for with_post in (False, True):
        for pf, pl in ((None, None), pos):
            n_seg, summary = eng.window_log2_segments(*pen, with_post=with_post, pos_first=pf, pos_last=pl)
            seg = eng.get_log2_segments()
            assert n_seg.shape == (T,) and summary.shape == (T, 12) and len(seg) == int(n_seg.sum())
            per = split(seg, n_seg)
            for t in range(T):
                ws, wn, wsum = E.log2_segments_host(tabs[t], *pen, with_post=with_post, pos_first=pf, pos_last=pl)
                assert int(n_seg[t]) == wn, f"{what}: count of individual {t}"
                assert summary[t].tobytes() == wsum.tobytes(), f"{what}: summary of individual {t}"
                assert per[t].tobytes() == ws.tobytes(), f"{what}: records of individual {t} (posteriors {with_post})"
            n2, s2 = eng.window_log2_segments(*pen, with_post=with_post, pos_first=pf, pos_last=pl)
            assert n2.tobytes() == n_seg.tobytes() and s2.tobytes() == summary.tobytes()
            assert eng.get_log2_segments().tobytes() == seg.tobytes()
            assert eng.get_log2_segments().tobytes() == seg.tobytes()          # (the records again, without a new count)
            out = per
    return out


def blocks_of(per, n_win):
    """From the device's records and states_launch's C: per individual the block of every start and how many starts fall
    on a border, inside a block, and the whole blocks each segment covers."""
    C = states_launch(1, n_win)["C"]
    res = []
    for seg in per:
        first = seg["first"].astype(np.int64)
        end = first + seg["n_win"].astype(np.int64)
        # a block is whole inside [first, end) if it starts at or behind first and ends at or before end (the last block ends at n_win)
        whole = np.where(end == n_win, -(-end // C), end // C) - -(-first // C)
        res.append(dict(block=first // C, border=first % C == 0, whole=whole, C=C))
    return res


@pytest.mark.parametrize("n_win,shape,ld", [(601, dict(C=3, owners=201, last=1, trips=1), False),
                                            (1279, dict(C=5, owners=256, last=4, trips=1), False),
                                            (100, dict(C=1, owners=100, last=1, trips=1), False),
                                            (601, dict(C=3, owners=201, last=1, trips=1), True)])
def test_block_shapes(n_win, shape, ld):
    N, T = 30, 9
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and states_launch(T, n_win) == shape
        C = shape["C"]
        eng.run(list(range(3, 3 + T)), ld=ld)
        per = device_equals_twin(eng, T, U.PEN, what=f"{n_win} windows")
        if not ld:
            # the default penalties: one segment over all windows, no block but the first has a start
            for seg in per:
                assert len(seg) == 1 and int(seg[0]["first"]) == 0 and int(seg[0]["n_win"]) == n_win
        per = device_equals_twin(eng, T, SMALL, what=f"{n_win} windows, small penalties")
        info = blocks_of(per, n_win)
        print(f"{n_win} windows, ld {ld}, small penalties: segments per individual {[len(s) for s in per]}, largest span in whole "
              f"blocks {max(int(i['whole'].max()) for i in info)}, starts on a border "
              f"{[int(i['border'][1:].sum()) for i in info]}, most starts in a block "
              f"{max(int(np.bincount(i['block']).max()) for i in info)}")
        if not ld and n_win > 100:
            assert all(len(seg) > 1 for seg in per)
            assert {int(s) for seg in per for s in seg["state"]} == {0, 1, 2}
            assert any((i["whole"] >= 2).any() for i in info)
            assert any(i["border"][1:].any() for i in info) and any((~i["border"]).any() for i in info)
            if n_win == 1279:
                assert any((np.bincount(i["block"]) >= 2).any() for i in info)
        per = device_equals_twin(eng, T, DENSE, what=f"{n_win} windows, no penalties")
        info = blocks_of(per, n_win)
        print(f"{n_win} windows, ld {ld}, no penalties: segments per individual {[len(s) for s in per]}")
        if not ld and n_win == 1279:
            assert all(len(seg) > n_win / 3 for seg in per)
            assert any((np.bincount(i["block"], minlength=256)[:255] == C).any() for i in info)


def test_past_the_block_cap():
    """1100 individuals (of 40, repeated) for 1024 workgroups: 76 workgroups take a second individual and reuse their LDS; the
    compact record buffer's offsets run over all 1100 counts."""
    N, T, n_win = 40, 1100, 5
    alle, nr, na = U.covered_reads(5, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win
        assert states_launch(T, n_win) == dict(C=1, owners=5, last=1, trips=2)
        eng.run([t % N for t in range(T)], ld=False)
        per = device_equals_twin(eng, T, DENSE, what="past the block cap")
        for t in range(1024, T):
            assert per[t].tobytes() == per[t % N].tobytes()
        assert len({p.tobytes() for p in per}) > 1
        assert len({len(p) for p in per}) > 1            # (the offsets are not a multiple of one count)
        assert per[T - 1].tobytes() == per[(T - 1) % N].tobytes() and len(per[T - 1]) >= 1


def test_posteriors_in_the_records():
    N, T, n_win = 30, 3, 601
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        eng.run([4, 7, 11], ld=False)
        post, _, _ = eng.window_log2_posteriors(*SMALL)
        n_seg, _ = eng.window_log2_segments(*SMALL, with_post=True)
        per = split(eng.get_log2_segments(), n_seg)
        for t in range(T):
            assert len(per[t]) > 1
            for r in per[t]:
                f, n, s = int(r["first"]), int(r["n_win"]), int(r["state"])
                g = post[t, f:f + n, s]
                assert float(r["post_min"]) == float(g.min())
                assert int(r["post_q"]) == sum(round(float(x) * 2 ** 32) for x in g)      # (exact product, half to even)
        # without them the two fields are 0 and the rest is the same
        n0, _ = eng.window_log2_segments(*SMALL)
        bare = eng.get_log2_segments()
        full = np.concatenate(per)
        assert n0.tobytes() == n_seg.tobytes() and (bare["post_q"] == 0).all() and (bare["post_min"] == 0.0).all()
        for k in ("first", "n_win", "state", "reserved", "e"):
            assert bare[k].tobytes() == full[k].tobytes()


def test_errors():
    alle, nr, na = U.covered_reads(3, 40, 20)
    with engine(alle, nr, na, 2) as eng:
        with pytest.raises(E.EngineError, match="ibdg_window_log2_segments: no results"):
            eng.window_log2_segments(*U.PEN)
        with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
            eng.get_log2_segments(10)
        eng.run([1, 2], ld=False)
        n = eng.n_windows
        with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
            eng.get_log2_segments(10)
        for pen in ((0.0, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, float("nan")), (-1.0, 0.5, 0.5)):
            with pytest.raises(E.EngineError, match=r"ibdg_window_log2_segments: p\d\d = .* is not in \(0, 1\]"):
                eng.window_log2_segments(*pen)
        cnt, summ = np.zeros(2, dtype=np.uint64), np.zeros((2, 12), dtype=np.uint64)
        assert eng.lib.ibdg_window_log2_segments(eng.ctx, 0.5, 0.5, 0.5, 0, None, None, None, summ.ctypes.data) != 0
        assert eng.lib.ibdg_window_log2_segments(eng.ctx, 0.5, 0.5, 0.5, 0, None, None, cnt.ctypes.data, None) != 0
        pf, pl = positions(n)
        with pytest.raises(E.EngineError, match="ibdg_window_log2_segments: pos_first without pos_last"):
            eng.window_log2_segments(*U.PEN, pos_first=pf)
        with pytest.raises(E.EngineError, match="ibdg_window_log2_segments: pos_last without pos_first"):
            eng.window_log2_segments(*U.PEN, pos_last=pl)
        bad = pl.copy()
        bad[n - 1] = pf[n - 1] - np.uint64(1)
        with pytest.raises(E.EngineError, match=f"ibdg_window_log2_segments: window {n - 1} ends at"):
            eng.window_log2_segments(*U.PEN, pos_first=pf, pos_last=bad)
        with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
            eng.get_log2_segments(10)                                   # (none of the refused calls counts)
        per = device_equals_twin(eng, 2, DENSE)
        total = sum(len(p) for p in per)
        with pytest.raises(E.EngineError, match=f"ibdg_get_log2_segments: room for {total - 1} records, {total} are there"):
            eng.get_log2_segments(total - 1)
        assert len(eng.get_log2_segments(total + 5)) == total + 5       # (more room than records is fine)
        # a states or posteriors call rewrites the paths the records are cut from
        eng.window_log2_states(*U.PEN)
        with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
            eng.get_log2_segments(total)
        eng.window_log2_segments(*DENSE)
        eng.run([1, 2], ld=False)
        with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
            eng.get_log2_segments(total)
        eng.set_option("log_windows", 0)
        eng.run([1, 2], ld=False)
        with pytest.raises(E.EngineError, match="option log_windows"):
            eng.window_log2_segments(*U.PEN)


# ---- the host program --------------------------------------------------------------------------------------------------

def _run(args, cwd, out):
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([EXE] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))}


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("key", ["synA/ld_default", "synA/ld_varsites", "synA/nonld_all_targets_w2", "synB/ld_w37"])
def test_cli_every_route_gives_the_same_bytes(key, post, tmp_path):
    """The routes of test_gpu_log_posteriors.py with --segments: one context and --stats-only counts on the device and 104 bytes
    per individual leave it; two contexts, or files per individual, run the twin on the gathered tables."""
    args, inp = A.run_args(key)
    c0, c1 = A.golden()["cases"][key]["ranges"]["both"]["range"]
    stats = ["--log-stats", "--states", "--arm-stats", f"{c0},{c1}", "--p01", "0.05", "--p02", "0.01", "--p12", "0.05"]
    stats += ["--posteriors"] if post else []
    segs = stats + ["--segments"]
    full = {d: _run(args + segs + ["--summary-only", "--devices", d], inp, tmp_path / f"full{len(d)}") for d in ("0", "0,0")}
    only = {d: _run(args + segs + ["--stats-only", "--devices", d], inp, tmp_path / f"only{len(d)}") for d in ("0", "0,0")}
    run_files = ["UNKWN.logarmstats.txt", "UNKWN.logibdsegments.txt", "UNKWN.logibdstates.txt"]
    run_files = sorted(run_files + (["UNKWN.logibdposteriors.txt"] if post else []))
    assert sorted(only["0"]) == sorted(only["0,0"]) == run_files
    assert sorted(full["0"]) == sorted(full["0,0"])
    per = [fn for fn in full["0"] if fn.endswith(".logsegments.txt")]
    assert len(per) >= 2 and len(per) == len([fn for fn in full["0"] if fn.endswith(".loghiddengem.txt")])
    for fn in run_files + per:
        assert full["0"][fn] == full["0,0"][fn], fn
    for fn in run_files:
        assert only["0"][fn] == full["0"][fn] == only["0,0"][fn], fn
    # every logsegments.txt against its loghiddengem.txt and summary.txt, every row of logibdsegments.txt against its logsegments.txt
    lines = {}
    for fn in per:
        ind = fn.split(".")[1]
        lines[ind] = S.individual_consistent(full["0"][fn], full["0"][f"UNKWN.{ind}.loghiddengem.txt"],
                                             full["0"][f"UNKWN.{ind}.summary.txt"], post, fn)
    order = [l.split("\t")[0] for l in full["0"]["UNKWN.logibdsegments.txt"].decode().splitlines() if not l.startswith("#")]
    S.run_consistent(full["0"]["UNKWN.logibdsegments.txt"], {ind: lines[ind] for ind in order})
    # every file the run writes without the option is unchanged
    plain = _run(args + stats + ["--summary-only"], inp, tmp_path / "plain")
    assert sorted(plain) == sorted(fn for fn in full["0"] if fn not in per and fn != "UNKWN.logibdsegments.txt")
    for fn, data in plain.items():
        assert full["0"][fn] == data, fn


@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_stats_only_over_batches_of_individuals_equals_the_single_runs(devices, tmp_path):
    """31 individuals with --stats-only and every log-domain statistic: a batch of 30, then the one queued ahead of its
    statistics calls -- on one context the paths, posteriors and segments are found on the device, on two the tables are
    gathered for the host twins.  Only the statistics files are written, and an individual's line in each is the line of its
    run alone (which writes its files too)."""
    import batch_cases as B
    got = B.run(["--stats-only", "--devices", devices], B.NAMES, tmp_path)
    assert sorted(got) == sorted(B.STATS_FILES)
    B.check_statistics(got)
