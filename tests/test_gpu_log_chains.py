"""GPU tier: window chains on the device.  ibdg_set_window_chains, then ibdg_window_log2_states / _posteriors /
_segments and ibdg_get_log2_segments against the _chains_host twins on the run's own log tables, on every byte: on the blocking
shapes of tests/test_gpu_log_states_trips.py with starts on, before and behind every block border; past the block cap; the
lifetime of the chains (the setter makes kept products stale, a run keeps the chains, a new site list clears them); the
setter's refusals; and the host program's routes with --chain-gap."""
import os
import subprocess

import numpy as np
import pytest

import armstats_check as A
import log_states_util as U
from ibdgem_amd import engine as E
from test_gpu_log_segments import positions, split
from test_gpu_log_states_trips import engine, states_launch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
SMALL = (0.5, 0.25, 0.5)


def start_sets(n_win):
    """Window 1; the last window; every block's first window w0 = k C, w0 - 1 and w0 + 1; two consecutive windows; every window."""
    C = states_launch(1, n_win)["C"]
    w0 = list(range(C, n_win, C))
    sets = {"first": [1], "last": [n_win - 1], "w0": w0, "w0-1": [w - 1 for w in w0], "w0+1": [w + 1 for w in w0],
            "two": [n_win // 2, n_win // 2 + 1], "every": list(range(1, n_win))}
    return {k: sorted(set(w for w in v if 1 <= w < n_win)) for k, v in sets.items()}


def device_equals_twin(eng, tabs, pen, starts, what):
    """Every product of the three calls with the chains that are set on `eng`, against the twins with `starts`."""
    T, n = len(tabs), eng.n_windows
    path, score, count = eng.window_log2_states(*pen)
    post, expect, log2_z = eng.window_log2_posteriors(*pen)
    twins = [(E.log2_states_host(tabs[t], *pen, starts=starts), E.log2_posteriors_host(tabs[t], *pen, starts=starts)) for t in range(T)]
    for t, ((wp, ws, wc), (wpost, wexp, wz)) in enumerate(twins):
        assert path[t].tobytes() == wp.tobytes(), f"{what}: path of individual {t}"
        assert score[t].tobytes() == ws.tobytes(), f"{what}: scores of individual {t}"
        assert count[t].tobytes() == wc.tobytes(), f"{what}: counts of individual {t}"
        assert post[t].tobytes() == wpost.tobytes(), f"{what}: posteriors of individual {t}"
        assert expect[t].tobytes() == wexp.tobytes(), f"{what}: expect of individual {t}"
        assert np.float64(log2_z[t]).tobytes() == np.float64(wz).tobytes(), f"{what}: log2 Z of individual {t}"
    pos = positions(n)
    for with_post in (False, True):
        for pf, pl in ((None, None), pos):
            n_seg, summary = eng.window_log2_segments(*pen, with_post=with_post, pos_first=pf, pos_last=pl)
            per = split(eng.get_log2_segments(), n_seg)
            for t in range(T):
                ws, wn, wsum = E.log2_segments_host(tabs[t], *pen, with_post=with_post, pos_first=pf, pos_last=pl, starts=starts)
                assert int(n_seg[t]) == wn, f"{what}: count of individual {t}"
                assert summary[t].tobytes() == wsum.tobytes(), f"{what}: summary of individual {t}"
                assert per[t].tobytes() == ws.tobytes(), f"{what}: records of individual {t} (posteriors {with_post})"
                assert set(starts) <= set(per[t]["first"].tolist())
    return path


@pytest.mark.parametrize("pen", [U.PEN, SMALL])
@pytest.mark.parametrize("n_win,shape", [(100, dict(C=1, owners=100, last=1, trips=1)),
                                         (601, dict(C=3, owners=201, last=1, trips=1)),
                                         (1279, dict(C=5, owners=256, last=4, trips=1))])
def test_device_equals_twin_on_every_byte(n_win, shape, pen):
    N, T = 30, 9
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and states_launch(T, n_win) == shape
        assert eng.n_window_chains == 1
        eng.run(list(range(3, 3 + T)), ld=False)
        tabs = eng.window_log2_all(T)
        plain = device_equals_twin(eng, tabs, pen, [], "no chains")
        differs = 0
        for name, starts in start_sets(n_win).items():
            eng.set_window_chains(starts)
            assert eng.n_window_chains == len(starts) + 1
            path = device_equals_twin(eng, tabs, pen, starts, f"{n_win} windows, starts {name}")
            differs += path.tobytes() != plain.tobytes()
        assert differs > 0                                                # (the chains do change paths on these tables)
        eng.set_window_chains([])
        assert eng.n_window_chains == 1
        assert device_equals_twin(eng, tabs, pen, [], "chains cleared").tobytes() == plain.tobytes()


def test_past_the_block_cap():
    """1100 individuals (of 40, repeated) for 1024 workgroups: 76 workgroups take a second individual with the same mask."""
    N, T, n_win = 40, 1100, 5
    alle, nr, na = U.covered_reads(5, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and states_launch(T, n_win) == dict(C=1, owners=5, last=1, trips=2)
        eng.set_window_chains([1, 3])                                     # (before the run: the chains belong to the site list)
        eng.run([t % N for t in range(T)], ld=False)
        tabs = eng.window_log2_all(T)
        path = device_equals_twin(eng, tabs, (1.0, 1.0, 1.0), [1, 3], "past the block cap")
        assert path[1024:].tobytes() == path[1024 % N:1024 % N + 76].tobytes()
        assert len({p.tobytes() for p in path}) > 1


def test_the_chains_live_as_long_as_the_site_list():
    N, T, n_win = 30, 4, 601
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    starts = [7, 300, 301, 599]
    with engine(alle, nr, na, 2) as eng:
        eng.run([1, 2, 3, 4], ld=False)
        tabs = eng.window_log2_all(T)
        first = eng.window_log2_states(*SMALL)
        post1 = eng.window_log2_posteriors(*SMALL)
        n1, _ = eng.window_log2_segments(*SMALL, with_post=True)
        rec1 = eng.get_log2_segments()
        eng.set_window_chains(starts)
        # the kept path, posteriors and records are stale: the same calls now give the chained bytes
        with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
            eng.get_log2_segments()
        chained = eng.window_log2_states(*SMALL)
        postc = eng.window_log2_posteriors(*SMALL)
        for t in range(T):
            wp, ws, wc = E.log2_states_host(tabs[t], *SMALL, starts=starts)
            assert chained[0][t].tobytes() == wp.tobytes() and chained[1][t].tobytes() == ws.tobytes()
            assert postc[0][t].tobytes() == E.log2_posteriors_host(tabs[t], *SMALL, starts=starts)[0].tobytes()
        assert chained[1].tobytes() != first[1].tobytes() and postc[0].tobytes() != post1[0].tobytes()
        nc, _ = eng.window_log2_segments(*SMALL, with_post=True)
        assert [int(x) for x in nc] == [E.log2_segments_host(tabs[t], *SMALL, with_post=True, starts=starts)[1] for t in range(T)]
        assert nc.tobytes() != n1.tobytes()
        # a second run on the same list keeps them
        eng.run([1, 2, 3, 4], ld=False)
        assert eng.n_window_chains == 5
        again = eng.window_log2_states(*SMALL)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, chained))
        # a refused call leaves them in place
        for bad, msg in (([0], r"starts\[0\] = 0 "), ([601], r"starts\[0\] = 601 is not below the 601 windows"),
                         ([5, 4], r"starts\[1\] = 4 does not lie above starts\[0\] = 5"),
                         ([5, 5], r"starts\[1\] = 5 does not lie above starts\[0\] = 5")):
            with pytest.raises(E.EngineError, match="ibdg_set_window_chains: " + msg):
                eng.set_window_chains(bad)
        assert eng.lib.ibdg_set_window_chains(eng.ctx, None, 2) != 0
        assert "ibdg_set_window_chains: NULL starts with n_starts = 2" in eng.lib.ibdg_last_error(eng.ctx).decode()
        assert eng.n_window_chains == 5
        again = eng.window_log2_states(*SMALL)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, chained))
        # clearing them brings the first bytes back
        eng.set_window_chains([])
        assert eng.n_window_chains == 1
        back = eng.window_log2_states(*SMALL)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(back, first))
        assert eng.window_log2_posteriors(*SMALL)[0].tobytes() == post1[0].tobytes()
        n2, _ = eng.window_log2_segments(*SMALL, with_post=True)
        assert n2.tobytes() == n1.tobytes() and eng.get_log2_segments().tobytes() == rec1.tobytes()
        # a new site upload clears them
        eng.set_window_chains(starts)
        assert eng.n_window_chains == 5
        eng.upload_sites(np.arange(len(nr)), nr, na, 2)
        assert eng.n_window_chains == 1
        eng.run([1, 2, 3, 4], ld=False)
        fresh = eng.window_log2_states(*SMALL)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(fresh, first))
        # ... and so does a new panel, which leaves no windows
        eng.set_window_chains(starts)
        eng.upload_panel(E.pack_alleles_fast(alle), alle.shape[1] // 2)
        assert eng.n_window_chains == 0


def test_no_site_list_no_chains():
    with E.Engine(0, 0.02, 20) as eng:
        assert eng.n_window_chains == 0
        with pytest.raises(E.EngineError, match="ibdg_set_window_chains: no valid site list"):
            eng.set_window_chains([1])
        with pytest.raises(E.EngineError, match="ibdg_set_window_chains: no valid site list"):
            eng.set_window_chains([])


# ---- the host program --------------------------------------------------------------------------------------------------

def _run(args, cwd, out):
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([EXE] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))}


@pytest.mark.parametrize("key", ["synA/ld_default", "synA/ld_varsites", "synA/nonld_all_targets_w2"])
def test_cli_every_route_gives_the_same_bytes(key, tmp_path):
    """One context with --stats-only sets the chains on the device once per site list; files per individual and two contexts
    hand the starts to the twins in the output job: the same bytes on every route, and other bytes than without the option."""
    args, inp = A.run_args(key)
    stats = ["--log-stats", "--states", "--posteriors", "--segments", "--p01", "0.05", "--p02", "0.01", "--p12", "0.05"]
    plain = _run(args + stats + ["--summary-only"], inp, tmp_path / "plain")
    # a gap that the fifth largest distance between two windows of the first individual exceeds
    summ = next(plain[fn] for fn in sorted(plain) if fn.endswith(".summary.txt"))
    rows = [l.split("\t") for l in summ.decode().splitlines() if not l.startswith("#")]
    dist = sorted(int(rows[w][1]) - int(rows[w - 1][2]) for w in range(1, len(rows)))
    gap = max(dist[-min(5, len(dist))] - 1, 1)
    chain = stats + ["--chain-gap", str(gap)]
    full = {d: _run(args + chain + ["--summary-only", "--devices", d], inp, tmp_path / f"full{len(d)}") for d in ("0", "0,0")}
    only = {d: _run(args + chain + ["--stats-only", "--devices", d], inp, tmp_path / f"only{len(d)}") for d in ("0", "0,0")}
    run_files = ["UNKWN.logibdposteriors.txt", "UNKWN.logibdsegments.txt", "UNKWN.logibdstates.txt"]
    assert sorted(only["0"]) == sorted(only["0,0"]) == run_files
    assert sorted(full["0"]) == sorted(full["0,0"]) == sorted(plain)
    for fn in full["0"]:
        if not fn.endswith(".tab.txt"):
            assert full["0"][fn] == full["0,0"][fn], fn
    for fn in run_files:
        assert only["0"][fn] == full["0"][fn] == only["0,0"][fn], fn
    # the chains are there, and the segments break at them
    per = [fn for fn in full["0"] if fn.endswith(".logsegments.txt")]
    assert len(per) >= 2
    n_chains = 0
    for fn in per:
        lines = [l.split("\t") for l in full["0"][fn].decode().splitlines()]
        assert lines[0][0] == "Chain"
        ids = [int(r[0]) for r in lines[1:]]
        assert ids == sorted(ids) and ids[0] == 1
        n_chains = max(n_chains, ids[-1])
        ind = fn.split(".")[1]
        srows = [l.split("\t") for l in full["0"][f"UNKWN.{ind}.summary.txt"].decode().splitlines() if not l.startswith("#")]
        starts = [w for w in range(1, len(srows)) if int(srows[w][1]) - int(srows[w - 1][2]) > gap]
        assert ids[-1] == len(starts) + 1
        assert set(w + 1 for w in starts) <= {int(r[3]) for r in lines[1:]}      # First_Window, 1-based
    assert n_chains >= 2
    assert any(full["0"][fn] != plain[fn] for fn in run_files)
