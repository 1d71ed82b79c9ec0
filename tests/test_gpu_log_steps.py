"""GPU tier: step shifts on the device.  ibdg_set_window_steps, then ibdg_window_log2_states / _posteriors /
_segments and ibdg_get_log2_segments against the _steps_host twins on the run's own log tables, on every byte: on the blocking
shapes of tests/test_gpu_log_chains.py with the shift patterns of tests/steps_cases.py, with and without chains; the identities
against what was there before; past the block cap; the lifetime of the steps; and the host program's routes with
--switch-scale."""
import os

import numpy as np
import pytest

import armstats_check as A
import log_states_util as U
from ibdgem_amd import engine as E
from steps_cases import BIG, shift_sets
from test_gpu_log_chains import SMALL, _run, start_sets
from test_gpu_log_segments import positions, split
from test_gpu_log_states_trips import engine, states_launch

pytestmark = pytest.mark.gpu


def device_equals_twin(eng, tabs, pen, starts, shift, what):
    """Every product of the three calls with the chains and steps that are set on `eng`, against the twins with `starts`, `shift`."""
    T, n = len(tabs), eng.n_windows
    kw = dict(starts=starts, shift=shift)
    path, score, count = eng.window_log2_states(*pen)
    post, expect, log2_z = eng.window_log2_posteriors(*pen)
    for t in range(T):
        wp, ws, wc = E.log2_states_host(tabs[t], *pen, **kw)
        wpost, wexp, wz = E.log2_posteriors_host(tabs[t], *pen, **kw)
        assert np.isfinite(wpost).all(), f"{what}: the twin's posteriors of individual {t}"
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
                ws, wn, wsum = E.log2_segments_host(tabs[t], *pen, with_post=with_post, pos_first=pf, pos_last=pl, **kw)
                assert int(n_seg[t]) == wn, f"{what}: count of individual {t}"
                assert summary[t].tobytes() == wsum.tobytes(), f"{what}: summary of individual {t}"
                assert per[t].tobytes() == ws.tobytes(), f"{what}: records of individual {t} (posteriors {with_post})"
                assert set(starts) <= set(per[t]["first"].tolist())
    return path, score, post, expect, log2_z


def same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("pen", [U.PEN, SMALL])
@pytest.mark.parametrize("n_win,shape", [(100, dict(C=1, owners=100, last=1, trips=1)),
                                         (601, dict(C=3, owners=201, last=1, trips=1)),
                                         (1279, dict(C=5, owners=256, last=4, trips=1))])
def test_device_equals_twin_on_every_byte(n_win, shape, pen):
    N, T = 30, 9
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and states_launch(T, n_win) == shape
        assert not eng.has_window_steps()
        eng.run(list(range(3, 3 + T)), ld=False)
        tabs = eng.window_log2_all(T)
        plain = device_equals_twin(eng, tabs, pen, [], None, "no steps")
        chains = start_sets(n_win)["w0"]                                  # (every w0: a start meets a shifted window in "w0")
        differs = 0
        for name, shift in shift_sets(n_win).items():
            eng.set_window_steps(shift)
            assert eng.has_window_steps()
            got = device_equals_twin(eng, tabs, pen, [], shift, f"{n_win} windows, shifts {name}")
            differs += got[0].tobytes() != plain[0].tobytes()
            eng.set_window_chains(chains)
            device_equals_twin(eng, tabs, pen, chains, shift, f"{n_win} windows, shifts {name}, chains")
            eng.set_window_chains([])
        assert differs > 0                                                # (the shifts do change paths on these tables)
        eng.set_window_steps(None)
        assert not eng.has_window_steps()
        assert same(device_equals_twin(eng, tabs, pen, [], None, "steps cleared"), plain)


@pytest.mark.parametrize("n_win", [100, 601, 1279])
def test_the_identities_on_the_device(n_win):
    N, T = 30, 9
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    p, up, down = (2.0 ** -10, 2.0 ** -20, 2.0 ** -10), (2.0 ** -7, 2.0 ** -17, 2.0 ** -7), (2.0 ** -13, 2.0 ** -23, 2.0 ** -13)

    def products(pen):
        return list(eng.window_log2_states(*pen)) + list(eng.window_log2_posteriors(*pen))

    def records(pen):
        n_seg, summary = eng.window_log2_segments(*pen, with_post=True)
        return [n_seg, summary, eng.get_log2_segments()]

    with engine(alle, nr, na, 2) as eng:
        eng.run(list(range(3, 3 + T)), ld=False)
        for pen in (U.PEN, SMALL):
            plain, plain_recs = products(pen), records(pen)
            # (a) all shifts 0
            eng.set_window_steps(np.zeros(n_win, dtype=np.int32))
            assert same(products(pen), plain) and same(records(pen), plain_recs)
            # (b) a free step where a chain would start: every byte but the segments'
            for name in ("w0", "w0+1", "two"):
                starts = start_sets(n_win)[name]
                shift = np.zeros(n_win, dtype=np.int32)
                shift[starts] = BIG
                eng.set_window_steps(shift)
                free = products(pen)
                eng.set_window_steps(None)
                eng.set_window_chains(starts)
                assert same(free, products(pen)), name
                eng.set_window_chains([])
        # (c) a constant shift is other penalties
        want_up, up_recs, want_down, down_recs = products(up), records(up), products(down), records(down)
        eng.set_window_steps(np.full(n_win, 3 * 65536, dtype=np.int32))
        assert same(products(p), want_up) and same(records(p), up_recs)
        eng.set_window_steps(np.full(n_win, -3 * 65536, dtype=np.int32))
        assert same(products(p), want_down) and same(records(p), down_recs)


def test_past_the_block_cap():
    """1100 individuals (of 40, repeated) for 1024 workgroups: 76 workgroups take a second individual with the same shifts."""
    N, T, n_win = 40, 1100, 5
    alle, nr, na = U.covered_reads(5, 2 * n_win, N)
    shift = np.array([0, 5 * 65536 + 77, -BIG, BIG, -9 * 65536 - 1], dtype=np.int32)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and states_launch(T, n_win) == dict(C=1, owners=5, last=1, trips=2)
        eng.set_window_steps(shift)                                       # (before the run: the steps belong to the site list)
        eng.set_window_chains([3])
        eng.run([t % N for t in range(T)], ld=False)
        tabs = eng.window_log2_all(T)
        path = device_equals_twin(eng, tabs, (0.5, 0.5, 0.5), [3], shift, "past the block cap")[0]
        assert path[1024:].tobytes() == path[1024 % N:1024 % N + 76].tobytes()
        assert len({p.tobytes() for p in path}) > 1


def test_the_steps_live_as_long_as_the_site_list():
    N, T, n_win = 30, 4, 601
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    shift = shift_sets(n_win)["random"]
    with engine(alle, nr, na, 2) as eng:
        eng.run([1, 2, 3, 4], ld=False)
        tabs = eng.window_log2_all(T)
        first = eng.window_log2_states(*SMALL)
        post1 = eng.window_log2_posteriors(*SMALL)
        n1, _ = eng.window_log2_segments(*SMALL, with_post=True)
        rec1 = eng.get_log2_segments()
        eng.set_window_steps(shift)
        # the kept path, posteriors and records are stale: the same calls now give the shifted bytes
        with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
            eng.get_log2_segments()
        stepped = eng.window_log2_states(*SMALL)
        posts = eng.window_log2_posteriors(*SMALL)
        for t in range(T):
            wp, ws, wc = E.log2_states_host(tabs[t], *SMALL, shift=shift)
            assert stepped[0][t].tobytes() == wp.tobytes() and stepped[1][t].tobytes() == ws.tobytes()
            assert posts[0][t].tobytes() == E.log2_posteriors_host(tabs[t], *SMALL, shift=shift)[0].tobytes()
        assert stepped[1].tobytes() != first[1].tobytes() and posts[0].tobytes() != post1[0].tobytes()
        ns, _ = eng.window_log2_segments(*SMALL, with_post=True)
        assert [int(x) for x in ns] == [E.log2_segments_host(tabs[t], *SMALL, with_post=True, shift=shift)[1] for t in range(T)]
        # a second run on the same list keeps them
        eng.run([1, 2, 3, 4], ld=False)
        assert eng.has_window_steps()
        assert same(eng.window_log2_states(*SMALL), stepped)
        # a refused call leaves them in place
        bad = shift.copy()
        bad[17] = BIG + 1
        for arg, msg in ((bad, r"shift\[17\] = 1073741825 is not within \+-2\^30"),
                         (shift[:-1], "600 shifts for the 601 windows of the site list"),
                         (np.zeros(602, dtype=np.int32), "602 shifts for the 601 windows of the site list")):
            with pytest.raises(E.EngineError, match="ibdg_set_window_steps: " + msg):
                eng.set_window_steps(arg)
        assert eng.lib.ibdg_set_window_steps(eng.ctx, None, n_win) != 0
        assert "ibdg_set_window_steps: NULL shift with n = 601" in eng.lib.ibdg_last_error(eng.ctx).decode()
        assert eng.has_window_steps()
        assert same(eng.window_log2_states(*SMALL), stepped)
        # clearing them brings the first bytes back
        eng.set_window_steps(None)
        assert not eng.has_window_steps()
        assert same(eng.window_log2_states(*SMALL), first)
        assert eng.window_log2_posteriors(*SMALL)[0].tobytes() == post1[0].tobytes()
        n2, _ = eng.window_log2_segments(*SMALL, with_post=True)
        assert n2.tobytes() == n1.tobytes() and eng.get_log2_segments().tobytes() == rec1.tobytes()
        # a new site upload clears them
        eng.set_window_steps(shift)
        assert eng.has_window_steps()
        eng.upload_sites(np.arange(len(nr)), nr, na, 2)
        assert not eng.has_window_steps()
        eng.run([1, 2, 3, 4], ld=False)
        assert same(eng.window_log2_states(*SMALL), first)
        # ... and so does a new panel
        eng.set_window_steps(shift)
        eng.upload_panel(E.pack_alleles_fast(alle), alle.shape[1] // 2)
        assert not eng.has_window_steps()


def test_no_site_list_no_steps():
    with E.Engine(0, 0.02, 20) as eng:
        assert not eng.has_window_steps()
        with pytest.raises(E.EngineError, match="ibdg_set_window_steps: no valid site list"):
            eng.set_window_steps(np.zeros(4, dtype=np.int32))
        with pytest.raises(E.EngineError, match="ibdg_set_window_steps: no valid site list"):
            eng.set_window_steps(None)


# ---- the host program --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["scale", "map", "chain-gap"])
@pytest.mark.parametrize("key", ["synA/ld_default", "synA/ld_varsites", "synA/nonld_all_targets_w2"])
def test_cli_every_route_gives_the_same_bytes(key, variant, tmp_path):
    """One context with --stats-only sets the steps on the device once per site list; files per individual and two contexts
    hand the shifts to the twins in the output job: the same bytes on every route, and other bytes than without the option."""
    args, inp = A.run_args(key)
    stats = ["--log-stats", "--states", "--posteriors", "--segments", "--p01", "0.05", "--p02", "0.01", "--p12", "0.05"]
    plain = _run(args + stats + ["--summary-only"], inp, tmp_path / "plain")
    summ = next(plain[fn] for fn in sorted(plain) if fn.endswith(".summary.txt"))
    rows = [l.split("\t") for l in summ.decode().splitlines() if not l.startswith("#")]
    centre = [(int(r[1]) + int(r[2])) * 0.5 for r in rows]
    dist = sorted(centre[w] - centre[w - 1] for w in range(1, len(rows)))
    steps = stats + ["--switch-scale", repr(dist[len(dist) // 2] + 0.25)]                     # the median distance of two windows
    if variant == "map":
        # a map over the middle half of the windows, the rate changing from entry to entry; X: a kilobase at 1 cM/Mb
        lo, hi = centre[len(centre) // 4], centre[3 * len(centre) // 4]
        cm, text = 0.0, "pos rate cM\n"
        for k in range(9):
            text += f"{lo + (hi - lo) * k / 8!r} 0 {cm!r}\n"
            cm += (hi - lo) / 8 * 1e-6 * (0.2 + k % 3)
        (tmp_path / "map.txt").write_text(text)
        steps = stats + ["--switch-scale", "0.001", "--genetic-map", str(tmp_path / "map.txt")]
    elif variant == "chain-gap":
        gaps = sorted(int(rows[w][1]) - int(rows[w - 1][2]) for w in range(1, len(rows)))
        steps += ["--chain-gap", str(max(gaps[-min(5, len(gaps))] - 1, 1))]
    full = {d: _run(args + steps + ["--summary-only", "--devices", d], inp, tmp_path / f"full{len(d)}") for d in ("0", "0,0")}
    only = {d: _run(args + steps + ["--stats-only", "--devices", d], inp, tmp_path / f"only{len(d)}") for d in ("0", "0,0")}
    run_files = ["UNKWN.logibdposteriors.txt", "UNKWN.logibdsegments.txt", "UNKWN.logibdstates.txt"]
    assert sorted(only["0"]) == sorted(only["0,0"]) == run_files
    assert sorted(full["0"]) == sorted(full["0,0"]) == sorted(plain)
    for fn in full["0"]:
        if not fn.endswith(".tab.txt"):
            assert full["0"][fn] == full["0,0"][fn], fn
    for fn in run_files:
        assert only["0"][fn] == full["0"][fn] == only["0,0"][fn], fn
    assert any(full["0"][fn] != plain[fn] for fn in run_files)
    for fn in plain:                                                      # what the steps do not reach is the run's without them
        if fn.endswith(".summary.txt"):
            assert full["0"][fn] == plain[fn], fn
