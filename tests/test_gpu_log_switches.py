"""GPU tier: k_log2_switches (ibdg_window_log2_switches) against its host twin on every byte -- on the run's own log tables at the
shapes of tests/test_gpu_log_posteriors.py, and on the hard tables of tests/hard_tables.py with dense chain starts and edge shifts
at the sizes where a thread's trip counts differ and its blocks straddle the mask's words; once against the exact truth of
tests/hp_switch_ref.py, so that the tier does not rest on the twin alone; the fit on the resident table against the host fit; what
the call makes stale and what it refuses; and the host program's routes with --switches."""
import os
import subprocess

import numpy as np
import pytest

import armstats_check as A
import hard_tables as HT
import hp_post_ref as H
import hp_switch_ref as W
import log_states_util as U
from ibdgem_amd import engine as E
from test_gpu_log_hard_tables import N, T, forms, run_of, table_set
from test_gpu_log_states_trips import engine, states_launch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
SMALL = (0.5, 0.25, 0.5)


def device_equals_twin(eng, tabs, pen=U.PEN, starts=(), shift=None, what=""):
    """sw and expect of the tables on the device against the twin on every byte, under the chains and steps the context has
    (starts, shift: the same, for the twin); the same expect when sw is not asked for; the same bytes from a second call.
    Returns (sw, expect)."""
    n, n_t = eng.n_windows, len(tabs)
    sw, expect = eng.window_log2_switches(*pen)
    assert sw.shape == (n_t, n, 3) and expect.shape == (n_t, 3)
    for t in range(n_t):
        ws, we, _ = E.log2_switches_host(tabs[t], *pen, starts=starts, shift=shift)
        assert sw[t].tobytes() == ws.tobytes(), f"{what}: switch probabilities of individual {t}"
        assert expect[t].tobytes() == we.tobytes(), f"{what}: expectations of individual {t}"
    assert not np.isnan(sw).any() and not np.isnan(expect).any() and (sw >= 0.0).all(), what
    s2, e2 = eng.window_log2_switches(*pen, want_sw=False)
    assert s2 is None and e2.tobytes() == expect.tobytes(), what + ": without the rows"
    s3, e3 = eng.window_log2_switches(*pen)
    assert s3.tobytes() == sw.tobytes() and e3.tobytes() == expect.tobytes(), what + ": a second call"
    return sw, expect


def test_past_the_block_cap():
    """1100 individuals (of 40, repeated) for 1024 workgroups: 76 workgroups take a second individual and reuse their LDS."""
    N, T, n_win = 40, 1100, 5
    alle, nr, na = U.covered_reads(5, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win
        assert states_launch(T, n_win) == dict(C=1, owners=5, last=1, trips=2)
        eng.run([t % N for t in range(T)], ld=False)
        sw, expect = device_equals_twin(eng, eng.window_log2_all(T), pen=SMALL, what="past the block cap")
        assert sw[1024:].tobytes() == sw[1024 % N:1024 % N + 76].tobytes()
        assert expect[1024:].tobytes() == expect[1024 % N:1024 % N + 76].tobytes()
        assert len({s.tobytes() for s in sw}) > 1


@pytest.mark.parametrize("n_win,shape", [(601, dict(C=3, owners=201, last=1, trips=1)),
                                         (1279, dict(C=5, owners=256, last=4, trips=1)),
                                         (100, dict(C=1, owners=100, last=1, trips=1))])
def test_block_shapes(n_win, shape):
    N, T = 30, 9
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and states_launch(T, n_win) == shape
        eng.run(list(range(3, 3 + T)), ld=False)
        tabs = eng.window_log2_all(T)
        device_equals_twin(eng, tabs, what=f"{n_win} windows")
        sw, _ = device_equals_twin(eng, tabs, pen=SMALL, what=f"{n_win} windows, small penalties")
        assert (sw.sum(axis=2) > 0.01).any()               # with penalties of about a bit the steps do switch


@pytest.mark.parametrize("n_win,shape", [(1279, dict(C=5, owners=256, last=4, trips=1)),
                                         (1531, dict(C=6, owners=256, last=1, trips=1)),
                                         (8193, dict(C=33, owners=249, last=9, trips=1))])
def test_hard_tables_with_dense_chains_and_edge_shifts(n_win, shape):
    """Every family of hard_tables.LONG_FAMILIES through ibdg_set_window_log2, five individuals a table set, plain and with
    dense_chain_starts and edge_shifts together, at both penalty sets: both sides of the counted rule (an edge shift of +2^30
    caps every penalty, one of -3 bits none) and dead chains (the dead families, and the tables an edge shift of -2^30 kills)."""
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    starts, rnd = HT.dense_chain_starts(n_win), HT.edge_shifts(n_win, 9)
    with engine(alle, nr, na, 2) as eng:
        assert states_launch(T, n_win) == shape
        run_of(eng, n_win)
        seen_dead = seen_capped = False
        for family in HT.LONG_FAMILIES:
            tabs, pen, own, mine = table_set(family, n_win)
            eng.set_window_log2_all(tabs)
            all_forms = forms(family, n_win, pen, own, starts=starts, rnd=rnd)
            for p, st, sh in [all_forms[i] for i in ([0, 3] if len(all_forms) == 4 else [0, 3, 4, 7])]:
                eng.set_window_chains(st)
                eng.set_window_steps(sh)
                what = f"{family}, {n_win} windows, penalties {p}, {len(st)} starts, shifts {sh is not None}"
                sw, expect = device_equals_twin(eng, tabs, p, st, sh, what)
                counted = E.log2_switches_host(None, *p, want_sw=False, starts=st, shift=sh, n_win=n_win)[2]
                assert (expect <= counted.astype(np.float64) * (1 + 1e-9)).all(), what
                seen_capped |= sh is not None and int(counted.max()) < n_win - 1 - len(st)
                if family in HT.DEAD and (family == "dead-shift" or sh is None or sh is own):
                    assert not sw[mine].any() and not expect[mine].any(), what + ": the rule's zeros"
                    seen_dead = True
            eng.set_window_chains([])
            eng.set_window_steps(None)
        assert seen_dead and seen_capped


def test_device_against_the_exact_truth():
    """601 windows (C = 3, a last block of one window), two individuals, both penalty sets: the device's own outputs within the
    counted bar of hp_switch_ref of the exact pairwise forward-backward."""
    N, T, n_win = 30, 2, 601
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    assert (H.Rn(n_win) + W.Q + H.blocking(n_win)[0] + 8) * 2.0 ** -53 <= 1e-10
    with engine(alle, nr, na, 2) as eng:
        eng.run([4, 11], ld=False)
        tabs = eng.window_log2_all(T)
        for pen in (U.PEN, SMALL):
            sw, expect = eng.window_log2_switches(*pen)
            for t in range(T):
                worst = W.check(W.Truth(tabs[t], *pen), sw[t].tolist(), expect[t].tolist())
                print(f"device, 601 windows, penalties {pen}, individual {t}: largest error / bar {worst:.3g}")


def test_the_fit_on_the_device_is_the_host_fit():
    """Five iterations over a set table with chains and steps: the resident table, the device's sums, the context's prior and the
    update function against the host twin's loop over the same tables, on every byte."""
    n_win = 601
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    rng = np.random.default_rng(17)
    tabs = rng.normal(-3000.0, 400.0, (T, n_win, 1)) + rng.uniform(-6.0, 6.0, (T, n_win, 3))
    starts, shift = HT.chain_starts(n_win), HT.shifts(n_win, 9)
    with engine(alle, nr, na, 2) as eng:
        run_of(eng, n_win)
        eng.set_window_log2_all(tabs)
        for st, sh in (([], None), (starts, shift)):
            eng.set_window_chains(st)
            eng.set_window_steps(sh)
            prior, counted = eng.window_log2_switches_prior(*SMALL)
            _, wp, wc = E.log2_switches_host(None, *SMALL, want_sw=False, starts=st, shift=sh, n_win=n_win)
            assert prior.tobytes() == wp.tobytes() and counted.tolist() == wc.tolist()
            got = eng.fit_switch_penalties((0.5, 0.5, 0.5), 5)
            want = E.fit_switch_penalties_host(list(tabs), (0.5, 0.5, 0.5), 5, starts=st, shift=sh)
            assert got.shape == (5, 3) and got.tobytes() == want.tobytes()
            assert len({row.tobytes() for row in got}) == 5 and (got > 0.0).all() and (got <= 1.0).all()


def test_what_goes_stale_and_what_is_refused():
    alle, nr, na = U.covered_reads(3, 40, 20)
    with engine(alle, nr, na, 2) as eng:
        with pytest.raises(E.EngineError, match="ibdg_window_log2_switches: no results"):
            eng.window_log2_switches(*U.PEN)
        eng.run([1, 2], ld=False)
        for pen in ((0.0, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, float("nan")), (-1.0, 0.5, 0.5)):
            with pytest.raises(E.EngineError, match=r"ibdg_window_log2_switches: p\d\d = .* is not in \(0, 1\]"):
                eng.window_log2_switches(*pen)
            with pytest.raises(E.EngineError, match=r"ibdg_window_log2_switches_prior: p\d\d = .* is not in \(0, 1\]"):
                eng.window_log2_switches_prior(*pen)
        assert eng.lib.ibdg_window_log2_switches(eng.ctx, 0.5, 0.5, 0.5, None, None) != 0
        assert "ibdg_window_log2_switches: NULL expect" in eng.lib.ibdg_last_error(eng.ctx).decode()
        n = eng.n_windows
        tabs = eng.window_log2_all(2)
        # the call runs over the posteriors' scratch: posteriors kept from before are made again, not served from what it left
        post, pe, pz = eng.window_log2_posteriors(*SMALL)
        n_seg, _ = eng.window_log2_segments(*SMALL, with_post=True)
        recs = eng.get_log2_segments()
        device_equals_twin(eng, tabs, pen=SMALL, what="behind the posteriors")
        with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
            eng.get_log2_segments(int(n_seg.sum()))
        p2, e2, z2 = eng.window_log2_posteriors(*SMALL)
        assert p2.tobytes() == post.tobytes() and e2.tobytes() == pe.tobytes() and z2.tobytes() == pz.tobytes()
        eng.window_log2_switches(*SMALL, want_sw=False)
        n2, _ = eng.window_log2_segments(*SMALL, with_post=True)
        assert n2.tobytes() == n_seg.tobytes() and eng.get_log2_segments().tobytes() == recs.tobytes()
        # a set table, new chains and new steps are what the next call sees
        other = tabs[::-1].copy()
        eng.set_window_log2_all(other)
        device_equals_twin(eng, other, pen=SMALL, what="a set table")
        if n >= 3:
            eng.set_window_chains([2])
            device_equals_twin(eng, other, pen=SMALL, starts=[2], what="new chains")
            sh = np.full(n, 70000, dtype=np.int32)
            eng.set_window_steps(sh)
            _, expect = device_equals_twin(eng, other, pen=SMALL, starts=[2], shift=sh, what="new steps")
            assert eng.window_log2_switches_prior(*SMALL)[1].tolist() == [0, n - 2, 0]       # 70000 quanta cap 0.5, not 0.25
            assert not expect[:, [0, 2]].any()
        eng.set_option("log_windows", 0)
        eng.run([1, 2], ld=False)
        with pytest.raises(E.EngineError, match="option log_windows"):
            eng.window_log2_switches(*U.PEN)


# ---- the host program --------------------------------------------------------------------------------------------------

def _run(args, cwd, out):
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([EXE] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))}


@pytest.mark.parametrize("key", ["synA/ld_default", "synA/ld_varsites", "synA/nonld_all_targets_w2", "synB/ld_w37"])
def test_cli_every_route_gives_the_same_bytes(key, tmp_path):
    """The routes of test_gpu_log_posteriors.py with --switches: one context and --stats-only computes on the device and 24 bytes
    per individual leave it; two contexts, or files per individual, run the twin on the gathered tables."""
    args, inp = A.run_args(key)
    c0, c1 = A.golden()["cases"][key]["ranges"]["both"]["range"]
    stats = ["--log-stats", "--states", "--arm-stats", f"{c0},{c1}", "--p01", "0.05", "--p02", "0.01", "--p12", "0.05", "--chain-gap", "20000",
             "--switch-scale", "3000"]
    opt = stats + ["--switches"]
    full = {d: _run(args + opt + ["--summary-only", "--devices", d], inp, tmp_path / f"full{len(d)}") for d in ("0", "0,0")}
    only = {d: _run(args + opt + ["--stats-only", "--devices", d], inp, tmp_path / f"only{len(d)}") for d in ("0", "0,0")}
    run_files = ["UNKWN.logarmstats.txt", "UNKWN.logibdstates.txt", "UNKWN.logibdswitches.txt"]
    assert sorted(only["0"]) == sorted(only["0,0"]) == run_files
    assert sorted(full["0"]) == sorted(full["0,0"])
    per = [fn for fn in full["0"] if fn.endswith(".logswitches.txt")]
    assert len(per) >= 2 and len(per) == len([fn for fn in full["0"] if fn.endswith(".loghiddengem.txt")])
    for fn in run_files + per:
        assert full["0"][fn] == full["0,0"][fn], fn
    for fn in run_files:
        assert only["0"][fn] == full["0"][fn] == only["0,0"][fn], fn
    lines = [l.split("\t") for l in full["0"]["UNKWN.logibdswitches.txt"].decode().splitlines()]
    # (-v: a site list per individual, and the prior shown is their sum, which the line says)
    assert [l[0].split(" (")[0] for l in lines[-5:]] == ["# Total", "# Prior", "# Counted", "# Penalties", "# Next"]
    assert "varsites" in key or lines[-4][0] == "# Prior"
    assert lines[-2][1:] == ["5.000000e-02", "1.000000e-02", "5.000000e-02"]
    # every file the run writes without the option is unchanged
    plain = _run(args + stats + ["--summary-only"], inp, tmp_path / "plain")
    assert sorted(plain) == sorted(fn for fn in full["0"] if fn not in per and fn != "UNKWN.logibdswitches.txt")
    for fn, data in plain.items():
        assert full["0"][fn] == data, fn
