"""GPU tier: the table store and k_log2_switch_expect (ibdg_log2_store_*) against the host twin on every byte -- batches
appended to the store, the kernel past its grid cap where every workgroup reuses its scratch, the block shapes and hard tables of
tests/test_gpu_log_switches.py, the fit over the store against ibdg_log2_fit_host, the store's lifetime, what stays fresh, and the
host program's routes with --fit-penalties."""
import os
import subprocess

import numpy as np
import pytest

import armstats_check as A
import golden_io as G
import hard_tables as HT
import log_states_util as U
from ibdgem_amd import engine as E
from test_chain_gap_cli import starts_from
from test_fit_cli import fit_text
from test_gpu_log_hard_tables import table_set
from test_gpu_parity import bg_counts
from test_gpu_log_states_trips import engine, states_launch
from test_log_switches_host import simulated
from test_switch_scale_cli import shifts_from

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
N = 30
SMALL = (0.5, 0.25, 0.5)
HALF = (0.5, 0.5, 0.5)


def random_tables(T, n_win, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(-3000.0, 400.0, (T, n_win, 1)) + rng.uniform(-6.0, 6.0, (T, n_win, 3))


def fill(eng, tabs, batches):
    """A store reserved for the tables, which go in batch by batch: a run of that many individuals, its table set, appended."""
    eng.log2_store_reserve(len(tabs))
    at = 0
    for b in batches:
        eng.run([t % N for t in range(at, at + b)], ld=False)
        eng.set_window_log2_all(tabs[at:at + b])
        eng.log2_store_append()
        at += b
        assert eng.log2_store_count() == at
    assert at == len(tabs)


def store_equals_twin(eng, tabs, pen, starts=(), shift=None, what=""):
    expect = eng.log2_store_switches(*pen)
    assert expect.shape == (len(tabs), 3)
    for t, tab in enumerate(tabs):
        we = E.log2_switches_host(tab, *pen, want_sw=False, starts=starts, shift=shift)[1]
        assert expect[t].tobytes() == we.tobytes(), f"{what}: expectations of individual {t}"
    assert not np.isnan(expect).any(), what
    assert eng.log2_store_switches(*pen).tobytes() == expect.tobytes(), what + ": a second call"
    return expect


def test_batches_go_in_and_equal_one_batch():
    """Batches of 3, 1 and 4 individuals: the store's expectations equal the twin's per individual and those of
    ibdg_window_log2_switches over the same eight tables as one run's, plain and with chains and steps."""
    n_win = 257
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    tabs = random_tables(8, n_win, 5)
    starts, shift = HT.chain_starts(n_win), HT.shifts(n_win, 9)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and eng.log2_store_count() == 0
        fill(eng, tabs, [3, 1, 4])
        eng.run(list(range(8)), ld=False)
        eng.set_window_log2_all(tabs)
        for st, sh in (([], None), (starts, shift)):
            eng.set_window_chains(st)
            eng.set_window_steps(sh)
            for pen in (U.PEN, SMALL):
                expect = store_equals_twin(eng, tabs, pen, st, sh, f"batches, {len(st)} starts")
                assert expect.tobytes() == eng.window_log2_switches(*pen, want_sw=False)[1].tobytes()
        assert eng.log2_store_count() == 8


def test_past_the_grid_cap_every_workgroup_reuses_its_scratch():
    """5 windows x 2053 individuals with distinct tables, in two batches: more than two full trips of the grid-stride loop at any
    cap up to STATES_MAX_BLOCKS = 1024 (the kernel's own is 3 workgroups per CU: 768 on 256 CUs), so every workgroup runs three
    individuals over one scratch.  Under a shift of -2^30 into window 3 the tables whose windows 2 and 3 leave different states
    alive are dead (the dead-chain rule: zeros), the others live; which is which is drawn per individual, so that at either cap a
    workgroup takes a dead chain behind a live one and the reverse."""
    n_win, many = 5, 2 * 1024 + 5
    alle, nr, na = U.covered_reads(5, 2 * n_win, N)
    tabs = random_tables(many, n_win, 11)
    dead = np.random.default_rng(12).random(many) < 0.4
    tabs[dead, 2] = (-10.0, -5000.0, -5000.0)
    tabs[dead, 3] = (-5000.0, -10.0, -5000.0)
    tabs[dead, 2:4, :] += np.arange(dead.sum())[:, None, None] * 2.0 ** -8          # (distinct, and as dead)
    assert len({t.tobytes() for t in tabs}) == many
    for cap in (768, 1024):
        pairs = {(bool(dead[t]), bool(dead[t + cap])) for t in range(many - cap)}
        assert (True, False) in pairs and (False, True) in pairs
        assert many > 2 * cap
    shift = np.zeros(n_win, dtype=np.int32)
    shift[3] = -HT.SHIFT_MAX
    pen = HT.PENS[0]
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and states_launch(many, n_win)["trips"] == 3
        fill(eng, tabs, [1100, many - 1100])
        eng.set_window_steps(shift)
        expect = store_equals_twin(eng, tabs, pen, shift=shift, what="past the grid cap")
        assert not expect[dead].any() and (expect[~dead].sum(axis=1) > 0.0).all()
        eng.set_window_steps(None)
        expect = store_equals_twin(eng, tabs, SMALL, what="past the grid cap, no shifts")
        assert (expect.sum(axis=1) > 0.0).sum() > many - dead.sum()


def test_601_windows_seven_individuals():
    n_win, T = 601, 7
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    tabs = random_tables(T, n_win, 3)
    with engine(alle, nr, na, 2) as eng:
        assert states_launch(T, n_win) == dict(C=3, owners=201, last=1, trips=1)
        fill(eng, tabs, [T])
        store_equals_twin(eng, tabs, U.PEN, what="601 windows")
        expect = store_equals_twin(eng, tabs, SMALL, what="601 windows, small penalties")
        assert (expect > 1.0).any()


@pytest.mark.parametrize("n_win,per,shape", [(1279, 5, dict(C=5, owners=256, last=4, trips=1)),
                                             (8193, 2, dict(C=33, owners=249, last=9, trips=1))])
def test_hard_tables_with_dense_chains_and_edge_shifts(n_win, per, shape):
    """`per` tables of every family of hard_tables.LONG_FAMILIES in one store, under both penalty sets, the dead families' own
    penalties and shifts, plain and with dense_chain_starts and edge_shifts together."""
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    starts, rnd = HT.dense_chain_starts(n_win), HT.edge_shifts(n_win, 9)
    sets = {f: table_set(f, n_win) for f in HT.LONG_FAMILIES}
    tabs = np.concatenate([sets[f][0][:per] for f in HT.LONG_FAMILIES])
    own = sets["dead-shift"][2]
    at = {f: i * per for i, f in enumerate(HT.LONG_FAMILIES)}
    with engine(alle, nr, na, 2) as eng:
        assert states_launch(per, n_win) == shape
        fill(eng, tabs, [per] * len(HT.LONG_FAMILIES))
        seen_dead = False
        for pen, st, sh in [(HT.PENS[0], [], None), (HT.PENS[1], starts, rnd), (HT.PENS[0], [], own),
                            (HT.UNDERFLOW_PEN, [], None), (HT.UNDERFLOW_PEN, starts, rnd)]:
            eng.set_window_chains(st)
            eng.set_window_steps(sh)
            what = f"{n_win} windows, penalties {pen}, {len(st)} starts, shifts {sh is not None}"
            expect = store_equals_twin(eng, tabs, pen, st, sh, what)
            counted = E.log2_switches_host(None, *pen, want_sw=False, starts=st, shift=sh, n_win=n_win)[2]
            assert (expect <= counted.astype(np.float64) * (1 + 1e-9)).all(), what
            if sh is own:
                mine = expect[at["dead-shift"]:at["dead-shift"] + 2]
                assert not mine.any(), what + ": the rule's zeros"
                seen_dead = True
        assert seen_dead


def test_the_fit_over_the_store_is_the_host_fit():
    """Three appended batches, plain and with chains and shifts: rows, stood and fitted of ibdg_log2_store_fit against
    ibdg_log2_fit_host over the same tables on every byte, with a limit it reaches and one it does not need."""
    n_win = 601
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    # eight chains of 601 windows drawn from the model (tests/test_log_switches_host.py): measured with the twin on the CPU, the
    # fit stands at iteration 21 / 20 (plain, from the two starts) and 24 / 17 (with chains and shifts), never within 5
    tabs = np.stack(simulated(0, chains=8, n=n_win))
    starts, shift = HT.chain_starts(n_win), HT.shifts(n_win, 9)
    with engine(alle, nr, na, 2) as eng:
        fill(eng, tabs, [3, 1, 4])
        for st, sh in (([], None), (starts, shift)):
            eng.set_window_chains(st)
            eng.set_window_steps(sh)
            for p0, limit in ((HALF, 5), (HALF, 60), ((0.05, 0.01, 0.2), 60)):
                rows, stood, fitted = eng.log2_store_fit(p0, limit)
                wr, ws, wf = E.log2_fit_host(list(tabs), p0, limit, starts=st, shift=sh)
                assert len(rows) == len(wr) and rows.tobytes() == wr.tobytes(), f"rows from {p0}, limit {limit}"
                assert stood == ws and fitted.tobytes() == wf.tobytes()
                assert stood == (limit == 60) and (limit == 60 or len(rows) == 5)
                print(f"from {p0}, limit {limit}, {len(st)} starts: {len(rows)} iterations, stood {stood}, fitted {fitted.tolist()}")
        rows, stood, fitted = eng.log2_store_fit(HALF, 0)
        assert len(rows) == 0 and not stood and fitted.tolist() == list(HALF)


def test_lifetime_and_refusals():
    alle, nr, na = U.covered_reads(3, 40, 20)
    with engine(alle, nr, na, 2) as eng:
        n = eng.n_windows
        with pytest.raises(E.EngineError, match=r"ibdg_log2_store_append: no results \(call ibdg_run\)"):
            eng.log2_store_append()
        eng.run([1, 2], ld=False)
        with pytest.raises(E.EngineError, match="ibdg_log2_store_append: no store"):
            eng.log2_store_append()
        with pytest.raises(E.EngineError, match="ibdg_log2_store_switches: no store"):
            eng.log2_store_switches(*SMALL)
        eng.log2_store_reserve(3)
        assert eng.log2_store_switches(*SMALL).shape == (0, 3)
        rows, stood, fitted = eng.log2_store_fit(HALF, 4)
        assert len(rows) == 0 and not stood and fitted.tolist() == list(HALF)
        eng.log2_store_append()
        with pytest.raises(E.EngineError, match="2 individuals stored and 2 more, beyond the reserve of 3"):
            eng.log2_store_append()
        assert eng.log2_store_count() == 2
        tabs = eng.window_log2_all(2)
        store_equals_twin(eng, tabs, SMALL, what="the run's own tables")
        for pen in ((0.0, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, float("nan"))):
            with pytest.raises(E.EngineError, match=r"ibdg_log2_store_switches: p\d\d = .* is not in \(0, 1\]"):
                eng.log2_store_switches(*pen)
            with pytest.raises(E.EngineError, match=r"ibdg_log2_store_fit: p\d\d = .* is not in \(0, 1\]"):
                eng.log2_store_fit(pen, 3)
        assert eng.lib.ibdg_log2_store_switches(eng.ctx, 0.5, 0.5, 0.5, None) != 0
        assert "ibdg_log2_store_switches: NULL expect" in eng.lib.ibdg_last_error(eng.ctx).decode()
        assert eng.lib.ibdg_log2_store_fit(eng.ctx, None, 3, None, None, None, None) != 0
        assert "ibdg_log2_store_fit: NULL p" in eng.lib.ibdg_last_error(eng.ctx).decode()
        # a run does not touch the store; a run without log tables cannot be appended
        eng.set_option("log_windows", 0)
        eng.run([3], ld=False)
        with pytest.raises(E.EngineError, match="ibdg_log2_store_append: the last run kept no window logs"):
            eng.log2_store_append()
        assert eng.log2_store_count() == 2
        eng.set_option("log_windows", 1)
        eng.run([3], ld=False)
        store_equals_twin(eng, tabs, SMALL, what="behind another run")
        eng.log2_store_append()
        assert eng.log2_store_count() == 3
        # a new site list empties it and takes the reserve away
        eng.upload_sites(np.arange(len(nr)), nr, na, 2)
        assert eng.log2_store_count() == 0
        with pytest.raises(E.EngineError, match=r"ibdg_log2_store_switches: no results"):
            eng.log2_store_switches(*SMALL)
        with pytest.raises(E.EngineError, match=r"ibdg_log2_store_append: no results"):
            eng.log2_store_append()
        eng.run([1, 2], ld=False)
        with pytest.raises(E.EngineError, match="ibdg_log2_store_append: no store"):
            eng.log2_store_append()
        with pytest.raises(E.EngineError, match="ibdg_log2_store_fit: no store"):
            eng.log2_store_fit(HALF, 2)
        eng.log2_store_reserve(2)
        eng.log2_store_append()
        assert eng.log2_store_count() == 2 and n == eng.n_windows
        # and so does a new panel
        eng.upload_panel(E.pack_alleles_fast(alle), alle.shape[1] // 2)
        assert eng.log2_store_count() == 0
        with pytest.raises(E.EngineError, match="ibdg_log2_store_reserve: no valid site list"):
            eng.log2_store_reserve(2)


def test_what_stays_fresh():
    """The counterpart of test_gpu_log_switches.test_what_goes_stale_and_what_is_refused: the store's call runs over scratch of
    its own, so the posteriors and the segment records made before it are still served behind it -- ibdg_get_log2_segments, which
    ibdg_window_log2_switches makes refuse, answers with the same records."""
    n_win = 100
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        eng.run([1, 2, 5], ld=False)
        tabs = eng.window_log2_all(3)
        eng.log2_store_reserve(3)
        eng.log2_store_append()
        post, pe, pz = eng.window_log2_posteriors(*SMALL)
        n_seg, _ = eng.window_log2_segments(*SMALL, with_post=True)
        recs = eng.get_log2_segments()
        store_equals_twin(eng, tabs, SMALL, what="behind the posteriors")
        eng.log2_store_fit(HALF, 3)
        assert eng.get_log2_segments(int(n_seg.sum())).tobytes() == recs.tobytes()
        p2, e2, z2 = eng.window_log2_posteriors(*SMALL)
        assert p2.tobytes() == post.tobytes() and e2.tobytes() == pe.tobytes() and z2.tobytes() == pz.tobytes()
        # (a posteriors call drops the records whatever its penalties -- LogStates' own rule, not the store's doing)
        with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
            eng.get_log2_segments(int(n_seg.sum()))


# ---- the host program --------------------------------------------------------------------------------------------------

def _run(args, cwd, out):
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([EXE] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))}


def run_log_tables(key, gap=20000, scale=3000.0):
    """The log2 window tables of a golden case's run, made by the engine itself, with the chain starts of --chain-gap and the
    step shifts of --switch-scale over its windows: (tabs [T][n_win][3], starts, shift)."""
    tag, case = key.split("/")
    flags, panel, names, refids, pu_id, per_target = G.case_setup(tag, case)
    tab, _, _, fo, site_rows = per_target[names[0]]                            # (no -v, no -D: one site list for all)
    with E.Engine(0, flags["eps"], flags["max_cov"]) as eng:
        eng.set_option("log_windows", 1)
        eng.upload_panel(E.pack_alleles_fast(panel.alleles), len(panel.names))
        eng.upload_sites(site_rows, tab.n_ref, tab.n_alt, flags["window"], f_override=fo)
        eng.run([panel.index(n) for n in names], ld=flags["ld"], bg_count=bg_counts(refids, len(panel.names)), pu_id=pu_id)
        tabs = eng.window_log2_all(len(names))
        first, last, _ = eng.windows()
    pos_first, pos_last = tab.pos[first], tab.pos[last]
    return tabs, starts_from(pos_first, pos_last, gap), shifts_from(pos_first, pos_last, scale)


@pytest.mark.parametrize("key", ["synA/ld_default", "synA/nonld_all_targets_w2", "synB/ld_w37"])
def test_cli_every_route_gives_the_same_bytes(key, tmp_path):
    """The routes of test_gpu_log_switches.py with --fit-penalties: one context keeps every batch's tables in its store and
    iterates there, with --stats-only and with files per individual; two contexts that share the windows leave the gathered tables
    to the host, which iterates over them on its threads.  The same bytes from all four, and from the binding's
    ibdg_log2_fit_host over the run's own log tables, which the engine makes again here (run_log_tables); row 1 repeats the
    run's logibdswitches.txt and row 2 starts from its # Next; every other file equals the run without the option."""
    args, inp = A.run_args(key)
    c0, c1 = A.golden()["cases"][key]["ranges"]["both"]["range"]
    stats = ["--log-stats", "--states", "--arm-stats", f"{c0},{c1}", "--p01", "0.05", "--p02", "0.01", "--p12", "0.05", "--chain-gap", "20000",
             "--switch-scale", "3000", "--switches"]
    opt = stats + ["--fit-penalties", "12"]
    full = {d: _run(args + opt + ["--summary-only", "--devices", d], inp, tmp_path / f"full{len(d)}") for d in ("0", "0,0")}
    only = {d: _run(args + opt + ["--stats-only", "--devices", d], inp, tmp_path / f"only{len(d)}") for d in ("0", "0,0")}
    fn = "UNKWN.logibdfit.txt"
    fit = full["0"][fn]
    assert fit == full["0,0"][fn] == only["0"][fn] == only["0,0"][fn]
    lines = [l.split("\t") for l in fit.decode().splitlines()]
    sw = {l.split("\t")[0].split(" (")[0]: l.split("\t")[1:] for l in full["0"]["UNKWN.logibdswitches.txt"].decode().splitlines() if l.startswith("# ")}
    assert lines[1][1:4] == sw["# Penalties"] and lines[1][4:7] == sw["# Total"] and lines[1][7:10] == sw["# Prior"]
    assert lines[1][10:13] == sw["# Counted"]
    n_iter = int(lines[-2][1])
    assert lines[-2][0] == "# Iterations" and lines[-2][2] in ("stood", "limit") and len(lines) == n_iter + 4
    assert n_iter < 2 or lines[2][1:4] == sw["# Next"]
    assert lines[-3] == ["# Individuals", str(len([l for l in full["0"]["UNKWN.logibdstates.txt"].decode().splitlines() if not l.startswith("#")]))]
    # the binding's host loop over the run's own log tables: the engine driven as the program drives it (the case's panel, the
    # site list of its committed table, its comparison individuals in one run) gives the tables, the windows' first and last
    # positions give the chain starts and the shifts
    tabs, starts, shift = run_log_tables(key)
    rows, stood, fitted = E.log2_fit_host(list(tabs), (0.05, 0.01, 0.05), 12, starts=starts, shift=shift)
    assert fit.decode() == fit_text(rows, stood, fitted, len(tabs)), "the file is not the binding's fit over the run's tables"
    assert len(rows) == n_iter
    print(f"{key}: {len(tabs)} individuals x {len(tabs[0])} windows, {n_iter} iterations, {lines[-2][2]}")
    # every file the run writes without the option is unchanged
    plain = _run(args + stats + ["--summary-only"], inp, tmp_path / "plain")
    assert sorted(plain) == sorted(f for f in full["0"] if f != fn)
    for f, data in plain.items():
        assert full["0"][f] == data and full["0,0"][f] == data, f
    plain_only = _run(args + stats + ["--stats-only"], inp, tmp_path / "plain_only")
    assert sorted(plain_only) == sorted(f for f in only["0"] if f != fn)
    for f, data in plain_only.items():
        assert only["0"][f] == data, f
