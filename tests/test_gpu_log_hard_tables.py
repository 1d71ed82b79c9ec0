"""GPU tier of the hard log tables (tests/hard_tables.py): the kernels of the log-domain state family -- k_log2_states,
k_log2_posteriors, k_log2_segments_count / _write, k_log2_alpha, k_log2_sample_paths -- against the host twin on every byte, on
tables that no run of the engine writes: NaN and infinite columns, emissions on both sides of 2^-1000, differences at the -2^24
clamp, products that end in .5, exact ties, block exponents in the thousands, and chains that die (the dead-chain rule, DESIGN
4.9).  The tables reach the device through ibdg_set_window_log2 behind an ordinary run; the twin is held to independent references
on the same tables by tests/test_hard_tables.py.

Every size of hard_tables.SIZES and every family, five individuals a table set, plain, with chain starts, with step shifts and
with both; the sums of ibdg_window_log2_llr_sums over tables with NaN and infinite entries; what a set table makes stale and what
a new run restores; a workgroup's second individual behind one of another kind; the errors of the entry point; and the host
program on inputs that reach a dead chain, one context and two."""
import numpy as np
import pytest

import hard_tables as HT
import log_states_util as U
from ibdgem_amd import engine as E
from test_gpu_log_samples import device_equals_twin as draws_equal_twin
from test_gpu_log_samples import _run, positions
from test_gpu_log_states_trips import engine, states_launch
from test_gpu_log_steps import device_equals_twin as products_equal_twin

pytestmark = pytest.mark.gpu

N, T = 30, 5
TARGETS = list(range(3, 3 + T))
STREAMS = np.arange(3, 3 + T, dtype=np.uint64)
U53 = 2.0 ** -53


def run_of(eng, n_win, targets=TARGETS):
    assert eng.n_windows == n_win
    eng.run(targets, ld=False)


def table_set(family, n):
    """(tables [T][n][3], penalties, the family's own shifts or None, the individuals that carry the family).  A finite family: its
    five variants.  A dead one: its two variants, then three finite tables that live under the same penalties and shifts."""
    if family not in HT.DEAD:
        return np.stack([HT.case(family, n, v).tab for v in range(T)]), None, None, list(range(T))
    c0, c1 = HT.case(family, n, 0), HT.case(family, n, 1)
    shift = None if c0.shift is None else np.minimum(c0.shift, c1.shift)          # (both pairs' shifts: 0 or -2^30)
    rest = [HT.case(f, n, 2).tab for f in ("naninf", "alternating", "clamp")]
    return np.stack([c0.tab, c1.tab] + rest), c0.pen, shift, [0, 1]


def forms(family, n, pen, own, starts=None, rnd=None):
    """[(penalties, starts, shift)]: plain, with chain starts, with shifts, with both.  A dead-shift table keeps its own shifts in
    all four (the others' shifts come from +-3 bits), and its chain starts keep away from the pairs.  starts, rnd: other chain
    starts and shifts than hard_tables.chain_starts and shifts(n, 9)."""
    starts = HT.chain_starts(n) if starts is None else starts
    rnd = HT.shifts(n, 9) if rnd is None else rnd
    if own is not None:
        rnd = np.where(own != 0, own, rnd).astype(np.int32)
        starts = [w for w in starts if own[w] == 0]
        return [(pen, [], own), (pen, starts, own), (pen, [], rnd), (pen, starts, rnd)]
    out = []
    for p in ([pen] if pen else HT.PENS):
        out += [(p, [], None)] + ([(p, starts, None), (p, [], rnd), (p, starts, rnd)] if n >= 2 else [])
    return out


def every_product(eng, tabs, pen, starts, shift, what, K=3, seed=8):
    """Chains and shifts set, then every product of the family against the twins on `tabs`.  Returns (post, log2_z)."""
    eng.set_window_chains(starts)
    eng.set_window_steps(shift)
    n = eng.n_windows
    _, _, post, expect, log2_z = products_equal_twin(eng, tabs, pen, starts, shift, what)
    p2, e2, z2 = eng.window_log2_posteriors(*pen, want_post=False)
    assert p2 is None and e2.tobytes() == expect.tobytes() and z2.tobytes() == log2_z.tobytes(), what + ": without post"
    streams = STREAMS if len(tabs) == T else np.arange(len(tabs), dtype=np.uint64)
    draws_equal_twin(eng, len(tabs), K, pen, seed, streams, starts=starts, shift=shift, pos=positions(n), what=what)
    assert not np.isnan(post).any() and not np.isnan(expect).any() and not np.isnan(log2_z).any(), what
    sums = post.sum(axis=2)
    assert ((sums == 0.0) | (np.abs(sums - 1.0) <= 4 * U53)).all(), what
    return post, log2_z


@pytest.mark.parametrize("n_win", HT.SIZES)
def test_every_family_device_equals_twin(n_win):
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        run_of(eng, n_win)
        for family in HT.FAMILIES:
            if family in HT.DEAD and n_win < 2:
                continue
            tabs, pen, own, mine = table_set(family, n_win)
            eng.set_window_log2_all(tabs)
            assert eng.window_log2_all(T).tobytes() == tabs.tobytes(), family       # NaN payloads and all
            for i, (p, starts, shift) in enumerate(forms(family, n_win, pen, own)):
                what = f"{family}, {n_win} windows, penalties {p}, starts {starts}, shifts {shift is not None}"
                post, log2_z = every_product(eng, tabs, p, starts, shift, what)
                if family in HT.FINITE:
                    assert (post.sum(axis=2) != 0.0).all() and np.isfinite(log2_z).all(), what
                elif family == "dead-shift" or HT.UNDERFLOW_DEAD(n_win):
                    if family == "dead-shift" or i == 0:                            # (shifts of their own may revive an underflow)
                        assert not post[mine].any() and (log2_z[mine] == -np.inf).all(), what + ": the rule's mark"
                    assert post[2:].any()
            eng.set_window_chains([])
            eng.set_window_steps(None)


def test_llr_sums_over_nan_and_infinite_entries():
    """ibdg_window_log2_llr_sums on the naninf tables against the long-double model: a range without a NaN or infinite entry
    within the model's bound, any other NaN -- the double-double's error term of an infinite entry is inf - inf."""
    n_win = 257
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    first = [0, 0, 5, 128, 129, 200, 250, 256]
    end = [n_win, 1, 128, 129, 255, 200, n_win, n_win]
    with engine(alle, nr, na, 2) as eng:
        run_of(eng, n_win)
        tabs = table_set("naninf", n_win)[0]
        eng.set_window_log2_all(tabs)
        got = eng.window_log2_llr_sums(first, end)
        want, bound = U.log_model(tabs, first, end)
        assert got.shape == (T, len(first), 4)
        seen = set()
        for s, (f, e) in enumerate(zip(first, end)):
            for t in range(T):
                for k, cols in enumerate(((2, 0), (1, 0))):
                    hi, lo = got[t, s, 2 * k], got[t, s, 2 * k + 1]
                    clean = bool(np.isfinite(tabs[t, f:e][:, cols]).all())
                    seen.add(clean)
                    assert np.isnan(hi) == (not clean), (t, s, k)
                    assert np.isnan(np.float64(want[t, s, k])) <= np.isnan(hi)       # a NaN of the model is one of the device
                    if clean:
                        assert abs(np.longdouble(hi) - want[t, s, k]) <= bound[t, s, k] and abs(lo) <= abs(hi) * 2.0 ** -52
        assert seen == {True, False} and (got[:, 5] == 0.0).all()                     # (an empty range)


def products(eng, pen, K=3):
    """Every kept product and the records, as bytes per individual."""
    path, score, count = eng.window_log2_states(*pen)
    post, expect, log2_z = eng.window_log2_posteriors(*pen)
    n_seg, summary = eng.window_log2_segments(*pen, with_post=True)
    recs = eng.get_log2_segments()
    off = np.concatenate([[0], np.cumsum(n_seg)]).astype(int)
    out = eng.window_log2_samples(*pen, K, 5, STREAMS)
    drawn = [eng.get_log2_sample_path(t, K - 1) for t in range(T)]
    return [b"".join(np.ascontiguousarray(x).tobytes() for x in (path[t], score[t], count[t], post[t], expect[t], log2_z[t], summary[t],
                                                                recs[off[t]:off[t + 1]], out[t], drawn[t])) for t in range(T)]


def test_a_set_table_its_stale_products_and_the_next_run():
    n_win, pen = 257, HT.PENS[0]
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        run_of(eng, n_win)
        own = eng.window_log2_all(T)
        linear = eng.window_ll_all(T)
        before = products(eng, pen)
        hard = own.copy()
        hard[0], hard[2] = HT.case("naninf", n_win, 0).tab, HT.case("edge1000", n_win, 1).tab
        eng.set_window_log2_all(hard)
        assert eng.window_log2_all(T).tobytes() == hard.tobytes()
        assert eng.window_ll_all(T).tobytes() == linear.tobytes()                     # nothing else of the run moved
        # the records and the draws of the old table are gone, not served
        with pytest.raises(E.EngineError, match="ibdg_get_log2_segments: no ibdg_window_log2_segments call"):
            eng.get_log2_segments(1)
        with pytest.raises(E.EngineError, match="ibdg_get_log2_sample_path: no ibdg_window_log2_samples call"):
            eng.get_log2_sample_path(0, 0)
        # the same calls with the same penalties: new where the table is new, and the twin's on the table that was set
        after = products(eng, pen)
        assert [a != b for a, b in zip(after, before)] == [True, False, True, False, False]
        every_product(eng, hard, pen, [], None, "a set table")
        # the run's own table set again gives the run's own results ...
        eng.set_window_log2_all(own)
        assert products(eng, pen) == before
        # ... and a new run writes its own table over a set one
        eng.set_window_log2_all(hard)
        assert products(eng, pen) == after
        eng.run(TARGETS, ld=False)
        assert eng.window_log2_all(T).tobytes() == own.tobytes() and products(eng, pen) == before
        eng.run(TARGETS[:2], ld=False)                                                  # another T: the table is the new run's size
        with pytest.raises(E.EngineError, match="ibdg_set_window_log2: 5 tables for the 2 comparison individuals"):
            eng.set_window_log2_all(hard)
        eng.set_window_log2_all(hard[:2])
        assert eng.window_log2_all(2).tobytes() == hard[:2].tobytes()


def test_past_the_block_cap():
    """1030 individuals for 1024 workgroups, the tables cycling through all eight families: individual 1024 + i follows individual i
    in a workgroup's LDS, and is of another kind (three families on).  Once under the dead-shift family's penalties and shifts, once
    under the dead-underflow family's penalties."""
    n_win, many = 257, 1030
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    kind = [((t + 3 * (t // 1024)) % 8, (t // 8) % 2) for t in range(many)]
    assert all(kind[t][0] != kind[t - 1024][0] for t in range(1024, many))
    made = {k: HT.case(HT.FAMILIES[k[0]], n_win, k[1]).tab for k in set(kind)}
    tabs = np.stack([made[k] for k in kind])
    assert tabs.nbytes == 1030 * 257 * 24
    shift = table_set("dead-shift", n_win)[2]
    streams = np.arange(many, dtype=np.uint64)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and states_launch(many, n_win) == dict(C=2, owners=129, last=1, trips=2)
        eng.run([t % N for t in range(many)], ld=False)
        eng.set_window_log2_all(tabs)
        for pen, sh, dead in ((HT.PENS[0], shift, "dead-shift"), (HT.UNDERFLOW_PEN, None, "dead-underflow")):
            eng.set_window_steps(sh)
            _, _, post, _, log2_z = products_equal_twin(eng, tabs, pen, [], sh, f"past the block cap, {dead}")
            draws_equal_twin(eng, many, 2, pen, 4, streams, shift=sh, what=f"past the block cap, {dead}")      # 2060 pairs
            assert not np.isnan(post).any()
            marked = [t for t in range(many) if HT.FAMILIES[kind[t][0]] == dead]
            assert any(t >= 1024 for t in marked) and not post[marked].any() and (log2_z[marked] == -np.inf).all()
            for t in range(1024, many):                 # equal tables, equal bytes: what a workgroup served first does not show
                twin_t = kind.index(kind[t])
                assert twin_t < 1024 and post[t].tobytes() == post[twin_t].tobytes()


def test_errors():
    alle, nr, na = U.covered_reads(3, 40, 20)
    with engine(alle, nr, na, 2) as eng:
        n = eng.n_windows
        tab = np.zeros((2, n, 3))
        with pytest.raises(E.EngineError, match=r"ibdg_set_window_log2: no results \(call ibdg_run\)"):
            eng.set_window_log2_all(tab)
        eng.run([1, 2], ld=False)
        before = eng.window_log2_all(2)
        kept = [x.tobytes() for x in eng.window_log2_posteriors(*U.PEN)]
        with pytest.raises(E.EngineError, match="ibdg_set_window_log2: 3 tables for the 2 comparison individuals of the last run"):
            eng.set_window_log2_all(np.zeros((3, n, 3)))
        assert eng.lib.ibdg_set_window_log2(eng.ctx, None, 2) != 0
        assert "ibdg_set_window_log2: NULL tab" in eng.lib.ibdg_last_error(eng.ctx).decode()
        with pytest.raises(ValueError, match="tabs: shape"):
            eng.set_window_log2_all(np.zeros((2, n + 1, 3)))
        # a refused call changes nothing
        assert eng.window_log2_all(2).tobytes() == before.tobytes()
        assert [x.tobytes() for x in eng.window_log2_posteriors(*U.PEN)] == kept
        eng.set_option("log_windows", 0)
        eng.run([1, 2], ld=False)
        with pytest.raises(E.EngineError, match=r"ibdg_set_window_log2: the last run kept no window logs \(option log_windows\)"):
            eng.set_window_log2_all(tab)


# ---- the host program ----------------------------------------------------------------------------------------------------

def test_the_host_program_reaches_a_dead_chain(tmp_path):
    """hard_tables.write_dead_chain_input: 200 sites whose first individual has no path under --switch-scale 1e308.  One context
    with --stats-only takes the posteriors, segments and draws from the kernels, two contexts and --summary-only from the twin on
    the gathered tables: the same bytes, with the rule's mark on the one individual."""
    args = HT.write_dead_chain_input(str(tmp_path))
    full = _run(args + ["--summary-only", "--devices", "0"], tmp_path, tmp_path / "full")
    only = {d: _run(args + ["--stats-only", "--devices", d], tmp_path, tmp_path / f"only{len(d)}") for d in ("0", "0,0")}
    HT.read_dead_chain_run(full)
    assert sorted(only["0"]) == sorted(only["0,0"]) == ["pu.logibdposteriors.txt", "pu.logibdsamples.txt", "pu.logibdsegments.txt",
                                                        "pu.logibdstates.txt"]
    for fn, data in only["0"].items():
        assert data == full[fn] == only["0,0"][fn], fn
