"""ibdg_log2_fit_host and ibdg_switch_fit_step: the fit of the switch penalties on the host, no device.

The twin's loop against the binding's older loop (fit_switch_penalties_host) on every byte of every iteration's penalties; every
row's total, prior and counted steps against ibdg_log2_switches_host; the stop rule restated in Python from the penalties'
integers; the iterations at which the simulated chains of tests/test_log_switches_host.py stand; a pair the data never shows;
chains and shifts on both sides of the counted rule; the fit continued from its own result; no iterations, no individuals; every
refusal; the step at a fixed point and at the clamps."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import hard_tables as HT
import hp_post_ref as H
from ibdgem_amd import engine as E
from test_log_switches_host import random_table, simulated, some_shifts, some_starts

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF, SMALL = (0.5, 0.5, 0.5), (1e-4, 1e-4, 1e-4)
# the first iteration of simulated(0) whose step stands, from HALF and from SMALL: measured with the library (see the test)
STANDS = {HALF: 29, SMALL: 21}


@pytest.fixture(scope="module", autouse=True)
def library():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def chains0():
    return simulated(0)


def quanta(p):
    """The penalties' integers as the library forms them (states_penalties): hp_post_ref.penalty is the same rule."""
    return [H.penalty(float(x)) for x in p]


def stands(p, nxt):
    return all(abs(a - b) <= 1 for a, b in zip(quanta(p), quanta(nxt)))


def next_of(rows, fitted):
    """The penalties after each iteration: the next row's, and the fitted ones after the last."""
    return np.vstack([rows["p"][1:], np.asarray(fitted)[None]]) if len(rows) else np.zeros((0, 3))


def check_rows(tabs, rows, stood, fitted, p0, starts=None, shift=None):
    """Every row against ibdg_log2_switches_host and the update; the stop rule restated; returns the rows' verdicts."""
    n = tabs[0].shape[0]
    assert rows["p"][0].tobytes() == np.asarray(p0, dtype=np.float64).tobytes()
    nxt = next_of(rows, fitted)
    verdicts = []
    for i, r in enumerate(rows):
        expect = [E.log2_switches_host(t, *r["p"], want_sw=False, starts=starts, shift=shift)[1] for t in tabs]
        _, prior, counted = E.log2_switches_host(None, *r["p"], want_sw=False, starts=starts, shift=shift, n_win=n)
        assert r["total"].tobytes() == E._total_in_order(expect).tobytes(), f"total of iteration {i + 1}"
        assert r["prior"].tobytes() == prior.tobytes() and r["counted"].tolist() == counted.tolist(), f"iteration {i + 1}"
        assert nxt[i].tobytes() == E.switch_penalty_update(r["p"], r["total"], len(tabs), r["prior"]).tobytes()
        row, step_next, step_stood = E.switch_fit_step(r["p"], r["total"], len(tabs), r["prior"], r["counted"])
        assert row.tobytes() == r.tobytes() and step_next.tobytes() == nxt[i].tobytes()
        assert step_stood == stands(r["p"], nxt[i])
        verdicts.append(step_stood)
    assert not any(verdicts[:-1]) and stood == (bool(verdicts) and verdicts[-1])
    return verdicts


@pytest.mark.parametrize("p0", [HALF, SMALL])
def test_the_simulated_chains_stand_where_measured(chains0, p0):
    """simulated(seed), 20 chains x 2000 windows.  Measured with the library's own quantisation (ibdg_log2_fit_host, max_iter 60)
    on the CPU: the first iteration whose step moves no integer by more than one quantum is
      from (0.5, 0.5, 0.5):    the 29th, 28th, 28th for seeds 0, 1, 2
      from (1e-4, 1e-4, 1e-4): the 21st, 21st, 20th
    and the fitted penalties of seed 0 are (0.0100919, 0.00138047, 0.0192222) from the first start and agree with those from the
    second to 1e-5 of their size.  This test runs seed 0: it stands at that iteration, not at the one before, and a limit below it
    ends the fit with `limit`."""
    n = STANDS[p0]
    rows, stood, fitted = E.log2_fit_host(chains0, p0, 60)
    assert len(rows) == n and stood
    verdicts = check_rows(chains0, rows, stood, fitted, p0)
    assert verdicts == [False] * (n - 1) + [True]
    # the same sequence as the binding's older loop, on every byte
    assert next_of(rows, fitted).tobytes() == E.fit_switch_penalties_host(chains0, p0, n).tobytes()
    # one iteration fewer: every row the same, and it has not stood
    r2, s2, f2 = E.log2_fit_host(chains0, p0, n - 1)
    assert len(r2) == n - 1 and not s2 and r2.tobytes() == rows[:n - 1].tobytes() and f2.tobytes() == rows["p"][n - 1].tobytes()
    # exactly n: stands at the limit
    r3, s3, f3 = E.log2_fit_host(chains0, p0, n)
    assert s3 and r3.tobytes() == rows.tobytes() and f3.tobytes() == fitted.tobytes()
    print(f"from {p0}: stood at iteration {n}, fitted {fitted.tolist()}")


def test_both_starts_reach_the_same_penalties(chains0):
    a = E.log2_fit_host(chains0, HALF, 60)[2]
    b = E.log2_fit_host(chains0, SMALL, 60)[2]
    assert (np.abs(a / b - 1.0) <= 1e-4).all()


def test_fitted_passed_back_continues_the_sequence(chains0):
    rows, stood, fitted = E.log2_fit_host(chains0, HALF, 12)
    assert len(rows) == 12 and not stood
    more, _, f2 = E.log2_fit_host(chains0, fitted, 5)
    whole, _, f3 = E.log2_fit_host(chains0, HALF, 17)
    assert whole[:12].tobytes() == rows.tobytes() and whole[12:].tobytes() == more.tobytes() and f2.tobytes() == f3.tobytes()


def test_a_pair_the_data_never_shows_runs_to_the_limit():
    """3 chains x 40 windows: no chain shows a 0<->2 switch, p02 falls by a constant factor per iteration towards the clamp and
    its integer moves by thousands of quanta every time: `limit` at N = 80 with p02 still falling."""
    tabs = simulated(0, chains=3, n=40)
    rows, stood, fitted = E.log2_fit_host(tabs, HALF, 80)
    assert len(rows) == 80 and not stood
    check_rows(tabs, rows, stood, fitted, HALF)
    p02 = next_of(rows, fitted)[:, 1]
    assert (p02[1:] < p02[:-1]).all() and 1e-300 < p02[-1] < 1e-30
    assert quanta(rows["p"][-1])[1] - quanta(fitted)[1] > 1000


@pytest.mark.parametrize("n", [100, 601])
def test_chains_and_shifts_on_both_sides_of_the_counted_rule(n):
    """Shifts that bring the largest penalty to 0, one quantum either side of it and to 2^30, with chain starts: as the penalties
    move, steps cross P_k + shift = 0 and `counted` changes between iterations."""
    tabs = [random_table(n, seed=s) for s in range(4)]
    p0 = (0.05, 0.01, 0.2)
    starts, shift = some_starts(n), some_shifts(n, p0)
    shift[3::11] = 3 * 65536                               # between the starting penalties' integers and the fitted ones'
    for st, sh in (((), None), (starts, None), ((), shift), (starts, shift)):
        rows, stood, fitted = E.log2_fit_host(tabs, p0, 12, starts=st, shift=sh)
        check_rows(tabs, rows, stood, fitted, p0, starts=st, shift=sh)
        want = E.fit_switch_penalties_host(tabs, p0, len(rows), starts=st, shift=sh)
        assert next_of(rows, fitted).tobytes() == want.tobytes()
        if sh is not None:
            assert len({tuple(c) for c in rows["counted"].tolist()}) > 1, "the counted steps never changed"
        else:
            assert len({tuple(c) for c in rows["counted"].tolist()}) == 1


def test_no_iterations_and_no_individuals():
    tabs = [random_table(30, seed=s) for s in range(2)]
    for r, s, f in (E.log2_fit_host(tabs, HALF, 0), E.log2_fit_host([], HALF, 7, n_win=30), E.log2_fit_host([], HALF, 0)):
        assert len(r) == 0 and not s and f.tolist() == list(HALF)
    # no windows: nothing to expect, the update keeps p, which stands at once
    r, s, f = E.log2_fit_host([np.zeros((0, 3))], HALF, 5)
    assert len(r) == 1 and s and f.tolist() == list(HALF) and r["total"].tolist() == [[0.0] * 3] and r["counted"].tolist() == [[0] * 3]


def test_every_refusal():
    lib = E.load_library()
    err = lambda: lib.ibdg_last_error(None).decode()
    tab = random_table(4)
    ptrs = (C.c_void_p * 2)(tab.ctypes.data, tab.ctypes.data)
    p = np.array(HALF)
    rows = np.zeros(3, dtype=E.FIT_ROW_DTYPE)
    n_rows, stood, fitted = C.c_size_t(7), C.c_int(7), np.full(3, 7.0)
    good = dict(tabs=C.addressof(ptrs), T=2, n=4, p=p.ctypes.data, starts=None, ns=0, shift=None, it=3, rows=rows.ctypes.data,
                n_rows=C.addressof(n_rows), stood=C.addressof(stood), fitted=fitted.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ibdg_log2_fit_host(a["tabs"], a["T"], a["n"], a["p"], a["starts"], a["ns"], a["shift"], a["it"], a["rows"], a["n_rows"],
                                      a["stood"], a["fitted"])

    for name in ("p", "n_rows", "stood", "fitted", "rows", "tabs"):
        assert call(**{name: None}) != 0 and f"ibdg_log2_fit_host: NULL {name}" in err(), name
    none = (C.c_void_p * 2)(tab.ctypes.data, None)
    assert call(tabs=C.addressof(none)) != 0 and "NULL table of individual 1" in err()
    for bad in ((0.0, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, math.nan)):
        q = np.array(bad)
        assert call(p=q.ctypes.data) != 0 and "is not in (0, 1]" in err() and "ibdg_log2_fit_host" in err()
    assert call(n=(1 << 21) + 1) != 0 and "2^21" in err()
    assert call(ns=2) != 0 and "NULL starts" in err()
    for bad, text in (([0], "starts[0] = 0"), ([4], "is not below the 4 windows"), ([2, 2], "strictly increasing")):
        s = np.array(bad, dtype=np.uint32)
        assert call(starts=s.ctypes.data, ns=len(s)) != 0 and text in err()
    sh = np.array([0, 0, (1 << 30) + 1, 0], dtype=np.int32)
    assert call(shift=sh.ctypes.data) != 0 and "shift[2]" in err()
    # a refused call writes nothing
    assert n_rows.value == 7 and stood.value == 7 and fitted.tolist() == [7.0] * 3 and not rows.tobytes().strip(b"\0")
    assert call() == 0 and n_rows.value == 3
    assert call(rows=None, it=0) == 0 and call(tabs=None, T=0) == 0
    with pytest.raises(ValueError):
        E.log2_fit_host([tab, random_table(5)], HALF, 2)
    # the step
    z3, c3 = np.zeros(3), np.zeros(3, dtype=np.uint64)
    row, nxt, st = np.zeros(1, dtype=E.FIT_ROW_DTYPE), np.zeros(3), C.c_int(0)
    args = [p.ctypes.data, z3.ctypes.data, 1, z3.ctypes.data, c3.ctypes.data, row.ctypes.data, nxt.ctypes.data, C.addressof(st)]
    for i, name in ((0, "p"), (1, "total"), (3, "prior"), (4, "counted"), (5, "row"), (6, "next"), (7, "stood")):
        a = list(args)
        a[i] = None
        assert lib.ibdg_switch_fit_step(*a) != 0 and f"ibdg_switch_fit_step: NULL {name}" in err()
    with pytest.raises(E.EngineError, match=r"ibdg_switch_fit_step: p02 = 0 is not in \(0, 1\]"):
        E.switch_fit_step((0.5, 0.0, 0.5), z3, 1, z3, c3)


def test_the_step_at_a_fixed_point_and_at_the_clamps():
    p = np.array([0.5, 0.01, 1e-5])
    prior, counted = np.array([4.0, 0.25, 0.125]), np.array([99, 98, 97], dtype=np.uint64)
    # a fixed point: total = T prior, next = p, stood
    row, nxt, stood = E.switch_fit_step(p, prior * 10, 10, prior, counted)
    assert nxt.tolist() == p.tolist() and stood
    assert row["p"].tolist() == p.tolist() and row["total"].tolist() == (prior * 10).tolist()
    assert row["prior"].tolist() == prior.tolist() and row["counted"].tolist() == [99, 98, 97]
    # one quantum is ln 2 / 65536 of p: a ratio of 1 + 1e-5 moves the integer by at most one, 1 + 1e-4 by several
    assert E.switch_fit_step(p, prior * 10 * (1 + 1e-5), 10, prior, counted)[2]
    assert not E.switch_fit_step(p, prior * 10 * (1 + 1e-4), 10, prior, counted)[2]
    # one pair alone keeps the step from standing
    assert not E.switch_fit_step(p, prior * 10 * np.array([1.0, 1.0, 2.0]), 10, prior, counted)[2]
    # the clamps: at 1 and staying there stands; 1e-300 is at the integers' clamp of -2^40 quanta only below 2^-16777216, so a
    # penalty that reaches 1e-300 from 1e-299 has moved
    _, nxt, stood = E.switch_fit_step([1.0, 1.0, 1.0], [1000.0, 3.0, 5.0], 1, [1.0, 1.0, 1.0], counted)
    assert nxt.tolist() == [1.0, 1.0, 1.0] and stood
    _, nxt, stood = E.switch_fit_step([0.5, 1e-299, 1.0], [1000.0, 1e-9, 3.0], 1, [1.0, 1.0, 1.0], counted)
    assert nxt.tolist() == [1.0, 1e-300, 1.0] and not stood
    _, nxt, stood = E.switch_fit_step([1.0, 1e-300, 1.0], [1.0, 1e-9, 1.0], 1, [1.0, 1.0, 1.0], counted)
    assert nxt.tolist() == [1.0, 1e-300, 1.0] and stood
    # inputs that carry no information keep p, which stands
    for bad in (0.0, math.nan, math.inf):
        _, nxt, stood = E.switch_fit_step(p, [bad] * 3, 10, prior, counted)
        assert nxt.tolist() == p.tolist() and stood
