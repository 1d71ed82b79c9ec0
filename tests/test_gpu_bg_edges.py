"""Background lists at every chunk and lane edge through every --LD form (the cases of tests/bg_cases.py).

Which individuals a -B list names and how often, where the comparison individual and the -N individual sit among the 64-lane
chunks, and what the two exclusions of src/ibdgem.c:714 and :742-750 leave over: every form handles that with code of its own
(ibd0_from_pass's masked own chunk, k_target_weights' background size, k_ld_mfma's eRef over a wave's weighted lanes and its
groups of eight half chunks, k_ld_popcount's chunk groups), and random multiplicities 0..2 reach none of it at its edges.
tests/test_bg_cases.py asserts what each case is from its arrays, and that a kernel with a wrong exclusion could not pass.  Here
  (a) every (case, form) goes through test_gpu_precision.run_form with the case's list, pu and targets(T): per-row values and
      LIBD2 bit for bit against the oracle, --LD within 1e-10 of it (the reference order bit for bit), the hp_ref bound of the
      form on the case's interesting individuals and the last one, and the variant, count unit and layout the C ABI reports;
      an empty background gives NaN in both --LD columns in every form, and leaves the context fit for the next one;
  (b) the counting forms give the same bits on the case's targets(4), NaN where the truth is NaN;
  (c) one context takes every background of panel A in turn, forwards and backwards, synchronously and queued, each run
      with the bits of (a)'s "popcount mx1" run, the IBD0 pass made and used exactly where last_count_unit says;
  (d) option "log_windows" against the truths and bars of tests/hp_log_ref.py.
No bar is new, and no case is skipped: on these shapes the tables are in LDS and k_ld_mfma takes every run (asserted).
test_report (-s) prints the largest ratios and the slowest item; DESIGN.md s2 records them.
"""
import time

import numpy as np
import pytest

import bg_cases as BC
import depth_cases as DC
import hp_log_ref as HL
import hp_ref as H
import test_gpu_log_windows as LW
import test_gpu_precision as P
from ibdgem_amd import engine as E
from test_gpu_depth_edges import EQUAL_FORMS
from test_gpu_parity import assert_bits, bg_counts

pytestmark = pytest.mark.gpu

LD = H.LD
WORST = {}          # (form, "normal" / "empty background") or "log ld" / "log rows" -> largest ratio to its bound, this module's runs
SLOWEST = [0.0, None]
TOTAL = [0.0]
ITEMS = [(name, form) for name in BC.NAMES for form in P.FORMS]
_PACKED, _ORACLE, _MX1, _TRUTH = {}, {}, {}, {}

# the two rules by which the sibling modules leave a (case, form) out apply to nothing here
for _name in BC.NAMES:
    _c = BC.make_case(_name)
    assert DC.tab_in_lds(_c["nr"], _c["na"], _c["W"]) and DC.mfma_takes(_c["nr"], _c["na"], _c["W"]), _name
    assert all(s["T"] < _c["n_ids"] - 1 for s in P.FORMS.values()), _name
assert len(ITEMS) == len(BC.NAMES) * len(P.FORMS) == 21 * 16


def packed(c):
    """A panel in the device's format, made once."""
    if c["n_ids"] not in _PACKED:
        _PACKED[c["n_ids"]] = E.pack_alleles_fast(c["alle"])
    return _PACKED[c["n_ids"]]


class CachedOracle:
    """The oracle with its comparisons kept per (case, individual): every form asks for the same ones."""

    def __init__(self, oracle, name):
        self.oracle, self.name, self.pdg = oracle, name, oracle.pdg

    def compare(self, alle, nr, na, t, **kw):
        key = (self.name, int(t))
        if key not in _ORACLE:
            _ORACLE[key] = self.oracle.compare(alle, nr, na, t, **kw)
        return _ORACLE[key]


def slowest(t0, what, counted=False):
    """(counted: the item's runs have gone through timed_run, which has added their time to the total)"""
    dt = time.perf_counter() - t0
    TOTAL[0] += 0.0 if counted else dt
    if dt > SLOWEST[0]:
        SLOWEST[:] = [dt, what]


def spec_for(name, form, T=None):
    """The FORMS entry as this case runs it, by the rules of test_gpu_depth_edges.spec_for: the tables are in LDS, so the IBD1
    form reports count unit 3, and k_ld_mfma takes every group."""
    c = BC.make_case(name)
    spec = dict(P.FORMS[form])
    if T is not None:
        spec["T"] = T
    assert P.tab_in_lds(c["nr"], c["na"], c["W"])
    if form == "popcount IBD1 form":
        spec["unit"] = 3
    return spec


def is_empty(name, t):
    return name in BC.EMPTY and t == BC.make_case(name)["target"]


def timed_run(oracle, name, form, T=None, keep=None):
    c = BC.make_case(name)
    spec = spec_for(name, form, T)
    targets = c["targets"](spec["T"])
    checked = BC.checked(name, spec["T"])
    keep = {} if keep is None else keep
    # run_form keeps the session's largest ratios per form in P.WORST: this run's are taken apart from them, then merged
    session = dict(P.WORST)
    P.WORST.clear()
    t0 = time.perf_counter()
    try:
        truths = P.run_form(CachedOracle(oracle, name), form, c["alle"], c["nr"], c["na"], c["W"], c["eps"], c["M"],
                            refids=c["refids"], pu=c["pu"], spec=spec, keep=keep, targets=targets, checked=checked)
    finally:
        for (f, normal), v in P.WORST.items():
            # (no truth here is subnormal, asserted below: what run_form files under "not normal" is the NaN of an empty background)
            k = (f, "normal" if normal else "empty background")
            WORST[k] = max(WORST.get(k, 0.0), v)
        for key, v in session.items():
            P.WORST[key] = max(P.WORST.get(key, 0.0), v)
    slowest(t0, f"{name} / {form}" + (f" T={T}" if T else ""))
    assert keep["targets"] == targets and sorted(keep["windows"]) == checked and len(truths) == len(checked)
    # every truth of a non-empty background is a normal double; an empty one is NaN in the truth and in the table
    for i, tr in zip(checked, truths):
        win = keep["windows"][i]
        if is_empty(name, targets[i]):
            assert tr["n_bg"] == 0 and np.isnan(win[:, :2]).all() and np.isfinite(win[:, 2]).all(), (name, form, targets[i])
        else:
            assert tr["n_bg"] > 0 and np.isfinite(win).all(), (name, form, targets[i])
            for key in ("ibd0", "ibd1"):
                assert (tr[key] >= LD(2.0) ** -1022).all(), (name, form, key)
    if form == "popcount mx1" and T is None:
        _MX1[name] = keep["windows"][0]
    return truths


def mx1_table(oracle, name):
    """The target's window table of (a)'s "popcount mx1" run of the case."""
    if name not in _MX1:
        timed_run(oracle, name, "popcount mx1")
    return _MX1[name]


# --------------------------------------------------------------------------- (a) every form
@pytest.mark.parametrize("name,form", ITEMS, ids=[f"{n}-{f.replace(' ', '_')}" for n, f in ITEMS])
def test_every_form_on_every_background(oracle, name, form):
    timed_run(oracle, name, form)


def _form_run(eng, spec, c, targets, refids, pu):
    if spec["variant"] == 3:
        eng.set_background_order(refids)
    eng.run(targets, ld=True, bg_count=bg_counts(refids, c["n_ids"]), pu_id=pu)
    assert eng.last_ld_variant() == spec["variant"]
    return [(eng.site_ll(i), eng.window_ll(i)) for i in range(len(targets))]


@pytest.mark.parametrize("form", list(P.FORMS), ids=[f.replace(" ", "_") for f in P.FORMS])
def test_a_full_background_after_an_empty_one(form):
    """The context that returned NaN for an empty background then runs the same individuals against everybody: the bits of a
    context that never saw the empty one."""
    t0 = time.perf_counter()
    for name in BC.EMPTY:
        c = BC.make_case(name)
        spec = spec_for(name, form)
        targets = c["targets"](spec["T"])
        full, no_pu = BC.full_background(name)
        tables = []
        for first_empty in (True, False):
            with E.Engine(0, c["eps"], c["M"]) as eng:
                for k, v in spec["opts"].items():
                    eng.set_option(k, v)
                eng.upload_panel(packed(c), c["n_ids"])
                eng.upload_sites(np.arange(len(c["nr"])), c["nr"], c["na"], c["W"])
                if first_empty:
                    got = _form_run(eng, spec, c, targets, c["refids"], c["pu"])
                    assert np.isnan(got[0][1][:, :2]).all() and np.isfinite(got[0][1][:, 2]).all(), (name, form)
                    assert all(np.isfinite(win).all() for _, win in got[1:]), (name, form)
                tables.append(_form_run(eng, spec, c, targets, full, no_pu))
        for i, ((site_a, win_a), (site_b, win_b)) in enumerate(zip(*tables)):
            assert np.isfinite(win_b).all()
            assert_bits(site_a, site_b, f"{name}: {form}, per-row values of {targets[i]} after the empty background")
            assert_bits(win_a, win_b, f"{name}: {form}, windows of {targets[i]} after the empty background")
    slowest(t0, f"empty, then full / {form}")


# --------------------------------------------------------------------------- (b) equal bits
@pytest.mark.parametrize("name", BC.NAMES)
def test_counting_forms_give_equal_bits(oracle, name):
    """The case's targets(4) through every counting form (single launches: four of them; the group of four: one launch of
    k_ld_popcount_mt, count unit 0): the window tables of all four are the same bits -- NaN at the same positions where the
    background is empty, whatever the NaN's payload, and the same bits in the third column there."""
    c = BC.make_case(name)
    tables = {}
    t0 = time.perf_counter()
    for form in EQUAL_FORMS:
        keep = {}
        timed_run(oracle, name, form, T=4, keep=keep)
        tables[form] = keep
    first = tables[EQUAL_FORMS[0]]
    assert first["targets"] == c["targets"](4) and sorted(first["windows"]) == [0, 1, 2, 3]
    for i, want in first["windows"].items():
        assert np.isnan(want[:, :2]).all() if is_empty(name, first["targets"][i]) else np.isfinite(want).all()
    for form in EQUAL_FORMS[1:]:
        assert tables[form]["targets"] == first["targets"]
        for i, want in first["windows"].items():
            got = tables[form]["windows"][i]
            assert (np.isnan(got) == np.isnan(want)).all(), f"{name}: {form}, NaN positions, individual {first['targets'][i]}"
            assert_bits(got, want, f"{name}: {form} vs {EQUAL_FORMS[0]}, individual {first['targets'][i]}")
    slowest(t0, f"{name} / equal bits, five forms", counted=True)


# --------------------------------------------------------------------------- (c) one context, many backgrounds
class PassModel:
    """plan_run's rule for single runs (ibdg_api.cpp): the runs on one upload and background add up; from the ibd0_after-th on
    they take the IBD0 pass (count unit 3), which that run makes; another background starts over."""

    def __init__(self, after):
        self.after, self.key, self.runs = after, None, 0

    def unit(self, c):
        key = (c["mult"].tobytes(), c["pu"])
        if key != self.key:
            self.key, self.runs = key, 0
        self.runs += 1
        return 3 if self.runs >= self.after else 2


def test_one_context_through_every_background(oracle):
    """Panel A, ibd0_after 2: every case's target with that case's background, in table order and back, each run twice -- the
    second one makes (or uses) the IBD0 pass of that background.  Then the same sequence queued (async 1, finalize_in_next
    1), only every third table read: the finalising steps of backgrounds of 1, of thousands and of nobody are made up for in
    front of a launch for another background, or ride in the next one.  Then three individuals per background in a queue
    (the case's second and third, then its target): run i's finalising step rides in run i + 1's launch with run i's own
    background size.  Every table read is the bits of the case's "popcount mx1" run."""
    want = {name: mx1_table(oracle, name) for name in BC.A_NAMES}
    t0 = time.perf_counter()
    sizes = {_n_bg(name) for name in BC.A_NAMES}
    assert {0, 1}.issubset(sizes) and max(sizes) > 4000, sorted(sizes)
    c0 = BC.make_case(BC.A_NAMES[0])
    sequence = [name for name in BC.A_NAMES + BC.A_NAMES[::-1] for _ in range(2)]
    with E.Engine(0, c0["eps"], c0["M"]) as eng:
        for k, v in dict(P.FORMS["popcount mx1"]["opts"], ibd0_after=2).items():
            eng.set_option(k, v)
        eng.upload_panel(packed(c0), c0["n_ids"])
        eng.upload_sites(np.arange(len(c0["nr"])), c0["nr"], c0["na"], c0["W"])
        model = PassModel(2)
        units = []

        def run(name, t=None):
            c = BC.make_case(name)
            eng.run([c["target"] if t is None else t], ld=True, bg_count=c["mult"], pu_id=c["pu"])
            unit = model.unit(c)
            units.append(unit)
            assert eng.last_ld_variant() == 2 and eng.ld_layout() == 1 and eng.last_count_unit() == unit, (name, len(units), unit)

        for k, name in enumerate(sequence):
            run(name)
            assert_bits(eng.window_ll(0), want[name], f"run {k} ({name}), count unit {units[-1]}")
        assert units.count(2) == 2 * len(BC.A_NAMES) - 1 and units[:4] == [2, 3, 2, 3]        # (the turn: one background four times)
        eng.set_option("async", 1)
        eng.set_option("finalize_in_next", 1)
        del units[:]
        for k, name in enumerate(sequence):
            run(name)
            if k % 3 == 2:
                assert_bits(eng.window_ll(0), want[name], f"queued run {k} ({name}), count unit {units[-1]}")
        assert 2 in units and 3 in units
        for name in BC.A_NAMES + BC.A_NAMES[::-1]:
            c = BC.make_case(name)
            second, third = c["targets"](3)[1:]
            for t in (second, third, c["target"]):
                run(name, t)
            assert units[-2:] == [3, 3]
            assert_bits(eng.window_ll(0), want[name], f"three queued individuals on the background of {name}")
        eng.set_option("async", 0)
        # ... and the context is as good as new: one more background, synchronously
        run(BC.A_NAMES[-1])
        assert_bits(eng.window_ll(0), want[BC.A_NAMES[-1]], "the last synchronous run")
    slowest(t0, "one context through every background of panel A")


def _n_bg(name):
    c = BC.make_case(name)
    w = c["mult"].astype(np.int64)
    w[c["target"]] = 0
    if c["pu"] >= 0:
        w[c["pu"]] = 0
    return int(w.sum())


# --------------------------------------------------------------------------- (d) log_windows
def _ratio(got, truth, bar, what, key):
    got = np.asarray(got, dtype=np.float64).astype(LD)
    nan = np.isnan(truth)
    assert (np.isnan(got) == nan).all(), f"{what}: NaN pattern"
    assert np.isfinite(got[~nan]).all() and np.isfinite(truth[~nan]).all(), what
    r = np.abs(got[~nan] - truth[~nan]) / bar[~nan]
    worst = float(r.max()) if r.size else 0.0
    print(f"{what}: largest ratio to the bar {worst:.3f}")
    WORST[key] = max(WORST.get(key, 0.0), worst)
    LW.WORST[key[4:]] = max(LW.WORST[key[4:]], worst)
    assert worst <= 1.0, f"{what}: worst ratio {worst:.3g}"


def log_truth(oracle, name, t):
    if (name, t) not in _TRUTH:
        c = BC.make_case(name)
        tr = HL.ld_log2_truth(c["alle"], c["nr"], c["na"], t, c["W"], c["eps"], c["M"], c["refids"], c["pu"])
        site = CachedOracle(oracle, name).compare(c["alle"], c["nr"], c["na"], t, window=c["W"], eps=c["eps"], max_cov=c["M"],
                                                  refids=c["refids"], pu_id=c["pu"])["site"]
        _TRUTH[name, t] = tr, HL.rows_log2_truth(site[:, 2:3], c["nr"], c["na"], c["W"])
    return _TRUTH[name, t]


@pytest.mark.parametrize("name", BC.NAMES)
def test_log_windows_on_every_background(oracle, name):
    """As test_gpu_depth_edges.test_log_windows_at_every_depth_edge, for the case's three interesting individuals in one run:
    columns 0 and 1 against the log2 truths (NaN where the background is empty), column 2 against the rows' sum, and the
    run's two tables against each other."""
    c = BC.make_case(name)
    t0 = time.perf_counter()
    targets = c["targets"](3)
    with LW.engine_for(c, dict(log_windows=1)) as eng:
        LW.run(eng, c, targets)
        assert eng.last_ld_variant() == 2
        tables = [(eng.window_log2(i), eng.window_ll(i)) for i in range(3)]
    for t, (lg, win) in zip(targets, tables):
        tr, (s, a) = log_truth(oracle, name, t)
        assert lg.shape == (len(tr["log0"]), 3) and win.shape == lg.shape
        assert np.isnan(tr["log0"]).all() and np.isnan(tr["log1"]).all() if is_empty(name, t) else tr["n_bg"] > 0
        for col, key in ((0, "log0"), (1, "log1")):
            _ratio(lg[:, col], tr[key], HL.ld_bar(tr[key], c["n_ids"]), f"{name} individual {t} log2 column {col}", "log ld")
        _ratio(lg[:, 2], s[:, 0], HL.rows_bar(s[:, 0], a[:, 0]), f"{name} individual {t} log2 column 2", "log rows")
        # the two tables of one run, where both are normal doubles: the --LD columns of a non-empty background by the
        # precondition, LIBD2 where its truth says so
        ok = np.ones(lg.shape, dtype=bool)
        ok[:, 2] = s[:, 0] >= -1022
        if is_empty(name, t):
            assert np.isnan(win[:, :2]).all()
            ok[:, :2] = False
        else:
            assert (tr["lin0"] >= LD(2.0) ** -1022).all() and (tr["lin1"] >= LD(2.0) ** -1022).all()
        assert ok[:, 2].any()
        rel = np.abs(np.exp2(lg[ok]) - win[ok]) / win[ok]
        print(f"{name} individual {t}: exp2(window_log2) off window_ll by at most {rel.max():.3e}")
        assert (win[ok] > 0).all() and rel.max() <= 1e-10, f"{name}: exp2(window_log2) off window_ll by {rel.max():.3e}"
    slowest(t0, f"{name} / log_windows")


# --------------------------------------------------------------------------- (e) the report
def test_report():
    """This module's largest ratios to the bounds, its slowest item and the time of all of them (printed with -s)."""
    for key in sorted(WORST, key=str):
        print(f"background edges: {str(key):44s} worst ratio {WORST[key]:.3f}")
    print(f"background edges: slowest item {SLOWEST[1]}: {SLOWEST[0]:.2f} s; all items {TOTAL[0]:.1f} s")
    assert all(v <= 1.0 for v in WORST.values())
