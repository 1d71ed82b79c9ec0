"""Every constructed --LD edge case through the routes a context takes when no option is set (tests/route_cases.py).

The 40 cases of depth_cases, gap_cases and bg_cases reach the device in their own modules through fresh contexts whose options
force one form, one synchronous run each.  The host program and bench.py set no such option: single runs count everything
until the eighth makes the IBD0 pass and takes the IBD1 form, the 22nd re-lays the site list out into compacted tiles (a sparse
list is compacted at the upload), queued runs leave their finalising step to the next launch, and groups of 15 take their IBD0
terms from whatever pass exists.  Here
  (a) every case goes through every entry of test_gpu_precision.ROUTE_FORMS -- the IBD1 form on compacted tiles (what bench.py
      times), groups of four and of 15 on compacted tiles, and no option at all -- with run_form: per-row values and LIBD2 bit
      for bit against the oracle, --LD within 1e-10 of it, the hp_ref bound of the form, and the variant, count unit and layout
      the C ABI reports; the counting forms must be the BITS of the module's first EQUAL_FORMS entry on the panel's own tiles
      ("popcount compacted" where those do not apply), the groups of 15 the bits of the same groups on the panel's own tiles;
  (b) every case lives the life of a default context: 24 queued single runs of six individuals in turn, (layout, count unit,
      window end) asserted against route_cases.expected after every run, the tables read after every run (pattern A) or after
      every third only (pattern B: finalising steps cross the pass run and the relayout's quiesce unread); then a run of 16 (a
      group of 15 with the pass that single runs made, on compacted tiles), a run of 9 through the groups of four, and the
      same list uploaded again.  Every table read is the bits of a lone synchronous run that counts everything;
  (c) one default context takes every background of the small panel in turn and back, nine queued runs each.
No bar is new, and no item is skipped (asserted).  test_report (-s) prints the largest ratios and the slowest item; DESIGN.md s2
records them.
"""
import functools
import time

import numpy as np
import pytest

import bg_cases as BC
import depth_cases as DC
import gap_cases as GC
import hp_ref as H
import route_cases as RC
import test_gpu_bg_edges as BG
import test_gpu_depth_edges as DE
import test_gpu_precision as P
import test_gpu_tile_gaps as TG
from ibdgem_amd import engine as E
from test_gpu_depth_edges import EQUAL_FORMS
from test_gpu_parity import assert_bits, bg_counts

pytestmark = pytest.mark.gpu

LD = H.LD
WORST = {}          # (form, "normal" / "not normal") -> largest ratio to its bound, this module's runs
SLOWEST = [0.0, None]
TOTAL = [0.0]
SIBLINGS = {"depth": DE, "gap": TG, "bg": BG}
_PACKED = {}


def _in_lds(case):
    c = RC.make_case(*case)
    return DC.tab_in_lds(c["nr"], c["na"], c["W"])


# the mfma forms are left out only where the tables are not in LDS (as test_gpu_depth_edges.ITEMS): full-depth-16
ITEMS = [(case, form) for case in RC.CASES for form in P.ROUTE_FORMS if not (P.ROUTE_FORMS[form]["hp"] == "mfma" and not _in_lds(case))]
N_MFMA_FORMS = sum(s["hp"] == "mfma" for s in P.ROUTE_FORMS.values())
assert len(P.ROUTE_FORMS) == 6 and N_MFMA_FORMS == 3
assert len(ITEMS) == 40 * 6 - N_MFMA_FORMS * sum(not _in_lds(case) for case in RC.CASES) == 237


def slowest(t0, what):
    dt = time.perf_counter() - t0
    TOTAL[0] += dt
    if dt > SLOWEST[0]:
        SLOWEST[:] = [dt, what]


def packed(c):
    """A panel in the device's format, made once."""
    key = id(c["alle"])
    if key not in _PACKED:
        _PACKED[key] = E.pack_alleles_fast(c["alle"])
    return _PACKED[key]


def overflowing(case):
    """The panel's own tiles do not serve the list (a gap of 256 pairs inside a run)."""
    return case[0] == "gap" and case[1] in TG.OVERFLOWING


@functools.lru_cache(maxsize=None)
def people(case, T):
    """The case's T comparison individuals, its target first: bg_cases' own lists; for the depth and gap cases the draw
    test_gpu_precision.run_form makes with the module's run_seed."""
    kind, name = case
    c = RC.make_case(kind, name)
    if kind == "bg":
        out = list(c["targets"](T))
    else:
        rng = np.random.default_rng(RC.MODULES[kind].run_seed(name, T))
        cand = np.array([x for x in range(c["n_ids"]) if x != c["pu"]])
        out = [int(x) for x in rng.choice(cand, size=T, replace=False)]
    assert out[0] == c["target"] and len(set(out)) == T
    return out


def is_empty(case, t):
    return case[0] == "bg" and BG.is_empty(case[1], t)


def spec_for(case, form):
    """The ROUTE_FORMS entry as this case runs it, by the rules of the three modules' spec_for: the gap cases fix their run
    structure (not where the form is "no option at all"); the IBD1 form reports count unit 3 where the tables are in LDS, else 2;
    groups that k_ld_mfma does not take are split by k_ld_popcount_mt's groups of four; a default context compacts a sparse list."""
    kind, name = case
    c = RC.make_case(kind, name)
    spec = dict(P.ROUTE_FORMS[form])
    spec["opts"] = dict(spec["opts"])
    defaults = form.startswith("defaults")
    if kind == "gap" and not defaults:
        spec["opts"].update(GC.run_opts(c))
    if form == "popcount IBD1 compacted":
        spec["unit"] = 3 if _in_lds(case) else 2
    if spec["hp"] == "mfma" and not DC.mfma_takes(c["nr"], c["na"], c["W"]):
        spec["hp"] = "popcount_mt"
        spec["unit"] = 0 if spec["T"] % 4 == 0 else (2, 3)
    if defaults:
        spec["layout"] = 2 if RC.sparse(c) else 1
    return spec


def bg_of(case):
    kind, name = case
    c = RC.make_case(kind, name)
    return dict(bg_count=c["mult"] if kind == "bg" else bg_counts(c["refids"], c["n_ids"]), pu_id=c["pu"])


def engine_for(case, opts):
    c = RC.make_case(*case)
    eng = E.Engine(0, c["eps"], c["M"])
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.upload_panel(packed(c), c["n_ids"])
        eng.upload_sites(np.arange(len(c["nr"])), c["nr"], c["na"], c["W"])
    except BaseException:
        eng.close()
        raise
    return eng


def _tables(case, spec, targets):
    """One synchronous run of `targets` in a fresh context with the spec's options: every individual's window table."""
    with engine_for(case, spec["opts"]) as eng:
        eng.run(targets, ld=True, **bg_of(case))
        assert eng.last_ld_variant() == spec["variant"], (case, eng.last_ld_variant())
        if spec["layout"] is not None:
            assert eng.ld_layout() in (spec["layout"] if isinstance(spec["layout"], tuple) else (spec["layout"],)), (case, eng.ld_layout())
        return [eng.window_ll(i) for i in range(len(targets))]


@functools.lru_cache(maxsize=None)
def sibling_tables(case, form, T):
    """The case's people(T) through entry `form` of test_gpu_precision.FORMS as the case's own module runs it."""
    return _tables(case, SIBLINGS[case[0]].spec_for(case[1], form, T), people(case, T))


@functools.lru_cache(maxsize=None)
def route_tables(case, form):
    """... through entry `form` of ROUTE_FORMS, all T tables (run_form keeps those of the individuals it checks)."""
    spec = spec_for(case, form)
    return _tables(case, spec, people(case, spec["T"]))


def counting_form(case):
    """The form the counting kernels' bits are held to: the first of EQUAL_FORMS on the panel's own tiles; where those do not
    apply, the compacted run of test_gpu_tile_gaps."""
    return "popcount compacted" if overflowing(case) else EQUAL_FORMS[0]


# --------------------------------------------------------------------------- (a) the route's forms
def timed_run(oracle, case, form):
    kind, name = case
    c = RC.make_case(kind, name)
    spec = spec_for(case, form)
    targets = people(case, spec["T"])
    checked = BC.checked(name, spec["T"]) if kind == "bg" else sorted({0, spec["T"] // 2, spec["T"] - 1})
    keep = {}
    orc = BG.CachedOracle(oracle, name) if kind == "bg" else oracle
    # run_form keeps the session's largest ratios per form in P.WORST: this run's are taken apart from them, then merged
    session = dict(P.WORST)
    P.WORST.clear()
    t0 = time.perf_counter()
    try:
        truths = P.run_form(orc, form, c["alle"], c["nr"], c["na"], c["W"], c["eps"], c["M"], refids=c["refids"], pu=c["pu"],
                            spec=spec, keep=keep, targets=targets, checked=checked)
    finally:
        for (f, normal), v in P.WORST.items():
            k = (f, "normal" if normal else "not normal")
            WORST[k] = max(WORST.get(k, 0.0), v)
        for key, v in session.items():
            P.WORST[key] = max(P.WORST.get(key, 0.0), v)
    assert keep["targets"] == targets and sorted(keep["windows"]) == checked and len(truths) == len(checked)
    for i, tr in zip(checked, truths):
        win = keep["windows"][i]
        if is_empty(case, targets[i]):
            assert tr["n_bg"] == 0 and np.isnan(win[:, :2]).all() and np.isfinite(win[:, 2]).all(), (case, form, targets[i])
        else:
            assert np.isfinite(win).all(), (case, form, targets[i])
    # the first comparison individual is the case's target: every one of its truths is a normal double (or NaN: nobody to compare with)
    if not is_empty(case, targets[0]):
        for key in ("ibd0", "ibd1"):
            assert (truths[0][key] >= LD(2.0) ** -1022).all(), (case, form, key)
    return spec, targets, keep["windows"]


@pytest.mark.parametrize("case,form", ITEMS, ids=[f"{c[0]}-{c[1]}-{f.replace(' ', '_')}" for c, f in ITEMS])
def test_every_route_form_on_every_case(oracle, case, form):
    t0 = time.perf_counter()
    spec, targets, windows = timed_run(oracle, case, form)
    T = spec["T"]
    if form.startswith("popcount"):
        # exact integer counts, the same additions in the same order: the bits of the form that counts by (mask, count) pairs
        want = sibling_tables(case, counting_form(case), T)
        for i, got in windows.items():
            assert_bits(got, want[i], f"{case}: {form} vs {counting_form(case)}, individual {targets[i]}")
    elif form.startswith("mfma"):
        # the run's other tables are the run's: part (b) holds a default context's group of 15 to all of them
        every = route_tables(case, form)
        for i, got in windows.items():
            assert_bits(got, every[i], f"{case}: {form}, a second run, individual {targets[i]}")
        if not overflowing(case):
            # compacted tiles give the bits of the panel's own (test_gpu_parity.test_compacted_tiles_give_the_bits_of_the_panel_tiles)
            want = sibling_tables(case, form.replace(" compacted", ""), T)
            for i in range(T):
                assert_bits(every[i], want[i], f"{case}: {form} vs the panel's own tiles, individual {targets[i]}")
        else:
            want = sibling_tables(case, counting_form(case), T)
            assert_bits(every[T - 1], want[T - 1], f"{case}: {form}, the single individual {targets[T - 1]}")
    else:
        # no option at all: the single individuals' tables are the counting kernels' bits whatever layout the upload chose
        want = sibling_tables(case, counting_form(case), T)
        single = range(T) if T == 1 or spec["hp"] != "mfma" else [T - 1]
        for i in single:
            if i in windows:
                assert_bits(windows[i], want[i], f"{case}: {form} vs {counting_form(case)}, individual {targets[i]}")
    slowest(t0, f"{case[0]} {case[1]} / {form}")


# --------------------------------------------------------------------------- (b) the life of a default context
@functools.lru_cache(maxsize=None)
def references(case):
    """individual -> window table of its lone synchronous run in the form that counts everything, on the reference layout of
    (a): one context, one run per individual that (b) or (c) reads."""
    kind, name = case
    form = "popcount compacted" if overflowing(case) else "popcount mx1"
    spec = SIBLINGS[kind].spec_for(name, form)
    who = sorted(set(people(case, 6)) | set(people(case, 16)))
    out = {}
    with engine_for(case, spec["opts"]) as eng:
        for t in who:
            eng.run([t], ld=True, **bg_of(case))
            assert (eng.last_ld_variant(), eng.last_count_unit(), eng.ld_layout(), eng.last_window_end()) == (2, 2, spec["layout"], 1), (case, t)
            out[t] = eng.window_ll(0)
            if is_empty(case, t):
                assert np.isnan(out[t][:, :2]).all() and np.isfinite(out[t][:, 2]).all(), (case, t)
            else:
                assert np.isfinite(out[t]).all(), (case, t)
    return out


def report(eng):
    return eng.ld_layout(), eng.last_count_unit(), eng.last_window_end()


def assert_triple(eng, want, case, what):
    got = report(eng)
    assert eng.last_ld_variant() == 2, (case, what)
    if case in RC.UNSURE_END:
        assert got[:2] == want[:2] and got[2] in (1, 2), f"{case} {what}: (layout, count unit, window end) {got}, expected {want[:2]}"
    else:
        assert got == want, f"{case} {what}: (layout, count unit, window end) {got}, expected {want}"
    return got


def assert_table(eng, i, case, t, ref, what):
    got = eng.window_ll(i)
    if is_empty(case, t):
        assert np.isnan(got[:, :2]).all(), f"{case} {what}: an empty background, individual {t}"
    assert_bits(got, ref[t], f"{case} {what}, individual {t}")


@functools.lru_cache(maxsize=None)
def life(case):
    """Patterns A and B and what follows them in context B; returns the triple context B reported after its 24th run."""
    c = RC.make_case(*case)
    ref = references(case)
    six, sixteen = people(case, 6), people(case, 16)
    order = RC.cycle(six)
    want = RC.expected(case, RC.N_RUNS)
    bg = bg_of(case)
    assert all(a != b for a, b in zip(order, order[1:]))
    sites = (np.arange(len(c["nr"])), c["nr"], c["na"], c["W"])
    # pattern A: every run is read, so each finalises behind itself
    with engine_for(case, {"async": 1}) as eng:
        for k, t in enumerate(order, 1):
            eng.run([t], ld=True, **bg)
            assert_triple(eng, want[k - 1], case, f"pattern A run {k}")
            assert_table(eng, 0, case, t, ref, f"pattern A run {k} {want[k - 1]}")
    # pattern B: every third run is read; the finalising steps of the others ride in the next launch -- across the pass run (8)
    # and the relayout (22)
    with engine_for(case, {"async": 1}) as eng:
        for k, t in enumerate(order, 1):
            eng.run([t], ld=True, **bg)
            ended = assert_triple(eng, want[k - 1], case, f"pattern B run {k}")
            if k in RC.READS_B:
                assert_table(eng, 0, case, t, ref, f"pattern B run {k} {want[k - 1]}")
        # a group of 15 and one: on compacted tiles by now, the IBD0 pass (where there is one) made by a single run
        eng.set_option("async", 0)
        eng.run(sixteen, ld=True, **bg)
        assert eng.ld_layout() == 2 and eng.last_ld_variant() == 2, case
        if _in_lds(case):
            spec = spec_for(case, "mfma compacted T16 tau1")
            assert eng.last_count_unit() in (spec["unit"] if isinstance(spec["unit"], tuple) else (spec["unit"],)), (case, eng.last_count_unit())
            group = route_tables(case, "mfma compacted T16 tau1")
            for i in range(15):
                assert_bits(eng.window_ll(i), group[i], f"{case}: the group of 15 of a default context, individual {sixteen[i]}")
        else:
            for i in range(15):
                assert_table(eng, i, case, sixteen[i], ref, "sixteen through the counting kernels")
        assert_table(eng, 15, case, sixteen[15], ref, "the one beside the group of 15")
        # nine through the groups of four
        eng.set_option("mfma_targets", 0)
        eng.run(sixteen[:9], ld=True, **bg)
        assert eng.ld_layout() == 2 and eng.last_ld_variant() == 2, case
        for i in range(9):
            assert_table(eng, i, case, sixteen[i], ref, "nine through the groups of four")
        eng.set_option("mfma_targets", 1)
        # the same site list again: the route starts over
        eng.set_option("async", 1)
        eng.upload_sites(*sites)
        eng.run([six[0]], ld=True, **bg)
        assert_triple(eng, want[0], case, "run 1 of the second upload")
        assert_table(eng, 0, case, six[0], ref, "run 1 of the second upload")
    return ended


@pytest.mark.parametrize("case", RC.CASES, ids=["-".join(c) for c in RC.CASES])
def test_the_life_of_a_default_context(case):
    t0 = time.perf_counter()
    fresh = life.cache_info().currsize
    life(case)
    if life.cache_info().currsize > fresh:
        slowest(t0, f"{case[0]} {case[1]} / the life of a default context")


def test_every_module_ends_on_the_form_the_benchmark_times():
    """From the reports of pattern B's 24th run, not from the model: (compacted tiles, IBD1 form, paired window end)."""
    ended = {case: life(case) for case in RC.CASES}
    for kind in RC.MODULES:
        assert any(t == (2, 3, 2) for case, t in ended.items() if case[0] == kind), (kind, ended)
    assert all(t[0] == 2 for t in ended.values())


# --------------------------------------------------------------------------- (c) one context, every small-panel background
def test_one_default_context_through_every_small_panel_background():
    """bg_cases.A_NAMES in order and back in ONE default context (async 1): per background nine queued single runs -- the case's
    second and third individual and its target, in turn --, the triple asserted after every run, the ninth run read.  The count
    towards the IBD0 pass restarts with every background (count unit 2 seven times, then 3); the relayout's credit belongs to the
    upload: the 22nd run -- the fourth on the third background -- compacts the list, and every later pass is made on compacted
    tiles.  At the turn the last background simply goes on."""
    t0 = time.perf_counter()
    first = ("bg", BC.A_NAMES[0])
    n_run, key, on_bg = 0, None, 0
    seen = set()
    with engine_for(first, {"async": 1}) as eng:
        for name in BC.A_NAMES + BC.A_NAMES[::-1]:
            case = ("bg", name)
            c = RC.make_case(*case)
            assert c["alle"] is RC.make_case(*first)["alle"] and c["nr"] is RC.make_case(*first)["nr"]
            ref = references(case)
            target, second, third = c["targets"](3)
            if (c["mult"].tobytes(), c["pu"]) != key:
                key, on_bg = (c["mult"].tobytes(), c["pu"]), 0
            # the model's runs on this background, the earlier runs on the upload as credit
            triples = RC.expected(case, on_bg + 9, first_credit=(n_run - on_bg) * RC.CREDIT_PER_RUN)[on_bg:]
            for k, want in enumerate(triples):
                t = (second, third, target)[k % 3]
                eng.run([t], ld=True, **bg_of(case))
                n_run += 1
                on_bg += 1
                assert_triple(eng, want, case, f"run {n_run}, the {on_bg}th on its background")
                seen.add(want)
            assert on_bg in (9, 18) and (on_bg == 18) == (n_run == 9 * (len(BC.A_NAMES) + 1))
            assert_table(eng, 0, case, target, ref, f"run {n_run}, the ninth of {name}")
    assert n_run == 2 * 9 * len(BC.A_NAMES) and seen == {(1, 2, 1), (1, 3, 2), (2, 2, 1), (2, 3, 2)}
    slowest(t0, "one default context through every background of panel A, and back")


# --------------------------------------------------------------------------- (d) the report
def test_report():
    """This module's largest ratios to the bounds per route form, its slowest item and the time of all of them (printed with -s)."""
    for key in sorted(WORST, key=str):
        print(f"default route: {str(key):44s} worst ratio {WORST[key]:.3f}")
    print(f"default route: slowest item {SLOWEST[1]}: {SLOWEST[0]:.2f} s; all items {TOTAL[0]:.1f} s")
    assert all(v <= 1.0 for v in WORST.values())
