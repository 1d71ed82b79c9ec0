"""Site lists with gaps on the panel's own tiles through every --LD form (the cases of tests/gap_cases.py).

On ibdg_ld_layout 1 every segment record tells the counting kernels' tile ring how many tile pairs to advance before the next
segment of the run, which half of the pair that one reads and which ring slot the pair sits in; k_ld_mfma fetches the segment
ahead by the tile number of the same control word.  Dense site lists advance by 0 or 1.  Here the advances are 0..255 in both
halves, at, below and above every ring depth, behind a run's last pair, across a run's end (where any gap is legal) and one pair
beyond what the control word holds (tests/test_gap_cases.py asserts all of that from the arrays).  A wrong slot, a stale pair
or an off-by-one in the counted wait gives plausible numbers, so every (case, form)
  (1) goes through test_gpu_precision.run_form: per-row values and LIBD2 bit for bit against the oracle, --LD within 1e-10 of
      it, the hp_ref bound of the form on three comparison individuals (the first one the case's target: normal doubles), and
      the variant, count unit and layout the C ABI reports;
  (2) the counting forms -- the gap-free compacted tiles among them -- and every ring depth in the vector, matrix-core, IBD1 and
      groups-of-four forms give the same bits; the matrix-core groups of 15 lie within both bounds of them;
  (3) the zero-coverage rendering and the row_index rendering give the same bits and the same windows;
  (4) 255 pairs run on the counting kernels, 256 take the strict kernel or the compacted tiles, and ld_variant 2 with the
      compacted tiles forbidden is the error ibdg_run has for a form that does not apply;
  (5) option "log_windows" against the truths and bars of tests/hp_log_ref.py.
Every run fixes the run structure gap_cases.run_structure models (windows_per_wave, guided_runs 0, a record budget that never
halves a run).  No bar is new.  test_report (-s) prints the largest ratios and the slowest item; DESIGN.md s2 records them.
"""
import time

import numpy as np
import pytest

import depth_cases as DC
import gap_cases as GC
import hp_log_ref as HL
import hp_ref as H
import test_gpu_log_windows as LW
import test_gpu_precision as P
from ibdgem_amd import engine as E
from test_gpu_depth_edges import EQUAL_FORMS
from test_gpu_launch_trips import RING_FORMS
from test_gpu_parity import assert_bits, assert_ld_close

pytestmark = pytest.mark.gpu

LD = H.LD
WORST = {}          # (form, "normal" / "subnormal") or "log ld" / "log rows" -> largest ratio to its bound, this module's runs
SLOWEST = [0.0, None]
ITEMS = [(name, form) for name in GC.LAYOUT1_NAMES for form in P.FORMS]
OVERFLOWING = ("edge-256", "boundary-shifted")
_PACKED = {}


def packed(name):
    """The case's panel in the device's format, made once (the twins share theirs)."""
    c = GC.make_case(name)
    key = id(c["alle"])
    if key not in _PACKED:
        _PACKED[key] = E.pack_alleles_fast(c["alle"])
    return _PACKED[key]


def slowest(t0, what):
    dt = time.perf_counter() - t0
    if dt > SLOWEST[0]:
        SLOWEST[:] = [dt, what]


def spec_for(name, form, T=None, wpw=None, **more):
    """The FORMS entry as this case runs it: the run structure fixed, and -- as test_gpu_depth_edges.spec_for -- count unit 3
    from the IBD1 form, since every case keeps its tables in LDS.  k_ld_mfma takes every case (test_gap_cases.py)."""
    c = GC.make_case(name)
    spec = dict(P.FORMS[form])
    spec["opts"] = dict(spec["opts"], **GC.run_opts(c, wpw), **more)
    if T is not None:
        spec["T"] = T
    assert DC.tab_in_lds(c["nr"], c["na"], c["W"]) and P.tab_in_lds(c["nr"], c["na"], c["W"])
    assert DC.mfma_takes(c["nr"], c["na"], c["W"])
    if form == "popcount IBD1 form":
        spec["unit"] = 3
    return spec


def timed_run(oracle, name, form, T=None, keep=None, spec=None, rows=False):
    c = GC.make_case(name)
    spec = spec or spec_for(name, form, T)
    alle, nr, na, idx = c["alle"], c["nr"], c["na"], None
    if rows:
        idx, nr, na = GC.row_index_rendering(c)
    # run_form keeps the session's largest ratios per form in P.WORST: this run's are taken apart from them, then merged
    session = dict(P.WORST)
    P.WORST.clear()
    t0 = time.perf_counter()
    try:
        truths = P.run_form(oracle, form, alle, nr, na, c["W"], c["eps"], c["M"], refids=c["refids"], pu=c["pu"],
                            seed=GC.run_seed(name, spec["T"]), spec=spec, keep=keep, rows=idx)
    finally:
        for (f, normal), v in P.WORST.items():
            k = (f, "normal" if normal else "subnormal")
            WORST[k] = max(WORST.get(k, 0.0), v)
        for key, v in session.items():
            P.WORST[key] = max(P.WORST.get(key, 0.0), v)
    slowest(t0, f"{name} / {form}" + (f" T={T}" if T else "") + (" row_index" if rows else ""))
    # the first comparison individual is the case's target: every one of its truths is a normal double
    for key in ("ibd0", "ibd1"):
        assert (truths[0][key] >= LD(2.0) ** -1022).all(), (name, form, key)
    return truths


def plain_run(name, opts, targets, *, variant=2, layout=1, unit=None, what=""):
    """One run of the zero-coverage rendering with `opts`; the window tables of every comparison individual."""
    c = GC.make_case(name)
    with E.Engine(0, c["eps"], c["M"]) as eng:
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.upload_panel(packed(name), c["n_ids"])
        eng.upload_sites(np.arange(len(c["nr"])), c["nr"], c["na"], c["W"])
        eng.run(targets, ld=True)
        assert eng.last_ld_variant() == variant and eng.ld_layout() == layout, (what, eng.last_ld_variant(), eng.ld_layout())
        if unit is not None:
            assert eng.last_count_unit() == unit, (what, eng.last_count_unit())
        return [eng.window_ll(i) for i in range(len(targets))]


# --------------------------------------------------------------------------- 1. every form
@pytest.mark.parametrize("name,form", ITEMS, ids=[f"{n}-{f.replace(' ', '_')}" for n, f in ITEMS])
def test_every_form_on_every_gap_case(oracle, name, form):
    timed_run(oracle, name, form)


# --------------------------------------------------------------------------- 2. equal bits
@pytest.mark.parametrize("name", GC.LAYOUT1_NAMES)
def test_counting_forms_and_ring_depths_give_equal_bits(oracle, name):
    """The same four comparison individuals through the five counting forms ("popcount compacted" has no gaps at all: the
    partner the others are held to), then through ring depths 2, 3, 4 and 8 of the vector, matrix-core, IBD1 and groups-of-four
    forms (the options of test_gpu_launch_trips.RING_FORMS), and -- where the case names a second run structure -- through
    that one as well: every window table is the first one's bits.  Fifteen individuals through k_ld_mfma, the four among them:
    within the bound of hp_ref, and within the two forms' bounds of the counting kernels' values."""
    c = GC.make_case(name)
    t0 = time.perf_counter()
    tables, truths = {}, None
    for form in EQUAL_FORMS:
        keep = {}
        tr = timed_run(oracle, name, form, T=4, keep=keep)
        tables[form] = keep
        truths = truths or tr
    first = tables[EQUAL_FORMS[0]]
    targets = first["targets"]
    assert targets[0] == c["target"] and sorted(first["windows"]) == [0, 2, 3]
    for form in EQUAL_FORMS[1:]:
        assert tables[form]["targets"] == targets
        for i, want in first["windows"].items():
            assert_bits(tables[form]["windows"][i], want, f"{name}: {form} vs {EQUAL_FORMS[0]}, individual {targets[i]}")
    structures = [None] + ([c["alt_wpw"]] if "alt_wpw" in c else [])
    for wpw in structures:
        for ring_form, (form, more, _, unit_lds, _) in RING_FORMS.items():
            unit = 0 if ring_form == "groups of four" else unit_lds         # four individuals: the group alone, no single launch
            for ring in GC.RING_DEPTHS:
                opts = dict(P.FORMS[form]["opts"], **more, **GC.run_opts(c, wpw), ring_slots=ring)
                what = f"{name}: {ring_form}, ring_slots {ring}" + (f", runs of {wpw} windows" if wpw else "")
                got = plain_run(name, opts, targets, unit=unit, what=what)
                for i, want in first["windows"].items():
                    assert_bits(got[i], want, f"{what}, individual {targets[i]}")
    # groups of 15 through the matrix cores
    rng = np.random.default_rng(15)
    others = [int(x) for x in rng.choice([i for i in range(c["n_ids"]) if i not in targets], size=11, replace=False)]
    N = c["n_ids"]
    B_m, B_p, A = H.fast_B("mfma", N), H.fast_B("popcount", N), H.FAST_A
    for form in ("mfma T15 tau0", "mfma T15 tau1"):
        opts = dict(P.FORMS[form]["opts"], **GC.run_opts(c))
        got = plain_run(name, opts, targets + others, unit=0, what=f"{name}: {form}")
        for tr, (i, cnt) in zip(truths, sorted(first["windows"].items())):
            assert_bits(got[i][:, 2], cnt[:, 2], f"{name}: {form} LIBD2, individual {targets[i]}")
            for col, key in ((0, "ibd0"), (1, "ibd1")):
                r = H.check(got[i][:, col], tr[key], B_m, A, f"{name}: {form}, individual {targets[i]} {key}")
                WORST[form, "normal"] = max(WORST.get((form, "normal"), 0.0), r)
                d = np.abs(got[i][:, col].astype(LD) - cnt[:, col].astype(LD))
                both = LD(B_m + B_p) * LD(H.U) * np.abs(tr[key]) + LD(2 * A) * H.TINY
                assert (d <= both).all(), f"{name}: {form} vs the counting kernels, individual {targets[i]} {key}: " \
                                          f"{float((d / both).max()):.3g} of both bounds"
    slowest(t0, f"{name} / equal bits, {len(EQUAL_FORMS)} forms, {len(structures) * 16} ring runs, two groups of 15")


# --------------------------------------------------------------------------- 3. the two renderings
@pytest.mark.parametrize("form", ["popcount mx1", "mfma T15 tau0"])
@pytest.mark.parametrize("name", GC.LAYOUT1_NAMES)
def test_zero_coverage_rows_and_an_omitting_row_index_give_the_same_bits(oracle, name, form):
    c = GC.make_case(name)
    a, b = {}, {}
    timed_run(oracle, name, form, keep=a)
    timed_run(oracle, name, form, keep=b, rows=True)
    assert a["targets"] == b["targets"] and sorted(a["windows"]) == sorted(b["windows"])
    for i, want in a["windows"].items():
        assert_bits(b["windows"][i], want, f"{name}: {form}, row_index rendering, individual {a['targets'][i]}")
    # ibdg_get_windows: the same windows over the same panel rows
    rows, nr, na = GC.row_index_rendering(c)
    bounds = []
    with E.Engine(0, c["eps"], c["M"]) as eng:
        for k, v in spec_for(name, form)["opts"].items():
            eng.set_option(k, v)
        eng.upload_panel(packed(name), c["n_ids"])
        for idx, r, al in ((np.arange(len(c["nr"])), c["nr"], c["na"]), (rows, nr, na)):
            eng.upload_sites(idx, r, al, c["W"])
            assert eng.ld_layout() == 1
            bounds.append(eng.windows())
    (f0, l0, n0), (f1, l1, n1) = bounds
    assert np.array_equal(n0, n1) and np.array_equal(f0, rows[f1]) and np.array_equal(l0, rows[l1])
    assert int(n0.sum()) == len(rows) and len(n0) == -(-len(rows) // c["W"])


# --------------------------------------------------------------------------- 4. the 255 | 256 edge
def test_255_pairs_run_on_the_counting_kernels(oracle):
    for form in ("popcount mx0", "popcount mx1", "popcount_mt T4"):
        spec = spec_for("edge-255", form)
        assert spec["variant"] == 2 and spec["layout"] == 1 and spec["hp"] in ("popcount", "popcount_mt")
        timed_run(oracle, "edge-255", form, spec=spec)
    c = GC.make_case("edge-255")
    # ... also where nothing forces them: the layout and the variant are the upload's own choice with the compacted tiles forbidden
    got = plain_run("edge-255", dict(GC.run_opts(c), ld_variant=2, compact_tiles=-1), [c["target"]], what="edge-255")
    assert np.isfinite(got[0]).all()


@pytest.mark.parametrize("name", OVERFLOWING)
def test_256_pairs_take_the_strict_kernel_or_the_compacted_tiles(oracle, name):
    c = GC.make_case(name)
    run = GC.run_opts(c)
    # compacted tiles forbidden, the variant left to the host: the strict kernel, correct windows and its hp_ref bound
    strict = dict(opts=dict(run, compact_tiles=-1), T=1, variant=1, unit=0, layout=0, hp=1)
    timed_run(oracle, name, "strict tree", spec=strict)
    # compacted tiles allowed: they take the list, with the bits of the form that asks for them
    auto, asked = {}, {}
    spec = spec_for(name, "popcount compacted")
    timed_run(oracle, name, "popcount compacted", keep=asked, spec=spec)
    timed_run(oracle, name, "popcount compacted", keep=auto, spec=dict(spec, opts=dict(spec["opts"], compact_tiles=0)))
    assert auto["targets"] == asked["targets"]
    for i, want in asked["windows"].items():
        assert_bits(auto["windows"][i], want, f"{name}: compact_tiles 0 vs 1")
    # the counting kernels demanded on the panel's own tiles: the error of a form that does not apply, and the context lives on
    rows, nr, na = GC.row_index_rendering(c)
    rs = GC.run_structure(c["nr"], c["na"], c["W"], c["wpw"])
    adv, _, _, in_run = GC.control_words(rs, 2)
    first_big = int(np.flatnonzero(in_run & (adv > 255))[0])
    n_ok = int(rs["seg"]["win"][first_big]) * c["W"]            # the sites of the windows in front of the long gap
    assert n_ok >= 2 * c["W"]
    with E.Engine(0, c["eps"], c["M"]) as eng:
        for k, v in dict(run, ld_variant=2, compact_tiles=-1).items():
            eng.set_option(k, v)
        eng.upload_panel(packed(name), c["n_ids"])
        eng.upload_sites(np.arange(len(c["nr"])), c["nr"], c["na"], c["W"])
        assert eng.ld_layout() == 0
        with pytest.raises(E.EngineError, match=r"ld_variant 2 \(exponent counting\) is not applicable here"):
            eng.run([c["target"]], ld=True)
        eng.upload_sites(rows[:n_ok], nr[:n_ok], na[:n_ok], c["W"])
        eng.run([c["target"]], ld=True)
        assert eng.last_ld_variant() == 2 and eng.ld_layout() == 1
        site, win = eng.site_ll(0), eng.window_ll(0)
    res = oracle.compare(c["alle"][rows[:n_ok]], nr[:n_ok], na[:n_ok], c["target"], window=c["W"], eps=c["eps"], max_cov=c["M"])
    assert_bits(site, res["site"], f"{name}: the next upload, per-row values")
    assert_bits(win[:, 2], res["win"][:, 2], f"{name}: the next upload, LIBD2")
    assert_ld_close(win[:, :2], res["win"][:, :2], f"{name}: the next upload, --LD")


def test_a_gap_between_two_runs_stays_on_the_panel_tiles(oracle):
    """boundary: 300 pairs and 301 between runs, layout 1, and the bits of its compacted run."""
    a, b = {}, {}
    timed_run(oracle, "boundary", "popcount mx1", keep=a)           # (asserts layout 1)
    timed_run(oracle, "boundary", "popcount compacted", keep=b)     # (asserts layout 2)
    assert a["targets"] == b["targets"]
    for i, want in b["windows"].items():
        assert_bits(a["windows"][i], want, "boundary: the panel's own tiles vs the compacted ones")


# --------------------------------------------------------------------------- 5. log_windows
def _ratio(got, truth, bar, what, key):
    got = np.asarray(got, dtype=np.float64).astype(LD)
    assert np.isfinite(got).all() and np.isfinite(truth).all(), what
    worst = float((np.abs(got - truth) / bar).max())
    print(f"{what}: largest ratio to the bar {worst:.3f}")
    WORST[key] = max(WORST.get(key, 0.0), worst)
    LW.WORST[key[4:]] = max(LW.WORST[key[4:]], worst)
    assert worst <= 1.0, f"{what}: worst ratio {worst:.3g}"


@pytest.mark.parametrize("name", ["ladder", "one-row-tiles"])
def test_log_windows_over_the_gaps(oracle, name):
    """As test_gpu_depth_edges.test_log_windows_at_every_depth_edge, on the panel's own tiles."""
    c = GC.make_case(name)
    t0 = time.perf_counter()
    tr = HL.ld_log2_truth(c["alle"], c["nr"], c["na"], c["target"], c["W"], c["eps"], c["M"], c["refids"], c["pu"])
    site = oracle.compare(c["alle"], c["nr"], c["na"], c["target"], ld=True, window=c["W"], eps=c["eps"], max_cov=c["M"],
                          refids=c["refids"], pu_id=c["pu"])["site"]
    s, a = HL.rows_log2_truth(site[:, 2:3], c["nr"], c["na"], c["W"])
    with LW.engine_for(c, dict(GC.run_opts(c), log_windows=1, ld_variant=2, compact_tiles=-1)) as eng:
        LW.run(eng, c, [c["target"]])
        assert eng.last_ld_variant() == 2 and eng.ld_layout() == 1
        lg, win = eng.window_log2(0), eng.window_ll(0)
    assert lg.shape == (len(tr["log0"]), 3) and win.shape == lg.shape
    for col, key in ((0, "log0"), (1, "log1")):
        _ratio(lg[:, col], tr[key], HL.ld_bar(tr[key], c["n_ids"]), f"{name} log2 column {col}", "log ld")
    _ratio(lg[:, 2], s[:, 0], HL.rows_bar(s[:, 0], a[:, 0]), f"{name} log2 column 2", "log rows")
    # the two tables of one run: the --LD columns are normal doubles by the precondition, LIBD2 where its truth says so
    assert (tr["lin0"] >= LD(2.0) ** -1022).all() and (tr["lin1"] >= LD(2.0) ** -1022).all()
    ok = np.ones(lg.shape, dtype=bool)
    ok[:, 2] = s[:, 0] >= -1022
    rel = np.abs(np.exp2(lg[ok]) - win[ok]) / win[ok]
    print(f"{name}: exp2(window_log2) off window_ll by at most {rel.max():.3e}")
    assert (win[ok] > 0).all() and rel.max() <= 1e-10, f"{name}: exp2(window_log2) off window_ll by {rel.max():.3e}"
    slowest(t0, f"{name} / log_windows")


# --------------------------------------------------------------------------- 6. the report
def test_report():
    """This module's largest ratios to the bounds, and its slowest item (printed with -s)."""
    for key in sorted(WORST, key=str):
        print(f"tile gaps: {str(key):44s} worst ratio {WORST[key]:.3f}")
    print(f"tile gaps: slowest item {SLOWEST[1]}: {SLOWEST[0]:.2f} s")
    assert all(v <= 1.0 for v in WORST.values())
