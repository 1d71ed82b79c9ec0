"""Option "log_windows": log2 of the window columns against the long-double truths of tests/hp_log_ref.py.

  * --LD LIBD0 / LIBD1 (k_ld_log): |got - truth| <= (B + 2) u / ln 2 + 2 u |truth|, B = hp_log_ref.log_B(n_ids) <= 40;
  * every other column (k_win_log_rows): |got - truth| <= 2 u sum |log2 s_i| + 2 u |truth|, s_i the oracle's per-site values.
The Poisson(30) cases with 100 rows a window first assert that at least half of the LINEAR LIBD0 column is exactly 0:
that is the regime the option exists for.  Largest ratios to the bars: test_report (-s), recorded in DESIGN.md s4.7.
"""
import numpy as np
import pytest

import hp_log_ref as HL
import hp_ref as H
from ibdgem_amd import engine as E
from test_gpu_parity import assert_bits, bg_counts

pytestmark = pytest.mark.gpu

LD = H.LD
WORST = {"ld": 0.0, "rows": 0.0}
_REF = {}


def reference(oracle, name):
    """The case's inputs and truths, computed once."""
    if name not in _REF:
        c = HL.make_case(name)
        tr = HL.ld_log2_truth(c["alle"], c["nr"], c["na"], c["target"], c["W"], c["eps"], c["M"], c["refids"], c["pu"])
        kw = dict(window=c["W"], eps=c["eps"], max_cov=c["M"], refids=c["refids"], pu_id=c["pu"])
        site_ld = oracle.compare(c["alle"], c["nr"], c["na"], c["target"], ld=True, **kw)["site"]
        site_nl = oracle.compare(c["alle"], c["nr"], c["na"], c["target"], ld=False, **kw)["site"]
        c.update(tr=tr, rows_ld=HL.rows_log2_truth(site_ld[:, 2:3], c["nr"], c["na"], c["W"]),
                 rows_nl=HL.rows_log2_truth(site_nl, c["nr"], c["na"], c["W"]))
        _REF[name] = c
    return _REF[name]


def engine_for(c, opts):
    eng = E.Engine(0, c["eps"], c["M"])
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.upload_panel(E.pack_alleles_fast(c["alle"]), c["n_ids"])
    eng.upload_sites(np.arange(len(c["nr"])), c["nr"], c["na"], c["W"])
    return eng


def run(eng, c, targets, ld=True):
    eng.run(targets, ld=ld, bg_count=bg_counts(c["refids"], c["n_ids"]), pu_id=c["pu"])


def within(got, truth, bar, what, key):
    got = np.asarray(got, dtype=np.float64).astype(LD)
    nan = np.isnan(truth)
    assert (np.isnan(got) == nan).all(), f"{what}: NaN pattern"
    assert np.isfinite(got[~nan]).all(), f"{what}: not finite"
    r = np.abs(got[~nan] - truth[~nan]) / bar[~nan]
    worst = float(r.max()) if r.size else 0.0
    print(f"{what}: largest ratio to the bar {worst:.3f}")
    WORST[key] = max(WORST[key], worst)
    assert worst <= 1.0, f"{what}: {int((r > 1).sum())}/{r.size} beyond the bar, worst ratio {worst:.3g}"


def check_ld_run(c, name, lg, win):
    tr = c["tr"]
    assert lg.shape == (len(tr["log0"]), 3)
    for col, key in ((0, "log0"), (1, "log1")):
        within(lg[:, col], tr[key], HL.ld_bar(tr[key], c["n_ids"]), f"{name} LD column {col}", "ld")
    s, a = c["rows_ld"]
    within(lg[:, 2], s[:, 0], HL.rows_bar(s[:, 0], a[:, 0]), f"{name} LD column 2", "rows")
    plain = c["spread"] is None and tr["n_bg"] > 0
    if plain and c["depth"] == 2:
        # the project's own bar between the two tables of one run
        ok = win > 1e-300
        assert ok.all(), f"{name}: a Poisson(2) window left the double range"
        rel = np.abs(np.exp2(lg[ok]) - win[ok]) / win[ok]
        assert rel.max() <= 1e-10, f"{name}: exp2(window_log2) off window_ll by {rel.max():.3e}"
    if plain and c["depth"] == 30 and c["W"] == 100:
        assert 2 * int((win[:, 0] == 0.0).sum()) >= len(win), f"{name}: the linear LIBD0 column has not underflowed"


@pytest.mark.parametrize("name", list(HL.CASES))
def test_log_windows_against_the_truths(oracle, name):
    """Both tile layouts, "site_results" 0 and 1, an --LD and a non-LD run each; the layouts agree bit for bit."""
    c = reference(oracle, name)
    flip = list(HL.CASES).index(name) & 1
    logs = []
    for compact, layout, sr in ((1, 2, flip), (-1, 1, 1 - flip)):
        with engine_for(c, dict(log_windows=1, compact_tiles=compact, site_results=sr)) as eng:
            run(eng, c, [c["target"]])
            assert eng.ld_layout() == layout and eng.last_ld_variant() == 2
            lg, win = eng.window_log2(0), eng.window_ll(0)
            check_ld_run(c, f"{name} layout {layout}", lg, win)
            logs.append(lg)
            run(eng, c, [c["target"]], ld=False)
            nl = eng.window_log2(0)
            s, a = c["rows_nl"]
            within(nl, s, HL.rows_bar(s, a), f"{name} non-LD", "rows")
            logs.append(nl)
    assert_bits(logs[0], logs[2], f"{name}: the two layouts, --LD")
    assert_bits(logs[1], logs[3], f"{name}: the two layouts, non-LD")


@pytest.mark.parametrize("name", ["N130-W100-e0.02-d2", "bg-mult-d30", "N700-W33-e0.02-d30"])
def test_one_individual_and_many_give_the_same_bits(oracle, name):
    c = reference(oracle, name)
    rng = np.random.default_rng(7)
    targets = [c["target"]] + [int(x) for x in rng.choice([i for i in range(c["n_ids"]) if i != c["target"]], 16, replace=False)]
    with engine_for(c, dict(log_windows=1)) as eng:
        single = {}
        for t in targets:
            run(eng, c, [t])
            single[t] = eng.window_log2(0)
        check_ld_run(c, f"{name} single", single[c["target"]], eng_ll(eng, c, c["target"]))
        for T in (5, 17):
            run(eng, c, targets[:T])
            every = eng.window_log2_all(T)
            for i, t in enumerate(targets[:T]):
                assert_bits(every[i], single[t], f"{name}: individual {t} in a run of {T}")
                assert_bits(eng.window_log2(i), every[i], f"{name}: window_log2_all against window_log2({i})")
            run(eng, c, targets[:T])
            assert_bits(eng.window_log2_all(T), every, f"{name}: a second run of {T}")
        # a queue of runs over different individuals
        eng.set_option("async", 1)
        for t in targets[:6]:
            run(eng, c, [t])
        eng.sync()
        assert_bits(eng.window_log2(0), single[targets[5]], f"{name}: the last of six queued runs")
        for t in targets[:3]:
            run(eng, c, [t], ld=False)
        eng.sync()
        queued = eng.window_log2(0)
        eng.set_option("async", 0)
        run(eng, c, [targets[2]], ld=False)
        assert_bits(queued, eng.window_log2(0), f"{name}: the last of three queued non-LD runs")


def eng_ll(eng, c, t):
    run(eng, c, [t])
    return eng.window_ll(0)


@pytest.mark.parametrize("ld", [True, False])
def test_the_option_changes_nothing_else(oracle, ld):
    c = reference(oracle, "N130-W33-e0.001-d2")
    targets = [c["target"], 77, 4]
    got = []
    for on in (0, 1):
        with engine_for(c, dict(log_windows=on)) as eng:
            run(eng, c, targets, ld=ld)
            got.append(([eng.window_ll(i) for i in range(3)], [eng.site_ll(i) for i in range(3)]))
            if not on:
                with pytest.raises(E.EngineError, match="log_windows"):
                    eng.window_log2(0)
                with pytest.raises(E.EngineError, match="log_windows"):
                    eng.window_log2_all(3)
    for i in range(3):
        assert_bits(got[1][0][i], got[0][0][i], f"window_ll of individual {i} with the option on")
        assert_bits(got[1][1][i], got[0][1][i], f"site_ll of individual {i} with the option on")


def test_errors(oracle):
    c = dict(reference(oracle, "N64-W33-e0.02-d2"))
    with engine_for(c, dict(log_windows=1)) as eng:
        run(eng, c, [1, 2])
        with pytest.raises(E.EngineError, match="no results for target 2"):
            eng.window_log2(2)
        eng.set_option("log_windows", 0)
        run(eng, c, [1, 2])
        with pytest.raises(E.EngineError, match="option log_windows"):
            eng.window_log2(0)
    for eps, M, why in ((1e-30, 20, "clamped"), (0.02, 60, "max_cov > 50")):
        bad = dict(c, eps=eps, M=M)
        with engine_for(bad, dict(log_windows=1)) as eng:
            with pytest.raises(E.EngineError, match=why):
                run(eng, bad, [1])
            run(eng, bad, [1], ld=False)            # (a non-LD run always produces the table)
            assert np.isfinite(eng.window_log2(0)).all()
    with pytest.raises(E.EngineError, match="log_windows must be"):
        with E.Engine(0, 0.02, 20) as eng:
            eng.set_option("log_windows", 2)


def test_report():
    """The largest ratios to the two bars over this session (printed with -s)."""
    print(f"log_windows: --LD columns {WORST['ld']:.3f} of (B + 2) u / ln 2 + 2 u |t| (B = {HL.log_B(130):.1f} at 130 "
          f"individuals), row-sum columns {WORST['rows']:.3f} of 2 u sum |log2 s| + 2 u |t|")
    assert all(v <= 1.0 for v in WORST.values())
