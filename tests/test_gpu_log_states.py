"""GPU tier: ibdg_window_log2_states (IBD-state paths over the log2 window table, on the device) against its host twin
ibdg_log2_states_host, bit for bit, on tables written by real runs with "log_windows" 1; and ibdg_window_log2_llr_sums
against the long-double model of tests/test_gpu_arm_stats.py with the table's own entries as terms (same 2^-50 bound)."""
import os
import subprocess

import numpy as np
import pytest

import hp_log_ref as HL
import log_states_util as U
from ibdgem_amd import engine as E
from test_gpu_arm_stats import dd_add, model, random_case, segments

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDENGEM = os.path.join(REPO, "ibdgem_amd", "host", "hiddengem")
HEAD = "# SEGMENT\tSTART\tEND\tLIBD0\tLIBD1\tLIBD2\tNUM_SITES\n"


def engine(alle, nr, na, W, eps=0.02, M=20, **opts):
    eng = E.Engine(0, eps, M)
    eng.set_option("log_windows", 1)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.upload_panel(E.pack_alleles_fast(alle), alle.shape[1] // 2)
    eng.upload_sites(np.arange(len(nr)), nr, na, W)
    return eng


# ---- device against twin --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_win", [1, 2, 3, 255, 256, 257, 513, 1000])
def test_non_ld_tables_of_every_block_shape(n_win):
    """Windows of 2 rows, every row with reads: n_win windows exactly.  255 / 256 / 257: the last thread without a window,
    every thread with one, two windows a thread with a partial last block; 1, 2, 3: one thread does it all."""
    N = 24
    alle, nr, na = U.covered_reads(n_win, 2 * n_win - 1, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win
        for T in (1, 5, 17):
            eng.run([(3 + 5 * i) % N for i in range(T)], ld=False)
            U.device_equals_twin(eng, T, what=f"n_win {n_win}, T {T}")
        eng.run([1, 2], ld=False)
        U.device_equals_twin(eng, 2, pen=(1.0, 0.5, 1e-300), what="other penalties")


@pytest.mark.parametrize("compact,layout", [(1, 2), (-1, 1)])
def test_ld_tables_on_both_tile_layouts(compact, layout):
    alle, nr, na = random_case(41, N=70, L=3000)
    with engine(alle, nr, na, 5, compact_tiles=compact) as eng:
        assert eng.n_windows > 256
        for T in (1, 17):
            eng.run([(2 + 3 * i) % 70 for i in range(T)], ld=True)
            assert eng.ld_layout() == layout
            tabs, _, _, _ = U.device_equals_twin(eng, T, what=f"--LD layout {layout}, T {T}")
            _, path, _, _ = U.device_equals_twin(eng, T, pen=(0.9, 0.9, 0.9), what=f"--LD layout {layout}, T {T}, small penalties")
            assert np.isfinite(tabs).all() and len(np.unique(path)) > 1


def test_nan_columns_of_an_empty_background_are_neutral_windows():
    alle, nr, na = random_case(42, N=70, L=2000)
    with engine(alle, nr, na, 3) as eng:
        bg = np.zeros(70, dtype=np.uint8)
        bg[3] = 1                                                  # the only background individual is the compared one
        eng.run([3], ld=True, bg_count=bg)
        tabs, path, score, count = U.device_equals_twin(eng, 1, what="empty background")
        assert np.isnan(tabs[0, :, :2]).all() and np.isfinite(tabs[0, :, 2]).all()
        assert (score == 0).all() and (path == 0).all() and count[0].tolist() == [eng.n_windows, 0, 0]


def test_equal_columns_tie_everywhere():
    """Every individual homozygous alternative: f = 1, and the three per-row values are the same P(D | 1/1)."""
    alle, nr, na = HL.spread_inputs(130, 7, False)
    alle, nr, na = np.tile(alle, (20, 1)), np.tile(nr, 20), np.tile(na, 20)
    with engine(alle, nr, na, 7) as eng:
        eng.run([0, 9, 64, 100, 129], ld=False)
        tabs, path, score, _ = U.device_equals_twin(eng, 5, what="equal columns")
        assert eng.n_windows > 60
        assert (tabs[..., 0] == tabs[..., 1]).all() and (tabs[..., 0] == tabs[..., 2]).all()
        assert (score == 0).all() and (path == 0).all()


# ---- the regime the log table exists for ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def deep():
    """Poisson(30) reads, -M 50, windows of 100 rows (hp_log_ref.issue_inputs): one --LD run of the related individual 0
    and four unrelated ones, the pileup's own individual (0) left out of every background as with -N."""
    alle, nr, na = HL.issue_inputs(30, True)
    targets = [0, 7, 50, 99, 129]
    with engine(alle, nr, na, 100, eps=0.02, M=50) as eng:
        eng.run(targets, ld=True, pu_id=0)
        n = eng.n_windows
        lin = eng.window_ll_all(5)
        tabs, path, score, count = U.device_equals_twin(eng, 5, what="Poisson(30)")
        first, end = [0, 0, 4, n // 2], [n, 4, n, n]
        _, log_sums = U.log_sums_match_model(eng, 5, first, end)
        lin_sums = eng.window_llr_sums(first, end)
        whole = eng.window_log2_llr_sums([1], [n - 1])
        parts = eng.window_log2_llr_sums([1] * (n - 3) + list(range(2, n - 1)), list(range(2, n - 1)) + [n - 1] * (n - 3))
    return dict(lin=lin, tabs=tabs, path=path, count=count, first=first, end=end, log_sums=log_sums, lin_sums=lin_sums,
                whole=whole, parts=parts, n=n)


def test_deep_coverage_poisons_the_linear_path_and_not_the_log_path(deep, tmp_path):
    lin, n = deep["lin"], deep["n"]
    assert 2 * int((lin[0, :, 0] == 0.0).sum()) >= n                          # the linear LIBD0 column has underflowed
    print("windows with all three linear columns 0, per individual:", (lin == 0.0).all(axis=2).sum(axis=1).tolist())
    poisoned = 0
    for t in range(5):
        fn = tmp_path / f"t{t}.summary.txt"
        fn.write_text(HEAD + "".join("%d\t%d\t%d\t%e\t%e\t%e\t100\n" % (w + 1, 100 * w, 100 * w + 99, *lin[t, w]) for w in range(n)))
        res = subprocess.run([HIDDENGEM, "-s", str(fn)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        rows = [l.split("\t") for l in res.stdout.splitlines()[1:] if not l.startswith("#")]
        assert len(rows) == n
        poisoned += any("nan" in x for r in rows for x in r[1:4])
    assert poisoned >= 1                                                     # hg_solve's scores are NaN
    assert np.isfinite(deep["tabs"]).all()
    assert (deep["count"].sum(axis=1) == n).all()                            # (device == twin: the fixture)
    assert (deep["path"][0] == 2).all()                                      # the reads ARE individual 0's


def test_deep_coverage_log_sums_differ_from_the_saturated_linear_sums(deep):
    """Individual 0, whose every linear LIBD0 is 0 (asserted above): each of its terms enters the linear sums as 1074 bits."""
    _, bound = U.log_model(deep["tabs"], deep["first"], deep["end"])
    diff = np.abs(deep["log_sums"][..., 0] - deep["lin_sums"][..., 0])
    print("log sums against linear sums, |difference| / bound per individual and range:", (diff / bound[..., 0]).tolist())
    assert (diff[0] > bound[0, :, 0]).all(), (diff[0].min(), bound[0, :, 0].max())


def test_deep_coverage_split_invariance(deep):
    """A range cut in two at every window: the parts' double-doubles added as the host program adds its devices' give
    the whole range's sum to the bit."""
    whole, parts, n = deep["whole"], deep["parts"], deep["n"]
    m = n - 3
    for t in range(5):
        for c in range(m):
            for k in (0, 2):
                acc = dd_add([0.0, 0.0], parts[t, c, k], parts[t, c, k + 1])
                acc = dd_add(acc, parts[t, m + c, k], parts[t, m + c, k + 1])
                assert acc[0] + acc[1] == whole[t, 0, k], (t, c, k)


# ---- ibdg_window_log2_llr_sums ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ld", [True, False])
def test_log_sums_match_the_long_double_model(ld):
    alle, nr, na = random_case(11)
    with engine(alle, nr, na, 50) as eng:
        n = eng.n_windows
        first, end = segments(n)
        for T in (1, 16, 61):
            eng.run([(7 + 3 * i) % 100 for i in range(T)], ld=ld)
            tabs, got = U.log_sums_match_model(eng, T, first, end)
            assert (got[:, 0, :] == 0).all()                           # the empty range
            # where nothing underflows the two statistics are the same number: a window's two tables agree to 1e-10
            # relative (the bar of tests/test_gpu_log_windows.py), i.e. 1e-10 / ln 2 per log and two logs per term
            lin = eng.window_llr_sums(first, end)
            _, b_lin = model(eng.window_ll_all(T), first, end)
            _, b_log = U.log_model(tabs, first, end)
            tol = b_lin[..., 0] + b_log[..., 0] + 2 * 1.45e-10 * np.array([max(e - f, 0) for f, e in zip(first, end)])
            assert (np.abs(lin[..., 0] - got[..., 0]) <= tol).all()
        bg = np.zeros(100, dtype=np.uint8)
        bg[3] = 1
        eng.run([3], ld=True, bg_count=bg)                             # NaN windows: NaN sums, the empty range still 0
        _, got = U.log_sums_match_model(eng, 1, [0, 2, 7], [n, 3, 7])
        assert np.isnan(got[0, :2, [0, 2]]).all() and (got[0, 2] == 0).all()


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_errors():
    alle, nr, na = random_case(12, N=20, L=300)
    with engine(alle, nr, na, 50) as eng:
        with pytest.raises(E.EngineError, match="no results"):
            eng.window_log2_states(*U.PEN)
        with pytest.raises(E.EngineError, match="no results"):
            eng.window_log2_llr_sums([0], [1])
        eng.run([1, 2], ld=True)
        n = eng.n_windows
        for pen in ((0.0, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, float("nan")), (-1.0, 0.5, 0.5)):
            with pytest.raises(E.EngineError, match=r"is not in \(0, 1\]"):
                eng.window_log2_states(*pen)
        assert eng.lib.ibdg_window_log2_states(eng.ctx, 0.5, 0.5, 0.5, None, None, None) != 0
        for first, end in (([4], [3]), ([0], [n + 1])):
            with pytest.raises(E.EngineError, match="ibdg_window_log2_llr_sums"):
                eng.window_log2_llr_sums(first, end)
        assert eng.window_log2_llr_sums([], []).shape == (2, 0, 4)
        U.device_equals_twin(eng, 2)
        eng.upload_sites(np.arange(len(nr)), nr, na, 25)              # a new upload replaces the results
        with pytest.raises(E.EngineError, match="no results"):
            eng.window_log2_states(*U.PEN)
        eng.set_option("log_windows", 0)
        eng.run([1, 2], ld=True)
        with pytest.raises(E.EngineError, match="option log_windows"):
            eng.window_log2_states(*U.PEN)
        with pytest.raises(E.EngineError, match="option log_windows"):
            eng.window_log2_llr_sums([0], [1])
        assert eng.window_llr_sums([0], [1]).shape == (2, 1, 4)        # (the linear sums do not need the option)


# ---- the host program: --log-stats on a device ---------------------------------------------------------------------------

import armstats_check as A            # noqa: E402
import pileup_list_util as PL         # noqa: E402

EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")


def _run(args, cwd, out):
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([EXE] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))}


@pytest.mark.parametrize("key", ["synA/ld_default", "synA/ld_varsites", "synA/nonld_all_targets_w2", "synB/ld_w37"])
def test_cli_every_route_gives_the_same_bytes(key, tmp_path):
    """One context and --stats-only: the paths and sums are found on the device and only counts and sums leave it.  Two
    contexts, or files per individual: the log tables are gathered and the output job runs the host twin.  Same bytes."""
    args, inp = A.run_args(key)
    c0, c1 = A.golden()["cases"][key]["ranges"]["both"]["range"]
    stats = ["--log-stats", "--states", "--arm-stats", f"{c0},{c1}", "--p01", "0.05", "--p02", "0.01", "--p12", "0.05"]
    full = {d: _run(args + stats + ["--summary-only", "--devices", d], inp, tmp_path / f"full{len(d)}") for d in ("0", "0,0")}
    only = {d: _run(args + stats + ["--stats-only", "--devices", d], inp, tmp_path / f"only{len(d)}") for d in ("0", "0,0")}
    run_files = ["UNKWN.logarmstats.txt", "UNKWN.logibdstates.txt"]
    assert sorted(only["0"]) == sorted(only["0,0"]) == run_files
    assert sorted(full["0"]) == sorted(full["0,0"])
    paths = [fn for fn in full["0"] if fn.endswith(".loghiddengem.txt")]
    assert len(paths) >= 2 and not [fn for fn in full["0"] if fn.endswith((".hiddengem.txt", ".armstats.txt", ".ibdstates.txt"))
                                    and not fn.endswith((".loghiddengem.txt", ".logarmstats.txt", ".logibdstates.txt"))]
    for fn in run_files + paths:
        assert full["0"][fn] == full["0,0"][fn], fn
    for fn in run_files:
        assert only["0"][fn] == full["0"][fn] == only["0,0"][fn], fn
    # the counts of logibdstates.txt are the states of the loghiddengem files
    rows = {l.split("\t")[0]: l.split("\t")[2:5] for l in full["0"]["UNKWN.logibdstates.txt"].decode().splitlines() if not l.startswith("#")}
    for fn in paths:
        st = [l.split("\t")[4] for l in full["0"][fn].decode().splitlines()[1:] if not l.startswith("#")]
        assert rows[fn.split(".")[1]] == [str(st.count(s)) for s in "012"], fn
    # everything else the run writes is what it writes without the option
    plain = _run(args + ["--summary-only"], inp, tmp_path / "plain")
    for fn, data in plain.items():
        assert full["0"][fn] == data, fn


def test_cli_pileup_list_gives_each_entrys_single_run(tmp_path):
    fix_in = os.path.join(REPO, "tests", "golden", "ibdgem-test", "input")
    panel = ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv", "--LD", "-w", "7"]
    stats = ["--log-stats", "--states", "--arm-stats", "300,600", "--stats-only"]
    lst = PL.write_list(tmp_path / "l.txt", [(f"sample{k}", f"test{k}.pileup") for k in (1, 2, 3)])
    got = _run(panel + stats + ["--pileup-list", lst, "--devices", "0,0"], fix_in, tmp_path / "list")
    want = {}
    for k in (1, 2, 3):
        want.update(_run(panel + stats + ["-P", f"test{k}.pileup", "-N", f"sample{k}"], fix_in, tmp_path / f"single{k}"))
    assert sorted(got) == sorted(want) and len(got) == 6
    for fn in want:
        assert got[fn] == want[fn], fn
