"""ibdg_log2_states_host: the integer log-domain IBD-state path on the host, no device.

Bars: (1) path, score and count equal, exactly, a restatement of the definition in Python integers written here;
(2) on tables whose linear columns stay in range and have no near-tie, the path is the one `hiddengem -s` finds from the
linear columns; (3) a window whose linear columns are all 0 poisons the linear path and not this one."""
import math
import os
import subprocess

import numpy as np
import pytest

from ibdgem_amd import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")
HIDDENGEM = os.path.join(HOST, "hiddengem")
HEAD = "# SEGMENT\tSTART\tEND\tLIBD0\tLIBD1\tLIBD2\tNUM_SITES\n"
Q = 65536


@pytest.fixture(scope="module", autouse=True)
def programs():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)


# ---- the definition, restated (Python integers; round() on a float is round-half-even) ---------------------------------

def py_emission(l):
    l = [float(x) for x in l]
    if any(math.isnan(x) for x in l) or not math.isfinite(max(l)):
        return [0, 0, 0]
    m = max(l)
    return [round(max(x - m, -16777216.0) * 65536.0) for x in l]      # (the product is exact: an integer-valued float or a tie)


def py_penalty(p):
    assert 0.0 < p <= 1.0
    return max(round(math.log2(p) * 65536.0), -(1 << 40))


def py_states(tab, p01, p02, p12):
    P01, P02, P12 = py_penalty(p01), py_penalty(p02), py_penalty(p12)
    pen = [[0, P01, P02], [P01, 0, P12], [P02, P12, 0]]
    n = len(tab)
    score, frm = [], []
    for i in range(n):
        e = py_emission(tab[i])
        if i == 0:
            score.append(e)
            frm.append([0, 1, 2])
            continue
        row, f = [], []
        for s in range(3):
            best, arg = None, 0
            for q in range(3):
                c = score[i - 1][q] + pen[q][s]
                if best is None or c > best:
                    best, arg = c, q
            row.append(best + e[s])
            f.append(arg)
        score.append(row)
        frm.append(f)
    path = [0] * n
    if n:
        last = score[-1]
        st = 0
        for s in range(3):
            if last[s] > last[st]:
                st = s
        for i in range(n - 1, -1, -1):
            path[i] = st
            st = frm[i][st]
    return path, score, [path.count(s) for s in range(3)]


def check_equals_restatement(tab, p=(1e-3, 1e-6, 1e-3)):
    tab = np.asarray(tab, dtype=np.float64).reshape(-1, 3)
    path, score, count = E.log2_states_host(tab, *p)
    wp, ws, wc = py_states(tab.tolist(), *p)
    assert path.tolist() == wp
    assert [[int(x) for x in r] for r in score] == ws
    assert [int(x) for x in count] == wc
    # the outputs nobody asked for change nothing
    p2, s2, c2 = E.log2_states_host(tab, *p, want_path=False, want_score=False)
    assert p2 is None and s2 is None and c2.tolist() == count.tolist()
    return path


# ---- (1) twin against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 3, 1000])
def test_sizes(n):
    rng = np.random.default_rng(n)
    tab = rng.normal(-300.0, 40.0, (n, 1)) + rng.normal(0.0, 4.0, (n, 3))
    check_equals_restatement(tab)
    check_equals_restatement(tab, (0.25, 0.01, 0.7))


def test_small_integer_tables_tie_on_most_windows():
    rng = np.random.default_rng(7)
    for n in (2, 3, 17, 400):
        tab = rng.integers(-3, 1, (n, 3)).astype(np.float64)
        path = check_equals_restatement(tab, (0.5, 0.5, 0.5))
        _, score, _ = E.log2_states_host(tab, 0.5, 0.5, 0.5)
        assert (score % Q == 0).all()                                   # log2(0.5) = -1 exactly: whole bits throughout
        if n >= 17:
            # windows at which the maximum over q is reached twice for some state: where "lowest state wins" decides `from`
            pen = np.array([[0, -Q, -Q], [-Q, 0, -Q], [-Q, -Q, 0]])
            cand = score[:-1, :, None] + pen[None]                       # [i-1][q][s]
            ties = int(((cand == cand.max(axis=1, keepdims=True)).sum(axis=1) > 1).any(axis=1).sum())
            assert ties > n // 2, ties
        assert len(path) == n


def test_nan_windows_first_last_and_in_runs():
    rng = np.random.default_rng(3)
    tab = rng.normal(-100.0, 10.0, (60, 3))
    tab[0] = np.nan
    tab[59, 1] = np.nan
    tab[20:31] = np.nan
    tab[40, 0] = np.nan
    check_equals_restatement(tab)
    _, score, _ = E.log2_states_host(tab, 1e-3, 1e-6, 1e-3)
    assert score[0].tolist() == [0, 0, 0]
    check_equals_restatement(np.full((5, 3), np.nan))


def test_infinite_columns_and_the_clamp():
    inf = math.inf
    tab = [[-10.0, -inf, -12.0], [-inf, -inf, -inf], [-5.0, inf, -5.0], [-1e9, -3.0, -2.0], [-16777216.5, -0.5, -1.0],
           [-16777217.0, 0.0, -16777215.99999], [-1.5 / 65536, 0.0, -2.5 / 65536]]
    check_equals_restatement(tab)
    _, score, _ = E.log2_states_host(np.array(tab[:1]), 1.0, 1.0, 1.0)
    assert score[0].tolist() == [0, -(1 << 40), -2 * Q]
    _, score, _ = E.log2_states_host(np.array(tab[3:4]), 1.0, 1.0, 1.0)
    assert score[0].tolist() == [-(1 << 40), -Q, 0]
    _, score, _ = E.log2_states_host(np.array(tab[6:7]), 1.0, 1.0, 1.0)
    assert score[0].tolist() == [-2, 0, -2]                             # ties to even


def test_no_penalty_and_tiny_penalties():
    rng = np.random.default_rng(11)
    tab = rng.normal(-50.0, 5.0, (200, 3))
    path = check_equals_restatement(tab, (1.0, 1.0, 1.0))
    assert path.tolist() == np.argmax(tab, axis=1).tolist()             # (no exact ties in these draws)
    check_equals_restatement(tab, (5e-324, 1e-300, 1.0))


@pytest.mark.parametrize("p", [(0.0, 0.5, 0.5), (0.5, -0.1, 0.5), (0.5, 0.5, 1.0000001), (math.nan, 0.5, 0.5),
                               (0.5, math.inf, 0.5)])
def test_penalties_out_of_range_are_refused(p):
    with pytest.raises(E.EngineError, match=r"is not in \(0, 1\]"):
        E.log2_states_host(np.zeros((4, 3)), *p)


def test_too_many_windows_names_the_bound():
    lib = E.load_library()
    count = np.zeros(3, dtype=np.uint64)
    tab = np.zeros(3)                               # never read: the count of windows is refused first
    assert lib.ibdg_log2_states_host(tab.ctypes.data, (1 << 21) + 1, 0.5, 0.5, 0.5, None, None, count.ctypes.data) != 0
    assert "2^21" in lib.ibdg_last_error(None).decode()
    assert lib.ibdg_log2_states_host(tab.ctypes.data, 1, 0.5, 0.5, 0.5, None, None, None) != 0


# ---- (2), (3) against the linear path of `hiddengem -s` ----------------------------------------------------------------

def hiddengem_rows(tmp_path, lin_text):
    """lin_text: per window the three columns as text.  Returns (states, score columns as text) of `hiddengem -s`."""
    fn = tmp_path / "t.summary.txt"
    fn.write_text(HEAD + "".join(f"{i + 1}\t{100 * i}\t{100 * i + 99}\t{a}\t{b}\t{c}\t100\n" for i, (a, b, c) in enumerate(lin_text)))
    res = subprocess.run([HIDDENGEM, "-s", str(fn)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rows = [l.split("\t") for l in res.stdout.splitlines()[1:] if not l.startswith("#")]
    assert len(rows) == len(lin_text)
    return [int(r[4]) for r in rows], [r[1:4] for r in rows]


def linear_case(rng):
    n = int(rng.integers(1, 400))
    sigma = float(rng.choice([0.5, 3.0, 15.0]))
    lift = float(rng.choice([2.0, 8.0, 30.0]))
    true = np.repeat(rng.integers(0, 3, (n + 19) // 20), 20)[:n]
    l = rng.normal(-200.0, 30.0, (n, 1)) + rng.normal(0.0, sigma, (n, 3))
    l[np.arange(n), true] += lift
    return [tuple("%e" % 2.0 ** x for x in row) for row in l]


def test_the_linear_path_where_it_is_sound(tmp_path):
    """200 cases of seed 1: windows in blocks of 20 of one true state, columns far inside the double range, read back
    from the summary's %e text -- the log path over log2 of those very values is the path `hiddengem -s` prints.
    Equality is a property of these inputs (no window sits on a near-tie of the two arithmetics), not a tolerance."""
    rng = np.random.default_rng(1)
    agree = 0
    for case in range(200):
        text = linear_case(rng)
        want, _ = hiddengem_rows(tmp_path, text)
        tab = np.log2(np.array([[float(x) for x in row] for row in text]))
        path, _, count = E.log2_states_host(tab, 1e-3, 1e-6, 1e-3)
        agree += path.tolist() == want
        assert [int(c) for c in count] == [path.tolist().count(s) for s in range(3)]
    assert agree == 200


def test_a_window_of_zeros_poisons_the_linear_path_only(tmp_path):
    n = 30
    logs = np.full((n, 3), -240.0)
    logs[:, 2] += 20.0                                                  # every window says IBD2 by 20 bits
    text = [tuple("%e" % 2.0 ** x for x in row) for row in logs]
    text[10] = ("0.000000e+00",) * 3                                   # window 11's columns left the double range
    states, scores = hiddengem_rows(tmp_path, text)
    assert states[:9] == [2] * 9 and states[9:] == [0] * 21
    assert all("nan" in s for row in scores[10:] for s in row)
    # what the log table holds for such a window is its true logs, far below 2^-1074 or not
    logs[10] = [-1500.0, -1500.0, -1480.0]
    path, _, count = E.log2_states_host(logs, 1e-3, 1e-6, 1e-3)
    assert path.tolist() == [2] * n and count.tolist() == [0, 0, n]


# ---- the host program without a device: --log-stats on the reference's three-sample fixture (non-LD) -------------------

IBDGEM = os.path.join(HOST, "ibdgem")
FIX_IN = os.path.join(REPO, "tests", "golden", "ibdgem-test", "input")
FIX = ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv", "-P", "test1.pileup", "-N", "sample1"]
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", IBDGEM_KEEP_TEARDOWN="1")


def ibdgem(args, out):
    os.makedirs(out, exist_ok=True)
    return subprocess.run([IBDGEM] + FIX + args + ["-O", str(out)], cwd=FIX_IN, capture_output=True, text=True, env=NO_DEVICE)


def host_log_table(tab_fn, window, eps=0.02, M=20, n_ids=3):
    """The run's log2 window table again, as the program's host path makes it (host_nonld): per row the three fp64 values
    of the library's host twins, per window of `window` rows with reads their log2 summed in long double in row order."""
    lib = E.load_library()
    pdg = np.empty((M + 1, M + 1, 3))
    assert lib.ibdg_pdg_table(eps, M, pdg.ctypes.data) == 0
    wins, acc, k = [], None, 0
    for line in open(tab_fn):
        if line.startswith("#") or not line.strip():
            continue
        c = line.split("\t")
        f = round(float(c[5]) * 2 * n_ids) / (2.0 * n_ids)                 # the panel's own frequency: alt count / 2N
        nr, na, a0, a1 = int(c[7]), int(c[8]), int(c[9]), int(c[10])
        if nr + na == 0:
            continue
        p = [float(x) for x in pdg[nr, na]]
        site = [lib.ibdg_pdg_ibd0(f, *p), lib.ibdg_pdg_ibd1(a0, a1, f, *p), p[a0 + a1]]
        for got, col in zip(site, c[11:14]):
            assert "%e" % got == col.strip(), line                         # (these are the rows the table prints)
        if k % window == 0:
            acc = [np.longdouble(0)] * 3
            wins.append(acc)
        for s in range(3):
            acc[s] = acc[s] + np.log2(np.longdouble(site[s]))
        k += 1
    return np.array([[np.float64(x) for x in w] for w in wins]).reshape(-1, 3)


def log_hiddengem_text(tab, pen):
    path, score, count = E.log2_states_host(tab, *pen)
    out = "Segment\tIBD0_LogScore\tIBD1_LogScore\tIBD2_LogScore\tInferred_State\n"
    for w in range(len(path)):
        out += "%d\t%.4f\t%.4f\t%.4f\t%d\n" % (w + 1, *(int(x) / 65536.0 for x in score[w]), path[w])      # (exact quotients)
    n = len(path)
    for s in range(3):
        out += "#%% IBD%d (n = %d): %.2f\n" % (s, count[s], float(count[s]) / n * 100)
    return out, count


@pytest.mark.parametrize("pen", [(), ("--p01", "0.5", "--p02", "0.25", "--p12", "0.5")])
def test_cli_log_stats_without_a_device(tmp_path, pen):
    W = 7
    res = ibdgem(["-w", str(W), "--log-stats", "--states", "--arm-stats", "300,600", "--log-summary", *pen], tmp_path / "a")
    assert res.returncode == 0, res.stderr
    files = sorted(os.listdir(tmp_path / "a"))
    want = ["sample1.logarmstats.txt", "sample1.logibdstates.txt"]
    for ind in ("sample1", "sample2", "sample3"):
        want += [f"sample1.{ind}.{k}.txt" for k in ("loghiddengem", "logsummary", "summary", "tab")]
    assert files == sorted(want)                                            # and none of the three linear files
    p = tuple(float(x) for x in pen[1::2]) or (1e-3, 1e-6, 1e-3)
    rows, states = [], 0
    for ind in ("sample1", "sample2", "sample3"):
        tab = host_log_table(tmp_path / "a" / f"sample1.{ind}.tab.txt", W)
        logsum = [l.split("\t") for l in open(tmp_path / "a" / f"sample1.{ind}.logsummary.txt") if not l.startswith("#")]
        assert len(logsum) == len(tab) > 10
        assert all("%f" % tab[w, s] == logsum[w][3 + s] for w in range(len(tab)) for s in range(3))
        text, count = log_hiddengem_text(tab, p)
        assert (tmp_path / "a" / f"sample1.{ind}.loghiddengem.txt").read_text() == text, ind
        n = len(tab)
        rows.append("%s\t%d\t%d\t%d\t%d\t%.3f\t%.3f\t%.3f" % (ind, n, *count, *(float(c) / n for c in count)))
        states += len(set(text.split("\n")[k].split("\t")[4] for k in range(1, n + 1)))
    frac = (tmp_path / "a" / "sample1.logibdstates.txt").read_text().splitlines()
    assert frac[1:4] == rows and frac[4].startswith("# Total segments = ")
    arm = (tmp_path / "a" / "sample1.logarmstats.txt").read_text().splitlines()
    assert arm[0].startswith("SAMPLE\tCHROM\t") and [l.split("\t")[0] for l in arm[1:]] == ["sample1", "sample2", "sample3"]
    # --stats-only: the two files of the run alone, the same bytes
    res = ibdgem(["-w", str(W), "--log-stats", "--states", "--arm-stats", "300,600", "--stats-only", *pen], tmp_path / "b")
    assert res.returncode == 0, res.stderr
    assert sorted(os.listdir(tmp_path / "b")) == ["sample1.logarmstats.txt", "sample1.logibdstates.txt"]
    for fn in os.listdir(tmp_path / "b"):
        assert (tmp_path / "b" / fn).read_bytes() == (tmp_path / "a" / fn).read_bytes(), fn
    # the linear statistics of the same run are other files with other numbers
    res = ibdgem(["-w", str(W), "--states", "--arm-stats", "300,600", "--stats-only", *pen], tmp_path / "c")
    assert res.returncode == 0 and sorted(os.listdir(tmp_path / "c")) == ["sample1.armstats.txt", "sample1.ibdstates.txt"]


def test_cli_log_stats_refusals(tmp_path):
    r = ibdgem(["--log-stats"], tmp_path)
    assert r.returncode == 1 and "--log-stats needs --arm-stats START,END and/or --states" in r.stderr
    r = ibdgem(["--log-stats", "--arm-stats", "1,2", "--plan"], tmp_path)
    assert r.returncode == 1 and "--log-stats writes files --plan does not make" in r.stderr
    r = ibdgem(["--log-stats", "--states", "--p01", "1.5"], tmp_path)
    assert r.returncode == 1 and "--p01 of 1.5 is not in (0, 1]" in r.stderr
    r = ibdgem(["--log-stats", "--states", "--p12", "0"], tmp_path)
    assert r.returncode == 1 and "--p12 of 0 is not in (0, 1]" in r.stderr
    assert os.listdir(tmp_path) == []
