"""The host program's --switch-scale and --genetic-map without a device, on the input of
tests/test_chain_gap_cli.py (60 sites 100 bp apart but for two gaps, -w 5).  The test forms the shifts itself from the START and
END columns of logsummary.txt with math.log2, and every log file is what the _steps_host twins give for them through engine.py."""
import bisect
import math
import os
import subprocess

import numpy as np
import pytest

import hp_post_ref as H
import segments_check as S
from ibdgem_amd import engine as E
from test_chain_gap_cli import BORDER, HOST, IBDGEM, INDS, LOGS, NO_DEVICE, PEN, REPO, W, N_SITES, files, ibdgem, starts_from, windows_of
from test_log_states_host import host_log_table

BIG = 1 << 30
# position, rate (not read), cumulative cM: the centre of window 0 (300) lies before the map, that of window 1 (800) on its first
# entry, those of windows 2 .. 4 inside it, that of window 5 (52 700) on its last entry, the rest behind it
MAP = [(800, 1.0, 0.0), (1000, 2.5, 0.0005), (2050.5, 0.1, 0.003), (30000, 1.0, 0.0031), (52700, 0.0, 0.9)]


@pytest.fixture(scope="module", autouse=True)
def programs():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)


def write_map(path, entries=MAP, header="position COMBINED_rate(cM/Mb) Genetic_Map(cM)\n"):
    path.write_text(header + "".join(f"{p!r}\t{r!r} {c!r}\n" for p, r, c in entries))
    return str(path)


def g_of(x, entries=MAP):
    """The option's rule, restated: linear between the entry at or below x and the next, the map's mean rate outside it."""
    p, c = [float(e[0]) for e in entries], [float(e[2]) for e in entries]
    mean = (c[-1] - c[0]) / (p[-1] - p[0])
    if x < p[0]:
        return c[0] + (x - p[0]) * mean
    if x >= p[-1]:
        return c[-1] + (x - p[-1]) * mean
    i = bisect.bisect_right(p, x) - 1
    return c[i] + (x - p[i]) * ((c[i + 1] - c[i]) / (p[i + 1] - p[i]))


def shifts_from(first, last, X, entries=None):
    """shift[w] = round(log2(D_w / X) * 65536) within +-2^30, -2^30 where D_w <= 0; D_w: the distance of the windows' centres."""
    out = [0]
    for w in range(1, len(first)):
        a, b = int(first[w]) + int(last[w]), int(first[w - 1]) + int(last[w - 1])
        D = (a - b) * 0.5 if entries is None else g_of(a * 0.5, entries) - g_of(b * 0.5, entries)
        out.append(max(-BIG, min(BIG, round(math.log2(D / X) * 65536.0))) if D > 0 else -BIG)
    return np.array(out, dtype=np.int32)


def files_are_the_twins(got, plain, out_dir, shifts_of, gap=None):
    """Every log file of `got` against the twins with shifts_of(first, last) (and the starts of `gap`); returns the shifts."""
    assert sorted(got) == sorted(plain)
    changed, lines, rows_states, rows_post, all_shifts = set(), {}, [], [], {}
    for ind in INDS:
        first, last = windows_of(got[f"pu.{ind}.logsummary.txt"])
        n = len(first)
        assert n == N_SITES // W
        shift = all_shifts[ind] = shifts_of(first, last)
        starts = starts_from(first, last, gap) if gap else []
        kw = dict(shift=shift, starts=starts) if gap else dict(shift=shift)
        tab = host_log_table(out_dir / f"pu.{ind}.tab.txt", W)
        path, score, count = E.log2_states_host(tab, *PEN, **kw)
        text = "Segment\tIBD0_LogScore\tIBD1_LogScore\tIBD2_LogScore\tInferred_State\n"
        for w in range(n):
            text += "%d\t%.4f\t%.4f\t%.4f\t%d\n" % (w + 1, *(int(x) / 65536.0 for x in score[w]), path[w])
        for s in range(3):
            text += "#%% IBD%d (n = %d): %.2f\n" % (s, count[s], float(count[s]) / n * 100)
        assert got[f"pu.{ind}.loghiddengem.txt"].decode() == text, ind
        rows_states.append("%s\t%d\t%d\t%d\t%d\t%.3f\t%.3f\t%.3f" % (ind, n, *count, *(float(c) / n for c in count)))
        post, expect, log2_z = E.log2_posteriors_host(tab, *PEN, **kw)
        text = "Segment\tPost_IBD0\tPost_IBD1\tPost_IBD2\tMax_State\n"
        for w in range(n):
            text += "%d\t%.6f\t%.6f\t%.6f\t%d\n" % (w + 1, *post[w], int(np.argmax(post[w])))
        assert got[f"pu.{ind}.logposteriors.txt"].decode() == text, ind
        rows_post.append([ind, str(n)] + ["%.3f" % e for e in expect] + ["%.6f" % (e / n) for e in expect] + ["%.6f" % log2_z])
        seg, n_seg, summary = E.log2_segments_host(tab, *PEN, with_post=True, pos_first=first, pos_last=last, **kw)
        head, rows = S.rows_of(got[f"pu.{ind}.logsegments.txt"])
        assert head == ("Chain\t" if gap else "") + S.HEADER + S.POST and len(rows) == n_seg       # no file changes its format
        for row, r in zip(rows, seg):
            row = row[1:] if gap else row
            e, s, f, l = [int(x) for x in r["e"]], int(r["state"]), int(r["first"]), int(r["first"] + r["n_win"]) - 1
            lr = e[s] - max(e[(s + 1) % 3], e[(s + 2) % 3])
            assert [int(x) for x in row[1:8]] == [s, f + 1, l + 1, first[f], last[l], int(last[l]) - int(first[f]) + 1, l - f + 1]
            assert row[9:13] == ["%.4f" % (np.longdouble(x) / 65536) for x in e + [lr]]
            assert row[13] == "%.6f" % (np.longdouble(int(r["post_q"])) / (np.longdouble(int(r["n_win"])) * 2 ** 32))
            assert row[14] == "%.6f" % float(r["post_min"])
        lines[ind] = [int(x) for x in summary]
        for fn in ("loghiddengem", "logposteriors", "logsegments"):
            changed.add(f"pu.{ind}.{fn}.txt")
    S.run_consistent(got["pu.logibdsegments.txt"], lines)
    assert got["pu.logibdstates.txt"].decode().splitlines()[1:4] == rows_states
    assert [l.split("\t") for l in got["pu.logibdposteriors.txt"].decode().splitlines()][1:4] == rows_post
    # what does not depend on the steps is the run's without the option, byte for byte
    for fn, data in plain.items():
        if fn not in changed and not fn.startswith("pu.logibd"):
            assert got[fn] == data, fn
    return all_shifts


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    res = ibdgem(LOGS, d / "out", d / "in")
    assert res.returncode == 0, res.stderr
    return files(d / "out")


def test_switch_scale_files_are_the_twins_with_the_shifts(tmp_path, plain):
    X = 650.0
    res = ibdgem(LOGS + ["--switch-scale", "650"], tmp_path / "a", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    shifts = files_are_the_twins(got, plain, tmp_path / "a", lambda f, l: shifts_from(f, l, X))
    sh = shifts[INDS[0]]
    assert sh[1] == round(math.log2(500.0 / 650.0) * 65536) < 0 < sh[BORDER // W] < BIG       # close windows cost more, the gaps less
    assert any(got[f"pu.{ind}.logposteriors.txt"] != plain[f"pu.{ind}.logposteriors.txt"] for ind in INDS)
    # --stats-only: the run's files alone, the same bytes
    res = ibdgem([a for a in LOGS if a != "--log-summary"] + ["--switch-scale", "650", "--stats-only"], tmp_path / "b", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    only = files(tmp_path / "b")
    assert sorted(only) == ["pu.logibdposteriors.txt", "pu.logibdsegments.txt", "pu.logibdstates.txt"]
    for fn, data in only.items():
        assert got[fn] == data, fn


def test_genetic_map_measures_the_distances(tmp_path, plain):
    X = 0.002
    fn = write_map(tmp_path / "map.txt")
    res = ibdgem(LOGS + ["--switch-scale", "0.002", "--genetic-map", fn], tmp_path / "a", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    first, last = windows_of(got[f"pu.{INDS[0]}.logsummary.txt"])
    centres = [(int(a) + int(b)) * 0.5 for a, b in zip(first, last)]
    assert centres[0] < MAP[0][0] == centres[1] and centres[5] == MAP[-1][0] < centres[6]      # before, on, inside, on, behind
    assert all(MAP[0][0] < c < MAP[-1][0] for c in centres[2:5])
    shifts = files_are_the_twins(got, plain, tmp_path / "a", lambda f, l: shifts_from(f, l, X, MAP))
    assert len(set(shifts[INDS[0]].tolist()[1:])) > 4
    res = ibdgem(LOGS + ["--switch-scale", "0.002"], tmp_path / "b", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    assert any(files(tmp_path / "b")[f"pu.{ind}.logposteriors.txt"] != got[f"pu.{ind}.logposteriors.txt"] for ind in INDS)


def test_switch_scale_with_chain_gap(tmp_path, plain):
    res = ibdgem(LOGS + ["--switch-scale", "2000.5", "--chain-gap", "10000"], tmp_path / "a", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    files_are_the_twins(got, plain, tmp_path / "a", lambda f, l: shifts_from(f, l, 2000.5), gap=10000)
    for ind in INDS:                                                      # the chain start is there, and begins a segment
        _, rows = S.rows_of(got[f"pu.{ind}.logsegments.txt"])
        assert {r[0] for r in rows} == {"1", "2"} and str(BORDER // W + 1) in {r[3] for r in rows}


def test_a_very_small_scale_makes_every_switch_free(tmp_path, plain):
    res = ibdgem(LOGS + ["--switch-scale", "1e-9"], tmp_path / "a", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    for ind in INDS:
        tab = host_log_table(tmp_path / "a" / f"pu.{ind}.tab.txt", W)
        path = [int(l.split("\t")[4]) for l in got[f"pu.{ind}.loghiddengem.txt"].decode().splitlines()[1:] if not l.startswith("#")]
        best = []
        for row in tab:
            e = H.emission(row)
            best.append(e.index(max(e)))                                  # (the lowest state of a tie)
        assert path == best, ind
    assert any(got[f"pu.{ind}.loghiddengem.txt"] != plain[f"pu.{ind}.loghiddengem.txt"] for ind in INDS)


def test_refusals(tmp_path):
    inp, out = tmp_path / "in", tmp_path / "out"
    fn = write_map(tmp_path / "map.txt")
    for opt, name in ((["--switch-scale", "1000"], "--switch-scale"), (["--switch-scale", "1000", "--genetic-map", fn], "--switch-scale")):
        r = ibdgem(opt + ["--states"], out, inp)
        assert r.returncode == 1 and f"{name} needs --log-stats and --states" in r.stderr
        r = ibdgem(opt + ["--log-stats", "--arm-stats", "300,600"], out, inp)
        assert r.returncode == 1 and f"{name} needs --log-stats and --states" in r.stderr
        r = ibdgem(opt + ["--log-stats", "--states", "--plan"], out, inp)
        assert r.returncode == 1 and "--plan does not make" in r.stderr     # (--states' own line comes first, as for --chain-gap)
    r = ibdgem(["--genetic-map", fn, "--log-stats", "--states"], out, inp)
    assert r.returncode == 1 and "--genetic-map needs --switch-scale X" in r.stderr
    r = ibdgem(["--genetic-map", fn, "--states"], out, inp)
    assert r.returncode == 1 and "--genetic-map needs --log-stats and --states" in r.stderr
    r = ibdgem(["--genetic-map", fn, "--log-stats", "--states", "--plan"], out, inp)
    assert r.returncode == 1 and "--plan does not make" in r.stderr
    for bad in ("0", "-5", "abc", "", "12x", "nan", "inf", "1e999", "0.0"):
        r = ibdgem(["--log-stats", "--states", "--switch-scale", bad], out, inp)
        assert r.returncode == 1 and f"Invalid switch scale (--switch-scale) '{bad}' (must be a decimal > 0" in r.stderr, bad
    assert os.listdir(out) == []


@pytest.mark.parametrize("body,msg", [
    ("800 1 0\n700 1 0.5\n", "line 3: position 700 does not lie above the 800 of the entry before it (strictly increasing)"),
    ("800 1 0\n900 1 0.5\n900 1 0.6\n", "line 4: position 900 does not lie above the 900"),
    ("800 1 0\n900 0.5\n", "line 3: not three numbers"),
    ("800 1 0\n900 1 x\n", "line 3: not three numbers"),
    ("800 1 0\n900 1 0.5 7\n", "line 3: not three numbers"),
    ("800 1 0\n900 1 nan\n", "line 3: not three numbers"),
    ("800 1 0\n", "has 1 entries; two make a rate"),
    ("", "has 0 entries; two make a rate"),
])
def test_a_malformed_map_is_refused(tmp_path, body, msg):
    fn = tmp_path / "bad.txt"
    fn.write_text("pos rate cM\n" + body)
    r = ibdgem(["--log-stats", "--states", "--switch-scale", "1", "--genetic-map", str(fn)], tmp_path / "out", tmp_path / "in")
    assert r.returncode == 1 and "genetic map (--genetic-map)" in r.stderr and msg in r.stderr, r.stderr
    assert os.listdir(tmp_path / "out") == []


def test_an_empty_or_missing_map_is_refused(tmp_path):
    (tmp_path / "empty.txt").write_text("")
    r = ibdgem(["--log-stats", "--states", "--switch-scale", "1", "--genetic-map", str(tmp_path / "empty.txt")], tmp_path / "out", tmp_path / "in")
    assert r.returncode == 1 and "is empty" in r.stderr
    r = ibdgem(["--log-stats", "--states", "--switch-scale", "1", "--genetic-map", str(tmp_path / "none.txt")], tmp_path / "out", tmp_path / "in")
    assert r.returncode == 1 and "cannot open the genetic map (--genetic-map)" in r.stderr


def test_usage_names_the_options():
    r = subprocess.run([IBDGEM, "--help"], capture_output=True, text=True, env=NO_DEVICE)
    assert "--switch-scale X" in r.stdout + r.stderr and "--genetic-map FILE" in r.stdout + r.stderr
