"""The host program's --chain-gap without a device: a non-LD run with -w 5 over an input the test writes itself
-- 60 sites 100 bp apart but for a gap of 50 000 on a window border and one of 1 000 000 inside a window (the reference's
fixture has a site every 100 bp and no gap at all).  The starts are derived from the START / END columns of logsummary.txt,
every log file is what the _chains_host twins give for them, and a gap no window reaches changes nothing but the Chain column."""
import os
import subprocess

import numpy as np
import pytest

import segments_check as S
from ibdgem_amd import engine as E
from test_log_states_host import host_log_table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "ibdgem_amd", "host")
IBDGEM = os.path.join(HOST, "ibdgem")
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", IBDGEM_KEEP_TEARDOWN="1")
INDS = ("indA", "indB", "indC")
W, N_SITES = 5, 60
BORDER, INNER = 25, 42                   # site 25 opens window 5: the gap in front of it lies on a border; 42 -> 43 is inside window 8
PEN = (1e-3, 1e-6, 1e-3)
LOGS = ["--log-summary", "--log-stats", "--states", "--posteriors", "--segments"]


@pytest.fixture(scope="module", autouse=True)
def programs():
    subprocess.run(["make", "-C", os.path.join(REPO, "ibdgem_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)


def site_positions():
    pos, p = [], 0
    for i in range(N_SITES):
        p += 50000 if i == BORDER else 1000000 if i == INNER + 1 else 100
        pos.append(p)
    return pos


def write_input(d):
    """A panel of three individuals (IMPUTE files) polymorphic at every site, and a pileup with reads at every site."""
    rng = np.random.default_rng(5)
    os.makedirs(d, exist_ok=True)
    pos = site_positions()
    with open(d / "p.legend", "w") as leg, open(d / "p.hap", "w") as hap, open(d / "p.pileup", "w") as pu:
        leg.write("ID pos allele0 allele1\n")
        for i, p in enumerate(pos):
            leg.write(f"SNP{i + 1} {p} A C\n")
            h = rng.integers(0, 2, 6)
            if h.sum() in (0, 6):
                h[i % 6] ^= 1
            hap.write(" ".join(str(x) for x in h) + "\n")
            depth = int(rng.integers(2, 7))
            bases = "".join(rng.choice(list("AaCc"), depth))
            pu.write(f"1\t{p}\tN\t{depth}\t{bases}\t{'I' * depth}\t{']' * depth}\n")
    (d / "p.indv").write_text("".join(ind + "\n" for ind in INDS))
    return ["-H", "p.hap", "-L", "p.legend", "-I", "p.indv", "-P", "p.pileup", "-N", "pu"]


def ibdgem(args, out, inp):
    os.makedirs(out, exist_ok=True)
    return subprocess.run([IBDGEM] + write_input(inp) + ["-w", str(W)] + args + ["-O", str(out)], cwd=inp, capture_output=True,
                          text=True, env=NO_DEVICE)


def files(d):
    out = {fn: (d / fn).read_bytes() for fn in sorted(os.listdir(d))}
    for fn in out:
        if fn.endswith(".tab.txt"):
            out[fn] = out[fn].split(b"\n", 1)[1]                          # (its first line repeats the command)
    return out


def windows_of(logsummary):
    rows = [l.split("\t") for l in logsummary.decode().splitlines() if not l.startswith("#")]
    return np.array([int(r[1]) for r in rows], dtype=np.uint64), np.array([int(r[2]) for r in rows], dtype=np.uint64)


def starts_from(first, last, gap):
    """The option's rule, restated: window w >= 1 starts a chain iff START[w] - END[w - 1] > gap."""
    return [w for w in range(1, len(first)) if int(first[w]) - int(last[w - 1]) > gap]


def test_chain_gap_files_are_the_chained_twins(tmp_path):
    res = ibdgem(LOGS + ["--chain-gap", "10000"], tmp_path / "a", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    res = ibdgem(LOGS, tmp_path / "plain", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    plain = files(tmp_path / "plain")
    assert sorted(got) == sorted(plain)
    changed, lines, rows_states, rows_post = set(), {}, [], []
    total_e = np.zeros(3)
    for ind in INDS:
        first, last = windows_of(got[f"pu.{ind}.logsummary.txt"])
        n = len(first)
        assert n == N_SITES // W
        starts = starts_from(first, last, 10000)
        assert starts == [BORDER // W]                                    # the border gap alone: the inner one starts nothing
        assert int(last[INNER // W]) - int(first[INNER // W]) > 1000000   # ... though the window holds it
        tab = host_log_table(tmp_path / "a" / f"pu.{ind}.tab.txt", W)
        assert len(tab) == n
        # loghiddengem.txt
        path, score, count = E.log2_states_host(tab, *PEN, starts=starts)
        text = "Segment\tIBD0_LogScore\tIBD1_LogScore\tIBD2_LogScore\tInferred_State\n"
        for w in range(n):
            text += "%d\t%.4f\t%.4f\t%.4f\t%d\n" % (w + 1, *(int(x) / 65536.0 for x in score[w]), path[w])
        for s in range(3):
            text += "#%% IBD%d (n = %d): %.2f\n" % (s, count[s], float(count[s]) / n * 100)
        assert got[f"pu.{ind}.loghiddengem.txt"].decode() == text, ind
        rows_states.append("%s\t%d\t%d\t%d\t%d\t%.3f\t%.3f\t%.3f" % (ind, n, *count, *(float(c) / n for c in count)))
        # logposteriors.txt
        post, expect, log2_z = E.log2_posteriors_host(tab, *PEN, starts=starts)
        text = "Segment\tPost_IBD0\tPost_IBD1\tPost_IBD2\tMax_State\n"
        for w in range(n):
            text += "%d\t%.6f\t%.6f\t%.6f\t%d\n" % (w + 1, *post[w], int(np.argmax(post[w])))
        assert got[f"pu.{ind}.logposteriors.txt"].decode() == text, ind
        rows_post.append([ind, str(n)] + ["%.3f" % e for e in expect] + ["%.6f" % (e / n) for e in expect] + ["%.6f" % log2_z])
        total_e += expect
        # logsegments.txt: the Chain column, then the file of --segments
        seg, n_seg, summary = E.log2_segments_host(tab, *PEN, with_post=True, pos_first=first, pos_last=last, starts=starts)
        head, rows = S.rows_of(got[f"pu.{ind}.logsegments.txt"])
        assert head == "Chain\t" + S.HEADER + S.POST and len(rows) == n_seg
        assert [int(r[0]) for r in rows] == [1 + sum(w <= int(f) for w in starts) for f in seg["first"]]
        assert {r[0] for r in rows} == {"1", "2"}
        for row, r in zip(rows, seg):
            row = row[1:]
            e, s, f, l = [int(x) for x in r["e"]], int(r["state"]), int(r["first"]), int(r["first"] + r["n_win"]) - 1
            lr = e[s] - max(e[(s + 1) % 3], e[(s + 2) % 3])
            assert [int(x) for x in row[1:8]] == [s, f + 1, l + 1, first[f], last[l], int(last[l]) - int(first[f]) + 1, l - f + 1]
            assert row[9:13] == ["%.4f" % (np.longdouble(x) / 65536) for x in e + [lr]]
            assert row[13] == "%.6f" % (np.longdouble(int(r["post_q"])) / (np.longdouble(int(r["n_win"])) * 2 ** 32))
            assert row[14] == "%.6f" % float(r["post_min"])
            assert not f < starts[0] <= l                                 # no segment, hence no base pair, crosses the gap
        lines[ind] = [int(x) for x in summary]
        for fn in ("loghiddengem", "logposteriors", "logsegments"):
            changed.add(f"pu.{ind}.{fn}.txt")
    S.run_consistent(got["pu.logibdsegments.txt"], lines)
    states = got["pu.logibdstates.txt"].decode().splitlines()
    assert states[1:4] == rows_states
    summ = [l.split("\t") for l in got["pu.logibdposteriors.txt"].decode().splitlines()]
    assert summ[1:4] == rows_post
    # what does not depend on the chains is the run's without the option, byte for byte
    for fn, data in plain.items():
        if fn not in changed and not fn.startswith("pu.logibd"):
            assert got[fn] == data, fn
    # --stats-only: the run's files alone, the same bytes
    res = ibdgem([a for a in LOGS if a != "--log-summary"] + ["--chain-gap", "10000", "--stats-only"], tmp_path / "b", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    only = files(tmp_path / "b")
    assert sorted(only) == ["pu.logibdposteriors.txt", "pu.logibdsegments.txt", "pu.logibdstates.txt"]
    for fn, data in only.items():
        assert got[fn] == data, fn


def test_a_gap_no_window_reaches_changes_the_chain_column_alone(tmp_path):
    res = ibdgem(LOGS + ["--chain-gap", "10000000"], tmp_path / "a", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    got = files(tmp_path / "a")
    res = ibdgem(LOGS, tmp_path / "plain", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    plain = files(tmp_path / "plain")
    assert sorted(got) == sorted(plain)
    for fn, data in plain.items():
        if fn.endswith(".logsegments.txt"):
            assert got[fn].decode().splitlines() == [("Chain\t" if k == 0 else "1\t") + l for k, l in enumerate(data.decode().splitlines())], fn
        else:
            assert got[fn] == data, fn
    # ... and the chained run does differ from it somewhere (the option is not ignored)
    res = ibdgem(LOGS + ["--chain-gap", "10000"], tmp_path / "c", tmp_path / "in")
    assert res.returncode == 0, res.stderr
    assert any(files(tmp_path / "c")[f"pu.{ind}.logposteriors.txt"] != plain[f"pu.{ind}.logposteriors.txt"] for ind in INDS)


def test_chain_gap_refusals(tmp_path):
    inp = tmp_path / "in"
    out = tmp_path / "out"
    r = ibdgem(["--chain-gap", "1000", "--states"], out, inp)
    assert r.returncode == 1 and "--chain-gap needs --log-stats and --states" in r.stderr
    r = ibdgem(["--chain-gap", "1000", "--log-stats", "--arm-stats", "300,600"], out, inp)
    assert r.returncode == 1 and "--chain-gap needs --log-stats and --states" in r.stderr
    r = ibdgem(["--chain-gap", "1000", "--log-stats", "--states", "--plan"], out, inp)
    assert r.returncode == 1 and "--plan does not make" in r.stderr
    for bad in ("0", "-5", "1.5", "1e4", "abc", "", "12x", "99999999999999999999999"):
        r = ibdgem(["--log-stats", "--states", "--chain-gap", bad], out, inp)
        assert r.returncode == 1 and f"Invalid chain gap (--chain-gap) '{bad}' (must be an integer >= 1" in r.stderr, bad
    assert os.listdir(out) == []


def test_usage_names_the_option():
    r = subprocess.run([IBDGEM, "--help"], capture_output=True, text=True, env=NO_DEVICE)
    assert "--chain-gap BP" in r.stdout + r.stderr
