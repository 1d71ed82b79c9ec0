"""--pileup-list against one process per pileup, on chr1-scale input (4M rows x 2504, bench.py's panel generator, the panel
cache in /dev/shm): P synthetic pileups of Poisson(2) depth with distinct seeds, for P in 1, 8, 32, timed as
  - one run with --pileup-list, and
  - P separate warm runs with --panel-cache (the page cache already holds the cache file),
for three jobs: T = 1 and T = 60 comparison individuals with --summary-only, and the whole panel with
--stats-only --arm-stats.  Wall clock of each, and per pileup.  Then, at the largest P: each job's list run again with
IBDGEM_TIMING=1, its phases averaged per pileup (which phase a pileup's share of the run goes to: reading and filtering
run beside the device work of the pileup before), and the list run with three contexts on the one GPU
(--devices 0,0,0).  With --parent EXE, the single -P run of the T = 1 job is
also timed with another build of the program (best of five each, alternating), to show the single run did not slow down.
    python tools/pileup_list_cost.py [--pileups 1,8,32] [--distinct 32] [--parent EXE]   (on a GPU box)
--distinct K: K distinct pileups are written; a list of P > K entries names them in turn under P names."""
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import bench


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


P_LIST = [int(x) for x in arg("--pileups", "1,8,32").split(",")]
DISTINCT = int(arg("--distinct", "32"))
PARENT = arg("--parent", None)
ROWS, N_IDS = 4_000_000, 2504
CENTROMERE = "18000000,22000000"
exe = os.path.join(bench.REPO, "ibdgem_amd", "host", "ibdgem")

dev = torch.device("cuda", 0)
panel, n_ref0, n_alt0 = bench.build_shard(torch, dev, 0, ROWS, N_IDS, 7, 20241008)
words = panel.cpu().numpy().view(np.uint64)
del panel
torch.cuda.empty_cache()
freq = np.bitwise_count(words).sum(axis=1, dtype=np.uint32) / (2.0 * N_IDS)

TAILS = {}
for r in range(21):
    for a in range(21 - r):
        c = r + a
        TAILS[r * 32 + a] = "N\t0\t*\t*\t*\n" if c == 0 else f"N\t{c}\t{'A' * r}{'C' * a}\t{'I' * c}\t{'I' * c}\n"


def write_pileup(fn, seed):
    rng = np.random.default_rng(seed)
    cov = np.minimum(rng.poisson(2.0, size=ROWS), 20)
    n_alt = rng.binomial(cov, freq)
    key = ((cov - n_alt) * 32 + n_alt).tolist()
    with open(fn, "w") as fh:
        for a in range(0, ROWS, 500_000):
            fh.write("".join([f"1\t{100 + 10 * i}\t{TAILS[key[i]]}" for i in range(a, min(ROWS, a + 500_000))]))


def timed(cmd, cwd, env=None, want_stderr=False):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **env) if env else None)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        print(" ".join(cmd[:12]), "...\n", r.stderr[-1500:], flush=True)
        sys.exit(1)
    return (wall, r.stderr) if want_stderr else wall


def per_pileup_phases(stderr, P):
    """'## time [NAME] phase s' lines: seconds per phase, summed over the pileups and divided by P"""
    ph = {}
    for l in stderr.splitlines():
        if l.startswith("## time [") and "] " in l:
            k, v = l[l.index("] ") + 2:].rsplit(" ", 1)
            ph[k] = ph.get(k, 0.0) + float(v) / P
    return sorted(ph.items(), key=lambda kv: -kv[1])


with tempfile.TemporaryDirectory(dir="/dev/shm") as d:
    bench.write_pileup_and_legend(d, n_ref0, n_alt0, N_IDS, ROWS)          # legend, indv (and a p.pileup not used here)
    open(os.path.join(d, "p.hap"), "w").write("placeholder\n")
    bench.write_panel_cache(os.path.join(d, "p.cache"), words, N_IDS, os.stat(os.path.join(d, "p.hap")))
    del words
    t0 = time.perf_counter()
    pileups = []
    for k in range(min(DISTINCT, max(P_LIST))):
        fn = f"s{k}.pileup"
        write_pileup(os.path.join(d, fn), 1000 + k)
        pileups.append(fn)
    print(f"{len(pileups)} distinct pileups of {ROWS} lines written in {time.perf_counter() - t0:.1f} s", flush=True)
    base = [exe, "-H", "p.hap", "-L", "p.legend", "-I", "p.indv", "--LD", "--threads", "16", "--panel-cache", "p.cache"]
    jobs = {"T=1 --summary-only": ["-s", "ind7", "--summary-only"],
            "T=60 --summary-only": ["-s", ",".join(f"ind{(7 + 41 * i) % N_IDS}" for i in range(60)), "--summary-only"],
            "whole panel --stats-only --arm-stats": ["--stats-only", "--arm-stats", CENTROMERE]}
    os.makedirs(os.path.join(d, "warm"))
    timed(base + jobs["T=1 --summary-only"] + ["-P", pileups[0], "-O", os.path.join(d, "warm")], d)   # warms the page cache
    print(f"{'job':40s} {'P':>3s} {'list run s':>11s} {'per pileup':>11s} {'P single runs s':>16s} {'per pileup':>11s}",
          flush=True)
    for job, extra in jobs.items():
        for P in P_LIST:
            names = [(f"s{k}", pileups[k % len(pileups)]) for k in range(P)]
            lst = os.path.join(d, f"list{P}.txt")
            with open(lst, "w") as fh:
                fh.writelines(f"{n}\t{p}\n" for n, p in names)
            out_l = tempfile.mkdtemp(dir=d)
            wl = timed(base + extra + ["--pileup-list", lst, "-O", out_l], d)
            out_s = tempfile.mkdtemp(dir=d)
            ws = sum(timed(base + extra + ["-P", p, "-N", n, "-O", out_s], d) for n, p in names)
            same = all(open(os.path.join(out_l, f), "rb").read() == open(os.path.join(out_s, f), "rb").read()
                       for f in os.listdir(out_s)) and sorted(os.listdir(out_l)) == sorted(os.listdir(out_s))
            print(f"{job:40s} {P:3d} {wl:11.3f} {wl / P:11.3f} {ws:16.3f} {ws / P:11.3f}   files identical: {same}",
                  flush=True)
            subprocess.run(["rm", "-rf", out_l, out_s])
    P = max(P_LIST)
    names = [(f"s{k}", pileups[k % len(pileups)]) for k in range(P)]
    lst = os.path.join(d, "list_max.txt")
    with open(lst, "w") as fh:
        fh.writelines(f"{n}\t{p}\n" for n, p in names)
    for job, extra in jobs.items():
        out_l = tempfile.mkdtemp(dir=d)
        wl, err = timed(base + extra + ["--pileup-list", lst, "-O", out_l], d, env={"IBDGEM_TIMING": "1"}, want_stderr=True)
        print(f"{job}, P = {P}, IBDGEM_TIMING=1: wall {wl:.3f} s, {wl / P:.3f} s per pileup; phases per pileup (s):", flush=True)
        for k, v in per_pileup_phases(err, P)[:8]:
            print(f"    {v:8.4f}  {k[:100]}", flush=True)
        out_3 = tempfile.mkdtemp(dir=d)
        w3 = timed(base + extra + ["--pileup-list", lst, "--devices", "0,0,0", "-O", out_3], d)
        same = sorted(os.listdir(out_l)) == sorted(os.listdir(out_3)) and all(
            open(os.path.join(out_l, f), "rb").read() == open(os.path.join(out_3, f), "rb").read() for f in os.listdir(out_l))
        print(f"{job}, P = {P}, --devices 0,0,0 (three contexts, one GPU): wall {w3:.3f} s, {w3 / P:.3f} s per pileup, "
              f"files identical to one context: {same}", flush=True)
        subprocess.run(["rm", "-rf", out_l, out_3])
    if PARENT:
        cmd_of = {"this build": exe, "parent build": os.path.abspath(PARENT)}
        times = {k: [] for k in cmd_of}
        out = tempfile.mkdtemp(dir=d)
        for rep in range(5):
            for k, e in cmd_of.items():
                times[k].append(timed([e] + base[1:] + jobs["T=1 --summary-only"] + ["-P", pileups[0], "-N", "s0", "-O", out], d))
        for k, v in times.items():
            print(f"single -P run, T=1 --summary-only, {k}: best {min(v):.3f} s, median {sorted(v)[2]:.3f} s "
                  f"({' '.join(f'{x:.3f}' for x in v)})", flush=True)
