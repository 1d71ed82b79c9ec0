"""Two builds of the host program on the whole-panel job, in alternating pairs in one call: the figure of
tools/many_summaries.py (--summary-only: engine + output per individual) and that of tools/arm_stats_cost.py (--arm-stats
--stats-only, per individual), both from the program's phase clocks, on their chr1-scale input (4M rows x 2504, bench.py's
generator, /dev/shm, panel cache), which is built once.  Each binary runs once unrecorded first; the order within a pair
alternates from pair to pair.  Build both binaries with the same command in the same directory: a build by the Makefile
against one by hand in another directory differed by 3 % in phases whose code was the same (profiles/host_conversation.txt).
For refactors of ibdgem.c that must not cost anything; tools/host_ab_compare.py is the companion for behaviour.
    python tools/host_cost_ab.py PARENT_EXE NEW_EXE [pairs, default 3] [individuals, default 240]   (on a GPU box)"""
import os, statistics, subprocess, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import numpy as np, torch
import bench

exes = {"parent": os.path.abspath(sys.argv[1]), "new": os.path.abspath(sys.argv[2])}
pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
n_ind = int(sys.argv[4]) if len(sys.argv) > 4 else 240
rows = 4_000_000
panel, n_ref, n_alt = bench.build_shard(torch, torch.device("cuda", 0), 0, rows, 2504, 7, 20241008)
words = panel.cpu().numpy().view(np.uint64)
del panel
torch.cuda.empty_cache()
LEGS = {"--summary-only": ["--summary-only"], "--arm-stats --stats-only": ["--arm-stats", "18000000,22000000", "--stats-only"]}

with tempfile.TemporaryDirectory(dir="/dev/shm") as d:
    bench.write_pileup_and_legend(d, n_ref, n_alt, 2504, rows)
    open(os.path.join(d, "p.hap"), "w").write("placeholder\n")
    bench.write_panel_cache(os.path.join(d, "p.cache"), words, 2504, os.stat(os.path.join(d, "p.hap")))
    del words
    names = ",".join(f"ind{(7 + 5 * i) % 2504}" for i in range(n_ind))
    base = ["-H", "p.hap", "-L", "p.legend", "-I", "p.indv", "-P", "p.pileup", "-s", names, "--LD", "--threads", "16",
            "--panel-cache", "p.cache", "-O", "o"]

    def one(which, leg):
        os.makedirs(os.path.join(d, "o"))
        t0 = time.perf_counter()
        r = subprocess.run([exes[which]] + base + LEGS[leg], cwd=d, env=dict(os.environ, IBDGEM_TIMING="1"), capture_output=True,
                           text=True, timeout=300)
        wall = time.perf_counter() - t0
        subprocess.run(["rm", "-rf", os.path.join(d, "o")], check=True)
        if r.returncode != 0:
            print(r.stderr[-800:])
            sys.exit(1)
        own = sum(float(l.rsplit(" ", 1)[1]) for l in r.stderr.splitlines()
                  if l.startswith(("## time per individual", "## time output files of the last")))
        return own / n_ind * 1e3, wall

    for leg in LEGS:
        for which in exes:
            one(which, leg)
        print(f"{n_ind} individuals, --LD {leg}: ms per individual from the phase clocks (wall clock of the process, s)", flush=True)
        res = {"parent": [], "new": []}
        for k in range(pairs):
            for which in (("parent", "new") if k % 2 == 0 else ("new", "parent")):
                ms, wall = one(which, leg)
                res[which].append(ms)
                print(f"  pair {k + 1} {which:6s} {ms:.3f} ({wall:.2f})", flush=True)
        for which, v in res.items():
            print(f"  {which:6s} min {min(v):.3f} median {statistics.median(v):.3f} max {max(v):.3f}", flush=True)
