"""The whole-panel job with --arm-stats: --summary-only (every window table copied back and written as text) against
--arm-stats ... --stats-only (the arm sums taken on the device, one small file), on chr1-scale input (4M rows x 2504,
bench.py's generator) in /dev/shm with a panel cache, 240 individuals: wall clock and IBDGEM_TIMING=1 phases of each,
best of two.  With --rocprof DIR, one more --stats-only run under `rocprofv3 --kernel-trace --stats` (no counters)
writes its kernel statistics to DIR.
    python tools/arm_stats_cost.py [individuals] [--rocprof DIR]   (on a GPU box)"""
import os, sys, tempfile, subprocess, time, glob
sys.path.insert(0, os.getcwd())
import numpy as np, torch
import bench

args = [a for a in sys.argv[1:] if not a.startswith("--")]
prof_dir = sys.argv[sys.argv.index("--rocprof") + 1] if "--rocprof" in sys.argv else None
if prof_dir:
    args = [a for a in args if a != prof_dir]
    prof_dir = os.path.abspath(prof_dir)          # (the runs go in a scratch directory)
n_ind = int(args[0]) if args else 240
rows = 4_000_000
dev = torch.device("cuda", 0)
panel, n_ref, n_alt = bench.build_shard(torch, dev, 0, rows, 2504, 7, 20241008)
words = panel.cpu().numpy().view(np.uint64)
del panel
torch.cuda.empty_cache()
exe = os.path.join(bench.REPO, "ibdgem_amd", "host", "ibdgem")
CENTROMERE = "18000000,22000000"           # (the synthetic rows lie at 100 + 10 i: a 4 Mbp range in the middle, both arms populated)


def phases(stderr):
    ph = {}
    for l in stderr.splitlines():
        if l.startswith("## time "):
            k, v = l[8:].rsplit(" ", 1)
            ph[k] = ph.get(k, 0.0) + float(v)
    return ph


with tempfile.TemporaryDirectory(dir="/dev/shm") as d:
    bench.write_pileup_and_legend(d, n_ref, n_alt, 2504, rows)
    open(os.path.join(d, "p.hap"), "w").write("placeholder\n")
    st = os.stat(os.path.join(d, "p.hap"))
    bench.write_panel_cache(os.path.join(d, "p.cache"), words, 2504, st)
    del words
    names = ",".join(f"ind{(7 + 5 * i) % 2504}" for i in range(n_ind))
    base = [exe, "-H", "p.hap", "-L", "p.legend", "-I", "p.indv", "-P", "p.pileup", "-s", names, "--LD", "--threads", "16",
            "--panel-cache", "p.cache"]
    legs = {"--summary-only": ["--summary-only"],
            "--arm-stats --summary-only": ["--arm-stats", CENTROMERE, "--summary-only"],
            "--arm-stats --stats-only": ["--arm-stats", CENTROMERE, "--stats-only"]}
    outs = {}
    for name, extra in legs.items():
        out = os.path.join(d, "o_" + str(len(outs)))
        os.makedirs(out)
        outs[name] = out
        best = None
        for rep in range(2):
            t0 = time.perf_counter()
            r = subprocess.run(base + extra + ["-O", out], cwd=d, env=dict(os.environ, IBDGEM_TIMING="1"),
                               capture_output=True, text=True, timeout=600)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                print(r.stderr[-800:])
                sys.exit(1)
            ph = phases(r.stderr)
            if best is None or wall < best[0]:
                best = (wall, ph)
        wall, ph = best
        own = sum(v for k, v in ph.items() if k.startswith("per individual") or k.startswith("output files of the last"))
        print(f"{n_ind} individuals, {name}: wall {wall:.3f} s, per-individual phases {own:.3f} s "
              f"({own / n_ind * 1e3:.3f} ms per individual), files {len(os.listdir(out))}", flush=True)
        print("    " + " | ".join(f"{k[:60]} {v:.3f}" for k, v in ph.items()), flush=True)
    a = open(os.path.join(outs["--arm-stats --summary-only"], "UNKWN.armstats.txt")).read()
    b = open(os.path.join(outs["--arm-stats --stats-only"], "UNKWN.armstats.txt")).read()
    print(f"armstats files of --summary-only and --stats-only identical: {a == b}; first lines:")
    print("    " + "\n    ".join(b.splitlines()[:3]))
    if prof_dir:
        os.makedirs(prof_dir, exist_ok=True)
        out = os.path.join(d, "o_prof")
        os.makedirs(out)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof_dir, "-o", "arm", "--output-format", "csv",
                            "--"] + base + legs["--arm-stats --stats-only"] + ["-O", out], cwd=d, capture_output=True,
                           text=True, timeout=900, env=dict(os.environ, IBDGEM_KEEP_TEARDOWN="1"))   # (an orderly exit: the
                                                                                                   # tracer's buffers flush)
        if r.returncode != 0:
            print(r.stderr[-800:])
            sys.exit(1)
        for f in glob.glob(os.path.join(prof_dir, "**", "*kernel_stats.csv"), recursive=True):
            lines = open(f).read().splitlines()
            print(f"kernel statistics ({os.path.basename(f)}):")
            print("    " + lines[0])
            for l in lines[1:]:
                if "llr" in l or "k_ld" in l or "rows_windows" in l or "win_ibd2" in l:
                    print("    " + l)
