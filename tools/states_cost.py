"""What --states adds to the whole-panel job: `ibdgem --LD --summary-only` over every panel individual (chr1-scale input:
4M rows x 2504, bench.py's generator, in /dev/shm with a panel cache) without and with --states, the same build,
alternating, five pairs: wall clock of each run, the medians, the difference per individual, and the IBDGEM_TIMING=1
phases of the last pair (which lane the run waits for).  Then one `--stats-only --states` run, and
`hiddengem --summary-list` over the summaries against one `hiddengem -s` process per summary (the first LIST_N of them).
    python tools/states_cost.py [individuals, default 2504] [LIST_N, default 320]   (on a GPU box)"""
import os, sys, tempfile, subprocess, time, statistics
sys.path.insert(0, os.getcwd())
import numpy as np, torch
import bench

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n_ind = int(args[0]) if args else 2504
list_n = int(args[1]) if len(args) > 1 else 320
rows = 4_000_000
dev = torch.device("cuda", 0)
panel, n_ref, n_alt = bench.build_shard(torch, dev, 0, rows, 2504, 7, 20241008)
words = panel.cpu().numpy().view(np.uint64)
del panel
torch.cuda.empty_cache()
host = os.path.join(bench.REPO, "ibdgem_amd", "host")
exe, hg = os.path.join(host, "ibdgem"), os.path.join(host, "hiddengem")


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
    base = [exe, "-H", "p.hap", "-L", "p.legend", "-I", "p.indv", "-P", "p.pileup", "--LD", "--threads", "16",
            "--panel-cache", "p.cache"]
    if n_ind < 2504:
        base += ["-s", ",".join(f"ind{(7 + 5 * i) % 2504}" for i in range(n_ind))]
    legs = {"plain": ["--summary-only"], "states": ["--summary-only", "--states"]}
    outs = {k: os.path.join(d, "o_" + k) for k in list(legs) + ["only"]}
    for o in outs.values():
        os.makedirs(o)

    def one(name, extra):
        t0 = time.perf_counter()
        r = subprocess.run(["timeout", "-k", "10", "600"] + base + extra + ["-O", outs[name]], cwd=d,
                           env=dict(os.environ, IBDGEM_TIMING="1"), capture_output=True, text=True)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            print(r.stderr[-800:])
            sys.exit(1)
        return wall, phases(r.stderr)

    one("plain", legs["plain"])                          # a first run of each, not counted (page cache, the files' pages)
    one("states", legs["states"])
    walls, last = {"plain": [], "states": []}, {}
    for pair in range(5):
        for name in ("plain", "states") if pair % 2 == 0 else ("states", "plain"):
            w, ph = one(name, legs[name])
            walls[name].append(w)
            last[name] = ph
        print(f"pair {pair}: plain {walls['plain'][-1]:.3f} s, --states {walls['states'][-1]:.3f} s", flush=True)
    med = {k: statistics.median(v) for k, v in walls.items()}
    print(f"{n_ind} individuals, --summary-only: median wall {med['plain']:.3f} s (min {min(walls['plain']):.3f}, max {max(walls['plain']):.3f})")
    print(f"{n_ind} individuals, --summary-only --states: median wall {med['states']:.3f} s (min {min(walls['states']):.3f}, "
          f"max {max(walls['states']):.3f})")
    print(f"added by --states: {med['states'] - med['plain']:.3f} s, {(med['states'] - med['plain']) / n_ind * 1e3:.3f} ms per individual")
    for name in ("plain", "states"):
        print(f"phases of the last {name} run:")
        for k, v in sorted(last[name].items(), key=lambda kv: -kv[1])[:8]:
            print(f"    {v:8.3f} s  {k[:100]}")
    w, ph = one("only", ["--stats-only", "--states"])
    same = open(os.path.join(outs["only"], "UNKWN.ibdstates.txt"), "rb").read() == \
        open(os.path.join(outs["states"], "UNKWN.ibdstates.txt"), "rb").read()
    print(f"{n_ind} individuals, --stats-only --states: wall {w:.3f} s; ibdstates.txt equals the --summary-only run's: {same}")
    print("    " + "\n    ".join(open(os.path.join(outs["states"], "UNKWN.ibdstates.txt")).read().splitlines()[-4:]))

    # hiddengem: one process per summary against one --summary-list run
    names = sorted(f[6:-12] for f in os.listdir(outs["states"]) if f.endswith(".summary.txt"))[:list_n]
    t0 = time.perf_counter()
    single = {}
    for n in names:
        r = subprocess.run([hg, "-s", os.path.join(outs["states"], f"UNKWN.{n}.summary.txt")], capture_output=True)
        if r.returncode != 0:
            sys.exit(1)
        single[n] = r.stdout
    t_single = time.perf_counter() - t0
    lst, hg_out = os.path.join(d, "summaries.txt"), os.path.join(d, "hg")
    os.makedirs(hg_out)
    with open(lst, "w") as fh:
        for n in names:
            fh.write(f"{n}\t{os.path.join(outs['states'], f'UNKWN.{n}.summary.txt')}\n")
    t0 = time.perf_counter()
    r = subprocess.run([hg, "--summary-list", lst, "--out-dir", hg_out, "--fractions", os.path.join(d, "frac.txt"), "--threads", "16"],
                       capture_output=True, text=True)
    t_list = time.perf_counter() - t0
    if r.returncode != 0:
        print(r.stderr[-800:])
        sys.exit(1)
    same = all(open(os.path.join(hg_out, n + ".hiddengem.txt"), "rb").read() == single[n] ==
               open(os.path.join(outs["states"], f"UNKWN.{n}.hiddengem.txt"), "rb").read() for n in names)
    print(f"hiddengem over {len(names)} summaries: one -s process each {t_single:.3f} s ({t_single / len(names) * 1e3:.2f} ms each); "
          f"--summary-list --threads 16 {t_list:.3f} s ({t_list / len(names) * 1e3:.2f} ms each); "
          f"tables identical to each other and to ibdgem --states: {same}")
