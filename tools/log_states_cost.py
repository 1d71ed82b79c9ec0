"""What the log-domain statistics cost at bench.py's shape (4M rows x 2504 individuals, W = 100, bench.py's generator):
per batch of T comparison individuals of one --LD run with "log_windows" 1, the wall clock of
  ibdg_window_log2_states      counts only (what --stats-only takes off the device), with the paths, with paths and scores,
  ibdg_log2_states_host        the host twin over the same tables (one thread), after ibdg_get_window_log2_all,
  ibdg_window_log2_llr_sums    two arms, against ibdg_window_llr_sums over the linear table,
each the best and median of --reps calls, in ms per comparison individual; and that device and twin agree on every byte.
The kernels' own times (k_log2_states, k_llr_partial<true>) come from a kernel trace of this script:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/log_states_cost.py --reps 3
--panel-job N: then the whole-panel job of tools/states_cost.py (chr1-scale input in /dev/shm with a panel cache) over N
individuals, `--LD --stats-only --states` (linear: tables fetched, paths on the host) against `--LD --stats-only --states
--log-stats` (paths on the device), alternating, three pairs of wall clocks and the IBDGEM_TIMING=1 phases of the last.
    python tools/log_states_cost.py [--sites N] [--reps R] [--batches 1,60,240] [--panel-job N]   (on a GPU box)"""
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import bench
import ibdgem_amd
from ibdgem_amd import engine as E


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROWS, N_IDS, W = arg("--sites", 4_000_000), 2504, 100
REPS = arg("--reps", 5)
BATCHES = [int(x) for x in arg("--batches", "1,60,240").split(",")]
PEN = (1e-3, 1e-6, 1e-3)

PANEL_JOB = arg("--panel-job", 0)

dev = torch.device("cuda", 0)
panel, n_ref, n_alt = bench.build_shard(torch, dev, 0, ROWS, N_IDS, 7, 20241008)
torch.cuda.synchronize()
words = panel.cpu().numpy().view(np.uint64) if PANEL_JOB else None
eng = ibdgem_amd.Engine(0, 0.02, 20)
eng.set_option("site_results", 0)
eng.set_option("log_windows", 1)
eng.upload_panel_dev(panel.data_ptr(), panel.shape[0], N_IDS)
eng.upload_sites(np.arange(ROWS, dtype=np.uint32), n_ref, n_alt, W)
del panel
torch.cuda.empty_cache()
n = eng.n_windows
print(f"{ROWS} rows x {N_IDS} individuals, W = {W}, {n} windows ({n * 24 / 1e6:.2f} MB of log table per individual), "
      f"{-(-n // 256)} windows a thread; {REPS} repetitions", flush=True)


def clock(fn):
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return out, ms[0], ms[len(ms) // 2]


for T in BATCHES:
    eng.run([(7 + 41 * i) % N_IDS for i in range(T)], ld=True)
    eng.sync()
    eng.window_log2_states(*PEN, want_path=False, want_score=False)            # (buffers allocated: untimed)
    (_, _, c0), b0, m0 = clock(lambda: eng.window_log2_states(*PEN, want_path=False, want_score=False))
    (p1, _, c1), b1, m1 = clock(lambda: eng.window_log2_states(*PEN, want_score=False))
    (p2, s2, c2), b2, m2 = clock(lambda: eng.window_log2_states(*PEN))
    tabs, bt, mt = clock(lambda: eng.window_log2_all(T))
    twin, bh, mh = clock(lambda: [E.log2_states_host(tabs[t], *PEN) for t in range(T)])
    same = all(twin[t][0].tobytes() == p2[t].tobytes() and twin[t][1].tobytes() == s2[t].tobytes() and
               twin[t][2].tobytes() == c2[t].tobytes() for t in range(T))
    same = same and c0.tobytes() == c1.tobytes() == c2.tobytes() and p1.tobytes() == p2.tobytes()
    first, end = [0, n // 2 + 100], [n // 2 - 100, n]
    _, bl, ml = clock(lambda: eng.window_log2_llr_sums(first, end))
    _, bq, mq = clock(lambda: eng.window_llr_sums(first, end))
    f = 1.0 / T
    print(f"T = {T:3d}, ms per comparison individual, best (median):\n"
          f"  device, counts only       {b0 * f:8.4f} ({m0 * f:.4f})\n"
          f"  device, paths             {b1 * f:8.4f} ({m1 * f:.4f})\n"
          f"  device, paths and scores  {b2 * f:8.4f} ({m2 * f:.4f})\n"
          f"  tables to the host        {bt * f:8.4f} ({mt * f:.4f})\n"
          f"  host twin, one thread     {bh * f:8.4f} ({mh * f:.4f})\n"
          f"  log arm sums (two arms)   {bl * f:8.4f} ({ml * f:.4f})   linear: {bq * f:.4f} ({mq * f:.4f})\n"
          f"  device == twin on every byte: {same}; windows per state of individual 0: {c2[0].tolist()}", flush=True)
eng.close()


if PANEL_JOB:
    host = os.path.join(bench.REPO, "ibdgem_amd", "host")
    with tempfile.TemporaryDirectory(dir="/dev/shm") as d:
        bench.write_pileup_and_legend(d, n_ref, n_alt, N_IDS, ROWS)
        open(os.path.join(d, "p.hap"), "w").write("placeholder\n")
        bench.write_panel_cache(os.path.join(d, "p.cache"), words, N_IDS, os.stat(os.path.join(d, "p.hap")))
        del words
        base = [os.path.join(host, "ibdgem"), "-H", "p.hap", "-L", "p.legend", "-I", "p.indv", "-P", "p.pileup", "--LD", "--threads", "16",
                "--panel-cache", "p.cache", "--stats-only", "--states"]
        if PANEL_JOB < N_IDS:
            base += ["-s", ",".join(f"ind{(7 + 5 * i) % N_IDS}" for i in range(PANEL_JOB))]
        legs = {"linear": [], "log": ["--log-stats"]}
        walls, last = {k: [] for k in legs}, {}
        for pair in range(4):                               # (the first pair is not counted: page cache)
            for name in ("linear", "log") if pair % 2 == 0 else ("log", "linear"):
                out = os.path.join(d, "o_" + name)
                os.makedirs(out, exist_ok=True)
                t0 = time.perf_counter()
                r = subprocess.run(["timeout", "-k", "10", "300"] + base + legs[name] + ["-O", out], cwd=d,
                                   env=dict(os.environ, IBDGEM_TIMING="1"), capture_output=True, text=True)
                wall = time.perf_counter() - t0
                if r.returncode != 0:
                    print(r.stderr[-800:])
                    sys.exit(1)
                if pair:
                    walls[name].append(wall)
                ph = {}
                for l in r.stderr.splitlines():
                    if l.startswith("## time "):
                        k, v = l[8:].rsplit(" ", 1)
                        ph[k] = ph.get(k, 0.0) + float(v)
                last[name] = ph
            if pair:
                print(f"pair {pair}: linear {walls['linear'][-1]:.3f} s, --log-stats {walls['log'][-1]:.3f} s", flush=True)
        for name in legs:
            print(f"{PANEL_JOB} individuals, --LD --stats-only --states {' '.join(legs[name])}: median wall "
                  f"{statistics.median(walls[name]):.3f} s (min {min(walls[name]):.3f}, max {max(walls[name]):.3f}); phases of the last run:")
            for k, v in sorted(last[name].items(), key=lambda kv: -kv[1])[:5]:
                print(f"    {v:8.3f} s  {k[:100]}")
        for name, fn in (("linear", "UNKWN.ibdstates.txt"), ("log", "UNKWN.logibdstates.txt")):
            print(name + ":\n    " + "\n    ".join(open(os.path.join(d, "o_" + name, fn)).read().splitlines()[-4:]))
