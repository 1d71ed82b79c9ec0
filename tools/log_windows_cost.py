"""What option "log_windows" costs at bench.py's shape (4M rows x 2504 individuals, W = 100, bench.py's generator): ms per
comparison individual of queued --LD runs with the option off and on, for T = 1 (a new individual per step) and T = 60,
legs alternating, best and median of five each.  The difference per individual of the T = 1 legs is what k_ld_log and
k_win_log_rows add to a step; k_ld_log's own time comes from a kernel trace of this script:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/log_windows_cost.py --steps 20 --reps 1
(counters in a run of their own).  The sanity ceiling is the strict multiplying kernel's launch at this shape (k_ld_window,
7.4 ms).
    python tools/log_windows_cost.py [--sites N] [--steps K] [--reps R]   (on a GPU box)"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import bench
import ibdgem_amd


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROWS, N_IDS, W = arg("--sites", 4_000_000), 2504, 100
STEPS, REPS = arg("--steps", 60), arg("--reps", 5)

dev = torch.device("cuda", 0)
panel, n_ref, n_alt = bench.build_shard(torch, dev, 0, ROWS, N_IDS, 7, 20241008)
torch.cuda.synchronize()


def engine(log):
    eng = ibdgem_amd.Engine(0, 0.02, 20)
    eng.set_option("site_results", 0)
    eng.set_option("log_windows", log)
    eng.upload_panel_dev(panel.data_ptr(), panel.shape[0], N_IDS)
    eng.upload_sites(np.arange(ROWS, dtype=np.uint32), n_ref, n_alt, W)
    return eng


def leg(eng, T, steps):
    """ms per comparison individual of `steps` queued runs of T individuals, a new set per step"""
    sets = [[(7 + 41 * (i + 60 * k)) % N_IDS for i in range(T)] for k in range(2)]
    eng.set_option("async", 1)
    for k in range(4):
        eng.run(sets[k % 2], ld=True)
    eng.sync()
    t0 = time.perf_counter()
    for k in range(steps):
        eng.run(sets[k % 2], ld=True)
    eng.sync()
    dt = time.perf_counter() - t0
    eng.set_option("async", 0)
    return dt / steps / T * 1e3


engs = {0: engine(0), 1: engine(1)}
del panel
torch.cuda.empty_cache()
for eng in engs.values():                       # the one-off work of a site list in use (re-layout, IBD0 pass): untimed
    for k in range(30):
        eng.run([(7 + k) % N_IDS], ld=True)
    eng.sync()
print(f"{ROWS} rows x {N_IDS} individuals, W = {W}, {engs[1].n_windows} windows, layout {engs[1].ld_layout()}; "
      f"{STEPS} queued steps per leg (T = 60: {max(2, STEPS // 10)}), {REPS} alternating repetitions", flush=True)
for T, steps in ((1, STEPS), (60, max(2, STEPS // 10))):
    ms = {0: [], 1: []}
    for rep in range(REPS):
        for log in (0, 1):
            ms[log].append(leg(engs[log], T, steps))
    for log in (0, 1):
        v = sorted(ms[log])
        print(f"T = {T:2d} log_windows {log}: best {v[0]:.4f} median {v[len(v) // 2]:.4f} ms per comparison individual "
              f"({' '.join(f'{x:.4f}' for x in ms[log])})", flush=True)
    print(f"T = {T:2d}: the option adds {min(ms[1]) - min(ms[0]):.4f} ms per comparison individual (best against best)", flush=True)
lg = engs[1].window_log2(0)
print(f"finite logs: {bool(np.isfinite(lg).all())}; smallest log2 LIBD0 {lg[:, 0].min():.1f}", flush=True)
for eng in engs.values():
    eng.close()
