"""What --switches costs at bench.py's shape (4M rows x 2504 individuals, W = 100, bench.py's generator): per batch of T
comparison individuals of one --LD run with "log_windows" 1, the wall clock of
  ibdg_window_log2_switches    the expectations only (what --stats-only takes off the device), and with the rows,
  ibdg_window_log2_posteriors  expect and log2 Z only, beside it on the same tables (the same three passes),
  ibdg_log2_switches_host      the host twin over the same tables (one thread), after ibdg_get_window_log2_all: with that copy,
                               the ceiling the device route has to stay under; and once on the table that says nothing (the prior),
each the best and median of --reps calls, in ms per comparison individual -- the switches keep nothing, and every timed
posteriors call stands behind an untimed one with other penalties --; and that device and twin agree on every byte.
The kernels' own times (k_log2_switches beside k_log2_posteriors) come from a kernel trace of this script, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/log_switches_cost.py --reps 3 --batches 60,240
    python tools/log_switches_cost.py [--sites N] [--reps R] [--batches 60,240]   (on a GPU box)"""
import os
import sys
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
BATCHES = [int(x) for x in arg("--batches", "60,240").split(",")]
PEN = (1e-3, 1e-6, 1e-3)
OTHER = (0.25, 0.125, 0.25)

dev = torch.device("cuda", 0)
panel, n_ref, n_alt = bench.build_shard(torch, dev, 0, ROWS, N_IDS, 7, 20241008)
torch.cuda.synchronize()
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


def clock(fn, before=None):
    """before: untimed, in front of every repetition"""
    ms = []
    for _ in range(REPS):
        if before:
            before()
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return out, ms[0], ms[len(ms) // 2]


for T in BATCHES:
    eng.run([(7 + 41 * i) % N_IDS for i in range(T)], ld=True)
    eng.sync()
    eng.window_log2_switches(*PEN, want_sw=False)                              # (buffers allocated: untimed)
    (_, e0), b0, m0 = clock(lambda: eng.window_log2_switches(*PEN, want_sw=False))
    (s1, e1), b1, m1 = clock(lambda: eng.window_log2_switches(*PEN))
    _, bp, mp = clock(lambda: eng.window_log2_posteriors(*PEN, want_post=False),
                      lambda: eng.window_log2_posteriors(*OTHER, want_post=False))
    tabs, bt, mt = clock(lambda: eng.window_log2_all(T))
    twin, bh, mh = clock(lambda: [E.log2_switches_host(tabs[t], *PEN) for t in range(T)])
    _, bn, mn = clock(lambda: E.log2_switches_host(None, *PEN, want_sw=False, n_win=n))
    same = all(twin[t][0].tobytes() == s1[t].tobytes() and twin[t][1].tobytes() == e1[t].tobytes() for t in range(T))
    same = same and e0.tobytes() == e1.tobytes()
    f = 1.0 / T
    print(f"T = {T:3d}, ms per comparison individual, best (median):\n"
          f"  device, the expectations only    {b0 * f:8.4f} ({m0 * f:.4f})\n"
          f"  device, with the rows            {b1 * f:8.4f} ({m1 * f:.4f})\n"
          f"  device, posteriors, sums only    {bp * f:8.4f} ({mp * f:.4f})\n"
          f"  tables to the host               {bt * f:8.4f} ({mt * f:.4f})\n"
          f"  host twin, one thread            {bh * f:8.4f} ({mh * f:.4f})\n"
          f"  ceiling (tables + twin)          {(bt + bh) * f:8.4f}; the device route is {'below' if b0 < bt + bh else 'NOT below'} it\n"
          f"  the prior, once a site list (ms) {bn:8.4f} ({mn:.4f})\n"
          f"  device == twin on every byte: {same}; expected switches of individual 0: {e1[0].tolist()}",
          flush=True)
eng.close()
