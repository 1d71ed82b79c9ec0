"""What --sample-paths costs at bench.py's shape (4M rows x 2504 individuals, W = 100, bench.py's generator: 34 599 windows): for a
batch of T comparison individuals of one --LD run with "log_windows" 1 and K draws each, the wall clock of
  ibdg_window_log2_samples   alpha, the draws in chunks of pairs, their segment words, 120 K bytes per individual out,
  ibdg_log2_samples_host     the host twin over the same tables (one thread), after ibdg_get_window_log2_all: with that copy, the
                             ceiling the device route has to stay under,
the device call as the best and median of --reps calls -- every timed call behind an untimed one with other penalties and one
draw, so that it finds no alpha kept from the repetition before --, the twin once; and that device and twin agree on every
byte.  The kernels' own times (k_log2_alpha, k_log2_sample_paths, k_log2_segments_count, k_log2_sample_records) come from a
kernel trace of this script without the twin, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/log_samples_cost.py --reps 2 --no-twin
    python tools/log_samples_cost.py [--sites N] [--reps R] [--targets 60] [--draws 1000] [--no-twin]   (on a GPU box)"""
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
REPS, T, K = arg("--reps", 3), arg("--targets", 60), arg("--draws", 1000)
TWIN = "--no-twin" not in sys.argv
PEN = (1e-3, 1e-6, 1e-3)
OTHER = (0.25, 0.125, 0.25)
SEED = 1

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
pairs = T * K
chunk = min(pairs, (256 << 20) // (n + 8 * 28))
print(f"{ROWS} rows x {N_IDS} individuals, W = {W}, {n} windows, {-(-n // 256)} windows a thread; T = {T}, K = {K}: {pairs} pairs, "
      f"{pairs * n / 1e9:.2f} G window steps, {-(-pairs // chunk)} chunks of {chunk} pairs; {REPS} repetitions", flush=True)

targets = [(7 + 41 * i) % N_IDS for i in range(T)]
streams = np.array(targets, dtype=np.uint64)
pos_first = np.arange(n, dtype=np.uint64) * 1000 + 1
pos_last = pos_first + 900
eng.run(targets, ld=True)
eng.sync()
eng.window_log2_samples(*PEN, K, SEED, streams, pos_first, pos_last)            # (buffers allocated: untimed)
ms = []
for _ in range(REPS):
    eng.window_log2_samples(*OTHER, 1, SEED, streams)                          # (alpha is stale for the timed call)
    t0 = time.perf_counter()
    out = eng.window_log2_samples(*PEN, K, SEED, streams, pos_first, pos_last)
    ms.append((time.perf_counter() - t0) * 1e3)
ms.sort()
t0 = time.perf_counter()
again = eng.window_log2_samples(*PEN, K, SEED, streams, pos_first, pos_last)    # alpha kept: the draws alone
kept = (time.perf_counter() - t0) * 1e3
print(f"device call, ms: best {ms[0]:.2f}, median {ms[len(ms) // 2]:.2f} ({ms[0] / T:.3f} per individual, "
      f"{ms[0] * 1e6 / (pairs * n):.4f} ns per window step); with alpha kept {kept:.2f}; the same bytes again: "
      f"{again.tobytes() == out.tobytes()}", flush=True)
win = out[:, :, :3].mean(axis=1)
print(f"mean windows per state of individual 0: {win[0].tolist()}; draws of individual 0 with an IBD1 or IBD2 segment: "
      f"{int((out[0, :, 4] + out[0, :, 5] > 0).sum())} of {K}", flush=True)
if TWIN:
    t0 = time.perf_counter()
    tabs = eng.window_log2_all(T)
    copy = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    twin = [E.log2_samples_host(tabs[t], *PEN, K, SEED, int(streams[t]), pos_first=pos_first, pos_last=pos_last, want_paths=False)[1]
            for t in range(T)]
    host = (time.perf_counter() - t0) * 1e3
    same = all(twin[t].tobytes() == out[t].tobytes() for t in range(T))
    p = eng.get_log2_sample_path(T - 1, K - 1)
    one = E.log2_samples_host(tabs[T - 1], *PEN, K, SEED, int(streams[T - 1]))[0][K - 1]
    print(f"tables to the host {copy:.2f} ms, host twin on one thread {host:.1f} ms ({host / T:.2f} per individual, "
          f"{host * 1e6 / (pairs * n):.3f} ns per window step)\n"
          f"ceiling (tables + twin) {copy + host:.1f} ms; the device route is {'below' if ms[0] < copy + host else 'NOT below'} it, "
          f"{(copy + host) / ms[0]:.0f} times\n"
          f"device == twin on every byte: {same}; the last draw's path drawn again == the twin's: {p.tobytes() == one.tobytes()}", flush=True)
eng.close()
