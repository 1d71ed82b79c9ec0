"""What --fit-penalties costs at bench.py's shape (4M rows x 2504 individuals, W = 100, bench.py's generator) with the log2 tables
of all 2504 individuals in the context's store (--LD runs of 60 with "log_windows" 1, each appended): the wall clock of
  ibdg_log2_store_fit          25 iterations at the most from (1e-3, 1e-6, 1e-3), and one ibdg_log2_store_switches (an iteration's
                               launch and its 24 bytes per individual) on its own,
  the parent's only way        the same expectations without a store: per batch of 60 ibdg_set_window_log2 (the batch's table back
                               up from the host) and ibdg_window_log2_switches, 42 batches an iteration,
  ibdg_log2_switches_host      the twin on one thread for a sample of individuals, scaled to all,
  k_log2_switch_expect         against k_log2_switches<.., false> per individual at T = 240 on the same tables: --reps alternating
                               pairs of ibdg_log2_store_switches and ibdg_window_log2_switches in this one process,
each in ms, best and median of --reps; and that the store's expectations equal the parent's way and the twin on every byte.
    python tools/log_fit_cost.py [--sites N] [--individuals T] [--reps R] [--iterations I]   (on a GPU box)"""
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


ROWS, N_IDS, W, BATCH = arg("--sites", 4_000_000), 2504, 100, 60
T_ALL = arg("--individuals", N_IDS)
REPS = arg("--reps", 5)
ITER = arg("--iterations", 25)
PEN = (1e-3, 1e-6, 1e-3)

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
print(f"{ROWS} rows x {N_IDS} individuals, W = {W}, {n} windows ({n * 24 / 1e6:.2f} MB of log table per individual; "
      f"{T_ALL * n * 24 / 1e9:.2f} GB for {T_ALL}); {REPS} repetitions", flush=True)


def clock(fn, reps=REPS):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return out, ms[0], ms[len(ms) // 2]


# ---- the two kernels per individual at T = 240, alternating ----
T = 240
eng.run([(7 + 41 * i) % N_IDS for i in range(T)], ld=True)
eng.sync()
eng.log2_store_reserve(T)
eng.log2_store_append()
e_new = eng.log2_store_switches(*PEN)                                          # (buffers allocated: untimed)
_, e_old = eng.window_log2_switches(*PEN, want_sw=False)
pairs = []
for _ in range(max(REPS, 5)):
    t0 = time.perf_counter()
    eng.log2_store_switches(*PEN)
    t1 = time.perf_counter()
    eng.window_log2_switches(*PEN, want_sw=False)
    t2 = time.perf_counter()
    pairs.append(((t1 - t0) * 1e3 / T, (t2 - t1) * 1e3 / T))
new, old = sorted(p[0] for p in pairs), sorted(p[1] for p in pairs)
print(f"T = {T}, ms per individual, alternating pairs (store kernel, k_log2_switches without the rows):\n  " +
      ", ".join(f"{a:.5f} / {b:.5f}" for a, b in pairs) +
      f"\n  best {new[0]:.5f} / {old[0]:.5f}, median {new[len(new) // 2]:.5f} / {old[len(old) // 2]:.5f}, "
      f"spread {new[-1] - new[0]:.5f} / {old[-1] - old[0]:.5f}; the same bytes: {e_new.tobytes() == e_old.tobytes()}", flush=True)

# ---- the whole panel in the store ----
targets = [(7 + 41 * i) % N_IDS for i in range(T_ALL)]
eng.log2_store_reserve(T_ALL)
host_tabs = []
t0 = time.perf_counter()
for b0 in range(0, T_ALL, BATCH):
    eng.run(targets[b0:b0 + BATCH], ld=True)
    eng.log2_store_append()
    host_tabs.append(eng.window_log2_all(len(targets[b0:b0 + BATCH])))
print(f"{len(host_tabs)} runs of {BATCH}, each appended and copied to the host: {(time.perf_counter() - t0) * 1e3:.1f} ms", flush=True)
assert eng.log2_store_count() == T_ALL
expect = eng.log2_store_switches(*PEN)                                         # (scratch allocated: untimed)
_, b1, m1 = clock(lambda: eng.log2_store_switches(*PEN))
(rows, stood, fitted), bf, mf = clock(lambda: eng.log2_store_fit(PEN, ITER), reps=max(1, REPS // 2))
print(f"store of {T_ALL}: one ibdg_log2_store_switches {b1:.3f} ({m1:.3f}) ms = {b1 / T_ALL:.5f} ms per individual;\n"
      f"  ibdg_log2_store_fit, limit {ITER}: {len(rows)} iterations, {'stood' if stood else 'limit'}, {bf:.1f} ({mf:.1f}) ms = "
      f"{bf / max(len(rows), 1):.3f} ms per iteration; fitted {fitted.tolist()}", flush=True)


def parents_way():
    out = []
    for tabs in host_tabs:
        if len(tabs) != eng.lib.ibdg_num_targets(eng.ctx):
            eng.run(targets[:len(tabs)], ld=True)                             # (a last, shorter batch needs a run of its size)
        eng.set_window_log2_all(tabs)
        out.append(eng.window_log2_switches(*PEN, want_sw=False)[1])
    return np.concatenate(out)


eng.run(targets[:BATCH], ld=True)
old_expect, bo, mo = clock(parents_way, reps=max(1, REPS // 2))
print(f"  the parent's way, one iteration ({len(host_tabs)} x set_window_log2 + window_log2_switches): {bo:.1f} ({mo:.1f}) ms; "
      f"{ITER} iterations {bo * ITER:.0f} ms; the same bytes: {old_expect.tobytes() == expect.tobytes()}", flush=True)
sample = [int(t) for t in np.linspace(0, T_ALL - 1, 8)]
twin, bh, mh = clock(lambda: [E.log2_switches_host(host_tabs[t // BATCH][t % BATCH], *PEN, want_sw=False)[1] for t in sample],
                     reps=max(1, REPS // 2))
same = all(twin[i].tobytes() == expect[t].tobytes() for i, t in enumerate(sample))
print(f"  the twin, one thread, {len(sample)} individuals: {bh / len(sample):.3f} ({mh / len(sample):.3f}) ms per individual, "
      f"{bh / len(sample) * T_ALL:.0f} ms an iteration over all; the same bytes: {same}", flush=True)
eng.close()
