"""What the step shifts (--switch-scale) cost at bench.py's shape (4M rows x 2504 individuals, W = 100, bench.py's
generator): with steps set k_log2_states and k_log2_posteriors read an int32 per window and form the window's own penalties or
weights; without them they are the instantiations that were there before.  Per
batch of T comparison individuals of one --LD run with "log_windows" 1, the wall clock of
  ibdg_window_log2_states      counts only,
  ibdg_window_log2_posteriors  expect and log2 Z only,
  ibdg_window_log2_segments    with the posteriors and the windows' positions, and ibdg_get_log2_segments, its records,
each the best and median of --reps calls in ms per comparison individual -- every timed call behind untimed calls with other
penalties, so that it finds nothing kept --, for one case per process:
  --steps 0    no steps set (the only case a build without ibdg_set_window_steps can run: IBDG_LIB=<the parent's library>),
  --steps 1    a shift on every window: log2 of distances drawn between a tenth and ten times the scale, as --switch-scale makes,
  --chains K   beside either: K - 1 chain starts spread evenly over the windows (default 1: none);
device == twin on every byte is checked too.
The kernels' own times come from a kernel trace of this script, in a run of its own per build and case:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/log_steps_cost.py --reps 3 --batches 60,240 --steps 0
    python tools/log_steps_cost.py --trace OUT       the medians (us) of each kernel's launches per grid size, from OUT's trace
    python tools/log_steps_cost.py [--sites N] [--reps R] [--batches 60,240] [--steps 0|1] [--chains K]   (on a GPU box)"""
import csv
import glob
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


KERNELS = ("k_log2_states", "k_log2_posteriors", "k_log2_segments_count", "k_log2_segments_write")

if "--trace" in sys.argv:
    # the kernel trace of a run above: one row per dispatch; the grid is the batch (a workgroup of 256 per individual)
    times = {}
    for fn in glob.glob(os.path.join(arg("--trace", "."), "**", "*kernel_trace.csv"), recursive=True):
        with open(fn, newline="") as fh:
            for row in csv.DictReader(fh):
                kn = row["Kernel_Name"]                                   # mangled or not, a template's instantiation or not
                name = next((k for k in KERNELS if any(k + c in kn for c in "(<EI") or kn.endswith(k)), None)
                if name is None:
                    continue
                grid = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0) // 256
                us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                times.setdefault((name, grid), []).append(us)
    for (name, grid), us in sorted(times.items()):
        print(f"{name:24s} T = {grid:4d}  median {statistics.median(us):8.1f} us  min {min(us):8.1f}  launches {len(us)}")
    sys.exit(0 if times else 1)

import numpy as np
import torch

import bench
import ibdgem_amd
from ibdgem_amd import engine as E

ROWS, N_IDS, W = arg("--sites", 4_000_000), 2504, 100
REPS = arg("--reps", 5)
BATCHES = [int(x) for x in arg("--batches", "60,240").split(",")]
CHAINS = arg("--chains", 1)
STEPS = arg("--steps", 0)
PEN = (1e-3, 1e-6, 1e-3)
OTHER = (0.25, 0.125, 0.25)          # what the untimed calls between two repetitions leave a path and posteriors for


def clock(fn, before=None):
    ms = []
    for _ in range(REPS):
        if before:
            before()
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return out, ms[0], ms[len(ms) // 2]


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
pf = np.arange(n, dtype=np.uint64) * np.uint64(7000) + np.uint64(10_000)
pl = pf + np.uint64(6500)
starts = [n * k // CHAINS for k in range(1, CHAINS)] if CHAINS > 1 else []
has_chains = hasattr(eng.lib, "ibdg_set_window_chains")
if starts and not has_chains:
    sys.exit("this build of the library has no ibdg_set_window_chains: --chains 0 is all it can run")
if starts:
    eng.set_window_chains(starts)
has_steps = hasattr(eng.lib, "ibdg_set_window_steps")
if STEPS and not has_steps:
    sys.exit("this build of the library has no ibdg_set_window_steps: --steps 0 is all it can run")
shift = None
if STEPS:
    shift = np.rint(np.random.default_rng(12).uniform(-np.log2(10.0), np.log2(10.0), n) * 65536.0).astype(np.int32)
    eng.set_window_steps(shift)
print(f"{ROWS} rows x {N_IDS} individuals, W = {W}, {n} windows, {-(-n // 256)} windows a thread; {len(starts) + 1} chain(s), "
      f"{'steps' if STEPS else 'no steps'}{'' if has_steps else ' (a build without steps)'}; {REPS} repetitions", flush=True)
kw = dict(starts=starts, shift=shift) if STEPS else dict(starts=starts)

for T in BATCHES:
    eng.run([(7 + 41 * i) % N_IDS for i in range(T)], ld=True)
    eng.sync()
    f = 1.0 / T
    eng.window_log2_segments(*PEN, with_post=True, pos_first=pf, pos_last=pl)           # (buffers allocated: untimed)
    eng.get_log2_segments()

    def stale():
        eng.window_log2_states(*OTHER, want_path=False, want_score=False)
        eng.window_log2_posteriors(*OTHER, want_post=False)

    (_, _, cnt), bs, ms_ = clock(lambda: eng.window_log2_states(*PEN, want_path=False, want_score=False), stale)
    (_, exp, z), bp, mp = clock(lambda: eng.window_log2_posteriors(*PEN, want_post=False), stale)
    (n1, s1), b1, m1 = clock(lambda: eng.window_log2_segments(*PEN, with_post=True, pos_first=pf, pos_last=pl), stale)
    r1, bg, mg = clock(lambda: eng.get_log2_segments())
    same = "not checked"
    if has_chains:
        tabs = eng.window_log2_all(T)
        same = True
        for t in range(0, T, max(T // 12, 1)):                                          # a dozen individuals of the batch
            wseg, wn, wsum = E.log2_segments_host(tabs[t], *PEN, with_post=True, pos_first=pf, pos_last=pl, **kw)
            _, wexp, wz = E.log2_posteriors_host(tabs[t], *PEN, want_post=False, **kw)
            _, _, wc = E.log2_states_host(tabs[t], *PEN, want_path=False, want_score=False, **kw)
            off = int(n1[:t].sum())
            same = same and int(n1[t]) == wn and s1[t].tobytes() == wsum.tobytes() and r1[off:off + wn].tobytes() == wseg.tobytes()
            same = same and exp[t].tobytes() == wexp.tobytes() and float(z[t]) == wz and cnt[t].tobytes() == wc.tobytes()
    print(f"T = {T:3d}: {int(n1.sum())} segments; ms per comparison individual, best (median):\n"
          f"  states, counts only                    {bs * f:8.4f} ({ms_ * f:.4f})\n"
          f"  posteriors, expect and log2 Z only     {bp * f:8.4f} ({mp * f:.4f})\n"
          f"  segments, with posteriors              {b1 * f:8.4f} ({m1 * f:.4f})\n"
          f"  ... their records                      {bg * f:8.4f} ({mg * f:.4f})\n"
          f"  device == twin on every byte: {same}", flush=True)
eng.close()
