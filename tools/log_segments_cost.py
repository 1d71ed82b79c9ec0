"""What --segments costs at bench.py's shape (4M rows x 2504 individuals, W = 100, bench.py's generator): per batch of T
comparison individuals of one --LD run with "log_windows" 1, the wall clock of
  ibdg_window_log2_states      counts only: the yardstick (the call --stats-only --states makes anyway),
  ibdg_window_log2_posteriors  expect and log2 Z only, likewise,
  ibdg_window_log2_segments    without and with the posteriors (it runs the kernels of the two calls above and then counts:
                               what it adds is its time less theirs), with the windows' positions,
  ibdg_get_log2_segments       the records of that call,
  the three calls in turn      states, posteriors, segments with the posteriors, as --stats-only --posteriors --segments issues
                               them per batch (the segments call then finds the path and the posteriors made),
  ibdg_log2_segments_host      the host twin over the same tables (one thread), after ibdg_get_window_log2_all,
each the best and median of --reps calls, in ms per comparison individual -- every timed call behind untimed calls with other
penalties, so that it finds nothing kept from the repetition before --; and that device and twin agree on every byte.
The kernels' own times (k_log2_segments_count, k_log2_segments_write beside k_log2_states) come from a kernel trace of this
script, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/log_segments_cost.py --reps 3 --batches 60,240
    python tools/log_segments_cost.py [--sites N] [--reps R] [--batches 60,240] [--twin-only]   (on a GPU box)
--twin-only needs no device: the twin's time per individual on a random table of the same number of windows."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np

from ibdgem_amd import engine as E


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROWS, N_IDS, W = arg("--sites", 4_000_000), 2504, 100
REPS = arg("--reps", 5)
BATCHES = [int(x) for x in arg("--batches", "60,240").split(",")]
PEN = (1e-3, 1e-6, 1e-3)
SMALL = (0.5, 0.25, 0.5)             # about a bit a switch: many segments, for the records' cost
OTHER = (0.25, 0.125, 0.25)          # what the untimed calls between two repetitions leave a path and posteriors for


def clock(fn, before=None):
    """before: untimed, in front of every repetition (a call with OTHER penalties, so that the timed one finds nothing kept)"""
    ms = []
    for _ in range(REPS):
        if before:
            before()
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return out, ms[0], ms[len(ms) // 2]


def positions(n):
    first = np.arange(n, dtype=np.uint64) * np.uint64(7000) + np.uint64(10_000)
    return first, first + np.uint64(6500)


if "--twin-only" in sys.argv:
    n = arg("--windows", 34_599)
    rng = np.random.default_rng(20241008)
    tab = rng.normal(-3000.0, 400.0, (n, 1)) + rng.uniform(-30.0, 30.0, (n, 3))
    pf, pl = positions(n)
    print(f"{n} windows, random table of +-30 bits, one host thread; {REPS} repetitions, ms per individual, best (median):")
    for name, pen in (("default penalties", PEN), ("(0.5, 0.25, 0.5)", SMALL)):
        (_, _, c), bs, ms_ = clock(lambda: E.log2_states_host(tab, *pen, want_score=False))
        (_, k0, _), b0, m0 = clock(lambda: E.log2_segments_host(tab, *pen, pos_first=pf, pos_last=pl))
        (_, k1, _), b1, m1 = clock(lambda: E.log2_segments_host(tab, *pen, with_post=True, pos_first=pf, pos_last=pl))
        print(f"  {name}: {k0} segments\n"
              f"    ibdg_log2_states_host                     {bs:8.3f} ({ms_:.3f})\n"
              f"    ibdg_log2_segments_host                   {b0:8.3f} ({m0:.3f})\n"
              f"    ibdg_log2_segments_host, with posteriors  {b1:8.3f} ({m1:.3f})", flush=True)
    sys.exit(0)

import torch

import bench
import ibdgem_amd

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
pf, pl = positions(n)
print(f"{ROWS} rows x {N_IDS} individuals, W = {W}, {n} windows ({n * 24 / 1e6:.2f} MB of log table per individual), "
      f"{-(-n // 256)} windows a thread; {REPS} repetitions", flush=True)

for T in BATCHES:
    eng.run([(7 + 41 * i) % N_IDS for i in range(T)], ld=True)
    eng.sync()
    f = 1.0 / T
    for name, pen in (("default penalties", PEN), ("(0.5, 0.25, 0.5)", SMALL)):
        eng.window_log2_segments(*pen, with_post=True, pos_first=pf, pos_last=pl)       # (buffers allocated: untimed)
        eng.get_log2_segments()
        def stale():
            eng.window_log2_states(*OTHER, want_path=False, want_score=False)
            eng.window_log2_posteriors(*OTHER, want_post=False)

        def as_shard_run():                  # the three calls of --stats-only --posteriors --segments on one batch
            eng.window_log2_states(*pen, want_path=False, want_score=False)
            eng.window_log2_posteriors(*pen, want_post=False)
            return eng.window_log2_segments(*pen, with_post=True, pos_first=pf, pos_last=pl)

        _, bs, ms_ = clock(lambda: eng.window_log2_states(*pen, want_path=False, want_score=False), stale)
        _, bp, mp = clock(lambda: eng.window_log2_posteriors(*pen, want_post=False), stale)
        (n0, s0), b0, m0 = clock(lambda: eng.window_log2_segments(*pen, pos_first=pf, pos_last=pl), stale)
        r0, bg0, mg0 = clock(lambda: eng.get_log2_segments())
        (n1, s1), b1, m1 = clock(lambda: eng.window_log2_segments(*pen, with_post=True, pos_first=pf, pos_last=pl), stale)
        r1, bg1, mg1 = clock(lambda: eng.get_log2_segments())
        (n2, s2), b2, m2 = clock(as_shard_run, stale)
        tabs, bt, mt = clock(lambda: eng.window_log2_all(T))
        twin, bh, mh = clock(lambda: [E.log2_segments_host(tabs[t], *pen, with_post=True, pos_first=pf, pos_last=pl) for t in range(T)])
        same = n0.tobytes() == n1.tobytes() == n2.tobytes() and s0.tobytes() == s1.tobytes() == s2.tobytes()
        same = same and all(int(n1[t]) == twin[t][1] and s1[t].tobytes() == twin[t][2].tobytes() for t in range(T))
        same = same and r1.tobytes() == b"".join(twin[t][0].tobytes() for t in range(T))
        add0, add1 = b0 - bs, b1 - bs - bp
        print(f"T = {T:3d}, {name}: {int(n1.sum())} segments ({int(n1.sum()) * 56 / T:.0f} bytes of records per individual); ms per "
              f"comparison individual, best (median):\n"
              f"  states, counts only                    {bs * f:8.4f} ({ms_ * f:.4f})\n"
              f"  posteriors, expect and log2 Z only     {bp * f:8.4f} ({mp * f:.4f})\n"
              f"  segments, no posteriors                {b0 * f:8.4f} ({m0 * f:.4f})   adds {add0 * f:.4f} to the states call: "
              f"{'under' if add0 < bs else 'NOT under'} that call's own time\n"
              f"  ... their records                      {bg0 * f:8.4f} ({mg0 * f:.4f})\n"
              f"  segments, with posteriors              {b1 * f:8.4f} ({m1 * f:.4f})   adds {add1 * f:.4f} to the two calls\n"
              f"  ... their records                      {bg1 * f:8.4f} ({mg1 * f:.4f})\n"
              f"  states, posteriors, segments in turn   {b2 * f:8.4f} ({m2 * f:.4f})   the three calls alone add up to {(bs + bp + b1) * f:.4f}\n"
              f"  tables to the host                     {bt * f:8.4f} ({mt * f:.4f})\n"
              f"  host twin with posteriors, one thread  {bh * f:8.4f} ({mh * f:.4f})\n"
              f"  device == twin on every byte: {same}; summary of individual 0: {s1[0].tolist()}", flush=True)
eng.close()
