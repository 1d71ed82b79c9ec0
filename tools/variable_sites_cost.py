"""What -v costs per comparison individual, with the site lists made on the device against the parent build (the host's scan
of every panel row per individual): `ibdgem -v --LD --summary-only` on chr1-scale input (4M rows x 2504, bench.py's
generator, window 100, the panel cache in /dev/shm and warm) for T comparison individuals, the two programs alternating,
three pairs: wall clock of each run, per individual, and the IBDGEM_TIMING=1 phases of the last pair.  The new program
with IBDGEM_VARSITES=host beside them (its own host path) and the files of all three compared.  With --whole-panel the
same pairs with every individual of the panel (-S), once.  Then one run of the new program under
`rocprofv3 --kernel-trace --stats` for the selection kernels' own times, and the engine's clocks
(ibdg_upload_ms: selection, preparation) for a few individuals through ctypes.
    python tools/variable_sites_cost.py --parent EXE [--individuals 60] [--whole-panel] [--no-trace | --trace-only]   (on a GPU box)"""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import bench


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


PARENT = arg("--parent", None)
T = int(arg("--individuals", "60"))
ROWS, N_IDS = 4_000_000, 2504
exe = os.path.join(bench.REPO, "ibdgem_amd", "host", "ibdgem")

dev = torch.device("cuda", 0)
panel, n_ref, n_alt = bench.build_shard(torch, dev, 0, ROWS, N_IDS, 7, 20241008)
words = panel.cpu().numpy().view(np.uint64)
del panel
torch.cuda.empty_cache()


def phases(stderr):
    ph = {}
    for l in stderr.splitlines():
        if l.startswith("## time "):
            k, v = l[8:].rsplit(" ", 1)
            ph[k] = ph.get(k, 0.0) + float(v)
    return ph


def files_of(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


with tempfile.TemporaryDirectory(dir="/dev/shm") as d:
    bench.write_pileup_and_legend(d, n_ref, n_alt, N_IDS, ROWS)
    open(os.path.join(d, "p.hap"), "w").write("placeholder\n")
    bench.write_panel_cache(os.path.join(d, "p.cache"), words, N_IDS, os.stat(os.path.join(d, "p.hap")))
    args = ["-H", "p.hap", "-L", "p.legend", "-I", "p.indv", "-P", "p.pileup", "--LD", "-v", "--summary-only", "--threads", "16",
            "--panel-cache", "p.cache"]
    builds = {"new": (exe, {})}
    if PARENT:
        builds["parent"] = (os.path.abspath(PARENT), {})
    builds["new, IBDGEM_VARSITES=host"] = (exe, {"IBDGEM_VARSITES": "host"})

    def one(name, targets, limit=900):
        out = tempfile.mkdtemp(dir=d)
        e, env = builds[name]
        t0 = time.perf_counter()
        r = subprocess.run(["timeout", "-k", "10", str(limit), e] + args + targets + ["-O", out], cwd=d,
                           env=dict(os.environ, IBDGEM_TIMING="1", **env), capture_output=True, text=True)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            print(name, "failed:", r.stderr[-1500:], flush=True)
            sys.exit(1)
        files = files_of(out)
        subprocess.run(["rm", "-rf", out])
        return wall, phases(r.stderr), files

    def compare(targets, n, pairs, label):
        one("new", targets)                              # not counted: the page cache, the first run's pages
        walls, last, files = {k: [] for k in builds}, {}, {}
        for pair in range(pairs):
            order = list(builds) if pair % 2 == 0 else list(builds)[::-1]
            for name in order:
                w, ph, fs = one(name, targets)
                walls[name].append(w)
                last[name], files[name] = ph, fs
            print(f"{label}, pair {pair}: " + ", ".join(f"{k} {walls[k][-1]:.3f} s ({walls[k][-1] / n * 1e3:.2f} ms per individual)"
                                                        for k in builds), flush=True)
        ref = files["new, IBDGEM_VARSITES=host"]
        print(f"{label}: {len(ref)} files; identical to the host path's: " +
              ", ".join(f"{k}: {files[k] == ref}" for k in builds if k != "new, IBDGEM_VARSITES=host"), flush=True)
        if PARENT:
            print(f"{label}: new below parent in every pair: {all(a < b for a, b in zip(walls['new'], walls['parent']))}; "
                  f"parent / new per pair: {' '.join(f'{b / a:.2f}' for a, b in zip(walls['new'], walls['parent']))}", flush=True)
        for name in builds:
            print(f"{label}: phases of the last {name} run (s):")
            for k, v in sorted(last[name].items(), key=lambda kv: -kv[1])[:7]:
                print(f"    {v:8.3f}  {k[:100]}")
        sys.stdout.flush()

    some = ["-s", ",".join(f"ind{(7 + 41 * i) % N_IDS}" for i in range(T))]
    if "--trace-only" not in sys.argv:
        compare(some, T, 3, f"{T} individuals")
    if "--whole-panel" in sys.argv:
        compare([], N_IDS, 1, "whole panel")

    if "--no-trace" not in sys.argv:
        # the kernels' own times: the new program under the profiler (no counters in the same run)
        tr, out = os.path.join(d, "trace"), tempfile.mkdtemp(dir=d)
        r = subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tr,
                            "--", exe] + args + some + ["-O", out], cwd=d, capture_output=True, text=True,
                           env=dict(os.environ, IBDGEM_KEEP_TEARDOWN="1"))     # (an orderly end: the profiler writes its files at exit)
        if r.returncode != 0:
            print("rocprofv3 run failed:", r.stderr[-1500:], flush=True)
            sys.exit(1)
        print(f"rocprofv3 --kernel-trace --stats, {T} individuals (average per launch):")
        found = glob.glob(os.path.join(tr, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            print("    no kernel_stats.csv under", tr, ":", [os.path.relpath(os.path.join(a, f), tr) for a, _, fs in os.walk(tr) for f in fs])
        for fn in found:
            for row in csv.DictReader(open(fn)):
                full = row["Name"]
                if "k_sel" in full or "k_prep" in full or "gather" in full:
                    n = full[full.index("k_"):].split("(")[0] if "k_" in full else full
                    print(f"    {n[:40]:40s} calls {row['Calls']:>5s} avg {float(row['AverageNs']) / 1e3:8.1f} us")
        sys.stdout.flush()

# the engine's own clocks of a selection: ibdg_upload_ms out[0] = the selection, out[1] = the preparation behind it
import ibdgem_amd
with ibdgem_amd.Engine(0, 0.02, 20) as eng:
    eng.upload_panel(words, N_IDS)
    t0 = time.perf_counter()
    eng.upload_candidates(None, n_ref, n_alt)
    print(f"ibdg_upload_candidates, {ROWS} candidates: {(time.perf_counter() - t0) * 1e3:.2f} ms")
    for t in (7, 48, 1000, 2503, 7):
        eng.select_variable_sites(t, 100)
        ms, n_sel = eng.upload_ms(), eng.n_sites
        eng.upload_sites(None, n_ref, n_alt, 100)
        full = eng.upload_ms()
        print(f"individual {t}: {n_sel} of {ROWS} candidates selected; select: selection {ms['h2d']:.3f} ms, preparation "
              f"{ms['device_prep']:.3f} ms, call {ms['call']:.3f} ms; plain upload of all rows: copies {full['h2d']:.3f}, preparation "
              f"{full['device_prep']:.3f}, call {full['call']:.3f}")
