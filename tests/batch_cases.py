"""31 comparison individuals of synA -- a batch of 30, one more queued ahead -- and the 31 runs of one individual each that
every batched run of the host program must equal: its files byte for byte, its statistics files line for line.  The single
runs are made once per test session (eight at a time) and shared by the GPU tests of the features they carry."""
import functools
import os
import tempfile
from concurrent.futures import ThreadPoolExecutor

import golden_io as G
import pileup_list_util as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
INPUT = os.path.join(G.GOLD, "synA", "input")
NAMES = [f"ind{(3 + 11 * k) % 70}" for k in range(31)]
# every statistic of the log-domain window table, over windows of 16 rows with both chromosome arms populated
STATS = ["--LD", "-w", "16", "--log-stats", "--states", "--posteriors", "--segments", "--arm-stats", "30000,40000"]
STATS_FILES = ["UNKWN.logarmstats.txt", "UNKWN.logibdstates.txt", "UNKWN.logibdposteriors.txt", "UNKWN.logibdsegments.txt"]
_keep = []


def run(extra, names, out):
    os.makedirs(out, exist_ok=True)
    r = U.run(EXE, G.cases("synA")["base_args"] + STATS + extra + ["-s", ",".join(names), "-O", str(out)], INPUT)
    assert r.returncode == 0, r.stderr[-3000:]
    return U.output_files(out)


@functools.lru_cache(maxsize=None)
def singles():
    """{name: the files of its run alone, with --log-summary --summary-only}"""
    _keep.append(tempfile.TemporaryDirectory())
    with ThreadPoolExecutor(8) as pool:
        files = pool.map(lambda n: run(["--log-summary", "--summary-only"], [n], os.path.join(_keep[-1].name, n)), NAMES)
    return dict(zip(NAMES, files))


def line_of(data, name):
    """an individual's line(s) of a statistics file"""
    return [l for l in data.decode().splitlines() if l.split("\t")[0] == name]


def check_statistics(files):
    for fn in STATS_FILES:
        for name in NAMES:
            want = line_of(singles()[name][fn], name)
            assert len(want) == 1 and line_of(files[fn], name) == want, (fn, name)
