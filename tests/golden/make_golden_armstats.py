#!/usr/bin/env python3
"""Regenerate tests/golden/armstats/cases.json (run in the build container only, where the reference tree lies).

For the committed 17-digit summaries of a few synthetic cases (tests/golden/syn{A,B}/<case>/, see make_golden.py) and
five centromeric ranges per case, this runs the reference's own bin/chrarm-stats.py (loaded with importlib, its
centromere table replaced by the case's chromosome and range) and stores, per comparison individual:
  line   what the script printed: CHROM, parm_IBD2/IBD0, qarm_IBD2/IBD0, parm_IBD1/IBD0, qarm_IBD1/IBD0 (%.3e)
  sums   the four sums in the script's long double (repr strings), recomputed here in the script's order, for the
         tests' check of values near a %.3e rounding boundary
Ranges (picked from the windows of the individual with the fewest):
  both       both arms populated
  p_nan      c0 < END_0 (the p-arm is nan)
  p_zero     c0 == END_0 (the p-arm is 0)
  c0_at_end  c0 equal to some window's END
  c1_at_start  c1 equal to some window's START
A range after which no window starts (the script raises there) is not generated.  No reference binary is needed.

Usage:  python tests/golden/make_golden_armstats.py        (needs /root/reference)
"""
import gzip
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
CASES = [("synA", "ld_default"), ("synA", "ld_bg_self_nan"), ("synA", "ld_bg20_w64"), ("synA", "ld_varsites"),
         ("synB", "ld_w37"), ("synA", "nonld_flags"), ("synA", "nonld_all_targets_w2")]


def load_script():
    spec = importlib.util.spec_from_file_location("chrarm_stats", os.path.join(REF, "bin", "chrarm-stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def read_summary(path):
    with gzip.open(path, "rt") as fh:
        return fh.read().splitlines()


def windows(lines):
    rows = [l.split() for l in lines[1:] if l]
    return [int(r[1]) for r in rows], [int(r[2]) for r in rows]


def ranges(start, end):
    n = len(end)
    assert n >= 3, n
    return {
        "both": (end[n // 3] + 1, start[2 * n // 3] - 1),
        "p_nan": (end[0] - 1, start[n // 2]),
        "p_zero": (end[0], start[n // 2] + 1),
        "c0_at_end": (end[n // 2], start[min(n // 2 + 1, n - 1)]),
        "c1_at_start": (end[n // 4], start[3 * n // 4]),
    }


def q_exists(start, end, c0, c1):
    """The script reaches a window after the centromere (it raises at end of file otherwise)."""
    k = next((i for i, e in enumerate(end) if e >= c0), len(end))
    return any(start[i] >= c1 for i in range(k, len(end)))


def long_double_sums(lines, c0, c1):
    """The script's control flow and arithmetic (np.float128), returning its four sums."""
    tiny = np.float128(np.nextafter(0.0, 1.0))                  # the script's resolve(): 2^-1074, the smallest double
    res = lambda v: tiny if v == 0 else v
    rows = [l.split() for l in lines[1:] if l]
    vals = [(int(r[1]), int(r[2]), np.float128(r[3]), np.float128(r[4]), np.float128(r[5])) for r in rows]
    p20 = p10 = q20 = q10 = np.float128(0)
    if vals[0][1] > c0:
        p20 = p10 = np.float128(np.nan)
    i = 0
    while vals[i][1] < c0:
        p20 += np.log2(res(vals[i][4]) / res(vals[i][2]))
        p10 += np.log2(res(vals[i][3]) / res(vals[i][2]))
        i += 1
    while vals[i][0] < c1:
        i += 1
    for v in vals[i:]:
        q20 += np.log2(res(v[4]) / res(v[2]))
        q10 += np.log2(res(v[3]) / res(v[2]))
    return [p20, q20, p10, q10]


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found")
    mod = load_script()
    out = {"ranges": {}, "cases": {}}
    for tag, case in CASES:
        meta = json.load(open(os.path.join(HERE, tag, "cases.json")))
        args = meta["base_args"] + meta["cases"][case]
        d = os.path.join(HERE, tag, case)
        files = sorted(f for f in os.listdir(d) if f.endswith(".summary.txt.gz"))
        names = [f.split(".")[1] for f in files]
        # the comparison order of the run (-s list, or -S file order)
        if "-s" in args:
            order = args[args.index("-s") + 1].split(",")
        else:
            order = [l.strip() for l in open(os.path.join(HERE, tag, "input", args[args.index("-S") + 1])) if l.strip()]
        assert sorted(order) == sorted(names), (case, order, names)
        with gzip.open(os.path.join(HERE, tag, "input", "reads.pileup.gz"), "rt") as fh:
            chrom = args[args.index("-c") + 1] if "-c" in args else fh.readline().split()[0]
        wins = {ind: windows(read_summary(os.path.join(d, f"UNKWN.{ind}.summary.txt.gz"))) for ind in order}
        pilot = min(order, key=lambda ind: len(wins[ind][0]))      # (with -v every individual has windows of its own)
        rng = {k: v for k, v in ranges(*wins[pilot]).items() if v[0] <= v[1] and all(q_exists(*wins[i], *v) for i in order)}
        out["ranges"][f"{tag}/{case}"] = rng
        per = {}
        for rname, (c0, c1) in rng.items():
            lines_out = {}
            for ind in order:
                lines = read_summary(os.path.join(d, f"UNKWN.{ind}.summary.txt.gz"))
                with tempfile.TemporaryDirectory() as tmp:
                    sf = os.path.join(tmp, "s.txt")
                    with open(sf, "w") as fh:
                        fh.write("\n".join(lines) + "\n")
                    mod.hg19_centrmrs = {chrom: [c0, c1]}
                    try:
                        mod.get_chrarm_stats("hg19", {chrom: sf}, os.path.join(tmp, "o"))
                    except IndexError:
                        print(f"{tag}/{case} {rname} {ind}: the script ran past the last window", file=sys.stderr)
                        raise
                    printed = open(os.path.join(tmp, "o.txt")).read().splitlines()[1]
                sums = long_double_sums(lines, c0, c1)
                mine = "\t".join([chrom] + ["%.3e" % s for s in sums])
                assert mine == printed, (case, rname, ind, mine, printed)
                text = [np.format_float_scientific(v, unique=True) for v in sums]   # plain decimals: np.longdouble(text)
                assert all(np.longdouble(t) == v or (np.isnan(v) and t == "nan") for t, v in zip(text, sums)), text
                lines_out[ind] = {"line": printed, "sums": text}
            per[rname] = {"range": [c0, c1], "individuals": lines_out}
        out["cases"][f"{tag}/{case}"] = {"order": order, "chrom": chrom, "ranges": per}
    os.makedirs(os.path.join(HERE, "armstats"), exist_ok=True)
    with open(os.path.join(HERE, "armstats", "cases.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
