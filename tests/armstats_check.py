"""Checks of an *.armstats.txt file (ibdgem --arm-stats) against tests/golden/armstats/cases.json, the lines the
reference's bin/chrarm-stats.py printed for the committed 17-digit summaries (make_golden_armstats.py).

A number must equal the script's text, except where the script's long-double sum lies within the error bound of a
%.3e rounding boundary: then the two sides may round apart, and the check shows that they are that close."""
import json
import os

import numpy as np

import golden_io as G

HEADER = "SAMPLE\tCHROM\tparm_IBD2/IBD0\tqarm_IBD2/IBD0\tparm_IBD1/IBD0\tqarm_IBD1/IBD0"


def golden():
    with open(os.path.join(G.GOLD, "armstats", "cases.json")) as fh:
        return json.load(fh)


def run_args(key):
    tag, case = key.split("/")
    meta = G.cases(tag)
    return meta["base_args"] + meta["cases"][case], os.path.join(G.GOLD, tag, "input")


def read_armstats(path):
    with open(path) as fh:
        lines = fh.read().splitlines()
    assert lines[0] == HEADER
    return [l.split("\t") for l in lines[1:]]


def _bound(key, ind):
    """2^-48 per unit of sum(|log2 L2'| + |log2 L1'| + 2 |log2 L0'| + 1) over the individual's windows: fp64 logs, the
    17-digit text the script read and the --LD sums' ~1e-15 agreement with the reference, with room to spare."""
    tag, case = key.split("/")
    rows = [l.split() for l in G.read_lines(os.path.join(G.GOLD, tag, case, f"UNKWN.{ind}.summary.txt.gz"))[1:] if l]
    v = np.array([[float(x) for x in r[3:6]] for r in rows]).reshape(-1, 3)
    v = np.where(v == 0, 2.0 ** -1074, v)
    with np.errstate(invalid="ignore"):
        lg = np.abs(np.log2(v))
    tot = np.nansum(lg[:, 0] * 2 + lg[:, 1] + lg[:, 2] + 1)
    return float(tot) * 2.0 ** -48


def check(got_rows, key, rname):
    """got_rows: the parsed lines of one run's armstats file.  Returns the number of values that rounded apart from the
    script's text at a rounding boundary (each one checked to lie within the bound)."""
    g = golden()["cases"][key]
    entry = g["ranges"][rname]["individuals"]
    assert [r[0] for r in got_rows] == g["order"]
    near = 0
    for row in got_rows:
        want = entry[row[0]]
        wf = want["line"].split("\t")
        assert row[1] == wf[0] == g["chrom"]
        b = _bound(key, row[0])
        for k in range(4):
            near += check_value(row[2 + k], wf[1 + k], want["sums"][k], b, f"{key} {rname} {row[0]} column {k}")
    return near


def check_value(got, want, sum_text, bound, where=""):
    """One number: `got` must be the script's text `want`, unless the script's long-double sum (`sum_text`, a plain
    decimal) lies within `bound` of a %.3e rounding boundary -- then `got` may be the neighbouring rounding, and must
    lie within the bound of the sum.  Returns 1 in that case, 0 when the texts agree."""
    if got == want:
        return 0
    assert "nan" not in (got, want), (where, got, want)
    v = np.longdouble(sum_text)
    lo, hi = "%.3e" % float(v - np.longdouble(bound)), "%.3e" % float(v + np.longdouble(bound))
    assert lo != hi, f"{where}: {got} vs {want} and no %.3e boundary within {bound:.3g} of {sum_text}"
    assert got in (lo, hi), f"{where}: {got} is neither rounding within {bound:.3g} of {sum_text} ({lo}, {hi})"
    return 1
