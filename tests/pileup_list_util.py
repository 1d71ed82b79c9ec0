"""Helpers of the --pileup-list tests: pileup variants of a golden case and the single runs they must equal."""
import gzip
import os
import random
import subprocess

import golden_io as G


def thinned_pileups(tag, out_dir, n, seed=7):
    """`n` pileups of a synthetic case's reads.pileup.gz: the file itself first, then copies with 10-30 % of the lines
    dropped (every other one gzip-compressed); returns absolute paths."""
    src = os.path.join(G.GOLD, tag, "input", "reads.pileup.gz")
    lines = gzip.open(src, "rt").read().splitlines(keepends=True)
    paths = [src]
    for k in range(1, n):
        rng = random.Random(seed * 1000 + k)
        drop = 0.1 + 0.1 * (k % 3)
        kept = [l for l in lines if rng.random() >= drop]
        fn = os.path.join(str(out_dir), f"{tag}_v{k}.pileup" + (".gz" if k % 2 else ""))
        with (gzip.open(fn, "wt") if k % 2 else open(fn, "w")) as fh:
            fh.writelines(kept)
        paths.append(fn)
    return paths


def write_list(fn, entries):
    with open(fn, "w") as fh:
        fh.write("# NAME PATH\n")
        for name, path in entries:
            fh.write(f"{name}\t{path}\n")
    return str(fn)


def strip_pileup_args(args):
    """a case's arguments without -P / -N and their values"""
    out, skip = [], False
    for a in args:
        if skip:
            skip = False
            continue
        if a in ("-P", "-N"):
            skip = True
            continue
        out.append(a)
    return out


def run(exe, args, cwd, env=None, timeout=600):
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=timeout)


def output_files(d):
    """{file name: bytes} of an output directory, the tab files without their first line (the echoed command)"""
    out = {}
    for fn in sorted(os.listdir(d)):
        data = open(os.path.join(d, fn), "rb").read()
        if fn.endswith(".tab.txt"):
            assert data.startswith(b"# Entered command: "), fn
            data = data.split(b"\n", 1)[1] if b"\n" in data else b""
        out[fn] = data
    return out
