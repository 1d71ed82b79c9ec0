"""Golden files of `ibdgem --states` and `hiddengem --summary-list` (tests/golden/states), produced by RUNNING the
unmodified reference programs on the development machine: oracle/_ref/hiddengem (built by `make -C oracle ref`) and
the reference checkout's bin/sum-hiddengem.py (REFERENCE_DIR, default /root/reference; needs pandas).  Only what they
print is written:

  fixture/<set>/<pileup>.<individual>.hiddengem.txt   reference hiddengem on the summary files this project's ibdgem
                                                      writes for the reference's fixture (no device: non-LD), with
                                                      the penalties of <set> (states.json)
  fixture/<set>/<pileup>.fractions.txt                sum-hiddengem.py over those, one line per individual
  lists/<list>.fractions.txt                          sum-hiddengem.py over the committed tests/golden/hidden/*.out of
                                                      the cases of <list> (states.json)

Every table has at most 12288 windows, the reference binary's fixed array size (asserted here).

    python tests/golden/make_golden_states.py
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(REPO, "oracle", "_ref", "hiddengem")
SCRIPT = os.path.join(os.environ.get("REFERENCE_DIR", "/root/reference"), "bin", "sum-hiddengem.py")
IBDGEM = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
OUT = os.path.join(HERE, "states")
MAX_WINDOWS = 12288

SETS = {"default": [], "pen": ["--p01", "0.5", "--p02", "0.25", "--p12", "0.9"]}
PILEUPS = ["sample1", "sample2", "sample3"]
INDIVIDUALS = ["sample1", "sample2", "sample3"]


def n_windows(path):
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as fh:
        return sum(1 for l in fh if l.strip() and not l.startswith("#"))


def fractions(entries, out_fn, tmp):
    """sum-hiddengem.py -i LIST -o out_fn over (name, path of a hiddengem table)"""
    lst = os.path.join(tmp, "list.txt")
    with open(lst, "w") as fh:
        for name, path in entries:
            fh.write(f"{name}\t{path}\n")
    subprocess.run([sys.executable, SCRIPT, "-i", lst, "-o", out_fn], check=True)


def main():
    assert os.path.exists(REF), "run `make -C oracle ref` first"
    assert os.path.exists(SCRIPT), SCRIPT
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(os.path.join(OUT, "lists"))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", IBDGEM_KEEP_TEARDOWN="1")
    fix_in = os.path.join(HERE, "ibdgem-test", "input")
    with tempfile.TemporaryDirectory() as tmp:
        for k, pu in enumerate(PILEUPS):
            subprocess.run([IBDGEM, "-H", "test.hap", "-L", "test.legend", "-I", "test.indv", "-P", f"test{k + 1}.pileup", "-N", pu,
                            "-O", tmp], cwd=fix_in, env=env, check=True, capture_output=True)
        for sname, pen in SETS.items():
            d = os.path.join(OUT, "fixture", sname)
            os.makedirs(d)
            for pu in PILEUPS:
                entries = []
                for ind in INDIVIDUALS:
                    summ = os.path.join(tmp, f"{pu}.{ind}.summary.txt")
                    assert n_windows(summ) <= MAX_WINDOWS
                    res = subprocess.run([REF, "-s", summ] + pen, check=True, capture_output=True)
                    fn = os.path.join(d, f"{pu}.{ind}.hiddengem.txt")
                    with open(fn, "wb") as fh:
                        fh.write(res.stdout)
                    entries.append((ind, fn))
                fractions(entries, os.path.join(d, f"{pu}.fractions.txt"), tmp)
        with open(os.path.join(HERE, "hidden", "cases.json")) as fh:
            cases = json.load(fh)
        lists = {"default35": [c["name"] for c in cases if not c["args"]]}
        for c in cases:
            assert n_windows(os.path.join(HERE, c["input"])) <= MAX_WINDOWS
            if c["args"]:
                lists[c["name"]] = [c["name"]]
        assert len(lists["default35"]) == 35 and len(lists) == 5
        for lname, names in lists.items():
            fractions([(n, os.path.join(HERE, "hidden", n + ".out")) for n in names],
                      os.path.join(OUT, "lists", lname + ".fractions.txt"), tmp)
    with open(os.path.join(OUT, "states.json"), "w") as fh:
        json.dump({"sets": SETS, "pileups": PILEUPS, "individuals": INDIVIDUALS, "lists": lists}, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
