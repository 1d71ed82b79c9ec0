"""Two builds of the host program on the committed fixture: same exit code, same stderr with the clock values stripped
(so the same messages and the same sequence of IBDGEM_TIMING phase names), same output files byte for byte (the tables'
"# Entered command" line apart: it names the program).  For refactors of ibdgem.c that must not change behaviour.
    python tools/host_ab_compare.py PARENT_EXE NEW_EXE [--no-device] [--ld]
--no-device hides the GPUs (the host's own non-LD path); --ld adds --LD to every run (needs a device)."""
import os, re, shutil, subprocess, sys, tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(REPO, "tests", "golden", "ibdgem-test", "input")
PANEL = ["-H", "test.hap", "-L", "test.legend", "-I", "test.indv"]
ONE = PANEL + ["-P", "test1.pileup", "-N", "sample1"]
RUNS = {
    "plain": ONE,
    "one individual": ONE + ["-s", "sample2"],
    "summary-only, several -s": ONE + ["--summary-only", "-s", "sample1,sample2,sample3"],
    "-v": ONE + ["-v"],
    "-v, host scan": ONE + ["-v"],
    "-D": ONE + ["-D", "1"],
    "pileup-list": PANEL + ["--pileup-list", "LIST"],
    "pileup-list, -v, states": PANEL + ["--pileup-list", "LIST", "-v", "--states", "--log-summary"],
    "arm-stats, stats-only": ONE + ["--arm-stats", "10,20", "--stats-only"],
    "arm-stats": ONE + ["--arm-stats", "10,20"],
    "states": ONE + ["--states"],
    "states, stats-only, arm-stats": ONE + ["--states", "--stats-only", "--arm-stats", "10,20"],
    "log-summary": ONE + ["--log-summary"],
    "several contexts": ONE + ["--devices", "0,0,0", "--arm-stats", "10,20"],
    "plan": ONE + ["--plan"],
    "no output directory": ONE + ["--states", "--log-summary"],
    # a file of the second individual cannot be opened (a directory has its name) while the first one's are being written
    "summary blocked": ONE + ["--states", "--log-summary"],
    "logsummary blocked": ONE + ["--states", "--log-summary"],
    "hiddengem blocked": ONE + ["--states", "--log-summary", "--summary-only"],
    "hiddengem blocked in a list": PANEL + ["--pileup-list", "LIST", "--states"],
}


def strip(text):
    """messages in order, then every pileup's phase names in order (a list's pileups are read beside one another)"""
    text = re.sub(r"(?m)^Run time: .*$", "Run time:", text)
    lines, phases = [], {}
    for l in text.splitlines():
        m = re.match(r"## time (\[\S+\] )?(.*) \S+$", l)
        if m:
            phases.setdefault(m.group(1) or "", []).append(m.group(2))
        else:
            lines.append(l)
    return "\n".join(lines + [f"## time {tag}{name}" for tag in sorted(phases) for name in phases[tag]])


def run(exe, name, args, env):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "o")
        if name != "no output directory":
            os.makedirs(out)
        if "blocked" in name:
            os.makedirs(os.path.join(out, f"sample1.sample2.{name.split()[0]}.txt"))
        lst = os.path.join(d, "list.txt")
        with open(lst, "w") as fh:
            fh.write("".join(f"sample{k} test{k}.pileup\n" for k in (1, 2, 3)))
        args = [lst if a == "LIST" else a for a in args] + ["-O", out]
        if name == "-v, host scan":
            env = dict(env, IBDGEM_VARSITES="host")
        r = subprocess.run([exe] + args, cwd=FIX, env=env, capture_output=True, text=True, timeout=300)
        files = {}
        for fn in sorted(os.listdir(out)) if os.path.isdir(out) else []:
            data = open(os.path.join(out, fn), "rb").read() if os.path.isfile(os.path.join(out, fn)) else b"(directory)"
            if data.startswith(b"# Entered command"):
                data = data.split(b"\n", 1)[1]
            files[fn] = data
        return r.returncode, strip(r.stderr).replace(d, "TMP"), r.stdout.replace(d, "TMP"), files


def main():
    exes = [a for a in sys.argv[1:] if not a.startswith("--")]
    env = dict(os.environ, IBDGEM_TIMING="1", IBDGEM_KEEP_TEARDOWN="1")
    if "--no-device" in sys.argv:
        env.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    bad = 0
    for name, args in RUNS.items():
        if "--no-device" in sys.argv and "--devices" in args:
            continue
        if "--ld" in sys.argv and "--plan" not in args:
            args = args + ["--LD"]
        a, b = (run(os.path.abspath(e), name, args, env) for e in exes)
        phases = [l for l in a[1].splitlines() if l.startswith("## time")]
        same = a == b
        bad += not same
        print(f"{'same' if same else 'DIFFERENT'}: {name}: exit {a[0]}, {len(phases)} phase lines, {len(a[3])} files", flush=True)
        if not same:
            for what, x, y in zip(("exit code", "stderr", "stdout", "files"), a, b):
                if x != y:
                    print(f"  {what} differ" + (f":\n--- parent\n{x[-1500:]}\n--- new\n{y[-1500:]}" if what == "stderr" else ""))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
