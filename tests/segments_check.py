"""What the tests of --segments share (test_segments_cli.py, test_gpu_log_segments.py): the files of one individual against
each other, and the run's logibdsegments.txt against the individuals' logsegments.txt."""
import itertools
from fractions import Fraction

HEADER = ("Segment\tState\tFirst_Window\tLast_Window\tStart\tEnd\tLength\tNum_Windows\tNum_Sites\tIBD0_LogSum\tIBD1_LogSum\t"
          "IBD2_LogSum\tLog2_LR")
POST = "\tPost_Mean\tPost_Min"
RUN_HEADER = "# ID" + "".join(f"\tIBD{s}_{c}" for s in range(3) for c in ("N_SEG", "LONGEST_WIN", "TOTAL_BP", "LONGEST_BP"))


def rows_of(data):
    """(header, rows as lists of strings) of a logsegments.txt"""
    lines = data.decode().splitlines()
    return lines[0], [l.split("\t") for l in lines[1:]]


def individual_consistent(segments, hiddengem, summary, with_post, what=""):
    """A logsegments.txt against the same individual's loghiddengem.txt (its path column, run-length-encoded here) and
    summary.txt (START, END, NUM_SITES).  Returns the 12 numbers of the individual's line of logibdsegments.txt."""
    head, rows = rows_of(segments)
    assert head == HEADER + (POST if with_post else ""), what
    path = [int(l.split("\t")[4]) for l in hiddengem.decode().splitlines()[1:] if not l.startswith("#")]
    summ = [l.split("\t") for l in summary.decode().splitlines() if not l.startswith("#")]
    assert len(summ) == len(path), what
    runs = [(s, len(list(g))) for s, g in itertools.groupby(path)]
    assert len(rows) == len(runs), what
    line, f = [0] * 12, 0
    for k, (row, (s, n)) in enumerate(zip(rows, runs)):
        assert len(row) == 13 + 2 * with_post, what
        assert [int(x) for x in row[:4]] == [k + 1, s, f + 1, f + n], (what, k)
        start, end = int(summ[f][1]), int(summ[f + n - 1][2])
        assert [int(x) for x in row[4:9]] == [start, end, end - start + 1, n, sum(int(summ[w][6]) for w in range(f, f + n))], (what, k)
        sums = [Fraction(x) for x in row[9:12]]
        assert max(sums) <= 0, (what, k)
        # Log2_LR is the state's sum less the larger of the others (each printed with 4 decimals: half a unit of the last each)
        lr = sums[s] - max(sums[(s + 1) % 3], sums[(s + 2) % 3])
        assert abs(Fraction(row[12]) - lr) <= Fraction(3, 20000), (what, k)
        if with_post:
            mean, mn = float(row[13]), float(row[14])
            assert 0.0 <= mn <= mean + 1e-6 and mean <= 1.0, (what, k)
        line[s] += 1
        line[3 + s] = max(line[3 + s], n)
        line[6 + s] += end - start + 1
        line[9 + s] = max(line[9 + s], end - start + 1)
        f += n
    assert f == len(path), what
    return line


def run_consistent(run_file, lines):
    """logibdsegments.txt against {individual: the 12 numbers of individual_consistent}, in the file's order; and its totals."""
    text = run_file.decode().splitlines()
    assert text[0] == RUN_HEADER
    body = [l.split("\t") for l in text[1:] if not l.startswith("#")]
    assert [r[0] for r in body] == list(lines)
    total = [0] * 12
    for r in body:
        want = lines[r[0]]
        # the file goes state by state, the summary group by group
        assert [int(x) for x in r[1:]] == [want[3 * k + s] for s in range(3) for k in range(4)], r[0]
        for i in range(12):
            total[i] = max(total[i], want[i]) if (i // 3) & 1 else total[i] + want[i]
    assert text[1 + len(body):] == [f"# Total IBD{s}: N_SEG = {total[s]}, LONGEST_WIN = {total[3 + s]}, TOTAL_BP = {total[6 + s]}, "
                                    f"LONGEST_BP = {total[9 + s]}" for s in range(3)]
