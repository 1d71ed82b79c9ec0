"""The route a context with no option set takes through the --LD kernels, restated from the inputs alone, for the 40 constructed
cases of depth_cases, gap_cases and bg_cases (numpy only: importable without a device).

The host program sets no option, so its single runs on one site list move through the forms by three host rules (ibdg_api.cpp):

  layout      sparse_sites at the upload: fewer than 1 covered row in 4 (compact_density) between the upload's first and last
              site -> the compacted tiles (ibdg_ld_layout 2) from run 1.  Otherwise relayout_when_paid: every single run adds 12
              to the upload's credit (mx_counts 1), and the run in which it reaches compact_targets = 256 -- the 22nd -- re-lays
              the list out before its launch.  A new upload starts over; another background does not.
  count unit  plan_run: the single runs on one upload AND background add up; from the ibd0_after-th (8th) on they take the
              IBD1 form (ibdg_last_count_unit 3), which the 8th makes the IBD0 pass for -- where the power tables are in LDS
              (depth_cases.tab_in_lds); otherwise every run counts everything (2).  The relayout drops the pass, not the count.
  window end  2 (the paired end, option pair_sums) where the unit is 3 and the 1 KiB of scratch per wave costs no workgroup
              per CU: min(4, 160 KiB / LDS bytes) with and without it, test_gpu_pair_sums.ibd1_lds_bytes over the layout's
              largest run (max_seg), windows per wave (16, halved while a run's records exceed record_lds_bytes = 12 KiB), the
              table length ct_max + 1 and rings of 2; else 1.

The runs are the host's guided ones (guided_runs 4, make_runs): remaining windows / workgroups in flight, at most 16, where the
workgroups in flight are n_cu * (16 / waves per chunk group) / chunk groups.  N_CU is the MI355X's 256; every case here has fewer
windows than workgroups in flight, so every run is ONE window -- test_route_cases.py asserts that, and that the window end
expected() gives does not depend on it: on the layouts a case's route takes, any run length from 1 to 16 gives the same one,
except for the cases of UNSURE_END.

expected(case, n_runs) never reads anything back from the engine; tests/test_gpu_default_route.py asserts it after every run.
"""
import functools

import numpy as np

import bg_cases as BC
import depth_cases as DC
import gap_cases as GC

N_CU = 256                  # compute units of an MI355X
IBD0_AFTER = 8              # ibdg_ctx::Options::ibd0_after
COMPACT_TARGETS = 256       # ... compact_targets
CREDIT_PER_RUN = 12         # relayout_when_paid: a single individual with mx_counts 1
COMPACT_DENSITY = 4         # ... compact_density
WINDOWS_PER_WAVE = 16       # ... wpg
RECORD_LDS_BYTES = 12 * 1024
RING_SLOTS = 2
GUIDED = 4

MODULES = {"depth": DC, "gap": GC, "bg": BC}
CASES = [(kind, name) for kind, mod in MODULES.items() for name in mod.NAMES]

# Cases whose window end the model does not pin down (assert only `end in (1, 2)` for them), with the reason.  At most 4.
# None today: on the layouts its route takes, every case has the same window end for every run length (test_route_cases.py).
UNSURE_END = ()


def make_case(kind, name):
    return MODULES[kind].make_case(name)


def covered(c):
    return np.flatnonzero(c["nr"].astype(np.int64) + c["na"] > 0)


def sparse(c):
    """sparse_sites (ibdg_api.cpp) for the np.arange(L) upload every test makes: the sites span the whole panel."""
    first_row, last_row = 0, len(c["nr"]) - 1
    return len(covered(c)) * COMPACT_DENSITY < last_row - first_row + 1


def guided_run_begins(n_win, g, n_chunks, n_cu=N_CU, guided=GUIDED):
    """make_runs (ibdg_api.cpp): runs of min(g, ceil(remaining windows / workgroups in flight)) windows."""
    n_cg = (n_chunks + 7) // 8
    waves = (n_chunks + n_cg - 1) // n_cg
    in_flight = max(1, n_cu * (16 // waves) // n_cg * max(1, guided) // 4)
    begins, w = [], 0
    while w < n_win:
        begins.append(w)
        w = min(w + min(g, max(1, (n_win - w + in_flight - 1) // in_flight)), n_win)
    return np.array(begins + [n_win], dtype=np.int64)


def max_seg(c, layout, begins):
    """The most (window, tile) segments in one run: on the panel's own tiles (layout 1) or the compacted ones (2: the windows'
    rows back to back, compact_align 1)."""
    seg = DC.segments(c["nr"], c["na"], c["W"], win_rows=c["W"] if layout == 2 else 0)
    return int(np.diff(np.searchsorted(seg["win"], begins, side="left")).max())


def n_windows(c):
    return -(-len(covered(c)) // c["W"])


def ibd1_lds_bytes(max_seg, win_per_group, tab_len, ring_slots, scratch):
    """As test_gpu_pair_sums.ibd1_lds_bytes (ld_lds_layout, ibdg_ld_layout.h), restated so that this module needs no device;
    test_route_cases.py holds the two against each other."""
    head = (max_seg * 32 + win_per_group * 8) * 4 + 15
    ring = (head + tab_len * 2 * 8 + 1023) & ~1023
    return ring + 8 * ring_slots * 1024 + (8 * 1024 if scratch else 0)


def paired_end(c, layout, run_len=None):
    """True where plan_run takes the paired window end for an IBD1 run on `layout`.  run_len: uniform runs of that many windows
    instead of the host's guided ones (the sensitivity check of test_route_cases.py)."""
    n_win, n_chunks = n_windows(c), (c["n_ids"] + 63) // 64
    g = WINDOWS_PER_WAVE
    while True:     # cut_segments: the run length halved until a run's records fit the budget
        begins = guided_run_begins(n_win, g, n_chunks) if run_len is None else GC.run_begins(n_win, min(g, run_len))
        m = max_seg(c, layout, begins)
        if m * GC.SEG_BYTES <= RECORD_LDS_BYTES or g == 1:
            break
        g = (g + 1) // 2
    tab_len = DC.ct_max(c["nr"], c["na"], c["W"]) + 1
    per_cu = [min(4, 160 * 1024 // ibd1_lds_bytes(m, g, tab_len, RING_SLOTS, s)) for s in (False, True)]
    return per_cu[0] == per_cu[1]


@functools.lru_cache(maxsize=None)
def _facts(kind, name):
    c = make_case(kind, name)
    in_lds = DC.tab_in_lds(c["nr"], c["na"], c["W"])
    return sparse(c), in_lds, {lay: in_lds and paired_end(c, lay) for lay in (1, 2)}


def expected(case, n_runs, *, ibd0_after=IBD0_AFTER, compact_targets=COMPACT_TARGETS, first_credit=0):
    """[(ibdg_ld_layout, ibdg_last_count_unit, ibdg_last_window_end)] for single runs 1..n_runs of a default context on one
    upload and one background of `case` = (kind, name).  first_credit: what earlier runs on the same upload (other backgrounds)
    have added to the relayout's credit."""
    is_sparse, in_lds, paired = _facts(*case)
    out, credit = [], first_credit
    for k in range(1, n_runs + 1):
        credit += CREDIT_PER_RUN
        layout = 2 if is_sparse or credit >= compact_targets else 1
        unit = 3 if in_lds and k >= ibd0_after else 2
        out.append((layout, unit, 2 if unit == 3 and paired[layout] else 1))
    return out


# --------------------------------------------------------------------------- the read patterns of test_gpu_default_route.py
N_RUNS = 24                                             # 22 reach the relayout, two more run behind it
READS_A = tuple(range(1, N_RUNS + 1))                   # pattern A: every run is read (1-based)
READS_B = tuple(range(3, N_RUNS + 1, 3))                # pattern B: runs 3, 6, ..., 24


def cycle(people, n_runs=N_RUNS):
    """The individual of every run: `people` in turn."""
    return [people[k % len(people)] for k in range(n_runs)]
