"""GPU tier: k_log2_posteriors (ibdg_window_log2_posteriors) against its host twin bit for bit, on the run's own log tables
and the shapes of tests/test_gpu_log_states_trips.py; once against the exact truth of tests/hp_post_ref.py, so that the tier
does not rest on the twin alone; and the host program's routes with --posteriors."""
import os
import subprocess

import numpy as np
import pytest

import armstats_check as A
import hp_post_ref as H
import log_states_util as U
from ibdgem_amd import engine as E
from test_gpu_log_states_trips import engine, states_launch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ibdgem_amd", "host", "ibdgem")
SMALL = (0.5, 0.25, 0.5)


def device_equals_twin(eng, T, pen=U.PEN, what=""):
    """post, expect and log2_z of the last run, device against twin on the same tables, bit for bit; the same expect and
    log2_z when post is not asked for; the same bytes from a second call.  Returns (tables, post, expect, log2_z)."""
    tabs = eng.window_log2_all(T)
    post, expect, log2_z = eng.window_log2_posteriors(*pen)
    n = eng.n_windows
    assert post.shape == (T, n, 3) and expect.shape == (T, 3) and log2_z.shape == (T,)
    for t in range(T):
        wp, we, wz = E.log2_posteriors_host(tabs[t], *pen)
        assert post[t].tobytes() == wp.tobytes(), f"{what}: posteriors of individual {t}"
        assert expect[t].tobytes() == we.tobytes(), f"{what}: expectations of individual {t}"
        assert np.float64(log2_z[t]).tobytes() == np.float64(wz).tobytes(), f"{what}: log2 Z of individual {t}"
    assert np.isfinite(post).all() and (np.abs(post.sum(axis=2) - 1.0) <= 4 * 2.0 ** -53).all()
    p2, e2, z2 = eng.window_log2_posteriors(*pen, want_post=False)
    assert p2 is None and e2.tobytes() == expect.tobytes() and z2.tobytes() == log2_z.tobytes()
    p3, e3, z3 = eng.window_log2_posteriors(*pen)
    assert p3.tobytes() == post.tobytes() and e3.tobytes() == expect.tobytes() and z3.tobytes() == log2_z.tobytes()
    return tabs, post, expect, log2_z


def test_past_the_block_cap():
    """1100 individuals (of 40, repeated) for 1024 workgroups: 76 workgroups take a second individual and reuse their LDS."""
    N, T, n_win = 40, 1100, 5
    alle, nr, na = U.covered_reads(5, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win
        assert states_launch(T, n_win) == dict(C=1, owners=5, last=1, trips=2)
        eng.run([t % N for t in range(T)], ld=False)
        _, post, expect, log2_z = device_equals_twin(eng, T, what="past the block cap")
        assert post[1024:].tobytes() == post[1024 % N:1024 % N + 76].tobytes()
        assert expect[1024:].tobytes() == expect[1024 % N:1024 % N + 76].tobytes()
        assert log2_z[1024:].tobytes() == log2_z[1024 % N:1024 % N + 76].tobytes()
        assert len({p.tobytes() for p in post}) > 1


@pytest.mark.parametrize("ld", [False, True])
@pytest.mark.parametrize("n_win,shape", [(601, dict(C=3, owners=201, last=1, trips=1)),
                                         (1279, dict(C=5, owners=256, last=4, trips=1)),
                                         (100, dict(C=1, owners=100, last=1, trips=1))])
def test_block_shapes(n_win, shape, ld):
    N, T = 30, 9
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    with engine(alle, nr, na, 2) as eng:
        assert eng.n_windows == n_win and states_launch(T, n_win) == shape
        eng.run(list(range(3, 3 + T)), ld=ld)
        device_equals_twin(eng, T, what=f"{n_win} windows")
        _, post, _, _ = device_equals_twin(eng, T, pen=SMALL, what=f"{n_win} windows, small penalties")
        # with penalties of about a bit no state owns the table: the posteriors are not all 0 and 1
        assert ((post > 0.01) & (post < 0.99)).any()


def test_device_against_the_exact_truth():
    """601 windows (C = 3, a last block of one window), two individuals, both penalty sets: the device's own outputs within
    the counted bar of hp_post_ref (R = 14) of the exact forward-backward."""
    N, T, n_win = 30, 2, 601
    alle, nr, na = U.covered_reads(n_win, 2 * n_win, N)
    assert H.Rn(n_win) * 2.0 ** -53 <= 1e-10
    with engine(alle, nr, na, 2) as eng:
        eng.run([4, 11], ld=False)
        tabs = eng.window_log2_all(T)
        for pen in (U.PEN, SMALL):
            post, expect, log2_z = eng.window_log2_posteriors(*pen)
            for t in range(T):
                _, worst = H.check(tabs[t], pen, post[t].tolist(), expect[t].tolist(), float(log2_z[t]))
                print(f"device, 601 windows, penalties {pen}, individual {t}: largest error / bar {worst:.3g}")


def test_errors():
    alle, nr, na = U.covered_reads(3, 40, 20)
    with engine(alle, nr, na, 2) as eng:
        with pytest.raises(E.EngineError, match="ibdg_window_log2_posteriors: no results"):
            eng.window_log2_posteriors(*U.PEN)
        eng.run([1, 2], ld=False)
        for pen in ((0.0, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, float("nan")), (-1.0, 0.5, 0.5)):
            with pytest.raises(E.EngineError, match=r"ibdg_window_log2_posteriors: p\d\d = .* is not in \(0, 1\]"):
                eng.window_log2_posteriors(*pen)
        e, z = np.zeros((2, 3)), np.zeros(2)
        assert eng.lib.ibdg_window_log2_posteriors(eng.ctx, 0.5, 0.5, 0.5, None, None, z.ctypes.data) != 0
        assert eng.lib.ibdg_window_log2_posteriors(eng.ctx, 0.5, 0.5, 0.5, None, e.ctypes.data, None) != 0
        device_equals_twin(eng, 2)
        eng.set_option("log_windows", 0)
        eng.run([1, 2], ld=False)
        with pytest.raises(E.EngineError, match="option log_windows"):
            eng.window_log2_posteriors(*U.PEN)


# ---- the host program --------------------------------------------------------------------------------------------------

def _run(args, cwd, out):
    os.makedirs(out, exist_ok=True)
    res = subprocess.run([EXE] + args + ["-O", str(out)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))}


@pytest.mark.parametrize("key", ["synA/ld_default", "synA/ld_varsites", "synA/nonld_all_targets_w2", "synB/ld_w37"])
def test_cli_every_route_gives_the_same_bytes(key, tmp_path):
    """The routes of test_gpu_log_states.py with --posteriors: one context and --stats-only computes on the device and 40
    bytes per individual leave it; two contexts, or files per individual, run the twin on the gathered tables."""
    args, inp = A.run_args(key)
    c0, c1 = A.golden()["cases"][key]["ranges"]["both"]["range"]
    stats = ["--log-stats", "--states", "--arm-stats", f"{c0},{c1}", "--p01", "0.05", "--p02", "0.01", "--p12", "0.05"]
    post = stats + ["--posteriors"]
    full = {d: _run(args + post + ["--summary-only", "--devices", d], inp, tmp_path / f"full{len(d)}") for d in ("0", "0,0")}
    only = {d: _run(args + post + ["--stats-only", "--devices", d], inp, tmp_path / f"only{len(d)}") for d in ("0", "0,0")}
    run_files = ["UNKWN.logarmstats.txt", "UNKWN.logibdposteriors.txt", "UNKWN.logibdstates.txt"]
    assert sorted(only["0"]) == sorted(only["0,0"]) == run_files
    assert sorted(full["0"]) == sorted(full["0,0"])
    per = [fn for fn in full["0"] if fn.endswith(".logposteriors.txt")]
    assert len(per) >= 2 and len(per) == len([fn for fn in full["0"] if fn.endswith(".loghiddengem.txt")])
    for fn in run_files + per:
        assert full["0"][fn] == full["0,0"][fn], fn
    for fn in run_files:
        assert only["0"][fn] == full["0"][fn] == only["0,0"][fn], fn
    # the expectations of logibdposteriors.txt are the sums of the logposteriors files (6 decimals a window)
    rows = {l.split("\t")[0]: l.split("\t") for l in full["0"]["UNKWN.logibdposteriors.txt"].decode().splitlines() if not l.startswith("#")}
    for fn in per:
        g = np.array([[float(x) for x in l.split("\t")[1:4]] for l in full["0"][fn].decode().splitlines()[1:]])
        row = rows[fn.split(".")[1]]
        assert int(row[1]) == len(g)
        assert (np.abs(g.sum(axis=0) - [float(x) for x in row[2:5]]) <= 0.5e-6 * len(g) + 0.5e-3).all(), fn
    # every file the run writes without the option is unchanged
    plain = _run(args + stats + ["--summary-only"], inp, tmp_path / "plain")
    assert sorted(plain) == sorted(fn for fn in full["0"] if fn not in per and fn != "UNKWN.logibdposteriors.txt")
    for fn, data in plain.items():
        assert full["0"][fn] == data, fn
