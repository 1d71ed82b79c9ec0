"""ctypes binding of include/ibdgem_hip.h (one class per ibdg_ctx).

Mirrors the C ABI one-to-one; no arithmetic happens here.  If
libibdgem_hip.so is missing or a call fails, an EngineError is raised -- there
is no fallback path.
"""
import ctypes as C
import os

import numpy as np

# IBDG_LIB: another build of the same ABI (used to A/B kernel variants on one box)
LIB_PATH = os.environ.get("IBDG_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libibdgem_hip.so")

# every symbol include/ibdgem_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "ibdg_abi_version": (C.c_int, []),
    "ibdg_device_count": (C.c_int, []),
    "ibdg_create": (_P, [C.c_int, C.c_double, C.c_uint]),
    "ibdg_destroy": (None, [_P]),
    "ibdg_last_error": (C.c_char_p, [_P]),
    "ibdg_pdg_table": (C.c_int, [C.c_double, C.c_uint, _P]),
    "ibdg_pdg_ibd0": (C.c_double, [C.c_double] * 4),
    "ibdg_pdg_ibd1": (C.c_double, [C.c_uint, C.c_uint] + [C.c_double] * 4),
    "ibdg_row_words": (C.c_size_t, [C.c_uint]),
    "ibdg_pack_alleles": (None, [_P, C.c_uint, _P]),
    "ibdg_pack_hap_text": (C.c_int, [C.c_char_p, C.c_uint, _P]),
    "ibdg_upload_panel": (C.c_int, [_P, _P, C.c_size_t, C.c_uint]),
    "ibdg_upload_panel_dev": (C.c_int, [_P, _P, C.c_size_t, C.c_uint]),
    "ibdg_upload_sites": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint]),
    "ibdg_upload_sites_dev": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint]),
    "ibdg_upload_candidates": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t]),
    "ibdg_num_candidates": (C.c_size_t, [_P]),
    "ibdg_select_variable_sites": (C.c_int, [_P, C.c_uint32, C.c_uint]),
    "ibdg_get_site_candidates": (C.c_int, [_P, _P]),
    "ibdg_upload_ms": (C.c_int, [_P, _P]),
    "ibdg_host_alloc": (_P, [C.c_size_t]),
    "ibdg_host_free": (None, [_P]),
    "ibdg_num_sites": (C.c_size_t, [_P]),
    "ibdg_num_windows": (C.c_size_t, [_P]),
    "ibdg_num_targets": (C.c_size_t, [_P]),
    "ibdg_upload_panel_fd": (C.c_int, [_P, C.c_int, C.c_uint64, C.c_size_t, C.c_uint]),
    "ibdg_get_windows": (C.c_int, [_P, _P, _P, _P]),
    "ibdg_run": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_int, C.c_int]),
    "ibdg_get_site_af": (C.c_int, [_P, _P]),
    "ibdg_get_site_ll": (C.c_int, [_P, C.c_size_t, _P]),
    "ibdg_get_window_ll": (C.c_int, [_P, C.c_size_t, _P]),
    "ibdg_get_window_ll_all": (C.c_int, [_P, _P]),
    "ibdg_get_window_log2": (C.c_int, [_P, C.c_size_t, _P]),
    "ibdg_get_window_log2_all": (C.c_int, [_P, _P]),
    "ibdg_set_window_log2": (C.c_int, [_P, _P, C.c_size_t]),
    "ibdg_window_llr_sums": (C.c_int, [_P, _P, _P, C.c_size_t, _P]),
    "ibdg_window_log2_llr_sums": (C.c_int, [_P, _P, _P, C.c_size_t, _P]),
    "ibdg_log2_states_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, _P, _P, _P]),
    "ibdg_window_log2_states": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, _P, _P, _P]),
    "ibdg_log2_posteriors_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, _P, _P, _P]),
    "ibdg_window_log2_posteriors": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, _P, _P, _P]),
    "ibdg_log2_segments_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, C.c_int, _P, _P, _P, C.c_size_t,
                                          _P, _P]),
    "ibdg_window_log2_segments": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, C.c_int, _P, _P, _P, _P]),
    "ibdg_get_log2_segments": (C.c_int, [_P, _P, C.c_size_t]),
    "ibdg_log2_states_chains_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, C.c_size_t]),
    "ibdg_log2_posteriors_chains_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P,
                                                   C.c_size_t]),
    "ibdg_log2_segments_chains_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, C.c_int, _P, _P, _P,
                                                 C.c_size_t, _P, _P, _P, C.c_size_t]),
    "ibdg_set_window_chains": (C.c_int, [_P, _P, C.c_size_t]),
    "ibdg_num_window_chains": (C.c_size_t, [_P]),
    "ibdg_log2_states_steps_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, C.c_size_t, _P]),
    "ibdg_log2_posteriors_steps_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P,
                                                  C.c_size_t, _P]),
    "ibdg_log2_segments_steps_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, C.c_int, _P, _P, _P,
                                                C.c_size_t, _P, _P, _P, C.c_size_t, _P]),
    "ibdg_set_window_steps": (C.c_int, [_P, _P, C.c_size_t]),
    "ibdg_has_window_steps": (C.c_int, [_P]),
    "ibdg_log2_samples_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, _P, C.c_size_t, _P, C.c_size_t,
                                         C.c_uint64, C.c_uint64, _P, _P, _P, _P]),
    "ibdg_window_log2_samples": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, C.c_size_t, C.c_uint64, _P, _P, _P, _P]),
    "ibdg_get_log2_sample_path": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P]),
    "ibdg_log2_switches_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_double, C.c_double, _P, C.c_size_t, _P, _P, _P, _P]),
    "ibdg_window_log2_switches": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, _P, _P]),
    "ibdg_window_log2_switches_prior": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, _P, _P]),
    "ibdg_switch_penalty_update": (C.c_int, [_P, _P, C.c_size_t, _P, _P]),
    "ibdg_switch_fit_step": (C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, _P, _P]),
    "ibdg_log2_fit_host": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P, _P]),
    "ibdg_log2_store_reserve": (C.c_int, [_P, C.c_size_t]),
    "ibdg_log2_store_append": (C.c_int, [_P]),
    "ibdg_log2_store_count": (C.c_size_t, [_P]),
    "ibdg_log2_store_switches": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, _P]),
    "ibdg_log2_store_fit": (C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, _P]),
    "ibdg_get_alt_counts": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P]),
    "ibdg_last_run_ms": (C.c_int, [_P, _P]),
    "ibdg_run_ms": (C.c_int, [_P, C.c_uint, _P]),
    "ibdg_run_kernel_ms": (C.c_int, [_P, C.c_uint, _P]),
    "ibdg_last_ld_variant": (C.c_int, [_P]),
    "ibdg_ld_layout": (C.c_int, [_P]),
    "ibdg_last_count_unit": (C.c_int, [_P]),
    "ibdg_last_window_end": (C.c_int, [_P]),
    "ibdg_set_option": (C.c_int, [_P, C.c_char_p, C.c_long]),
    "ibdg_set_background_order": (C.c_int, [_P, _P, C.c_size_t]),
    "ibdg_selftest": (C.c_int, [C.c_char_p]),
    "ibdg_sync": (C.c_int, [_P]),
}


class EngineError(RuntimeError):
    pass


_lib = None


def load_library(path=LIB_PATH):
    """dlopen the engine and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    if not os.path.exists(path):
        raise EngineError(f"{path} not found: build it with `make -C ibdgem_amd/csrc` "
                          "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        if (path != LIB_PATH or os.environ.get("IBDG_LIB")) and not hasattr(lib, name):
            continue                   # an older build of the ABI loaded for an A/B comparison (by path or through IBDG_LIB)
        fn = getattr(lib, name)        # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if path == LIB_PATH:
        _lib = lib
    return lib


class PinnedArray:
    """A numpy array over page-locked memory from ibdg_host_alloc (freed by close() or the collector)."""

    def __init__(self, shape, dtype):
        lib = load_library()
        self.dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * self.dtype.itemsize
        self.ptr = lib.ibdg_host_alloc(n)
        if not self.ptr:
            raise EngineError("ibdg_host_alloc failed")
        self._lib = lib
        buf = (C.c_char * max(n, 1)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._lib.ibdg_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_alleles(alleles):
    """uint8 [L][2N] (0/1) -> packed rows uint64 [L][row_words] via ibdg_pack_alleles."""
    lib = load_library()
    alleles = np.ascontiguousarray(alleles, dtype=np.uint8)
    L, two_n = alleles.shape
    n_ids = two_n // 2
    rw = lib.ibdg_row_words(n_ids)
    out = np.zeros((L, rw), dtype=np.uint64)
    for i in range(L):
        lib.ibdg_pack_alleles(alleles[i].ctypes.data, n_ids, out[i].ctypes.data)
    return out


def pack_alleles_fast(alleles):
    """Same layout as pack_alleles, vectorised in numpy (test/bench data preparation only)."""
    alleles = np.ascontiguousarray(alleles, dtype=np.uint8)
    L, two_n = alleles.shape
    n_ids = two_n // 2
    chunks = (n_ids + 63) // 64
    pad = np.zeros((L, chunks * 64, 2), dtype=np.uint8)
    pad[:, :n_ids, :] = alleles.reshape(L, n_ids, 2)
    # [L][chunk][bit][plane] -> [L][chunk][plane][bit]
    bits = pad.reshape(L, chunks, 64, 2).transpose(0, 1, 3, 2)
    by = np.packbits(bits, axis=-1, bitorder="little")          # [L][chunk][plane][8 bytes]
    return np.ascontiguousarray(by).view("<u8").reshape(L, chunks * 2)


def _starts(starts):
    """The chain starts as the library takes them: (contiguous uint32 array kept alive by the caller, pointer or None, count).
    The entries go as they are: the library checks them."""
    a = np.ascontiguousarray(starts, dtype=np.uint32).reshape(-1)
    return a, (a.ctypes.data if len(a) else None), len(a)


def _shift(shift, n):
    """The step shifts of a table of n windows as the twins take them: a contiguous int32 array [n] (kept alive by the caller).
    The entries go as they are: the library checks them."""
    a = np.ascontiguousarray(shift, dtype=np.int32).reshape(-1)
    if len(a) != n:
        raise ValueError(f"shift: {len(a)} entries, not the {n} windows")
    return a


def log2_states_host(log2_tab, p01, p02, p12, want_path=True, want_score=True, starts=None, shift=None):
    """The integer log-domain IBD-state path of one window table [n_win][3] on the host (ibdg_log2_states_host):
    (path uint8 [n_win] or None, score int64 [n_win][3] or None, count uint64 [3]).  starts: the windows >= 1 that start a chain
    (ibdg_log2_states_chains_host); None: the call without chains.  shift: the windows' step shifts, int32 [n_win]
    (ibdg_log2_states_steps_host); None: the call without steps."""
    lib = load_library()
    tab = np.ascontiguousarray(log2_tab, dtype=np.float64).reshape(-1, 3)
    n = tab.shape[0]
    path = np.zeros(n, dtype=np.uint8) if want_path else None
    score = np.zeros((n, 3), dtype=np.int64) if want_score else None
    count = np.zeros(3, dtype=np.uint64)
    args = (tab.ctypes.data, n, p01, p02, p12, None if path is None else path.ctypes.data,
            None if score is None else score.ctypes.data, count.ctypes.data)
    if shift is not None:
        keep, ptr, ns = _starts(() if starts is None else starts)
        sh = _shift(shift, n)
        rc = lib.ibdg_log2_states_steps_host(*args, ptr, ns, sh.ctypes.data)
    elif starts is None:
        rc = lib.ibdg_log2_states_host(*args)
    else:
        keep, ptr, ns = _starts(starts)
        rc = lib.ibdg_log2_states_chains_host(*args, ptr, ns)
    if rc != 0:
        raise EngineError(lib.ibdg_last_error(None).decode() or f"error {rc}")
    return path, score, count


def log2_posteriors_host(log2_tab, p01, p02, p12, want_post=True, starts=None, shift=None):
    """Forward-backward IBD-state probabilities of one window table [n_win][3] on the host (ibdg_log2_posteriors_host):
    (post float64 [n_win][3] or None, expect float64 [3], log2_z float).  starts, shift: as for log2_states_host
    (ibdg_log2_posteriors_chains_host, ibdg_log2_posteriors_steps_host)."""
    lib = load_library()
    tab = np.ascontiguousarray(log2_tab, dtype=np.float64).reshape(-1, 3)
    n = tab.shape[0]
    post = np.zeros((n, 3), dtype=np.float64) if want_post else None
    expect = np.zeros(3, dtype=np.float64)
    log2_z = C.c_double(0.0)
    args = (tab.ctypes.data, n, p01, p02, p12, None if post is None else post.ctypes.data, expect.ctypes.data,
            C.addressof(log2_z))
    if shift is not None:
        keep, ptr, ns = _starts(() if starts is None else starts)
        sh = _shift(shift, n)
        rc = lib.ibdg_log2_posteriors_steps_host(*args, ptr, ns, sh.ctypes.data)
    elif starts is None:
        rc = lib.ibdg_log2_posteriors_host(*args)
    else:
        keep, ptr, ns = _starts(starts)
        rc = lib.ibdg_log2_posteriors_chains_host(*args, ptr, ns)
    if rc != 0:
        raise EngineError(lib.ibdg_last_error(None).decode() or f"error {rc}")
    return post, expect, log2_z.value


# ibdg_segment (include/ibdgem_hip.h): 56 bytes, no padding
SEGMENT_DTYPE = np.dtype([("first", "<u4"), ("n_win", "<u4"), ("state", "<u4"), ("reserved", "<u4"), ("e", "<i8", (3,)),
                          ("post_q", "<u8"), ("post_min", "<f8")])
assert SEGMENT_DTYPE.itemsize == 56


def _positions(pos_first, pos_last, n):
    """The two position arrays as contiguous uint64 [n], or None; one alone stays alone (the library refuses it)."""
    out = []
    for p in (pos_first, pos_last):
        if p is not None:
            p = np.ascontiguousarray(p, dtype=np.uint64)
            if p.shape != (n,):
                raise ValueError(f"positions: {p.shape}, not ({n},)")
        out.append(p)
    return out


def log2_segments_host(log2_tab, p01, p02, p12, with_post=False, pos_first=None, pos_last=None, seg_cap=None, want_seg=True,
                       starts=None, shift=None):
    """The segments of one window table's path on the host (ibdg_log2_segments_host): (seg structured array of
    SEGMENT_DTYPE -- min(n_seg, seg_cap) records, all of them with seg_cap None -- or None, n_seg int, summary uint64 [12]).
    starts, shift: as for log2_states_host (ibdg_log2_segments_chains_host, ibdg_log2_segments_steps_host)."""
    lib = load_library()
    tab = np.ascontiguousarray(log2_tab, dtype=np.float64).reshape(-1, 3)
    n = tab.shape[0]
    pf, pl = _positions(pos_first, pos_last, n)
    cap = n if seg_cap is None else int(seg_cap)
    seg = np.zeros(cap + 1, dtype=SEGMENT_DTYPE) if want_seg else None        # (one more: nothing may land behind the cap)
    if seg is not None:
        seg[cap]["first"] = 0xffffffff
    n_seg = C.c_uint64(0)
    summary = np.zeros(12, dtype=np.uint64)
    args = (tab.ctypes.data, n, p01, p02, p12, int(bool(with_post)), None if pf is None else pf.ctypes.data,
            None if pl is None else pl.ctypes.data, None if seg is None else seg.ctypes.data, cap, C.addressof(n_seg),
            summary.ctypes.data)
    if shift is not None:
        keep, ptr, ns = _starts(() if starts is None else starts)
        sh = _shift(shift, n)
        rc = lib.ibdg_log2_segments_steps_host(*args, ptr, ns, sh.ctypes.data)
    elif starts is None:
        rc = lib.ibdg_log2_segments_host(*args)
    else:
        keep, ptr, ns = _starts(starts)
        rc = lib.ibdg_log2_segments_chains_host(*args, ptr, ns)
    if rc != 0:
        raise EngineError(lib.ibdg_last_error(None).decode() or f"error {rc}")
    if seg is not None:
        if seg[cap]["first"] != 0xffffffff:
            raise EngineError("ibdg_log2_segments_host wrote behind seg_cap")
        seg = seg[:min(cap, n_seg.value)].copy()
    return seg, n_seg.value, summary


def log2_samples_host(log2_tab, p01, p02, p12, n_samples, seed, stream, pos_first=None, pos_last=None, want_paths=True,
                      starts=None, shift=None):
    """n_samples IBD-state paths of one window table [n_win][3] drawn from the posterior on the host (ibdg_log2_samples_host):
    (paths uint8 [n_samples][n_win] or None, out uint64 [n_samples][15] -- per draw the windows per state, then the segments'
    summary of the drawn path).  seed, stream: uint64; a draw depends on them and its number alone.  starts, shift: as for
    log2_states_host."""
    lib = load_library()
    tab = np.ascontiguousarray(log2_tab, dtype=np.float64).reshape(-1, 3)
    n, K = tab.shape[0], int(n_samples)
    pf, pl = _positions(pos_first, pos_last, n)
    rows = K if 0 < K <= 65536 else 1                       # (a refused count writes nothing)
    paths = np.zeros((rows, n), dtype=np.uint8) if want_paths else None
    out = np.zeros((rows, 15), dtype=np.uint64)
    keep, ptr, ns = _starts(() if starts is None else starts)
    sh = None if shift is None else _shift(shift, n)
    rc = lib.ibdg_log2_samples_host(tab.ctypes.data, n, p01, p02, p12, ptr, ns, None if sh is None else sh.ctypes.data, K, seed, stream,
                                    None if pf is None else pf.ctypes.data, None if pl is None else pl.ctypes.data,
                                    None if paths is None else paths.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise EngineError(lib.ibdg_last_error(None).decode() or f"error {rc}")
    return paths, out


def log2_switches_host(log2_tab, p01, p02, p12, want_sw=True, starts=None, shift=None, n_win=None):
    """The switch probabilities of one window table [n_win][3] on the host (ibdg_log2_switches_host): (sw float64 [n_win][3] or
    None -- per step the probability of a 0<->1, 0<->2, 1<->2 switch --, expect float64 [3] -- their sums over the counted steps --,
    counted uint64 [3]).  log2_tab None with n_win: the table that says nothing, whose expect is the prior of
    switch_penalty_update.  starts, shift: as for log2_states_host."""
    lib = load_library()
    if log2_tab is None:
        tab, n = None, int(n_win)
    else:
        tab = np.ascontiguousarray(log2_tab, dtype=np.float64).reshape(-1, 3)
        n = tab.shape[0]
    sw = np.zeros((n, 3), dtype=np.float64) if want_sw else None
    expect = np.zeros(3, dtype=np.float64)
    counted = np.zeros(3, dtype=np.uint64)
    keep, ptr, ns = _starts(() if starts is None else starts)
    sh = None if shift is None else _shift(shift, n)
    rc = lib.ibdg_log2_switches_host(None if tab is None else tab.ctypes.data, n, p01, p02, p12, ptr, ns,
                                     None if sh is None else sh.ctypes.data, None if sw is None else sw.ctypes.data,
                                     expect.ctypes.data, counted.ctypes.data)
    if rc != 0:
        raise EngineError(lib.ibdg_last_error(None).decode() or f"error {rc}")
    return sw, expect, counted


def switch_penalty_update(p, total, n_individuals, prior):
    """One step of the switch penalties (ibdg_switch_penalty_update): next[k] = min(1, max(1e-300, p[k] * total[k] /
    (n_individuals * prior[k]))), or p[k] where total[k] or prior[k] is not finite and > 0.  float64 [3]."""
    lib = load_library()
    p, total, prior = (np.ascontiguousarray(x, dtype=np.float64).reshape(3) for x in (p, total, prior))
    nxt = np.zeros(3, dtype=np.float64)
    if lib.ibdg_switch_penalty_update(p.ctypes.data, total.ctypes.data, int(n_individuals), prior.ctypes.data, nxt.ctypes.data) != 0:
        raise EngineError(lib.ibdg_last_error(None).decode())
    return nxt


def _total_in_order(expect):
    """The individuals' expectations [T][3] added in their order from 0.0, as the host program adds them."""
    total = np.zeros(3, dtype=np.float64)
    for row in np.asarray(expect, dtype=np.float64).reshape(-1, 3):
        total = total + row
    return total


def fit_switch_penalties_host(tables, p, iterations, starts=None, shift=None):
    """The update repeated over given window tables (a list of [n_win][3], one per individual, of one site list) on the host:
    per iteration log2_switches_host on every table, the prior from the table that says nothing, switch_penalty_update.  Returns
    float64 [iterations][3], the penalties after each iteration.  Whether the sequence converges is an observation, not a
    theorem."""
    tabs = [np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3) for t in tables]
    p = np.array(p, dtype=np.float64).reshape(3)
    out = np.zeros((int(iterations), 3), dtype=np.float64)
    for it in range(int(iterations)):
        expect = [log2_switches_host(t, *p, want_sw=False, starts=starts, shift=shift)[1] for t in tabs]
        prior = log2_switches_host(None, *p, want_sw=False, starts=starts, shift=shift, n_win=tabs[0].shape[0] if tabs else 0)[1]
        p = switch_penalty_update(p, _total_in_order(expect), len(tabs), prior)
        out[it] = p
    return out


# ibdg_fit_row (include/ibdgem_hip.h): 96 bytes, no padding
FIT_ROW_DTYPE = np.dtype([("p", "<f8", (3,)), ("total", "<f8", (3,)), ("prior", "<f8", (3,)), ("counted", "<u8", (3,))])
assert FIT_ROW_DTYPE.itemsize == 96


def switch_fit_step(p, total, n_individuals, prior, counted):
    """One step of the fit (ibdg_switch_fit_step): (row, a FIT_ROW_DTYPE record of the arguments; next float64 [3], the update's;
    stood bool: no penalty's integer moved by more than one quantum)."""
    lib = load_library()
    p, total, prior = (np.ascontiguousarray(x, dtype=np.float64).reshape(3) for x in (p, total, prior))
    counted = np.ascontiguousarray(counted, dtype=np.uint64).reshape(3)
    row = np.zeros(1, dtype=FIT_ROW_DTYPE)
    nxt = np.zeros(3, dtype=np.float64)
    stood = C.c_int(0)
    if lib.ibdg_switch_fit_step(p.ctypes.data, total.ctypes.data, int(n_individuals), prior.ctypes.data, counted.ctypes.data,
                                row.ctypes.data, nxt.ctypes.data, C.addressof(stood)) != 0:
        raise EngineError(lib.ibdg_last_error(None).decode())
    return row[0], nxt, bool(stood.value)


def log2_fit_host(tables, p, max_iter, starts=None, shift=None, n_win=None):
    """The fit of the switch penalties over given window tables (a list of [n_win][3], one per individual of one site list) on
    the host (ibdg_log2_fit_host): (rows, a FIT_ROW_DTYPE array with one record per iteration made; stood bool; fitted float64
    [3]).  It ends behind the first iteration whose step stood, or behind max_iter.  n_win: the windows, for no tables."""
    lib = load_library()
    tabs = [np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3) for t in tables]
    n = tabs[0].shape[0] if tabs else int(n_win or 0)
    if any(t.shape[0] != n for t in tabs):
        raise ValueError("tables of different lengths")
    ptrs = (C.c_void_p * max(len(tabs), 1))(*[t.ctypes.data for t in tabs])
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(3)
    keep, ptr, ns = _starts(() if starts is None else starts)
    sh = None if shift is None else _shift(shift, n)
    rows = np.zeros(max(int(max_iter), 1), dtype=FIT_ROW_DTYPE)
    n_rows, stood = C.c_size_t(0), C.c_int(0)
    fitted = np.zeros(3, dtype=np.float64)
    rc = lib.ibdg_log2_fit_host(C.addressof(ptrs) if tabs else None, len(tabs), n, p.ctypes.data, ptr, ns,
                                None if sh is None else sh.ctypes.data, int(max_iter), rows.ctypes.data, C.addressof(n_rows),
                                C.addressof(stood), fitted.ctypes.data)
    if rc != 0:
        raise EngineError(lib.ibdg_last_error(None).decode() or f"error {rc}")
    return rows[:n_rows.value].copy(), bool(stood.value), fitted


class Engine:
    def __init__(self, device=0, epsilon=0.02, max_cov=20, lib_path=None):
        self.lib = load_library(lib_path) if lib_path else load_library()
        self.ctx = self.lib.ibdg_create(device, epsilon, max_cov)
        if not self.ctx:
            raise EngineError(self.lib.ibdg_last_error(None).decode())
        self.n_ids = 0

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.ibdg_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise EngineError(self.lib.ibdg_last_error(self.ctx).decode() or f"error {rc}")

    def set_option(self, name, value):
        self._chk(self.lib.ibdg_set_option(self.ctx, name.encode(), int(value)))

    def upload_panel(self, rows, n_ids):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        assert rows.ndim == 2 and rows.shape[1] == self.lib.ibdg_row_words(n_ids)
        self._chk(self.lib.ibdg_upload_panel(self.ctx, rows.ctypes.data, rows.shape[0], n_ids))
        self.n_ids = n_ids

    def upload_panel_fd(self, fd, offset, n_rows, n_ids):
        """Packed rows from an open file (n_rows x ibdg_row_words(n_ids) x 8 bytes from byte `offset`)."""
        self._chk(self.lib.ibdg_upload_panel_fd(self.ctx, int(fd), int(offset), int(n_rows), int(n_ids)))
        self.n_ids = n_ids

    def upload_panel_dev(self, dev_ptr, n_rows, n_ids):
        self._chk(self.lib.ibdg_upload_panel_dev(self.ctx, dev_ptr, n_rows, n_ids))
        self.n_ids = n_ids

    def upload_sites(self, row_index, n_ref, n_alt, window, f_override=None):
        """row_index None: site s is panel row s."""
        ri = None if row_index is None else np.ascontiguousarray(row_index, dtype=np.uint32)
        nr = np.ascontiguousarray(n_ref, dtype=np.uint8)
        na = np.ascontiguousarray(n_alt, dtype=np.uint8)
        fo = None if f_override is None else np.ascontiguousarray(f_override, dtype=np.float64)
        assert len(nr) == len(na) and (ri is None or len(ri) == len(nr))
        self._chk(self.lib.ibdg_upload_sites(self.ctx, None if ri is None else ri.ctypes.data, nr.ctypes.data,
                                             na.ctypes.data, None if fo is None else fo.ctypes.data, len(nr), window))

    def upload_sites_dev(self, row_index_ptr, n_ref_ptr, n_alt_ptr, n_sites, window, f_override=None):
        """The same with the three arrays in device memory (pointers; row_index_ptr may be None/0)."""
        fo = None if f_override is None else np.ascontiguousarray(f_override, dtype=np.float64)
        self._chk(self.lib.ibdg_upload_sites_dev(self.ctx, row_index_ptr or None, n_ref_ptr, n_alt_ptr,
                                                 None if fo is None else fo.ctypes.data, n_sites, window))

    def upload_candidates(self, row_index, n_ref, n_alt, f_override=None):
        """The rows of a pileup that passed every filter that does not depend on the comparison individual (-v); row_index
        None: candidate s is panel row s.  Kept on the device until replaced or until a panel is uploaded."""
        ri = None if row_index is None else np.ascontiguousarray(row_index, dtype=np.uint32)
        nr = np.ascontiguousarray(n_ref, dtype=np.uint8)
        na = np.ascontiguousarray(n_alt, dtype=np.uint8)
        fo = None if f_override is None else np.ascontiguousarray(f_override, dtype=np.float64)
        assert len(nr) == len(na) and (ri is None or len(ri) == len(nr)) and (fo is None or len(fo) == len(nr))
        self._chk(self.lib.ibdg_upload_candidates(self.ctx, None if ri is None else ri.ctypes.data, nr.ctypes.data,
                                                  na.ctypes.data, None if fo is None else fo.ctypes.data, len(nr)))

    @property
    def n_candidates(self):
        return self.lib.ibdg_num_candidates(self.ctx)

    def select_variable_sites(self, target, window):
        """The current site list = the candidates at which individual `target` is not 0/0, made on the device."""
        self._chk(self.lib.ibdg_select_variable_sites(self.ctx, int(target), int(window)))

    def site_candidates(self):
        """Candidate index of every site of a list made by select_variable_sites."""
        out = np.empty(self.n_sites, dtype=np.uint32)
        self._chk(self.lib.ibdg_get_site_candidates(self.ctx, out.ctypes.data))
        return out

    def upload_ms(self):
        """Clocks of the last upload of sites (ms): copies, device preparation, whole call."""
        out = (C.c_float * 3)()
        self._chk(self.lib.ibdg_upload_ms(self.ctx, out))
        return dict(h2d=out[0], device_prep=out[1], call=out[2])

    @property
    def n_sites(self):
        return self.lib.ibdg_num_sites(self.ctx)

    @property
    def n_windows(self):
        return self.lib.ibdg_num_windows(self.ctx)

    def windows(self):
        n = self.n_windows
        first = np.zeros(n, dtype=np.uint32)
        last = np.zeros(n, dtype=np.uint32)
        ncov = np.zeros(n, dtype=np.uint32)
        self._chk(self.lib.ibdg_get_windows(self.ctx, first.ctypes.data, last.ctypes.data, ncov.ctypes.data))
        return first, last, ncov

    def run(self, targets, ld=True, bg_count=None, pu_id=-1):
        t = np.ascontiguousarray(targets, dtype=np.uint32)
        bg = None if bg_count is None else np.ascontiguousarray(bg_count, dtype=np.uint8)
        if bg is not None:
            assert len(bg) == self.n_ids
        self._chk(self.lib.ibdg_run(self.ctx, t.ctypes.data, len(t), None if bg is None else bg.ctypes.data,
                                    int(pu_id), int(bool(ld))))
        self.n_targets = len(t)

    def site_af(self):
        out = np.empty(self.n_sites, dtype=np.float64)
        self._chk(self.lib.ibdg_get_site_af(self.ctx, out.ctypes.data))
        return out

    def site_ll(self, t=0, out=None):
        if out is None:
            out = np.empty((self.n_sites, 3), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= self.n_sites * 3 and out.flags.c_contiguous
        self._chk(self.lib.ibdg_get_site_ll(self.ctx, t, out.ctypes.data))
        return out

    def window_ll(self, t=0, out=None):
        if out is None:
            out = np.empty((self.n_windows, 3), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= self.n_windows * 3 and out.flags.c_contiguous
        self._chk(self.lib.ibdg_get_window_ll(self.ctx, t, out.ctypes.data))
        return out

    def window_ll_all(self, n_targets, out=None):
        """The window tables of all `n_targets` comparison individuals of the last run in one copy: [n_targets][n_windows][3]."""
        have = self.lib.ibdg_num_targets(self.ctx)
        if have != n_targets:       # (the C call copies what the LAST RUN produced, whatever the caller's buffer holds)
            raise EngineError(f"window_ll_all({n_targets}): the last run had {have} comparison individuals")
        if out is None:
            out = np.empty((n_targets, self.n_windows, 3), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= n_targets * self.n_windows * 3 and out.flags.c_contiguous
        self._chk(self.lib.ibdg_get_window_ll_all(self.ctx, out.ctypes.data))
        return out

    def window_log2(self, t=0, out=None):
        """log2 of LIBD0, LIBD1, LIBD2 per window of target t (option "log_windows"): [n_windows][3]."""
        if out is None:
            out = np.empty((self.n_windows, 3), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= self.n_windows * 3 and out.flags.c_contiguous
        self._chk(self.lib.ibdg_get_window_log2(self.ctx, t, out.ctypes.data))
        return out

    def window_log2_all(self, n_targets, out=None):
        """The log tables of all `n_targets` comparison individuals of the last run in one copy: [n_targets][n_windows][3]."""
        have = self.lib.ibdg_num_targets(self.ctx)
        if have != n_targets:
            raise EngineError(f"window_log2_all({n_targets}): the last run had {have} comparison individuals")
        if out is None:
            out = np.empty((n_targets, self.n_windows, 3), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= n_targets * self.n_windows * 3 and out.flags.c_contiguous
        self._chk(self.lib.ibdg_get_window_log2_all(self.ctx, out.ctypes.data))
        return out

    def set_window_log2_all(self, tabs):
        """tabs [T][n_windows][3] in place of the last run's log tables (ibdg_set_window_log2): for tests, and for callers that
        gathered a table elsewhere.  Any double goes; what the window_log2_* calls kept is stale afterwards."""
        a = np.ascontiguousarray(tabs, dtype=np.float64)
        if a.ndim != 3 or a.shape[1:] != (self.n_windows, 3):
            raise ValueError(f"tabs: shape {a.shape}, not [T][{self.n_windows}][3]")
        self._chk(self.lib.ibdg_set_window_log2(self.ctx, a.ctypes.data, a.shape[0]))

    def window_llr_sums(self, first, end):
        """Sums of log2(L2')-log2(L0') and log2(L1')-log2(L0') over the window ranges [first[s], end[s]) for every comparison
        individual of the last run: [T][n_seg][4] = {IBD2/IBD0 hi, lo, IBD1/IBD0 hi, lo} (double-doubles)."""
        first = np.ascontiguousarray(first, dtype=np.uint32)
        end = np.ascontiguousarray(end, dtype=np.uint32)
        assert first.shape == end.shape and first.ndim == 1
        out = np.zeros((self.lib.ibdg_num_targets(self.ctx), len(first), 4), dtype=np.float64)
        self._chk(self.lib.ibdg_window_llr_sums(self.ctx, first.ctypes.data, end.ctypes.data, len(first), out.ctypes.data))
        return out

    def window_log2_llr_sums(self, first, end):
        """window_llr_sums with the terms taken from the log2 table (option "log_windows"): +l2, -l0 and +l1, -l0."""
        first = np.ascontiguousarray(first, dtype=np.uint32)
        end = np.ascontiguousarray(end, dtype=np.uint32)
        assert first.shape == end.shape and first.ndim == 1
        out = np.zeros((self.lib.ibdg_num_targets(self.ctx), len(first), 4), dtype=np.float64)
        self._chk(self.lib.ibdg_window_log2_llr_sums(self.ctx, first.ctypes.data, end.ctypes.data, len(first), out.ctypes.data))
        return out

    def window_log2_states(self, p01, p02, p12, want_path=True, want_score=True):
        """Integer log-domain IBD-state paths of every comparison individual of the last run, on the device
        (ibdg_window_log2_states): (path uint8 [T][n_win] or None, score int64 [T][n_win][3] or None, count uint64 [T][3])."""
        T, n = self.lib.ibdg_num_targets(self.ctx), self.n_windows
        path = np.zeros((T, n), dtype=np.uint8) if want_path else None
        score = np.zeros((T, n, 3), dtype=np.int64) if want_score else None
        count = np.zeros((T, 3), dtype=np.uint64)
        self._chk(self.lib.ibdg_window_log2_states(self.ctx, p01, p02, p12, None if path is None else path.ctypes.data,
                                                   None if score is None else score.ctypes.data, count.ctypes.data))
        return path, score, count

    def window_log2_posteriors(self, p01, p02, p12, want_post=True):
        """Forward-backward IBD-state probabilities of every comparison individual of the last run, on the device
        (ibdg_window_log2_posteriors): (post float64 [T][n_win][3] or None, expect float64 [T][3], log2_z float64 [T])."""
        T, n = self.lib.ibdg_num_targets(self.ctx), self.n_windows
        post = np.zeros((T, n, 3), dtype=np.float64) if want_post else None
        expect = np.zeros((T, 3), dtype=np.float64)
        log2_z = np.zeros(T, dtype=np.float64)
        self._chk(self.lib.ibdg_window_log2_posteriors(self.ctx, p01, p02, p12, None if post is None else post.ctypes.data,
                                                       expect.ctypes.data, log2_z.ctypes.data))
        return post, expect, log2_z

    def window_log2_segments(self, p01, p02, p12, with_post=False, pos_first=None, pos_last=None):
        """The segments of every comparison individual's path of the last run, counted on the device
        (ibdg_window_log2_segments): (n_seg uint64 [T], summary uint64 [T][12]).  get_log2_segments has the records."""
        T, n = self.lib.ibdg_num_targets(self.ctx), self.n_windows
        pf, pl = _positions(pos_first, pos_last, n)
        n_seg = np.zeros(T, dtype=np.uint64)
        summary = np.zeros((T, 12), dtype=np.uint64)
        self._chk(self.lib.ibdg_window_log2_segments(self.ctx, p01, p02, p12, int(bool(with_post)),
                                                     None if pf is None else pf.ctypes.data,
                                                     None if pl is None else pl.ctypes.data, n_seg.ctypes.data,
                                                     summary.ctypes.data))
        self._seg_total = int(n_seg.sum())
        return n_seg, summary

    def get_log2_segments(self, cap=None):
        """The records of the last window_log2_segments call (ibdg_get_log2_segments): a structured array of SEGMENT_DTYPE, the
        individuals' segments back to back.  cap: the room offered (default: what that call counted)."""
        cap = getattr(self, "_seg_total", 0) if cap is None else int(cap)
        seg = np.zeros(max(cap, 1), dtype=SEGMENT_DTYPE)
        self._chk(self.lib.ibdg_get_log2_segments(self.ctx, seg.ctypes.data, cap))
        return seg[:cap]

    def window_log2_samples(self, p01, p02, p12, n_samples, seed, stream, pos_first=None, pos_last=None):
        """n_samples paths per comparison individual of the last run drawn from the posterior, on the device
        (ibdg_window_log2_samples): out uint64 [T][n_samples][15], the bytes of log2_samples_host with stream[t].  stream: uint64
        [T], by convention the individuals' indices in the panel."""
        T, n, K = self.lib.ibdg_num_targets(self.ctx), self.n_windows, int(n_samples)
        pf, pl = _positions(pos_first, pos_last, n)
        st = np.ascontiguousarray(stream, dtype=np.uint64).reshape(-1)
        if len(st) != T:
            raise ValueError(f"stream: {len(st)} entries, not the {T} individuals")
        out = np.zeros((T, K if 0 < K <= 65536 else 1, 15), dtype=np.uint64)
        self._chk(self.lib.ibdg_window_log2_samples(self.ctx, p01, p02, p12, K, seed, st.ctypes.data,
                                                    None if pf is None else pf.ctypes.data,
                                                    None if pl is None else pl.ctypes.data, out.ctypes.data))
        return out

    def window_log2_switches(self, p01, p02, p12, want_sw=True):
        """The switch probabilities of every comparison individual of the last run, on the device (ibdg_window_log2_switches):
        (sw float64 [T][n_win][3] or None, expect float64 [T][3]), the bytes of log2_switches_host under the context's chains and
        steps.  The posteriors kept from an earlier call go stale."""
        T, n = self.lib.ibdg_num_targets(self.ctx), self.n_windows
        sw = np.zeros((T, n, 3), dtype=np.float64) if want_sw else None
        expect = np.zeros((T, 3), dtype=np.float64)
        self._chk(self.lib.ibdg_window_log2_switches(self.ctx, p01, p02, p12, None if sw is None else sw.ctypes.data,
                                                     expect.ctypes.data))
        return sw, expect

    def window_log2_switches_prior(self, p01, p02, p12):
        """The prior of switch_penalty_update under the context's chains and steps (ibdg_window_log2_switches_prior, on the
        host): (expect float64 [3], counted uint64 [3])."""
        expect = np.zeros(3, dtype=np.float64)
        counted = np.zeros(3, dtype=np.uint64)
        self._chk(self.lib.ibdg_window_log2_switches_prior(self.ctx, p01, p02, p12, expect.ctypes.data, counted.ctypes.data))
        return expect, counted

    def fit_switch_penalties(self, p, iterations):
        """The update repeated over the resident table of the last run: per iteration window_log2_switches without the rows,
        the prior, switch_penalty_update.  Returns float64 [iterations][3], the bytes of fit_switch_penalties_host over the same
        tables, chains and steps."""
        p = np.array(p, dtype=np.float64).reshape(3)
        out = np.zeros((int(iterations), 3), dtype=np.float64)
        for it in range(int(iterations)):
            expect = self.window_log2_switches(*p, want_sw=False)[1]
            prior = self.window_log2_switches_prior(*p)[0]
            p = switch_penalty_update(p, _total_in_order(expect), len(expect), prior)
            out[it] = p
        return out

    def log2_store_reserve(self, n_individuals):
        """An empty table store for up to n_individuals log2 window tables of the site list at hand (ibdg_log2_store_reserve).  A
        new site list or panel empties it and takes the reserve away."""
        self._chk(self.lib.ibdg_log2_store_reserve(self.ctx, int(n_individuals)))

    def log2_store_append(self):
        """The log2 tables of the last run's individuals onto the store's end, device to device (ibdg_log2_store_append)."""
        self._chk(self.lib.ibdg_log2_store_append(self.ctx))

    def log2_store_count(self):
        """The individuals stored (ibdg_log2_store_count)."""
        return int(self.lib.ibdg_log2_store_count(self.ctx))

    def log2_store_switches(self, p01, p02, p12):
        """The expected counted switches of every stored individual under the context's chains and steps, one launch over the
        whole store (ibdg_log2_store_switches): float64 [count][3], the bytes of log2_switches_host per table.  Nothing kept from
        earlier calls goes stale."""
        expect = np.zeros((self.log2_store_count(), 3), dtype=np.float64)
        self._chk(self.lib.ibdg_log2_store_switches(self.ctx, p01, p02, p12, expect.ctypes.data))
        return expect

    def log2_store_fit(self, p, max_iter):
        """The fit over the store (ibdg_log2_store_fit): (rows FIT_ROW_DTYPE, stood bool, fitted float64 [3]), the bytes of
        log2_fit_host over the stored tables with the context's chains and steps."""
        p = np.ascontiguousarray(p, dtype=np.float64).reshape(3)
        rows = np.zeros(max(int(max_iter), 1), dtype=FIT_ROW_DTYPE)
        n_rows, stood = C.c_size_t(0), C.c_int(0)
        fitted = np.zeros(3, dtype=np.float64)
        self._chk(self.lib.ibdg_log2_store_fit(self.ctx, p.ctypes.data, int(max_iter), rows.ctypes.data, C.addressof(n_rows),
                                               C.addressof(stood), fitted.ctypes.data))
        return rows[:n_rows.value].copy(), bool(stood.value), fitted

    def get_log2_sample_path(self, t, k):
        """Draw k of individual t of the last window_log2_samples call, drawn again (ibdg_get_log2_sample_path): uint8 [n_win]."""
        path = np.zeros(max(self.n_windows, 1), dtype=np.uint8)
        self._chk(self.lib.ibdg_get_log2_sample_path(self.ctx, t, k, path.ctypes.data))
        return path[:self.n_windows]

    def set_window_chains(self, starts=()):
        """The windows >= 1 of the current site list that start a chain, for the three window_log2_* calls and
        get_log2_segments (ibdg_set_window_chains); none clears them.  A new site list or panel clears them too."""
        keep, ptr, ns = _starts(starts)
        self._chk(self.lib.ibdg_set_window_chains(self.ctx, ptr, ns))

    def set_window_steps(self, shift=None):
        """The step shifts of the current site list's windows, int32 [n_windows], for the three window_log2_* calls and
        get_log2_segments (ibdg_set_window_steps); None or an empty list clears them.  A new site list or panel clears them too."""
        a = np.ascontiguousarray(() if shift is None else shift, dtype=np.int32).reshape(-1)
        self._chk(self.lib.ibdg_set_window_steps(self.ctx, a.ctypes.data if len(a) else None, len(a)))

    def has_window_steps(self):
        """Whether the current site list has step shifts (ibdg_has_window_steps)."""
        return bool(self.lib.ibdg_has_window_steps(self.ctx))

    @property
    def n_window_chains(self):
        """The number of chains of the current site list (ibdg_num_window_chains): the starts set plus one; 0 without windows."""
        return self.lib.ibdg_num_window_chains(self.ctx)

    def alt_counts(self, first, n):
        out = np.empty(n, dtype=np.uint32)
        self._chk(self.lib.ibdg_get_alt_counts(self.ctx, first, n, out.ctypes.data))
        return out

    def last_run_ms(self):
        out = (C.c_float * 5)()
        self._chk(self.lib.ibdg_last_run_ms(self.ctx, out))
        return dict(total=out[0], alt_count=out[1], rows=out[2], ld=out[3])

    def run_ms(self, back):
        """Device times of the run `back` calls ago (0 = last); waits for the stream."""
        out = (C.c_float * 5)()
        self._chk(self.lib.ibdg_run_ms(self.ctx, back, out))
        return dict(total=out[0], alt_count=out[1], rows=out[2], ld=out[3])

    def run_kernel_ms(self, back=0):
        """Duration of the dominant --LD kernel of the run `back` calls ago (its own dispatch times)."""
        out = C.c_float()
        self._chk(self.lib.ibdg_run_kernel_ms(self.ctx, back, C.byref(out)))
        return out.value

    def set_background_order(self, ids):
        """Background list in the reference's order (reference-order mode); None/empty clears it."""
        a = np.ascontiguousarray([] if ids is None else ids, dtype=np.uint32)
        self._chk(self.lib.ibdg_set_background_order(self.ctx, a.ctypes.data if len(a) else None, len(a)))

    def last_ld_variant(self):
        return self.lib.ibdg_last_ld_variant(self.ctx)

    def last_count_unit(self):
        """2 = the last run's single-individual launches took the sums of a haplotype word on the matrix cores, 1 = by
        (mask, count) pairs, 0 = no such launch (ibdg_last_count_unit)."""
        return self.lib.ibdg_last_count_unit(self.ctx)

    def last_window_end(self):
        """2 = those launches summed two consecutive windows of a run in one tree (the IBD1 form's paired window end, option
        pair_sums), 1 = every window on its own, 0 = no such launch (ibdg_last_window_end)."""
        return self.lib.ibdg_last_window_end(self.ctx)

    def ld_layout(self):
        """0 none, 1 the panel's own tiles, 2 the compacted tiles of the site list (its rows with reads back to back)."""
        return self.lib.ibdg_ld_layout(self.ctx)

    def sync(self):
        self._chk(self.lib.ibdg_sync(self.ctx))
