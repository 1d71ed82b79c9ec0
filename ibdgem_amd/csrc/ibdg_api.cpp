// ibdg_api.cpp -- the C ABI of include/ibdgem_hip.h: host-side table building,
// validation, device memory and kernel sequencing.  No CPU implementation of
// the likelihood path lives here: without a HIP device every compute entry
// point fails with an error.
#include "../../include/ibdgem_hip.h"
#include "ibdg_ctx.h"
#include "ibdg_kernels.h"
#include "ibdg_states.h"

static_assert(sizeof(ibdg_segment) == 56, "ibdg_segment has no padding");

#include <hip/hip_runtime.h>

#include <cerrno>
#include <unistd.h>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

// libm pow through a volatile pointer: the compiler must not rewrite
// pow(x, 2.0) as x*x -- glibc's pow differs from x*x in the last bit for some
// inputs and the reference (src/ibd-math.c:93-95) calls the real pow.
double (*volatile libm_pow)(double, double) = std::pow;

std::string g_create_error;          // of the last failed ibdg_create; contexts may be created from several threads
std::mutex g_create_error_mu;

}  // namespace

namespace {

int fail(ibdg_ctx *c, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) {
        c->err = buf;
    } else {
        std::lock_guard<std::mutex> lk(g_create_error_mu);
        g_create_error = buf;
    }
    return 1;
}

#define HIP_TRY(c, call)                                                                        \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((c), "[::] ERROR in %s: %s: %s", __func__, #call, hipGetErrorString(e_)); \
    } while (0)

// The finalising launch a run left to its successor, when no successor took it
int flush_finalize(ibdg_ctx *c)
{
    if (c->fin.pending) {
        c->fin.pending = false;
        ibdg::launch_ld_finalize(c->fin.args, c->fin.count, c->stream, ibdg::KernelEvents());
        HIP_TRY(c, hipGetLastError());
    }
    return 0;
}

// The main stream waits for whatever stream2 still holds (queued, not a host wait).
int join_streams(ibdg_ctx *c)
{
    if (flush_finalize(c)) return 1;
    if (c->tl.s2_pending) {
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->tl.last_s2, 0));
        c->tl.s2_pending = false;
    }
    return 0;
}

// Host wait until both streams are idle (before results are read or inputs replaced).
int quiesce(ibdg_ctx *c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (join_streams(c)) return 1;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream3));     // (idle whenever the main stream is: every batch on it ends in an event the main stream waits for)
    c->tl.chain_ok = false;
    return 0;
}

int ensure(ibdg_ctx *c, DevBuf &b, size_t bytes)
{
    if (bytes == 0)
        bytes = 16;
    if (b.cap >= bytes)
        return 0;
    if (b.p) {
        // queued runs ("async") may still use the buffer: wait for them rather than rely on hipFree doing so
        if ((c->tl.s2_pending || c->tl.chain_ok) && quiesce(c))
            return 1;
        HIP_TRY(c, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    HIP_TRY(c, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    ++b.allocs;
    return 0;
}

// ---- what stops being valid when an input changes: each of these says all of it, and nobody else says any ----

// A panel goes up: the alt counts, the results (with what the log-domain calls kept of them: ls, and the window chains, which
// belong to the site list that goes, and the table store of that list), the layout, the site list
// and the candidates (they name rows of the panel that goes), and the device copies of targets / background weights, which
// were laid out for the previous panel.  The row
// table goes with up_gen (its alt counts and n_ids).  sites_gen stays: no run is accepted before the next upload of sites
// (sites_valid) and no background is taken for the same (prev_pu).
void panel_replaced(ibdg_ctx *c)
{
    ++c->up_gen;
    c->pan.counts_valid = false;
    c->have_results = false;
    c->ls.chains_clear();
    c->ls.steps_clear();
    c->lstore.empty();
    c->lay.pop_sites_ok = false;
    c->prev_targets.clear();
    c->bg.prev_bg.clear();
    c->bg.prev_pu = -2;
    c->bg.prev_has_bg = -1;
    c->bg.prev_lanes = 0;
    c->sites.n_sites = 0;
    c->sites.n_cov = c->sites.n_win = 0;
    c->sites.sites_valid = false;
    c->cand.valid = c->cand.sel_valid = false;
    c->cand.n_cand = 0;
}

// A site list goes up (from the host, the device or the candidates): the results (with ls and the window chains of the list
// before: ibdg_set_window_chains speaks of one list's windows; the table store, whose tables are over that list's windows), the layout and its credit, the
// window bounds, the -A triples, the selection map; with sites_gen the IBD0 pass, the fragment base, the images, a pending
// finalising step's right to ride along and stream3's order behind the prepared sites; with up_gen the row table; and
// the count of runs towards "ibd0_after".
void sites_replaced(ibdg_ctx *c)
{
    ++c->sites_gen;
    ++c->up_gen;
    c->sites.n_cov = 0;
    c->sites.n_win = 0;
    c->sites.sites_valid = false;
    c->sites.win_bounds_valid = false;
    c->sites.have_fo = false;
    c->cand.sel_valid = false;
    c->have_results = false;
    c->ls.chains_clear();
    c->ls.steps_clear();
    c->lstore.empty();
    c->lay.pop_sites_ok = false;
    c->lay.compact = false;
    c->lay.relayout_credit = 0;
    c->ibd0.drop();
}

// New segments, window constants and control words for the same site list (commit_layout, also from
// relayout_when_paid): everything keyed by sites_gen -- the IBD0 pass, the fragment base, the images, a pending finalising
// step, stream3's order.  The row table does not depend on the layout (up_gen stays).
void layout_changed(ibdg_ctx *c) { ++c->sites_gen; }

// New background multiplicities: the IBD0 pass and the count towards "ibd0_after" (both keyed by bg_gen); a pending
// finalising step is flushed by the run that brings them (ibdg_run: same_bg).
void background_changed(ibdg_ctx *c) { ++c->bg.bg_gen; }

// Other comparison individuals in the ring: the images in wtarget / twords are another individual's
void targets_changed(ibdg_ctx *c, const uint32_t *targets, size_t T)
{
    c->prev_targets.assign(targets, targets + T);
    c->img.drop();
}

// src/ibd-math.c:5-23: C(i,j) = (i*C(i-1,j-1))/j in unsigned long; 0 for j>i.
std::vector<unsigned long> nck_table(unsigned n)
{
    size_t d = (size_t)n + 1;
    std::vector<unsigned long> t(d * d);
    for (size_t i = 0; i < d; ++i)
        for (size_t j = 0; j < d; ++j)
            t[i * d + j] = j == 0 ? 1ul
                                  : (i == 0 ? 0ul : ((unsigned long)(unsigned)i * t[(i - 1) * d + (j - 1)]) / (unsigned)j);
    return t;
}

// src/ibd-math.c:46-81 over the whole reachable (n_ref, n_alt) grid.
void build_pdg_table(double eps, unsigned M, double *out)
{
    const size_t d = (size_t)M + 1;
    std::vector<unsigned long> nck = nck_table(M);
    for (size_t r = 0; r < d; ++r) {
        for (size_t a = 0; a < d; ++a) {
            double *o = out + (r * d + a) * 3;
            if (r + a > M) {       // never reached: rows with n_ref+n_alt > M are filtered (ibdgem.c:623)
                o[0] = o[1] = o[2] = std::nan("");
                continue;
            }
            if (r == 0 && a == 0) {
                o[0] = o[1] = o[2] = 1.0;
                continue;
            }
            const unsigned long c = nck[(r + a) * d + r];
            const unsigned ur = (unsigned)r, ua = (unsigned)a;
            double p00 = (double)c * libm_pow(1 - eps, ur) * libm_pow(eps, ua);
            double p01 = (double)c * libm_pow(0.5, ur) * libm_pow(0.5, ua);
            double p11 = (double)c * libm_pow(1 - eps, ua) * libm_pow(eps, ur);
            o[0] = p00 == 0.0 ? DBL_MIN : p00;
            o[1] = p01 == 0.0 ? DBL_MIN : p01;
            o[2] = p11 == 0.0 ? DBL_MIN : p11;
        }
    }
}

// x = m * 2^e, m in [0.5,1): extended-precision mantissa so that tables of b^n stay accurate
// to ~1e-19 for any n (plain pow underflows long before n*log2(b) leaves the int range).
struct ME {
    long double m;
    long long e;
};

ME me_norm(long double x, long long e)
{
    int k = 0;
    long double m = frexpl(x, &k);
    return ME{m, e + k};
}

ME me_powl(ME b, uint64_t n)
{
    ME r = me_norm(1.0L, 0);
    while (n) {
        if (n & 1)
            r = me_norm(r.m * b.m, r.e + b.e);
        b = me_norm(b.m * b.m, 2 * b.e);
        n >>= 1;
    }
    return r;
}

ME me_pow(double base, uint64_t n)
{
    ME r = me_norm(1.0L, 0), b = me_norm((long double)base, 0);
    while (n) {
        if (n & 1)
            r = me_norm(r.m * b.m, r.e + b.e);
        b = me_norm(b.m * b.m, 2 * b.e);
        n >>= 1;
    }
    return r;
}

// The fast --LD kernel replaces products of table entries by K*(1-e)^E1*e^E2*2^-E3.  That is
// only the same number when every reachable entry IS C*(1-e)^r*e^a etc. to rounding: no
// DBL_MIN clamp (src/ibd-math.c:77-79), no overflowed coefficient, 0 < e < 1.
bool lut_is_binomial(const std::vector<double> &lut, const std::vector<unsigned long> &nck, double eps,
                     unsigned M)
{
    if (!(eps > 0.0 && eps < 1.0) || M > 50)
        return false;
    const size_t d = (size_t)M + 1;
    const long double b = (long double)(double)(1 - eps), e = (long double)eps;
    for (size_t r = 0; r < d; ++r)
        for (size_t a = 0; a + r <= M; ++a) {
            if (r + a == 0)
                continue;
            const long double c = (long double)nck[(r + a) * d + r];
            const long double want[3] = {c * powl(b, (long double)r) * powl(e, (long double)a),
                                         c * powl(0.5L, (long double)(r + a)),
                                         c * powl(b, (long double)a) * powl(e, (long double)r)};
            for (int g = 0; g < 3; ++g) {
                const long double got = lut[(r * d + a) * 3 + g];
                if (!(want[g] > 1e-280L) || fabsl(got - want[g]) > 1e-14L * want[g])
                    return false;
            }
        }
    return true;
}

int pick_cpw(uint32_t n_chunks, long opt)
{
    if (opt >= 1 && opt <= 5)
        return (int)opt;
    if (n_chunks >= 5)
        return 5;
    return (int)n_chunks;   // 1..4
}

// Lay the panel geometry out for n_ids individuals and allocate device rows.
int prepare_panel(ibdg_ctx *c, size_t n_rows, unsigned n_ids)
{
    if (n_ids == 0)
        return fail(c, "[::] ERROR in ibdg_upload_panel: n_ids must be >= 1");
    c->pan.n_ids = n_ids;
    c->pan.n_rows = n_rows;
    c->pan.n_chunks = (n_ids + 63) / 64;
    c->pan.cpw = pick_cpw(c->pan.n_chunks, c->opt.cpw);
    c->pan.n_groups = (c->pan.n_chunks + c->pan.cpw - 1) / c->pan.cpw;
    c->pan.stride = 2u * c->pan.cpw * c->pan.n_groups;
    panel_replaced(c);
    c->pan.n_pairs = (uint32_t)(((n_rows + 255) / 256) * 4);     // 64-row tile pairs, padded to whole 8-tile octs
    if (ensure(c, c->pan.panel, n_rows * (size_t)c->pan.stride * 8) || ensure(c, c->pan.alt_count, n_rows * 4))
        return 1;
    if (c->tab.pop_lut_ok && ensure(c, c->pan.t32, (size_t)c->pan.n_chunks * c->pan.n_pairs * 64 * 16))
        return 1;
    // ... and room for the compacted tiles of a site list on all these rows at the usual window sizes (32 ceil(W / 32) / W
    // <= 1.3: W = 100, 50, 75..., 97 and more), so that a re-layout in the middle of a series of runs does not allocate:
    // a hipMalloc of gigabytes is normally 0.2 ms but now and then 270-370 ms (after somebody's large hipFree:
    // tools/hipmalloc_in_process.py), which is 300 runs' worth.  Other windows grow it when their turn comes.
    if (c->tab.pop_lut_ok && c->opt.compact >= 0 && c->opt.reserve_compact &&
        ensure(c, c->lay.t32c, (size_t)c->pan.n_chunks * (size_t)(c->pan.n_pairs * 1.3 + 8) * 64 * 16))
        return 1;
    // pow(1-f,2.0), pow(f,2.0) for every possible alt count (src/ibd-math.c:93-95 with
    // f = k/(2N), src/ibd-parse.c:98)
    const size_t K = 2 * (size_t)n_ids + 1;
    std::vector<double> pt(2 * K);
    for (size_t k = 0; k < K; ++k) {
        const double f = (double)k / (double)(int)(2u * n_ids);
        pt[2 * k] = libm_pow(1 - f, 2.0);
        pt[2 * k + 1] = libm_pow(f, 2.0);
    }
    if (ensure(c, c->pan.pow_tab, pt.size() * 8))
        return 1;
    HIP_TRY(c, hipMemcpyAsync(c->pan.pow_tab.p, pt.data(), pt.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

// A large panel in ordinary (pageable) host memory: a team of host threads copies it piece by piece into
// page-locked staging buffers (two per thread) and every piece goes to the device by DMA as soon as it is
// staged.  The runtime's own path for pageable memory locks the caller's pages chunk by chunk, which is quick
// for memory in huge pages (46 GB/s for a fresh anonymous allocation) and slow for 4 KiB pages -- a mapped
// file from the page cache, the host program's packed-panel cache: 0.18-0.28 s for 2.56 GB.
struct StageJob {
    ibdg_ctx *c;
    const char *src;        // rows in host memory, or
    int fd = -1;            // ... (src == nullptr) in a file, from byte `off` on
    uint64_t off = 0;
    bool io_failed = false;
    size_t rw, dw, n_rows, rows_per_piece;
    int worker, n_workers;
    hipError_t err = hipSuccess;
};

void stage_worker(StageJob *j)
{
    ibdg_ctx *c = j->c;
    if ((j->err = hipSetDevice(c->device)) != hipSuccess)
        return;
    const size_t n_pieces = (j->n_rows + j->rows_per_piece - 1) / j->rows_per_piece;
    int turn = 0;
    for (size_t p = (size_t)j->worker; p < n_pieces; p += (size_t)j->n_workers, turn ^= 1) {
        const int b = 2 * j->worker + turn;
        const size_t r0 = p * j->rows_per_piece, nr = std::min(j->rows_per_piece, j->n_rows - r0);
        if ((j->err = hipEventSynchronize(c->stg.stage_ev[b])) != hipSuccess)     // the buffer's previous piece has left
            return;
        if (j->src) {
            memcpy(c->stg.stage[b], j->src + r0 * j->rw, nr * j->rw);
        } else {
            // straight from the file (the page cache) into the page-locked buffer: no mapping of the file, hence no page
            // faults here and no 2.56 GB of page-table entries to take down when the process ends
            size_t done = 0;
            const size_t want = nr * j->rw;
            while (done < want) {
                const ssize_t k = pread(j->fd, (char *)c->stg.stage[b] + done, want - done, (off_t)(j->off + r0 * j->rw + done));
                if (k <= 0) {
                    if (k < 0 && errno == EINTR)
                        continue;
                    j->io_failed = true;
                    return;
                }
                done += (size_t)k;
            }
        }
        j->err = hipMemcpy2DAsync((char *)c->pan.panel.p + r0 * j->dw, j->dw, c->stg.stage[b], j->rw, j->rw, nr,
                                  hipMemcpyHostToDevice, c->stream);
        if (j->err == hipSuccess)
            j->err = hipEventRecord(c->stg.stage_ev[b], c->stream);
        if (j->err != hipSuccess)
            return;
    }
}

int staged_upload(ibdg_ctx *c, const void *src, size_t n_rows, size_t rw, size_t dw, int fd = -1, uint64_t off = 0)
{
    int T = (int)std::min<unsigned>((unsigned)c->opt.stage_workers, std::max(1u, std::thread::hardware_concurrency()));
    const size_t rows_per_piece = std::max<size_t>(1, ibdg_ctx::Staging::BYTES / rw);
    for (int b = 0; b < 2 * T; ++b) {
        if (!c->stg.stage[b])
            HIP_TRY(c, hipHostMalloc(&c->stg.stage[b], ibdg_ctx::Staging::BYTES, hipHostMallocDefault));
        if (!c->stg.stage_ev[b]) {
            HIP_TRY(c, hipEventCreateWithFlags(&c->stg.stage_ev[b], hipEventDisableTiming));
            HIP_TRY(c, hipEventRecord(c->stg.stage_ev[b], c->stream));       // "free" from the start
        }
    }
    std::vector<StageJob> jobs((size_t)T);
    std::vector<std::thread> th;
    for (int w = 0; w < T; ++w) {
        jobs[(size_t)w].c = c;
        jobs[(size_t)w].src = (const char *)src;
        jobs[(size_t)w].fd = fd;
        jobs[(size_t)w].off = off;
        jobs[(size_t)w].rw = rw;
        jobs[(size_t)w].dw = dw;
        jobs[(size_t)w].n_rows = n_rows;
        jobs[(size_t)w].rows_per_piece = rows_per_piece;
        jobs[(size_t)w].worker = w;
        jobs[(size_t)w].n_workers = T;
        th.emplace_back(stage_worker, &jobs[(size_t)w]);
    }
    for (auto &t : th)
        t.join();
    for (const StageJob &j : jobs) {
        if (j.err != hipSuccess)
            return fail(c, "[::] ERROR in ibdg_upload_panel: staged copy: %s", hipGetErrorString(j.err));
        if (j.io_failed)
            return fail(c, "[::] ERROR in ibdg_upload_panel_fd: the file ends before the rows do, or cannot be read");
    }
    return 0;
}

bool is_plain_host_memory(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();          // unknown to the runtime: ordinary memory
        return true;
    }
    return a.type == hipMemoryTypeUnregistered;
}

int copy_rows(ibdg_ctx *c, const void *src, size_t n_rows, hipMemcpyKind kind, int fd = -1, uint64_t off = 0)
{
    const size_t rw = ibdg_row_words(c->pan.n_ids) * 8, dw = (size_t)c->pan.stride * 8;
    if (n_rows == 0)
        return 0;
    if (rw != dw)
        HIP_TRY(c, hipMemsetAsync(c->pan.panel.p, 0, n_rows * dw, c->stream));
    if (fd >= 0) {
        if (staged_upload(c, nullptr, n_rows, rw, dw, fd, off))
            return 1;
    } else if (kind == hipMemcpyHostToDevice && n_rows * rw >= ((size_t)256 << 20) && c->opt.staged_upload &&
        is_plain_host_memory(src)) {
        if (staged_upload(c, src, n_rows, rw, dw))
            return 1;
    } else {
        HIP_TRY(c, hipMemcpy2DAsync(c->pan.panel.p, dw, src, rw, rw, n_rows, kind, c->stream));
    }
    if (!c->opt.count_in_run) {
        ibdg::launch_alt_count((const uint64_t *)c->pan.panel.p, c->pan.stride, n_rows, (uint32_t *)c->pan.alt_count.p,
                               c->stream);
        HIP_TRY(c, hipGetLastError());
        c->pan.counts_valid = true;
    }
    if (c->tab.pop_lut_ok) {
        // second resident layout of the same bits for the fast --LD kernel
        ibdg::launch_transpose32((const uint64_t *)c->pan.panel.p, c->pan.stride, n_rows, c->pan.n_chunks, c->pan.n_pairs,
                                 (uint32_t *)c->pan.t32.p, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

// Runs of consecutive windows for the workgroups of the exponent-counting kernel: g windows each,
// except towards the end of the grid, where they shrink (guided self-scheduling: remaining
// windows / workgroups in flight): workgroups are handed out in blockIdx order, so the last
// ones to start are short and the CUs run dry together instead of waiting for one last
// full-length run.  A function of the window count alone.
void make_runs(const ibdg_ctx *c, uint32_t g, std::vector<uint32_t> &runs)
{
    const uint32_t n_cg = (c->pan.n_chunks + 7) / 8, wpg_waves = (c->pan.n_chunks + n_cg - 1) / n_cg;
    const uint32_t in_flight = std::max<uint32_t>(1, (uint32_t)(c->n_cu * (16 / wpg_waves) / n_cg) * (uint32_t)std::max<long>(1, c->opt.guided) / 4);
    runs.clear();
    for (uint32_t w = 0; w < c->sites.n_win;) {
        runs.push_back(w);
        uint32_t len = g;
        if (c->opt.guided)
            len = std::min(g, std::max<uint32_t>(1, (c->sites.n_win - w + in_flight - 1) / in_flight));
        w = std::min(w + len, c->sites.n_win);
    }
    runs.push_back(c->sites.n_win);
}

// rho^n, sigma^n and (1-eps)^n for n < need, in extended precision; the bases come from the doubles
// the reference uses (epsilon and 1-epsilon, src/ibd-math.c:58-61).  The tables depend on epsilon
// only, so a context builds every entry once and keeps it.  Returns false when an exponent leaves
// the range of the 32-bit fields (the strict kernel then serves).
bool grow_pow_tables(ibdg_ctx *c, size_t need)
{
    if (need > c->tab.tab_fail_from) return false;
    if (need <= c->tab.p1_h.size()) return true;
    const size_t old = c->tab.p1_h.size(), n = std::max(need, std::min<size_t>(old + old / 2 + 256, c->tab.tab_fail_from));
    const long double one_me = (long double)(double)(1 - c->tab.eps);
    const ME rho = me_norm((long double)c->tab.eps / one_me, 0), sigma = me_norm(0.5L / one_me, 0);
    // tau = rho / sigma^2 = 4 eps (1 - eps): the same long-double eps and 1 - eps as rho and sigma are made of
    const ME tau = me_norm(4.0L * (long double)c->tab.eps * one_me, 0);
    const auto resize = [&](size_t k) { c->tab.p1_h.resize(k); c->tab.p2_h.resize(k); c->tab.p3_h.resize(k); c->tab.pb_h.resize(k); };
    resize(n);
    for (size_t k = old; k < n; ++k) {
        const ME x = me_powl(rho, k), y = me_powl(sigma, k), z = me_pow(1 - c->tab.eps, k), u = me_powl(tau, k);
        if (x.e < -2000000000LL / 3 || y.e < -2000000000LL / 3 || z.e < -2000000000LL / 3 || u.e < -2000000000LL / 3 ||
            u.e > 2000000000LL / 3) {
            c->tab.tab_fail_from = k;
            resize(k);
            c->tab.tab_dev = std::min(c->tab.tab_dev, k);
            return need <= k;
        }
        c->tab.p1_h[k].m = (double)x.m; c->tab.p1_h[k].e = (int32_t)x.e; c->tab.p1_h[k].pad = 0;
        c->tab.p2_h[k].m = (double)y.m; c->tab.p2_h[k].e = (int32_t)y.e; c->tab.p2_h[k].pad = 0;
        c->tab.p3_h[k].m = (double)u.m; c->tab.p3_h[k].e = (int32_t)u.e; c->tab.p3_h[k].pad = 0;
        c->tab.pb_h[k].m = (uint64_t)ldexpl(z.m, 64);        // exact: a 64-bit mantissa in [2^63, 2^64)
        c->tab.pb_h[k].e = (int32_t)z.e;
        c->tab.pb_h[k].pad = 0;
    }
    return true;
}

// Poll of one word in host memory until it holds `seq`; every 4096 spins `query` says whether the producer is still
// at work (0 = yes, 1 = it has finished, anything else = it has failed) and the wall clock is looked at.
// Returns 0 = the word arrived, 1 = the producer finished without writing it, 2 = timed out, < 0 = -(query's code).
template <class Q>
int poll_seq(const volatile uint32_t *flag, uint32_t seq, double timeout_s, Q query)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 1; *flag != seq; ++spins) {
        if ((spins & 0xfff) != 0)
            continue;
        const int q = query();
        if (q != 0) {
            if (*flag == seq)
                break;
            return q == 1 ? 1 : -q;
        }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
            return *flag == seq ? 0 : 2;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return 0;
}

double wait_timeout_s()
{
    // ten seconds: a preparation stage is a few hundred microseconds of device work.  (IBDG_WAIT_TIMEOUT_MS: for tests.)
    if (const char *e = getenv("IBDG_WAIT_TIMEOUT_MS"))
        return atof(e) * 1e-3;
    return 10.0;
}

// Wait until the preparation kernels have handed hand-over number `seq` of PrepInfo to the host's mirror: a poll of
// one word in host memory, which the last workgroup of the stage writes -- no copy to queue, no stream to drain
// (each of those is a round trip of 10-15 us; an upload has two).  The stream is asked now and then whether it
// has died under us, and the poll is bounded by wall time: a stream that neither finishes nor fails (a wedged queue)
// ends the call with an error instead of a host thread spinning for ever.  (The messages say ibdg_upload_sites whichever
// entry point the stage belongs to, like upload_sites_check's.)
int wait_info(ibdg_ctx *c, uint32_t seq)
{
    hipError_t last = hipSuccess;
    const int rc = poll_seq(&c->sites.info_h->seq, seq, wait_timeout_s(), [&]() {
        last = hipStreamQuery(c->stream);
        return last == hipErrorNotReady ? 0 : (last == hipSuccess ? 1 : 2);
    });
    if (rc == 0) return 0;
    if (rc == 1) return fail(c, "[::] ERROR in ibdg_upload_sites: the site preparation finished without reporting");
    if (rc == 2)
        return fail(c, "[::] ERROR in ibdg_upload_sites: the site preparation did not report within %.0f s (stream: %s)",
                    wait_timeout_s(), hipGetErrorString(hipStreamQuery(c->stream)));
    return fail(c, "[::] ERROR in ibdg_upload_sites: %s", hipGetErrorString(last));
}

// A PrepInfo nothing has been reported into: the device's block between uploads, and the mirror of an empty site list
ibdg::PrepInfo empty_prep_info()
{
    ibdg::PrepInfo i{};
    i.err_row_site = i.err_cov_site = i.first_row = 0xffffffffu;
    return i;
}

// One stage of the preparation and its hand-over (the protocol: ibdg_ctx::Sites).  launch(seq) queues the stage, whose last
// workgroup hands over as number seq, with the event records and waits that belong to it.  prep_dirty stays set on failure.
template <class L>
int hand_over(ibdg_ctx *c, L launch)
{
    c->sites.prep_dirty = true;
    const uint32_t seq = ++c->sites.prep_seq;
    if (launch(seq)) return 1;
    HIP_TRY(c, hipGetLastError());
    if (wait_info(c, seq)) return 1;
    c->sites.prep_dirty = false;                      // the stage's last workgroup has left everything clean
    return 0;
}

// ---- Segments, per-window constants, control words and power tables of the fast --LD kernel, built on the device from the
// covered-row list (ibdg_prep.hip); the host keeps what depends on the window count only (the run structure) and the
// epsilon-only power tables.  build_segments: plan, stages, verdict, commit. ----

enum class Built { yes, not_applicable, failed };     // not_applicable: this layout does not serve the list, another may

// One attempt at a layout: what plan_layout decides before anything is queued, then what stage B reported (cut_segments)
struct LayoutTry {
    bool compact = false;
    uint32_t win_rows = 0, n_pairs_c = 0;   // compacted tiles: virtual rows per window, tile pairs of them all (else 0)
    uint32_t seg_cap = 0, ring = 0;         // segments the device may write; ring depth of the control words
    uint32_t g = 0, n_runs = 0;             // windows per workgroup run: the first length, then the one the cut ended on
    ibdg::PrepInfo rep{};                   // stage B's last hand-over: n_segs, ct_max, max_seg, out_of_order, adv_overflow
    int tab_in_lds() const { return (size_t)(rep.ct_max + 1) * 32 <= 24 * 1024; }
    // what no run length mends: rows out of file order on the panel's own tiles; segments over the capacity (the device stopped writing)
    bool beyond_mending() const { return (!compact && rep.out_of_order) || rep.n_segs > seg_cap; }
};

// Returns false where the compacted tiles' row or pair numbers would leave 31 bits.  Touches no device, writes nothing into c.
bool plan_layout(const ibdg_ctx *c, bool compact, LayoutTry &P)
{
    // virtual rows per window of the compacted layout: the window rounded up to the alignment asked for (1 = the rows back
    // to back, 32 = every window on a tile boundary)
    const uint32_t align = (uint32_t)std::min<long>(32, std::max<long>(1, c->opt.compact_align));
    const uint64_t win_rows = ((uint64_t)c->sites.window + align - 1) / align * align;
    const uint64_t vtiles = ((uint64_t)c->sites.n_win * win_rows + 31) / 32;        // tiles of all its virtual rows
    const uint64_t pairs = (vtiles + 1) / 2;
    if (compact && (win_rows >= (1ull << 31) || pairs >= (1ull << 31))) return false;
    P.compact = compact; P.win_rows = compact ? (uint32_t)win_rows : 0u;
    P.n_pairs_c = compact ? (uint32_t)((pairs + 3) & ~3ull) : 0u;
    // segments <= windows + tiles spanned when the rows are in file order (otherwise the device stops
    // writing at the capacity and the exponent-counting kernel is not used); never more than stage A cleared
    uint64_t seg_cap = c->sites.n_cov;
    const uint32_t first_row = c->sites.first_row, last_row = c->sites.last_row;
    if (compact)
        seg_cap = std::min<uint64_t>(seg_cap, (uint64_t)c->sites.n_win + vtiles + 1);
    else if (last_row >= first_row)
        seg_cap = std::min<uint64_t>(seg_cap, (uint64_t)c->sites.n_win + ((last_row >> 5) - (first_row >> 5)) + 1);
    P.seg_cap = (uint32_t)std::min<uint64_t>(seg_cap, c->sites.seg_room);
    // windows per workgroup run: as many as keep the run's records within the LDS budget (cut_segments halves it)
    P.g = (uint32_t)std::max<long>(1, c->opt.wpg);
    if (!c->opt.guided && !c->opt.wpg_fixed) {
        // uniform runs and few windows (a shard of a chromosome, a small region): shorter runs, so that
        // the grid still holds several rounds of workgroups for every CU
        const uint64_t rows_of_blocks = (c->pan.n_chunks + 7) / 8;
        const uint64_t want_blocks = (uint64_t)c->n_cu * 2 * 5;          // CUs x resident blocks x rounds
        P.g = (uint32_t)std::min<uint64_t>(P.g, std::max<uint64_t>(1, (uint64_t)c->sites.n_win * rows_of_blocks / want_blocks));
    }
    P.ring = (uint32_t)c->opt.ring;
    return true;
}

// What stage B reads besides stage A's records and where it writes the windows' constants: the compacted tiles (the rows
// with reads, gathered and transposed into tiles that start with their window) and, once per context, the binomial coefficients
int layout_inputs(ibdg_ctx *c, const LayoutTry &T)
{
    if (T.compact) {
        if (ensure(c, c->lay.t32c, (size_t)c->pan.n_chunks * T.n_pairs_c * 64 * 16)) return 1;
        ibdg::launch_gather_transpose32((const uint64_t *)c->pan.panel.p, c->pan.stride, (const uint2 *)c->sites.rec_cov.p, c->sites.n_cov,
                                        c->sites.window, T.win_rows, c->pan.n_chunks, T.n_pairs_c, (uint32_t *)c->lay.t32c.p, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    if (ensure(c, c->lay.wconst, ((size_t)c->sites.n_win + 1) * sizeof(ibdg::WinConst))) return 1;
    if (ensure(c, c->lay.wraw, (size_t)c->sites.n_win * sizeof(ibdg::WinRaw))) return 1;
    if (c->tab.nck_dev.p) return 0;
    // the coefficients normalised here (C << clz(C), 64 - clz(C)): the device multiplies them as they are
    std::vector<ibdg::WinRaw> nn(c->tab.nck_h.size());
    for (size_t i = 0; i < nn.size(); ++i) {
        const unsigned long v = c->tab.nck_h[i];
        const int z = v ? __builtin_clzl(v) : 63;
        nn[i] = {v ? (uint64_t)v << z : (uint64_t)1 << 63, v ? 64 - z : 1, 0};         // (0 is never looked up: r <= cov)
    }
    if (ensure(c, c->tab.nck_dev, nn.size() * sizeof(ibdg::WinRaw))) return 1;
    // (a blocking copy, once per context: the kernel that reads the table runs on the second stream)
    HIP_TRY(c, hipMemcpy(c->tab.nck_dev.p, nn.data(), nn.size() * sizeof(ibdg::WinRaw), hipMemcpyHostToDevice));
    return 0;
}

// Stage B for the run structure in c->lay.runs.  The first pass cuts the segments, whose last kernel makes the control
// words for that structure; a later pass makes the control words anew for another one.
int queue_stage_b(ibdg_ctx *c, const ibdg::PrepSegArgs &sa, uint32_t n_runs, uint32_t ring, uint32_t seq, bool first_pass)
{
    const uint32_t *runs = (const uint32_t *)c->lay.runs.p;
    if (first_pass) {
        // (stream2 is idle: ibdg_upload_sites drained both streams before it began; it waits for stage A's records)
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->sites.ev_prepA, 0));
        ibdg::launch_prep_segments(sa, runs, n_runs, ring, c->stream, c->stream2);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->sites.ev_prep2, c->stream2));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->sites.ev_prep2, 0));      // before the hand-over (ct_max) and K'
    }
    ibdg::launch_prep_seg_flags(sa, runs, n_runs, ring, seq, c->stream, !first_pass);
    return 0;
}

// Stage B's first pass on runs of P.g windows, then the run length halved until a run's records fit the LDS budget
int cut_segments(ibdg_ctx *c, LayoutTry &T)
{
    ibdg::PrepSegArgs sa;
    sa.rec_cov = (const uint2 *)c->sites.rec_cov.p; sa.n_cov = c->sites.n_cov; sa.window = c->sites.window; sa.n_win = c->sites.n_win;
    sa.max_cov = c->tab.max_cov; sa.nck = (const ibdg::WinRaw *)c->tab.nck_dev.p; sa.compact = T.win_rows;
    sa.segs = (ibdg::Seg *)c->lay.segs.p; sa.seg_first = (uint32_t *)c->lay.seg_first.p; sa.seg_cap = T.seg_cap;
    sa.wconst = (ibdg::WinConst *)c->lay.wconst.p; sa.raw = (ibdg::WinRaw *)c->lay.wraw.p;
    sa.block_tmp = (uint32_t *)c->sites.scan_tmp.p; sa.info = (ibdg::PrepInfo *)c->sites.info_dev.p; sa.mirror = c->sites.info_h;
    for (bool first_pass = true;; T.g = (T.g + 1) / 2, first_pass = false) {
        // the run structure goes ahead of the kernels that make the control words for it
        make_runs(c, T.g, c->lay.runs_h);
        T.n_runs = (uint32_t)c->lay.runs_h.size() - 1;
        if (ensure(c, c->lay.runs, c->lay.runs_h.size() * 4)) return 1;
        // runs_h is a member: it outlives the copy (the next wait is the hand-over's)
        HIP_TRY(c, hipMemcpyAsync(c->lay.runs.p, c->lay.runs_h.data(), c->lay.runs_h.size() * 4, hipMemcpyHostToDevice, c->stream));
        if (hand_over(c, [&](uint32_t seq) { return queue_stage_b(c, sa, T.n_runs, T.ring, seq, first_pass); })) return 1;
        T.rep = *c->sites.info_h;
        if (T.beyond_mending() || (size_t)T.rep.max_seg * (sizeof(ibdg::Seg) + 8) <= (size_t)c->opt.recbytes || T.g == 1)
            return 0;
    }
}

// Every reason why the layout that was cut does not serve, in the order they are asked: rows out of file order on the
// panel's own tiles, segments over the capacity; rows too far apart for the record format (adv_overflow); a single window with
// thousands of tiles (LDS above 150 KiB); a power that leaves the 32-bit exponent field (asking grows the host's tables).
bool layout_refused(ibdg_ctx *c, const LayoutTry &T)
{
    return T.beyond_mending() || T.rep.adv_overflow ||
           ibdg::ld_popcount_lds_bytes(T.rep.max_seg, T.g, T.rep.ct_max + 1, T.tab_in_lds(), (int)T.ring, 0) > 150 * 1024 ||
           !grow_pow_tables(c, (size_t)T.rep.ct_max + 1);
}

// An accepted layout takes effect: the power tables' new entries, K', and c->lay's scalar fields (their only writer)
int commit_layout(ibdg_ctx *c, const LayoutTry &T)
{
    if (c->tab.tab_dev < c->tab.p1_h.size()) {     // new entries since the last upload
        const size_t n = c->tab.p1_h.size(), pe = n * sizeof(ibdg::PowEntry), wr = n * sizeof(ibdg::WinRaw);
        if (ensure(c, c->tab.pow1, pe) || ensure(c, c->tab.pow2, pe) || ensure(c, c->tab.pow3, pe) || ensure(c, c->tab.powb, wr)) return 1;
        HIP_TRY(c, hipMemcpyAsync(c->tab.pow3.p, c->tab.p3_h.data(), pe, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->tab.pow1.p, c->tab.p1_h.data(), pe, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->tab.pow2.p, c->tab.p2_h.data(), pe, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->tab.powb.p, c->tab.pb_h.data(), wr, hipMemcpyHostToDevice, c->stream));
        c->tab.tab_dev = n;
    }
    // K' = K * (1-eps)^(all reads of the window): with it a product is K' * rho^E2 * sigma^E3,
    // rho = eps/(1-eps), sigma = 1/(2(1-eps))  (E1 = reads - E2 - E3 eliminated)
    ibdg::launch_prep_win_kp(c->sites.n_win, (const ibdg::WinRaw *)c->lay.wraw.p, (const ibdg::WinRaw *)c->tab.powb.p,
                             (ibdg::WinConst *)c->lay.wconst.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    ibdg_ctx::Layout &L = c->lay;
    L.compact = T.compact;
    if (T.compact) L.n_pairs_c = T.n_pairs_c;
    L.wpg = T.g; L.n_runs = T.n_runs; L.seg_ring = (int)T.ring;
    L.max_seg = T.rep.max_seg; L.n_segs = T.rep.n_segs; L.ct_max = T.rep.ct_max; L.tab_in_lds = T.tab_in_lds();
    L.pop_sites_ok = true;
    layout_changed(c);
    return 0;
}

// One attempt at one layout.  It overwrites the buffers of the layout before (segments, constants, runs), so there is none
// from its start on; only an accepted one reaches commit_layout -- a refused or failed attempt leaves pop_sites_ok false
// and no other scalar of c->lay touched.  (The caller has seen to pop_lut_ok and n_cov > 0.)
Built build_segments(ibdg_ctx *c, bool compact)
{
    LayoutTry T;
    c->lay.pop_sites_ok = false;
    if (!plan_layout(c, compact, T)) return Built::not_applicable;
    if (layout_inputs(c, T) || cut_segments(c, T)) return Built::failed;
    if (layout_refused(c, T)) return Built::not_applicable;
    return commit_layout(c, T) ? Built::failed : Built::yes;
}

// Sparse coverage: on the panel's own tiles the exponent-counting kernels stream every 32-row tile between a
// window's first and last row, whether its rows carry reads or not; on the compacted tiles a window costs
// ceil(window / 32) tile words whatever the density, plus its share of the gather (~6 tile words' worth of time per
// 100 rows).  Below about one covered row in four the compacted layout is the faster one for a single run.
bool sparse_sites(const ibdg_ctx *c)
{
    if (c->sites.last_row < c->sites.first_row) return true;        // not even the ends are in file order
    const uint64_t span = (uint64_t)c->sites.last_row - c->sites.first_row + 1;
    return (uint64_t)c->sites.n_cov * (uint64_t)std::max<long>(1, c->opt.compact_density) < span;
}

// Segments for the layout the options and the site list ask for; the compacted one also serves when the panel's own
// tiles turn out not to apply (rows out of file order, rows too far apart for the control words).
int build_layout(ibdg_ctx *c)
{
    c->lay.pop_sites_ok = false;
    c->lay.compact = false;
    c->lay.pop_dense_enough = true;
    if (!c->tab.pop_lut_ok || c->sites.n_cov == 0) return 0;
    const bool sparse = sparse_sites(c);
    const bool want_compact = c->opt.compact > 0 || (c->opt.compact == 0 && sparse);
    Built b = build_segments(c, want_compact);
    if (b == Built::not_applicable && !want_compact && c->opt.compact == 0)
        b = build_segments(c, true);
    if (b == Built::failed) return 1;
    if (c->opt.compact < 0 && sparse)
        c->lay.pop_dense_enough = false;       // the caller forbade the layout this pileup wants: the strict kernel is the faster one
    return 0;
}

}  // namespace

extern "C" {

int ibdg_abi_version(void) { return IBDG_ABI_VERSION; }

int ibdg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

const char *ibdg_last_error(const ibdg_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int ibdg_pdg_table(double epsilon, unsigned max_cov, double *out)
{
    if (!out || max_cov < 1 || max_cov > 127)
        return 1;
    build_pdg_table(epsilon, max_cov, out);
    return 0;
}

// src/ibd-math.c:84-101 in k_site's operation order
double ibdg_pdg_ibd0(double f, double p00, double p01, double p11)
{
    if (p00 == 1 || p01 == 1 || p11 == 1)
        return 1.0;
    const double omf = 1 - f;
    const double t1 = libm_pow(omf, 2.0) * p00;
    const double t2 = ((2 * omf) * f) * p01;
    const double t3 = libm_pow(f, 2.0) * p11;
    double v = (t1 + t2) + t3;
    if (v == 0.0)
        v = DBL_MIN;
    return v;
}

// src/ibd-math.c:104-142
double ibdg_pdg_ibd1(unsigned a0, unsigned a1, double f, double p00, double p01, double p11)
{
    if (a0 > 1 || a1 > 1)
        return 1.0;                         // no branch of the reference's switch is taken
    const double omf = 1 - f;
    const unsigned g = a0 + a1;
    double v;
    if (g == 0)
        v = (f * p01) + (omf * p00);
    else if (g == 1)
        v = ((0.5 * p01) + ((0.5 * omf) * p00)) + ((0.5 * f) * p11);
    else
        v = (omf * p01) + (f * p11);
    if (v == 0.0)
        v = DBL_MIN;
    return v;
}

ibdg_ctx *ibdg_create(int device, double epsilon, unsigned max_cov)
{
    if (max_cov < 1 || max_cov > 127) {   // -M >= 1 (ibdgem.c:978); pileup rows have cov < 128 (pileup.c:223)
        fail(nullptr, "[::] ERROR: Invalid maximum estimated coverage (-M) of %u (must be 1..127).", max_cov);
        return nullptr;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        fail(nullptr, "[::] ERROR in ibdg_create: no HIP device available (%s); this engine has no CPU path",
             e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return nullptr;
    }
    if (device < 0 || device >= n) {
        fail(nullptr, "[::] ERROR in ibdg_create: device %d out of range (0..%d)", device, n - 1);
        return nullptr;
    }
    ibdg_ctx *c = new ibdg_ctx;
    c->device = device;
    c->tab.eps = epsilon;
    c->tab.max_cov = max_cov;
    auto bail = [&](const char *what, hipError_t err) {
        fail(nullptr, "[::] ERROR in ibdg_create: %s: %s", what, hipGetErrorString(err));
        ibdg_destroy(c);
        return (ibdg_ctx *)nullptr;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess)
        return bail("hipStreamCreate", e);
    {
        // stream2 carries the short memory-bound kernels (alt counts, per-site values, window products) beside the
        // --LD kernel, whose workgroups fill every wave slot of the chip: at the highest priority its workgroups
        // take the slots that free up first instead of queueing behind ~17 000 --LD workgroups
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess)
            lo = hi = 0;
        if ((e = hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, hi)) != hipSuccess)
            return bail("hipStreamCreate", e);
        if ((e = hipStreamCreateWithPriority(&c->stream3, hipStreamNonBlocking, hi)) != hipSuccess)
            return bail("hipStreamCreate", e);
        if ((e = hipEventCreateWithFlags(&c->ring.ready, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&c->ring.ev_s3sync, hipEventDisableTiming)) != hipSuccess)
            return bail("hipEventCreate", e);
    }
    for (auto &E : c->tl.evs) {
        for (hipEvent_t *ev : {&E.start_own, &E.ld_end, &E.k_start, &E.k_stop, &E.s2_start, &E.s2_count, &E.s2_end, &E.prep})
            if ((e = hipEventCreate(ev)) != hipSuccess) return bail("hipEventCreate", e);
    }
    for (hipEvent_t &ev : c->sites.ev_up)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreateWithFlags(&c->sites.ev_prep2, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreateWithFlags(&c->sites.ev_prepA, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    // (coherent: the kernels' stores must reach the host while the stream is still busy, not at its next drain)
    if ((e = hipHostMalloc((void **)&c->sites.info_h, sizeof(ibdg::PrepInfo), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess)
        return bail("hipHostMalloc", e);
    memset(c->sites.info_h, 0, sizeof(ibdg::PrepInfo));
    {
        int n_cu = 0;
        if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n_cu > 0)
            c->n_cu = n_cu;
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess)
            c->dev_mem_bytes = mem_total;
    }
    const size_t d = (size_t)max_cov + 1;
    c->tab.lut_h.resize(d * d * 3);
    build_pdg_table(epsilon, max_cov, c->tab.lut_h.data());
    c->tab.nck_h = nck_table(max_cov);
    c->tab.pop_lut_ok = lut_is_binomial(c->tab.lut_h, c->tab.nck_h, epsilon, max_cov);
    c->lay.planes = 1;
    while ((1u << c->lay.planes) <= max_cov)
        ++c->lay.planes;
    if (ensure(c, c->tab.lut, c->tab.lut_h.size() * 8)) {
        fail(nullptr, "%s", c->err.c_str());
        ibdg_destroy(c);
        return nullptr;
    }
    if ((e = hipMemcpy(c->tab.lut.p, c->tab.lut_h.data(), c->tab.lut_h.size() * 8, hipMemcpyHostToDevice)) != hipSuccess)
        return bail("hipMemcpy(lut)", e);
    return c;
}

void ibdg_destroy(ibdg_ctx *c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->device);
    if (c->stream3)
        (void)hipStreamSynchronize(c->stream3);
    if (c->stream2)
        (void)hipStreamSynchronize(c->stream2);
    if (c->stream)
        (void)hipStreamSynchronize(c->stream);
    c->free_bufs();
    for (hipEvent_t ev : c->sites.ev_up)
        if (ev)
            (void)hipEventDestroy(ev);
    if (c->sites.ev_prep2)
        (void)hipEventDestroy(c->sites.ev_prep2);
    if (c->sites.ev_prepA)
        (void)hipEventDestroy(c->sites.ev_prepA);
    for (int b = 0; b < 2 * ibdg_ctx::Staging::WORKERS; ++b) {
        if (c->stg.stage_ev[b])
            (void)hipEventDestroy(c->stg.stage_ev[b]);
        if (c->stg.stage[b])
            (void)hipHostFree(c->stg.stage[b]);
    }
    if (c->sites.info_h)
        (void)hipHostFree(c->sites.info_h);
    for (auto &E : c->tl.evs)
        for (hipEvent_t ev : {E.start_own, E.ld_end, E.k_start, E.k_stop, E.s2_start, E.s2_count, E.s2_end, E.prep})
            if (ev)
                (void)hipEventDestroy(ev);
    for (int i = 0; i < ibdg_ctx::Ring::STAGE_SLOTS; ++i) {
        if (c->ring.stage[i])
            (void)hipHostFree(c->ring.stage[i]);
        if (c->ring.stage_ev[i])
            (void)hipEventDestroy(c->ring.stage_ev[i]);
    }
    for (hipEvent_t ev : {c->ring.ready, c->ring.ev_s3sync, c->fb.ev_fb})
        if (ev)
            (void)hipEventDestroy(ev);
    if (c->stream3)
        (void)hipStreamDestroy(c->stream3);
    if (c->stream2)
        (void)hipStreamDestroy(c->stream2);
    if (c->stream)
        (void)hipStreamDestroy(c->stream);
    delete c;
}

size_t ibdg_row_words(unsigned n_ids) { return 2 * (((size_t)n_ids + 63) / 64); }

void ibdg_pack_alleles(const uint8_t *alleles, unsigned n_ids, uint64_t *row)
{
    const size_t words = ibdg_row_words(n_ids);
    memset(row, 0, words * 8);
    for (unsigned n = 0; n < n_ids; ++n) {
        const size_t w = 2 * (size_t)(n >> 6);
        const uint64_t bit = 1ull << (n & 63);
        if (alleles[2 * n] == 1) row[w] |= bit;
        if (alleles[2 * n + 1] == 1) row[w + 1] |= bit;
    }
}

int ibdg_pack_hap_text(const char *line, unsigned n_ids, uint64_t *row)
{
    const size_t words = ibdg_row_words(n_ids);
    memset(row, 0, words * 8);
    const size_t need = 4 * (size_t)n_ids - 1;
    if (strnlen(line, need) < need)
        return 1;
    int bad = 0;
    for (unsigned n = 0; n < n_ids; ++n) {
        const char c0 = line[4 * (size_t)n], c1 = line[4 * (size_t)n + 2];
        const size_t w = 2 * (size_t)(n >> 6);
        const uint64_t bit = 1ull << (n & 63);
        if (c0 == '1') row[w] |= bit; else if (c0 != '0') bad = 1;
        if (c1 == '1') row[w + 1] |= bit; else if (c1 != '0') bad = 1;
    }
    return bad;
}

int ibdg_upload_panel(ibdg_ctx *c, const uint64_t *rows, size_t n_rows, unsigned n_ids)
{
    if (!c) return 1;
    if (!rows && n_rows) return fail(c, "[::] ERROR in ibdg_upload_panel: rows is NULL");
    if (quiesce(c)) return 1;
    if (prepare_panel(c, n_rows, n_ids)) return 1;
    return copy_rows(c, rows, n_rows, hipMemcpyHostToDevice);
}

int ibdg_upload_panel_fd(ibdg_ctx *c, int fd, uint64_t offset, size_t n_rows, unsigned n_ids)
{
    if (!c) return 1;
    if (fd < 0) return fail(c, "[::] ERROR in ibdg_upload_panel_fd: not an open file");
    if (quiesce(c)) return 1;
    if (prepare_panel(c, n_rows, n_ids)) return 1;
    return copy_rows(c, nullptr, n_rows, hipMemcpyHostToDevice, fd, offset);
}

int ibdg_upload_panel_dev(ibdg_ctx *c, const void *dev_rows, size_t n_rows, unsigned n_ids)
{
    if (!c) return 1;
    if (!dev_rows && n_rows) return fail(c, "[::] ERROR in ibdg_upload_panel_dev: rows is NULL");
    if (quiesce(c)) return 1;
    if (prepare_panel(c, n_rows, n_ids)) return 1;
    // the source may have been produced on another stream (e.g. torch's): make it visible first
    HIP_TRY(c, hipDeviceSynchronize());
    return copy_rows(c, dev_rows, n_rows, hipMemcpyDeviceToDevice);
}

// The device's PrepInfo starts clean; afterwards every upload leaves it so (k_prep_scan, k_prep_mirror) -- unless it
// stopped half way: prep_dirty
static int clean_prep_info(ibdg_ctx *c)
{
    const bool fresh_info = !c->sites.info_dev.p;
    if (ensure(c, c->sites.info_dev, sizeof(ibdg::PrepInfo))) return 1;
    if (fresh_info || c->sites.prep_dirty) {
        const ibdg::PrepInfo init = empty_prep_info();
        HIP_TRY(c, hipMemcpyAsync(c->sites.info_dev.p, &init, sizeof init, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));          // `init` is a local
        c->sites.prep_dirty = false;
    }
    return 0;
}

// The -A triples {f, pow(1-f,2), pow(f,2)} with the host's libm, {NaN, 0, 0} where no frequency is given; whether any is
static bool fo_triples(const double *f_override, size_t n, std::vector<double> &out)
{
    bool any = false;
    out.resize(3 * n);
    for (size_t s = 0; s < n; ++s) {
        const double f = f_override[s];
        out[3 * s] = f;
        out[3 * s + 1] = f == f ? libm_pow(1 - f, 2.0) : 0.0;
        out[3 * s + 2] = f == f ? libm_pow(f, 2.0) : 0.0;
        any |= f == f;
    }
    return any;
}

// The steps of an upload of sites, in upload_sites_core's order.  First the buffers of stages A and B:
static int size_site_buffers(ibdg_ctx *c, size_t n_sites, unsigned window)
{
    // segments of stage B: at most one per site, and in file order at most windows + tiles of the panel
    // (compacted tiles: windows + tiles of their virtual rows, at most window + 31 per window)
    const size_t n_win_max = (n_sites + window - 1) / window;
    const size_t seg_room = std::min<size_t>(n_sites, std::max<size_t>(n_win_max + (c->pan.n_rows + 31) / 32 + 1,
                                                                      n_win_max + (n_win_max * ((size_t)window + 31) + 31) / 32 + 1));
    if (ensure(c, c->sites.rec_all, n_sites * 8) || ensure(c, c->sites.rec_cov, n_sites * 8) || ensure(c, c->sites.cov_site, n_sites * 4) ||
        ensure(c, c->sites.scan_tmp, ibdg::prep_scan_blocks(std::max<size_t>(n_sites, 1)) * 4) || clean_prep_info(c) ||
        (c->tab.pop_lut_ok && (ensure(c, c->lay.segs, seg_room * sizeof(ibdg::Seg)) || ensure(c, c->lay.seg_first, seg_room * 4))))
        return 1;
    c->sites.seg_room = c->tab.pop_lut_ok ? seg_room : 0;
    return 0;
}

// Stage A: the site records, the covered rows and their count, the first offending site
static int queue_stage_a(ibdg_ctx *c, const uint32_t *d_row, const uint8_t *d_ref, const uint8_t *d_alt, size_t n_sites, uint32_t seq)
{
    ibdg::PrepSiteArgs pa;
    pa.row_index = d_row; pa.n_ref = d_ref; pa.n_alt = d_alt; pa.n_sites = n_sites; pa.n_rows = c->pan.n_rows; pa.max_cov = c->tab.max_cov;
    pa.rec_all = (uint2 *)c->sites.rec_all.p; pa.rec_cov = (uint2 *)c->sites.rec_cov.p; pa.cov_site = (uint32_t *)c->sites.cov_site.p;
    pa.block_tmp = (uint32_t *)c->sites.scan_tmp.p; pa.info = (ibdg::PrepInfo *)c->sites.info_dev.p; pa.mirror = c->sites.info_h; pa.seq = seq;
    ibdg::launch_prep_sites(pa, c->stream);
    HIP_TRY(c, hipGetLastError());
    // (the hand-over comes from the scan, BEFORE the scatter kernel: whatever reads the site records on the second
    // stream waits for this event; the main stream is ordered anyway)
    HIP_TRY(c, hipEventRecord(c->sites.ev_prepA, c->stream));
    return 0;
}

// The selection in front of stage A (-v): the candidates at which `target` is not 0/0 into in_row / in_ref / in_alt (and
// fo), their candidate numbers into sel_cand, their count into the mirror's n_cov
static int queue_selection(ibdg_ctx *c, uint32_t target, uint32_t seq)
{
    ibdg::SelectArgs sa;
    sa.row = c->cand.have_rows ? (const uint32_t *)c->cand.row.p : nullptr; sa.fo = c->cand.have_fo ? (const double *)c->cand.fo.p : nullptr;
    sa.n_ref = (const uint8_t *)c->cand.ref.p; sa.n_alt = (const uint8_t *)c->cand.alt.p; sa.n_cand = c->cand.n_cand; sa.target = target;
    sa.t32 = c->tab.pop_lut_ok ? (const uint4 *)c->pan.t32.p : nullptr;      // (no transposed panel with a clamped table)
    sa.n_pairs = c->pan.n_pairs; sa.panel = (const uint64_t *)c->pan.panel.p; sa.stride = c->pan.stride;
    sa.out_row = (uint32_t *)c->sites.in_row.p; sa.out_ref = (uint8_t *)c->sites.in_ref.p; sa.out_alt = (uint8_t *)c->sites.in_alt.p;
    sa.out_cand = (uint32_t *)c->cand.sel_cand.p; sa.out_fo = (double *)c->sites.fo.p;
    sa.block_tmp = (uint32_t *)c->sites.scan_tmp.p; sa.info = (ibdg::PrepInfo *)c->sites.info_dev.p; sa.mirror = c->sites.info_h; sa.seq = seq;
    ibdg::launch_select_sites(sa, c->stream);
    return 0;
}

// The first offending site in file order, its row checked before its counts (as a loop over the sites would); 0: there is none
static int report_bad_site(ibdg_ctx *c, const uint32_t *d_row, const uint8_t *d_ref, const uint8_t *d_alt)
{
    const ibdg::PrepInfo &I = *c->sites.info_h;
    if (I.err_row_site == 0xffffffffu && I.err_cov_site == 0xffffffffu) return 0;
    c->sites.n_sites = 0;
    if (I.err_row_site <= I.err_cov_site) {
        uint32_t row = 0;
        HIP_TRY(c, hipMemcpy(&row, d_row + I.err_row_site, 4, hipMemcpyDeviceToHost));
        return fail(c, "[::] ERROR in ibdg_upload_sites: row_index[%zu]=%u outside the panel (%zu rows)",
                    (size_t)I.err_row_site, row, c->pan.n_rows);
    }
    uint8_t r = 0, a = 0;
    HIP_TRY(c, hipMemcpy(&r, d_ref + I.err_cov_site, 1, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(&a, d_alt + I.err_cov_site, 1, hipMemcpyDeviceToHost));
    return fail(c, "[::] ERROR in ibdg_upload_sites: site %zu has n_ref+n_alt=%u > max_cov=%u",
                (size_t)I.err_cov_site, (unsigned)r + a, c->tab.max_cov);
}

// Everything an upload of sites does once the three input arrays are on the device.  fo_ready: the sites' -A triples are in
// c->sites.fo already (ibdg_select_variable_sites compacts the candidates' there); f_override is not looked at.
static int upload_sites_core(ibdg_ctx *c, const uint32_t *d_row, const uint8_t *d_ref, const uint8_t *d_alt,
                             const double *f_override, size_t n_sites, unsigned window, bool fo_ready = false)
{
    sites_replaced(c);
    c->sites.n_sites = n_sites;
    c->sites.window = window;
    if (size_site_buffers(c, n_sites, window)) return 1;
    ibdg::PrepInfo &I = *c->sites.info_h;
    if (n_sites && hand_over(c, [&](uint32_t seq) { return queue_stage_a(c, d_row, d_ref, d_alt, n_sites, seq); })) return 1;
    if (n_sites == 0) {                           // nothing was launched: the mirror as stage A would have left it
        I = empty_prep_info();
        I.seq = c->sites.prep_seq;
    }
    if (report_bad_site(c, d_row, d_ref, d_alt)) return 1;
    c->sites.n_cov = I.n_cov;
    c->sites.first_row = I.first_row; c->sites.last_row = I.last_row;     // (the mirror is overwritten by stage B's hand-over)
    c->sites.n_win = (uint32_t)(((uint64_t)c->sites.n_cov + window - 1) / window);
    if (build_layout(c)) return 1;
    std::vector<double> fo;
    c->sites.have_fo = fo_ready || (f_override && fo_triples(f_override, n_sites, fo));
    if (c->sites.have_fo && !fo_ready) {
        if (ensure(c, c->sites.fo, fo.size() * 8)) return 1;
        HIP_TRY(c, hipMemcpyAsync(c->sites.fo.p, fo.data(), fo.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));          // `fo` is a local
    }
    return 0;
}

static int upload_sites_check(ibdg_ctx *c, const void *n_ref, const void *n_alt, bool have_rows, size_t n_sites, unsigned window)
{
    if (!c->pan.panel.p || c->pan.n_ids == 0) return fail(c, "[::] ERROR in ibdg_upload_sites: no panel uploaded");
    if (window < 1) return fail(c, "[::] ERROR: Invalid window size (-w) of %u (must be >= 1).", window);
    if (n_sites && (!n_ref || !n_alt)) return fail(c, "[::] ERROR in ibdg_upload_sites: NULL input array");
    if (n_sites > 0xffffffffull) return fail(c, "[::] ERROR in ibdg_upload_sites: more than 2^32-1 rows in one call");
    const size_t R = c->pan.n_rows;
    if (!have_rows && n_sites > R) return fail(c, "[::] ERROR in ibdg_upload_sites: row_index[%zu]=%zu outside the panel (%zu rows)", R, R, R);
    return 0;
}

// After the last kernel of an upload.  The call does not wait for it: everything the host needed it has polled
// for, the caller's arrays have been read, and whatever uses the prepared sites next is queued behind that kernel
// (K' of the windows) on the same stream.  The event clocks are read when somebody asks (ibdg_upload_ms).
static int upload_sites_finish(ibdg_ctx *c, int rc, std::chrono::steady_clock::time_point t0)
{
    if (rc) return rc;
    c->sites.sites_valid = true;
    HIP_TRY(c, hipEventRecord(c->sites.ev_up[2], c->stream));
    c->sites.up_ms_pending = true;
    c->sites.up_ms[2] = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

int ibdg_upload_sites(ibdg_ctx *c, const uint32_t *row_index, const uint8_t *n_ref, const uint8_t *n_alt,
                      const double *f_override, size_t n_sites, unsigned window)
{
    if (!c) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    if (upload_sites_check(c, n_ref, n_alt, row_index != nullptr, n_sites, window)) return 1;
    if (quiesce(c)) return 1;
    if (ensure(c, c->sites.in_ref, n_sites) || ensure(c, c->sites.in_alt, n_sites) || (row_index && ensure(c, c->sites.in_row, n_sites * 4)))
        return 1;
    HIP_TRY(c, hipEventRecord(c->sites.ev_up[0], c->stream));
    if (n_sites) {
        // 6 bytes per row (2 when the rows are the panel's own); pinned arrays (ibdg_host_alloc) go at link speed
        if (row_index)
            HIP_TRY(c, hipMemcpyAsync(c->sites.in_row.p, row_index, n_sites * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->sites.in_ref.p, n_ref, n_sites, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->sites.in_alt.p, n_alt, n_sites, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipEventRecord(c->sites.ev_up[1], c->stream));
    return upload_sites_finish(c, upload_sites_core(c, row_index ? (const uint32_t *)c->sites.in_row.p : nullptr,
                                                    (const uint8_t *)c->sites.in_ref.p, (const uint8_t *)c->sites.in_alt.p,
                                                    f_override, n_sites, window), t0);
}

int ibdg_upload_sites_dev(ibdg_ctx *c, const void *dev_row_index, const void *dev_n_ref, const void *dev_n_alt,
                          const double *f_override, size_t n_sites, unsigned window)
{
    if (!c) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    if (upload_sites_check(c, dev_n_ref, dev_n_alt, dev_row_index != nullptr, n_sites, window)) return 1;
    if (quiesce(c)) return 1;
    // the arrays may have been produced on another stream (e.g. torch's): make them visible first.  This waits for the
    // whole device -- other contexts' kernels included -- so a caller who knows the arrays are complete says so
    // (option "dev_inputs_ready") and its preparation can run under another context's --LD kernel.
    if (!c->opt.dev_inputs_ready)
        HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipEventRecord(c->sites.ev_up[0], c->stream));
    HIP_TRY(c, hipEventRecord(c->sites.ev_up[1], c->stream));
    const int rc = upload_sites_core(c, (const uint32_t *)dev_row_index, (const uint8_t *)dev_n_ref,
                                     (const uint8_t *)dev_n_alt, f_override, n_sites, window);
    // the caller may free or reuse its arrays when this returns: the last kernel that reads them (k_prep_site_scatter) must
    // be done.  Where the layout's second stage was waited for it is (nothing to wait for); a clamped table, an empty
    // site list or a layout without segments leave that stage out
    if (rc == 0 && n_sites)
        HIP_TRY(c, hipEventSynchronize(c->sites.ev_prepA));
    return upload_sites_finish(c, rc, t0);
}

// ---- -v: the site list of a comparison individual from the pileup's candidates, on the device ----

int ibdg_upload_candidates(ibdg_ctx *c, const uint32_t *row_index, const uint8_t *n_ref, const uint8_t *n_alt,
                           const double *f_override, size_t n_cand)
{
    if (!c) return 1;
    if (upload_sites_check(c, n_ref, n_alt, row_index != nullptr, n_cand, 1)) return 1;
    // what stage A checks per upload of sites, once for all the lists cut from these candidates -- and the selection kernels
    // index the panel with these rows
    for (size_t s = 0; s < n_cand; ++s) {
        if (row_index && row_index[s] >= c->pan.n_rows)
            return fail(c, "[::] ERROR in ibdg_upload_candidates: row_index[%zu]=%u outside the panel (%zu rows)", s,
                        row_index[s], c->pan.n_rows);
        if ((unsigned)n_ref[s] + n_alt[s] > c->tab.max_cov)
            return fail(c, "[::] ERROR in ibdg_upload_candidates: candidate %zu has n_ref+n_alt=%u > max_cov=%u", s,
                        (unsigned)n_ref[s] + n_alt[s], c->tab.max_cov);
    }
    if (quiesce(c)) return 1;
    c->cand.valid = false;
    if (ensure(c, c->cand.ref, n_cand) || ensure(c, c->cand.alt, n_cand) || (row_index && ensure(c, c->cand.row, n_cand * 4)))
        return 1;
    // the -A triples with the host's libm, once for every list cut from these candidates
    std::vector<double> fo;
    const bool have_fo = f_override && fo_triples(f_override, n_cand, fo);
    if (have_fo && ensure(c, c->cand.fo, fo.size() * 8)) return 1;
    if (n_cand) {
        if (row_index)
            HIP_TRY(c, hipMemcpyAsync(c->cand.row.p, row_index, n_cand * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->cand.ref.p, n_ref, n_cand, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->cand.alt.p, n_alt, n_cand, hipMemcpyHostToDevice, c->stream));
        if (have_fo)
            HIP_TRY(c, hipMemcpyAsync(c->cand.fo.p, fo.data(), fo.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));              // `fo` is a local, the arrays are the caller's
    }
    c->cand.n_cand = n_cand;
    c->cand.have_rows = row_index != nullptr;
    c->cand.have_fo = have_fo;
    c->cand.valid = true;
    return 0;
}

size_t ibdg_num_candidates(const ibdg_ctx *c) { return c && c->cand.valid ? c->cand.n_cand : 0; }

int ibdg_select_variable_sites(ibdg_ctx *c, uint32_t target, unsigned window)
{
    if (!c) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    if (!c->pan.panel.p || c->pan.n_ids == 0) return fail(c, "[::] ERROR in ibdg_select_variable_sites: no panel uploaded");
    if (!c->cand.valid) return fail(c, "[::] ERROR in ibdg_select_variable_sites: no candidates uploaded");
    if (target >= c->pan.n_ids)
        return fail(c, "[::] ERROR in ibdg_select_variable_sites: individual %u outside the panel (%u individuals)", target, c->pan.n_ids);
    if (window < 1) return fail(c, "[::] ERROR: Invalid window size (-w) of %u (must be >= 1).", window);
    if (quiesce(c)) return 1;
    const size_t n = c->cand.n_cand;
    if (ensure(c, c->sites.in_ref, n) || ensure(c, c->sites.in_alt, n) || (c->cand.have_rows && ensure(c, c->sites.in_row, n * 4)) ||
        ensure(c, c->cand.sel_cand, n * 4) || (c->cand.have_fo && ensure(c, c->sites.fo, n * 24)) ||
        ensure(c, c->sites.scan_tmp, ibdg::prep_scan_blocks(std::max<size_t>(n, 1)) * 4) || clean_prep_info(c))
        return 1;
    sites_replaced(c);                  // (the selection kernels overwrite in_* and sel_cand)
    HIP_TRY(c, hipEventRecord(c->sites.ev_up[0], c->stream));
    // the number selected comes with the scan's hand-over, like stage A's covered rows: the scatter kernel runs on while
    // the host sizes stage A's buffers and queues it behind
    if (n && hand_over(c, [&](uint32_t seq) { return queue_selection(c, target, seq); }))
        return 1;
    const size_t n_sel = n ? c->sites.info_h->n_cov : 0;
    HIP_TRY(c, hipEventRecord(c->sites.ev_up[1], c->stream));
    // candidates that are the panel's own rows: a selected site's candidate index is its row
    const uint32_t *d_row = (const uint32_t *)(c->cand.have_rows ? c->sites.in_row.p : c->cand.sel_cand.p);
    const int rc = upload_sites_core(c, d_row, (const uint8_t *)c->sites.in_ref.p, (const uint8_t *)c->sites.in_alt.p, nullptr, n_sel,
                                     window, c->cand.have_fo && n_sel);
    if (rc) {
        // (rows and read counts were checked per candidate by ibdg_upload_candidates; whatever is left names a SITE of the
        // selected list, whose candidate is that site's entry of ibdg_get_site_candidates' map)
        c->err += " [site list of individual " + std::to_string(target) + " selected from " + std::to_string(n) +
                  " candidates: a site number counts the selected candidates, in candidate order]";
        return rc;
    }
    c->cand.sel_valid = true;
    return upload_sites_finish(c, 0, t0);
}

int ibdg_get_site_candidates(ibdg_ctx *c, uint32_t *out)
{
    if (!c) return 1;
    if (!c->cand.sel_valid || !c->sites.sites_valid)
        return fail(c, "[::] ERROR in ibdg_get_site_candidates: the current site list was not made by ibdg_select_variable_sites");
    if (c->sites.n_sites == 0) return 0;
    if (!out) return fail(c, "[::] ERROR in ibdg_get_site_candidates: NULL output array");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->cand.sel_cand.p, c->sites.n_sites * 4, hipMemcpyDeviceToHost, c->stream));
    return quiesce(c);
}

int ibdg_upload_ms(ibdg_ctx *c, float out[3])
{
    if (!c || !out) return 1;
    if (c->sites.up_ms_pending) {
        HIP_TRY(c, hipEventSynchronize(c->sites.ev_up[2]));
        HIP_TRY(c, hipEventElapsedTime(&c->sites.up_ms[0], c->sites.ev_up[0], c->sites.ev_up[1]));
        HIP_TRY(c, hipEventElapsedTime(&c->sites.up_ms[1], c->sites.ev_up[1], c->sites.ev_up[2]));
        c->sites.up_ms_pending = false;
    }
    for (int i = 0; i < 3; ++i) out[i] = c->sites.up_ms[i];
    return 0;
}

void *ibdg_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess)
        return nullptr;
    return p;
}

void ibdg_host_free(void *p)
{
    if (p)
        (void)hipHostFree(p);
}

size_t ibdg_num_sites(const ibdg_ctx *c) { return c ? c->sites.n_sites : 0; }
size_t ibdg_num_windows(const ibdg_ctx *c) { return c ? c->sites.n_win : 0; }
size_t ibdg_num_targets(const ibdg_ctx *c) { return c && c->have_results ? c->n_targets : 0; }

int ibdg_get_windows(ibdg_ctx *c, uint32_t *first, uint32_t *last, uint32_t *n_covered)
{
    if (!c) return 1;
    if (c->sites.n_win && (first || last) && !c->sites.win_bounds_valid) {
        if (quiesce(c)) return 1;
        if (ensure(c, c->sites.win_first, (size_t)c->sites.n_win * 4) || ensure(c, c->sites.win_last, (size_t)c->sites.n_win * 4))
            return 1;
        ibdg::launch_prep_win_bounds((const uint32_t *)c->sites.cov_site.p, c->sites.n_cov, c->sites.window, c->sites.n_win,
                                     (uint32_t *)c->sites.win_first.p, (uint32_t *)c->sites.win_last.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        c->sites.win_first_h.resize(c->sites.n_win);
        c->sites.win_last_h.resize(c->sites.n_win);
        HIP_TRY(c, hipMemcpyAsync(c->sites.win_first_h.data(), c->sites.win_first.p, (size_t)c->sites.n_win * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->sites.win_last_h.data(), c->sites.win_last.p, (size_t)c->sites.n_win * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->sites.win_bounds_valid = true;
    }
    for (uint32_t w = 0; w < c->sites.n_win; ++w) {
        const uint64_t b = (uint64_t)w * c->sites.window;
        const uint64_t e = std::min<uint64_t>(b + c->sites.window, c->sites.n_cov);
        if (first) first[w] = c->sites.win_first_h[w];
        if (last) last[w] = c->sites.win_last_h[w];
        if (n_covered) n_covered[w] = (uint32_t)(e - b);
    }
    return 0;
}

}  // extern "C"

namespace {        // ibdg_run's stages

using Ring = ibdg_ctx::Ring;
using EvSet = ibdg_ctx::Timeline::EvSet;

// slot i of a buffer cut into n equal slots, each a multiple of `align` bytes (the per-individual ring, ibdg_ctx::Ring)
template <class P>
P *ring_slot(const DevBuf &b, int i, int n, size_t align = sizeof(P))
{
    return (P *)((char *)b.p + (size_t)i * (b.cap / n / align * align));
}

// The other streams join stream3's preparation of the run's individuals: once, before the first thing that reads it, or at
// the next run's entry when a run failed after it had queued its preparation.
int ring_settle(ibdg_ctx *c)
{
    Ring &R = c->ring;
    if (!R.unsettled) return 0;
    R.unsettled = false;
    HIP_TRY(c, hipEventRecord(R.ready, c->stream3));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, R.ready, 0));
    HIP_TRY(c, hipStreamWaitEvent(c->stream2, R.ready, 0));
    return 0;
}

// New comparison individuals into the next slot of the ring (slot 0 for more than AHEAD_MAX_T of them): their indices and
// k_target_weights' weights / background sizes, on stream3 in a queue of runs (ring_settle hands them over), else the main stream.
int ring_prepare(ibdg_ctx *c, const uint32_t *targets, size_t T, size_t lanes)
{
    Ring &R = c->ring;
    const bool ahead = T <= Ring::AHEAD_MAX_T;
    if (ensure(c, c->weight, (ahead ? Ring::SLOTS : 1) * T * lanes * 8) || ensure(c, c->nrefpanel, Ring::NREF_SLOTS * T * 8))       // (per slot: T background sizes, T individuals)
        return 1;
    // more than a few individuals: a page-locked slot for the indices (so that the copy is a queued one), grown when a run
    // brings more of them; up to IBDG_TG_INLINE of them travel in the weights kernel's arguments instead
    const bool inline_tg = T <= IBDG_TG_INLINE;
    int st = -1;
    if (!inline_tg) {
        if (R.stage_cap < T) {
            if (quiesce(c)) return 1;
            const size_t cap = std::max<size_t>(64, T);
            for (int i = 0; i < Ring::STAGE_SLOTS; ++i) {
                if (R.stage[i])
                    (void)hipHostFree(R.stage[i]);
                R.stage[i] = nullptr;
                HIP_TRY(c, hipHostMalloc((void **)&R.stage[i], cap * 4, hipHostMallocDefault));
                if (!R.stage_ev[i])
                    HIP_TRY(c, hipEventCreateWithFlags(&R.stage_ev[i], hipEventDisableTiming));
            }
            R.stage_cap = cap;
        }
        st = R.stage_next;
        R.stage_next = (st + 1) % Ring::STAGE_SLOTS;
        HIP_TRY(c, hipEventSynchronize(R.stage_ev[st]));      // (its copy was queued STAGE_SLOTS runs ago; never recorded: no wait)
        std::copy(targets, targets + T, R.stage[st]);
    }
    const bool on_s3 = ahead && c->opt.prep_ahead && c->opt.async;
    const hipStream_t ps = on_s3 ? c->stream3 : c->stream;
    if (on_s3)
        R.unsettled = true;
    // whoever still reads the ring slot this run's data go to (ring_mark_readers): the run four new individuals back, long
    // done (on the main stream the readers there are ahead of the preparation anyway)
    const int rs = ahead ? (R.cur + 1) % Ring::SLOTS : 0;
    for (int h = ahead ? rs : 0; h <= (ahead ? rs : Ring::SLOTS - 1); ++h) {
        if (R.main_pending[h] && on_s3)
            HIP_TRY(c, hipStreamWaitEvent(ps, R.main_read[h], 0));
        if (R.s2_pending[h])
            HIP_TRY(c, hipStreamWaitEvent(ps, R.s2_read[h], 0));
        R.main_pending[h] = R.s2_pending[h] = false;
    }
    R.cur = rs;
    R.nref = (R.nref + 1) % Ring::NREF_SLOTS;
    uint32_t *d_tg = ring_slot<uint32_t>(c->targets, R.cur, Ring::SLOTS);
    if (!inline_tg) {
        HIP_TRY(c, hipMemcpyAsync(d_tg, R.stage[st], T * 4, hipMemcpyHostToDevice, ps));
        HIP_TRY(c, hipEventRecord(R.stage_ev[st], ps));
    }
    ibdg::launch_target_weights((const double *)c->bg.base_w.p, d_tg, inline_tg ? targets : nullptr, (uint32_t)T, (uint32_t)lanes,
                                c->bg.base_sum, ring_slot<double>(c->weight, R.cur, Ring::SLOTS),
                                ring_slot<int>(c->nrefpanel, R.nref, Ring::NREF_SLOTS), ps);
    if (!on_s3) {
        // prepared on the main stream (more than AHEAD_MAX_T individuals, "prep_ahead" 0, no queue): the second stream reads
        // the individuals' indices too (k_rows_windows, k_row_table) and, in a queue of runs, starts behind the PREVIOUS
        // run's end only -- it must not overtake this copy / kernel
        HIP_TRY(c, hipEventRecord(R.ready, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, R.ready, 0));
    }
    targets_changed(c, targets, T);
    return 0;
}

// Who reads this run's slot -- every slot where the run used the buffers whole: the end of its launches on the main stream
// and stream2's last kernel (null: stream2 was not used).  ring_prepare waits for them before it writes the slot again.
void ring_mark_readers(ibdg_ctx *c, size_t T, hipEvent_t main_end, hipEvent_t s2_end)
{
    Ring &R = c->ring;
    const bool ahead = T <= Ring::AHEAD_MAX_T;
    for (int h = ahead ? R.cur : 0; h <= (ahead ? R.cur : Ring::SLOTS - 1); ++h) {
        R.main_read[h] = main_end; R.main_pending[h] = true;
        if (s2_end) { R.s2_read[h] = s2_end; R.s2_pending[h] = true; }
    }
}

// background multiplicity per individual without any comparison individual's own exclusion; the -N sample contributes
// nothing (src/ibdgem.c:714, :742-750).  Rare (once per program run): a host wait is fine here.
int set_background(ibdg_ctx *c, const uint8_t *bg_count, int pu_id, size_t lanes)
{
    std::vector<double> wb(lanes, 0.0);
    int sum = 0;
    for (unsigned n = 0; n < c->pan.n_ids; ++n) {
        const unsigned k = bg_count ? bg_count[n] : 1u;
        if ((int)n != pu_id && k != 0) {
            wb[n] = (double)k;
            sum += (int)k;
        }
    }
    if (ensure(c, c->bg.base_w, lanes * 8)) return 1;
    HIP_TRY(c, hipMemcpyAsync(c->bg.base_w.p, wb.data(), lanes * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));          // the host vector goes out of scope
    c->tl.chain_ok = false;
    background_changed(c);
    c->bg.base_sum = sum;
    c->bg.prev_pu = pu_id; c->bg.prev_has_bg = bg_count ? 1 : 0; c->bg.prev_lanes = lanes;
    c->bg.prev_bg.assign(bg_count, bg_count + (bg_count ? c->pan.n_ids : 0));
    return 0;
}

// Comparison individuals over one site list (the site list belongs to the pileup, not to the comparison individual:
// src/ibdgem.c:522 loops the individuals over the same rows): the compacted tiles' one-off gather is paid back by the fewer
// segments every later run counts.  The runs on an upload add up -- one run of 256 individuals, nine batches of 30, or
// sixteen runs of one individual through the counting kernel all reach the point where the re-layout has paid for itself
// (a rent-or-buy rule: never more than twice the cost of having known the number of runs beforehand).
// (a group of the matrix-core kernel costs the same whether it holds 3 or IBDG_TG individuals)
// (round 5: on the site list's rows back to back -- no padding, no rows without reads -- the counting kernel with its sums
// on the matrix cores takes 0.548 ms where the panel's own tiles take 0.606 and round 4's window-aligned tiles took
// 0.58-0.59, profiles/r05_layouts.txt: a single run saves 0.058 ms of the 1.3 ms the gather and the new segments
// cost, i.e. 22 runs pay for them -- an individual counts as 12; with (mask, count) pairs, option mx_counts 0, as 16)
// (a group of the matrix-core kernel saves 0.085 ms of 2.2 on the rows back to back -- 8.90 against 8.57 ms per 60 individuals,
// `many_comparison_individuals` of the bench's detail file, since the launch's groups share the tile words through an
// XCD's L2 --, i.e. fifteen groups pay for the re-layout: a group counts as 20; 45 earlier in round 5, when a group saved
// 0.18 ms, 15 until round 5)
int relayout_when_paid(ibdg_ctx *c, size_t T)
{
    if (!(c->tab.pop_lut_ok && c->lay.pop_sites_ok && !c->lay.compact && c->opt.compact == 0 && c->opt.variant != 1 &&
          c->opt.variant != 3 && c->lay.pop_dense_enough))
        return 0;
    const bool to_mfma = c->opt.mfma_targets && c->lay.tab_in_lds && T >= (size_t)c->opt.mfma_min;
    c->lay.relayout_credit += to_mfma ? (uint64_t)((T + IBDG_TG - 1) / IBDG_TG) * 20u : (uint64_t)T * (c->opt.mx_counts ? 12u : 16u);
    if (c->lay.relayout_credit >= (uint64_t)std::max<long>(1, c->opt.compact_targets)) {
        if (quiesce(c)) return 1;
        Built b = build_segments(c, true);
        if (b == Built::not_applicable)
            b = build_segments(c, false);  // back to the panel's own tiles (cannot be refused: it applied a moment ago)
        return b == Built::failed;
    }
    return 0;
}

// What a run does, decided on the host after the relayout and before its first launch (plan_run)
struct RunPlan {
    size_t T = 0, lanes = 0;
    bool ld = false, use_pop = false;   // --LD; through the exponent-counting kernels (else the strict ones)
    int variant = 0, count_unit = 0;    // what ibdg_last_ld_variant / ibdg_last_count_unit report
    int window_end = 0;                 // ... and ibdg_last_window_end
    bool recount = false, rows_on_main = false, dispatch_events = false, rt_build = false;
    // the individuals: [0, T_g) in n_gg groups of IBDG_TG through k_ld_mfma (gg_batch groups per launch), the T_cnt of
    // [T_g, T) through the counting kernels: n_grp groups of MT in k_ld_popcount_mt, then T_one one per workgroup
    size_t MT = 0, n_gg = 0, T_g = 0, gg_batch = 0, T_cnt = 0, n_grp = 0, T_one = 0;
    bool mfma_wg_sum = false;
    size_t ph_group = 0, part_bytes = 0;    // one k_ld_mfma group's partial sums; a half of `partial`
    int mx_counts = 0;
    long rho_shift = 0;
    bool ibd1 = false, ibd0_pass = false, fin_in_next = false, end_in_dispatch = false;
    bool pair_sums = false;             // the IBD1 form's paired window end (two windows per sum tree, LDS scratch)
    bool side_fast = false;             // stream2's kernels in their fast forms (beside k_ld_mfma)
    unsigned row_blocks = 0;            // workgroups of stream2's k_rows_windows (0: its full grid)
};

// The run's plan.  No HIP calls; the one state it changes is ibd0_runs, which counts runs across calls.
int plan_run(ibdg_ctx *c, size_t T, size_t lanes, int ld_mode, bool row_table, RunPlan &P)
{
    P.T = T; P.lanes = lanes; P.ld = ld_mode != 0;
    P.rt_build = row_table && !c->rt.fresh(*c);
    if (ld_mode) {
        const bool can = c->tab.pop_lut_ok && c->lay.pop_sites_ok && (c->lay.compact ? c->lay.t32c.p : c->pan.t32.p);
        if (c->opt.variant == 2 && !can)
            return fail(c, "[::] ERROR in ibdg_run: ld_variant 2 (exponent counting) is not applicable here "
                           "(clamped P(D|G) table, epsilon outside (0,1), max_cov > 50 or rows out of order)");
        P.use_pop = can && c->opt.variant != 1 && c->opt.variant != 3 && (c->opt.variant == 2 || c->lay.pop_dense_enough);
    }
    P.variant = ld_mode ? (P.use_pop ? 2 : (c->opt.variant == 3 ? 3 : 1)) : 0;
    P.recount = c->opt.count_in_run || !c->pan.counts_valid;
    // a non-LD run is one kernel: it goes to the main stream (no second stream to start, wait for and join)
    P.rows_on_main = !ld_mode && !P.recount;
    P.dispatch_events = P.use_pop && c->opt.dispatch_events && c->sites.n_win > 0;
    if (P.use_pop) {
        // Comparison individuals in groups of MT share one workgroup (and the counts that do not
        // depend on them) in k_ld_popcount_mt; what is left over goes one per workgroup.
        P.MT = (size_t)ibdg::ld_popcount_mt_width();
        const bool mt_fits = ibdg::ld_popcount_lds_bytes(c->lay.max_seg, c->lay.wpg, c->lay.ct_max + 1, c->lay.tab_in_lds, c->lay.seg_ring,
                                                         1) <= 150 * 1024;
        // Five or more comparison individuals: groups of IBDG_TG through the matrix cores (k_ld_mfma); the
        // last group may be short, fewer than mfma_min individuals take the counting kernels below.
        // (one group's partial sums and operands must stay modest: tiny windows over millions of rows go the old way)
        // (a group's partial sums: 16 doubles per window and half chunk -- per group of eight half chunks where the kernel's
        //  workgroups add their waves' sums up themselves, MfmaArgs::wg_sum)
        P.mfma_wg_sum = c->opt.mfma_wg_sum && ibdg::ld_mfma_wg_sum(c->lay.wpg, c->lay.ct_max + 1, c->lay.max_seg);
        P.ph_group = (size_t)c->sites.n_win * (P.mfma_wg_sum ? (size_t)((2 * c->pan.n_chunks + 7) / 8) * 128 : (size_t)c->pan.n_chunks * 2 * 128) + 128;
        const size_t group_bytes = P.ph_group + (size_t)c->lay.n_segs * 1024 + (size_t)c->sites.n_win * 512;
        if (c->opt.mfma_targets && c->lay.tab_in_lds && !P.dispatch_events && T >= (size_t)c->opt.mfma_min && (c->lay.compact ? c->lay.n_pairs_c : c->pan.n_pairs) < (1u << 21) && c->lay.n_segs < (1u << 21) &&     // (32-bit byte offsets of its buffer loads)
            group_bytes <= ((size_t)4 << 30) &&
            ibdg::ld_mfma_lds_bytes(c->lay.wpg, c->lay.ct_max + 1, c->lay.max_seg) <= 64 * 1024) {
            P.n_gg = T / IBDG_TG + (T % IBDG_TG >= (size_t)c->opt.mfma_min);
            P.T_g = std::min(P.n_gg * IBDG_TG, T);
        }
        P.T_cnt = T - P.T_g;
        P.n_grp = (c->opt.multi_target && mt_fits && P.T_cnt >= P.MT) ? P.T_cnt / P.MT : 0;
        P.T_one = P.T_cnt - P.n_grp * P.MT;
        // target operands (1 KiB per segment and group) and partial sums (32 B per window, chunk and individual)
        // exist for one batch of groups at a time: about 1 GiB of operands, eight groups at most
        // (option "mfma_batch_groups": at most that many groups per launch, within 1/16 of the device's memory for each of
        //  the two buffers)
        const size_t mem_cap = std::max<size_t>((size_t)1 << 30, c->dev_mem_bytes / 16);
        const size_t fit = std::min(c->lay.n_segs ? mem_cap / ((size_t)c->lay.n_segs * 1024) : P.n_gg, mem_cap / P.ph_group);
        P.gg_batch = std::min({std::max<size_t>(fit, 1), (size_t)std::max<long>(1, c->opt.mfma_batch), P.n_gg});
        // one comparison individual per workgroup: the counts of a haplotype word on the matrix cores where the larger
        // records leave the run's LDS image within reach (option "mx_counts")
        // ... and its power tables in LDS are plain doubles, rho^n as rho^n 2^(s n): s = the integer nearest to -log2 rho keeps
        // every entry, and every product of a rho and a sigma entry whose exponents add up to a window's reads, a normal number
        const double log2_rho = std::log2(c->tab.eps / (1 - c->tab.eps)), log2_sigma = std::log2(0.5 / (1 - c->tab.eps));
        // (8 where the table allows it: the window end then makes the exponent up with one subtraction)
        const bool shift8 = (double)(c->lay.ct_max + 1) * std::max(std::fabs(log2_rho + 8.0), std::fabs(log2_sigma)) <= 1000.0;
        P.rho_shift = shift8 ? 8 : std::lround(-log2_rho);
        const double per_read = std::max(std::fabs(log2_rho + (double)P.rho_shift), std::fabs(log2_sigma));
        P.mx_counts = c->opt.mx_counts && P.rho_shift >= 0 && P.rho_shift <= 40 &&
                      (!c->lay.tab_in_lds || (double)(c->lay.ct_max + 1) * per_read <= 1000.0) &&
                      ibdg::ld_popcount_lds_bytes(c->lay.max_seg, c->lay.wpg, c->lay.ct_max + 1, c->lay.tab_in_lds, c->lay.seg_ring, 2) <= 150 * 1024;
        P.part_bytes = T * (size_t)c->sites.n_win * c->pan.n_chunks * 16;
        // single individuals in the IBD1 form (counts on the matrix cores, tables in LDS): at once where the IBD0 pass exists,
        // otherwise when the runs on this upload and background have added up
        const bool p2_stale = !c->p2.fresh(*c, P.mx_counts);
        if (P.T_one && P.mx_counts && c->lay.tab_in_lds && c->opt.ibd0_after > 0) {
            if (!c->ibd0.fresh(*c))
                c->ibd0.made(*c);
            c->ibd0.ibd0_runs += P.T_one;
            P.ibd1 = !p2_stale || (P.n_gg > 0) || c->ibd0.ibd0_runs >= (uint64_t)c->opt.ibd0_after;
        }
        P.ibd0_pass = p2_stale && (P.n_gg > 0 || P.ibd1);
        // ... two windows per sum tree (option "pair_sums") where the 1 KiB of scratch per wave this takes leaves as many
        // workgroups on a CU as the form has without it: 160 KiB over the workgroup's LDS, rounded down, and no more than the
        // four workgroups of eight waves that the CU's wave slots hold at the kernel's 8 waves per SIMD (the LDS is sized for
        // eight waves whatever the panel)
        if (P.ibd1 && c->opt.pair_sums) {
            const auto per_cu = [&](int form) {
                return std::min<size_t>(4, (size_t)160 * 1024 / ibdg::ld_popcount_lds_bytes(c->lay.max_seg, c->lay.wpg, c->lay.ct_max + 1,
                                                                                           c->lay.tab_in_lds, c->lay.seg_ring, form));
            };
            P.pair_sums = per_cu(4) == per_cu(3);
        }
        P.fin_in_next = c->opt.fin_next && c->opt.async && P.T_one > 0 && P.T_one == P.T_cnt && P.n_gg == 0;
        // (option "end_in_dispatch": the run's end event is the --LD kernel's own completion signal -- no event packet
        // of its own behind the kernel -- where that kernel is the run's last launch on the main stream)
        // (not with "log_windows": the run's end is then an event behind everything its main stream holds, see ibdg_ctx::WinLog)
        P.end_in_dispatch = c->opt.end_in_dispatch && P.fin_in_next && !P.dispatch_events && P.T_one == T && !c->opt.log_windows;
        P.count_unit = P.T_one ? (P.mx_counts ? (P.ibd1 ? 3 : 2) : 1) : 0;
        P.window_end = P.T_one ? (P.pair_sums ? 2 : 1) : 0;
        // k_ld_mfma (4 waves per SIMD) leaves wave slots to the second stream: its kernels run in their fast forms
        // (also with a few individuals left to the counting kernels: T = 16 5.5 ms against 6.0; beside
        // k_ld_popcount_mt alone it makes no difference)
        P.side_fast = P.n_gg > 0;
    }
    // stream2's per-row values and window products, one launch (k_rows_windows).  Beside the exponent-counting --LD
    // kernel, which holds every wave slot, it gets few long-lived workgroups (opt.site_blocks per CU, shared among
    // the targets): its gathers wait on memory either way, and the --LD workgroups keep their wave slots
    // (not when the alt counts are recounted in this run: the second stream's chain count -> rows is then the
    // longer one of the two, and its kernels should be short; and not beside the matrix-core kernel, which leaves
    // half of the wave slots free)
    if (ld_mode && !P.recount && !P.side_fast && c->opt.site_blocks > 0)
        P.row_blocks = std::max<unsigned>(1u, (unsigned)((size_t)c->n_cu * c->opt.site_blocks / T));
    return 0;
}

// Two streams: the per-site kernel and the window products (memory-bound, few waves) run on stream2 beside the --LD
// kernels (VALU-bound) on the main stream.  stream2 starts a run when the main stream does (a wait in stream2's queue
// costs the main stream nothing; it also orders stream2 behind an upload of new targets); the main stream waits for
// stream2 when somebody needs the results (join_streams), not once per run.
// Timing: normally one event record per run on the main stream (a queued run takes the previous run's end as its start).
// With the option "dispatch_events" the exponent-counting launches carry events in their own dispatch packets instead
// (hipExtLaunchKernel: start of the first, stop of the last, and both of the dominant kernel -- the only way to time that
// kernel alone from inside the process).
// A finalising step flushed by this run (`flushed`) writes LIBD0 / LIBD1 of the rows a non-LD run's stream2 writes too: the
// previous run's end lies before that step, so it cannot be the start stream2 waits for.  (Steady queues never flush.)
int start_run(ibdg_ctx *c, const RunPlan &P, EvSet &E, bool flushed)
{
    E.recount = P.recount; E.ld = P.ld; E.rows_on_main = P.rows_on_main; E.has_kernel_times = P.dispatch_events;
    const bool chained = c->tl.chain_ok && c->opt.async;
    if (P.dispatch_events) {                       // (an --LD run: its stream2 writes no entry the step writes)
        E.start = E.start_own;                     // filled in by the first --LD dispatch
        if (chained)                               // stream2 keeps one run behind the main stream at most
            HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->tl.evs[c->tl.ev_head].ld_end, 0));
        return 0;
    }
    if (chained && !flushed) {
        E.start = c->tl.evs[c->tl.ev_head].ld_end;       // back-to-back runs: the previous end is this start
    } else {
        HIP_TRY(c, hipEventRecord(E.start_own, c->stream));
        E.start = E.start_own;
    }
    if (!P.rows_on_main)
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, E.start, 0));
    return 0;
}

ibdg::RowsArgs rows_args(const ibdg_ctx *c, int ld_mode, bool row_table)
{
    ibdg::RowsArgs sa{};
    sa.panel = (const uint64_t *)c->pan.panel.p; sa.stride = c->pan.stride; sa.n_ids = c->pan.n_ids;
    sa.rec_all = (const uint2 *)c->sites.rec_all.p; sa.n_sites = c->sites.n_sites;
    sa.lut = (const double *)c->tab.lut.p; sa.alt_count = (const uint32_t *)c->pan.alt_count.p; sa.pow_tab = (const double *)c->pan.pow_tab.p;
    sa.fo = c->sites.have_fo ? (const double *)c->sites.fo.p : nullptr;
    sa.targets = ring_slot<const uint32_t>(c->targets, c->ring.cur, Ring::SLOTS);
    sa.t32 = c->tab.pop_lut_ok ? (const uint4 *)c->pan.t32.p : nullptr; sa.n_pairs = c->pan.n_pairs;
    sa.cov_site = (const uint32_t *)c->sites.cov_site.p; sa.rec_cov = (const uint2 *)c->sites.rec_cov.p; sa.n_cov = c->sites.n_cov;
    sa.window = c->sites.window; sa.n_win = c->sites.n_win; sa.ld_mode = ld_mode ? 1 : 0;
    sa.site_ll = c->opt.site_results && !row_table ? (double *)c->site_ll.p : nullptr;
    sa.win_ll = (double *)c->win_ll.p;
    return sa;
}

// What the counting kernels' and k_ld_mfma's arguments share: the layout's tiles, segments, windows and runs, the power
// tables and the run's individuals (A: ibdg::PopArgs or ibdg::MfmaArgs, which name these fields alike)
template <class A>
void common_args(const ibdg_ctx *c, A &a, size_t lanes)
{
    const ibdg_ctx::Layout &L = c->lay;
    a.t32 = (const uint32_t *)(L.compact ? L.t32c.p : c->pan.t32.p); a.n_pairs = L.compact ? L.n_pairs_c : c->pan.n_pairs;
    a.n_chunks = c->pan.n_chunks;
    a.segs = (const ibdg::Seg *)L.segs.p; a.n_segs = L.n_segs; a.max_seg = L.max_seg;
    a.wconst = (const ibdg::WinConst *)L.wconst.p; a.n_win = c->sites.n_win; a.win_per_group = L.wpg;
    a.run_begin = (const uint32_t *)L.runs.p; a.n_runs = L.n_runs;
    a.pow_1me = (const ibdg::PowEntry *)c->tab.pow1.p; a.pow_eps = (const ibdg::PowEntry *)c->tab.pow2.p; a.tab_len = L.ct_max + 1;
    a.targets = ring_slot<const uint32_t>(c->targets, c->ring.cur, Ring::SLOTS); a.lanes = (uint32_t)lanes;
}

// The counting kernels' arguments, made once per run; the stages copy and adjust them.
ibdg::PopArgs pop_args(const ibdg_ctx *c, const RunPlan &P)
{
    const Ring &R = c->ring;
    ibdg::PopArgs pa;
    common_args(c, pa, P.lanes);
    pa.n_cgroups = (c->pan.n_chunks + 7) / 8;
    pa.waves_per_group = (c->pan.n_chunks + pa.n_cgroups - 1) / pa.n_cgroups;   // 40 chunks: 5 x 8; 9: 5 + 4; 2: 1 x 2
    pa.rec_ready = ring_slot<const uint32_t>(c->img.twords, R.cur, Ring::SLOTS, 16);
    pa.wc_ready = ring_slot<const uint32_t>(c->img.wtarget, R.cur, Ring::SLOTS, 16);
    pa.t_base = (uint32_t)P.T_g;
    pa.weight = ring_slot<const double>(c->weight, R.cur, Ring::SLOTS);
    pa.partial = (double *)((char *)c->partial.p + (P.fin_in_next ? (size_t)c->fin.half * P.part_bytes : 0));
    pa.ring_slots = (uint32_t)c->lay.seg_ring; pa.tab_in_lds = (uint32_t)c->lay.tab_in_lds;
    pa.mx_counts = (uint32_t)P.mx_counts; pa.rho_shift = (uint32_t)P.rho_shift; pa.sum_dpp = (uint32_t)c->opt.sum_dpp;
    return pa;
}

// k_ld_mfma's arguments: the counting kernels' site list, windows, tables and individuals, and its own operands and sums
ibdg::MfmaArgs mfma_args(const ibdg_ctx *c, const RunPlan &P)
{
    ibdg::MfmaArgs ma;
    common_args(c, ma, P.lanes);
    ma.pow_tau = (const ibdg::PowEntry *)c->tab.pow3.p;
    ma.plain_tau = c->opt.mfma_plain_tau ? 1u : 0u;
    ma.base_weight = (const double *)c->bg.base_w.p;
    ma.p2w = (const double *)c->p2.p2w.p; ma.p2c = (const double *)c->p2.p2c.p;
    ma.aimg = (uint4 *)c->aimg.p; ma.wc_slot = (uint4 *)c->wc_slot.p;
    // one batch's partial sums: t1 [groups][windows][half chunks][16], t0 [groups][windows][half chunks], ov [groups][windows][16]
    ma.part_t1 = (double *)c->partial_h.p; ma.wg_sum = P.mfma_wg_sum ? 1u : 0u;
    return ma;
}

// The IBD0 terms of this site list and background, once: a pass of the counting kernel that keeps every lane's weighted
// product (p2_out) and its sums per chunk; the images it reads are those of the run's first individual.  (A finalising
// step left by the run before has been flushed: the pass rewrites the sums it reads.)
int ibd0_pass(ibdg_ctx *c, const RunPlan &P, const ibdg::PopArgs &pa)
{
    if (ring_settle(c)) return 1;
    if (ensure(c, c->p2.p2w, (size_t)c->sites.n_win * P.lanes * 8) || ensure(c, c->p2.p2c, (size_t)c->sites.n_win * c->pan.n_chunks * 16) ||
        ensure(c, c->p2.p2_tw, (size_t)c->lay.n_segs * ibdg::ld_popcount_rec_bytes(P.mx_counts)) ||
        ensure(c, c->p2.p2_wt, (size_t)c->sites.n_win * 32))
        return 1;
    ibdg::PopArgs pp = pa;
    pp.rec_ready = (const uint32_t *)c->p2.p2_tw.p; pp.wc_ready = (const uint32_t *)c->p2.p2_wt.p;
    pp.weight = (const double *)c->bg.base_w.p; pp.t_base = 0;
    pp.partial = (double *)c->p2.p2c.p; pp.p2_out = (double *)c->p2.p2w.p;
    ibdg::launch_win_target(pp, 1, c->stream);
    if (ibdg::launch_ld_popcount(pp, 1, c->lay.planes, c->stream))
        return fail(c, "[::] ERROR in ibdg_run: unsupported number of weight bit-planes %d", c->lay.planes);
    c->p2.made(*c, P.mx_counts);
    return 0;
}

// groups of IBDG_TG individuals through the matrix cores (k_ld_mfma), gg_batch groups per launch
int launch_mfma_groups(ibdg_ctx *c, const RunPlan &P, EvSet &E)
{
    if (ring_settle(c)) return 1;
    ibdg::MfmaArgs ma = mfma_args(c, P);
    const int *d_nref = ring_slot<const int>(c->nrefpanel, c->ring.nref, Ring::NREF_SLOTS);
    for (size_t g0 = 0; g0 < P.n_gg; g0 += P.gg_batch) {
        const size_t nb = std::min(P.n_gg - g0, P.gg_batch);
        ma.t_base = (uint32_t)(g0 * IBDG_TG);
        ma.n_targets = (uint32_t)std::min(P.T_g - g0 * IBDG_TG, nb * IBDG_TG);
        ibdg::launch_win_target_g(ma, (unsigned)nb, c->stream);
        // the second stream (per-site values, window products; high priority) starts behind these
        // two short kernels rather than beside them: it starved them (0.57 ms instead of 0.06)
        if (g0 == 0)
            HIP_TRY(c, hipEventRecord(E.prep, c->stream));
        if (ibdg::launch_ld_mfma(ma, (unsigned)nb, c->stream, ibdg::KernelEvents()))
            return fail(c, "[::] ERROR in ibdg_run: the matrix-core --LD kernel could not be launched");
        ibdg::launch_ld_finalize_g(ma, (unsigned)nb, d_nref, (double *)c->win_ll.p, c->stream);
    }
    return 0;
}

// groups of MT individuals sharing a workgroup (k_ld_popcount_mt); `first` goes to the first launch and is used up
int launch_mt_groups(ibdg_ctx *c, const RunPlan &P, const ibdg::PopArgs &pa, ibdg::KernelEvents &first,
                     ibdg::KernelEvents dominant)
{
    if (ring_settle(c)) return 1;
    ibdg::PopArgs pm = pa;
    pm.mx_counts = 0;
    pm.rec_ready = (const uint32_t *)c->twords_mt.p; pm.wc_ready = (const uint32_t *)c->wtarget_mt.p;
    ibdg::launch_win_target_mt(pm, (unsigned)P.n_grp, c->stream, first);
    first = ibdg::KernelEvents();
    if (ibdg::launch_ld_popcount_mt(pm, (unsigned)P.n_grp, c->stream, P.T_one ? ibdg::KernelEvents() : dominant))
        return fail(c, "[::] ERROR in ibdg_run: the multi-target --LD kernel could not be launched");
    return 0;
}

// the single individuals [T_g + n_grp MT, T), one per workgroup (k_ld_popcount), with their images (k_win_target)
int launch_singles(ibdg_ctx *c, const RunPlan &P, ibdg::PopArgs pa, ibdg::KernelEvents first, ibdg::KernelEvents dominant,
                   bool same_inputs, EvSet &E)
{
    Ring &R = c->ring;
    pa.t_base = (uint32_t)(P.T_g + P.n_grp * P.MT);
    pa.ibd1 = P.ibd1 ? 1u : 0u;
    pa.pair_sums = P.pair_sums ? 1u : 0u;
    // (skipped when the previous run made the very same images: same prepared sites, same comparison individuals --
    // a caller that runs a comparison again, e.g. timed steps: one launch of ~10 us less per run, which on an
    // eighth of a chromosome is a tenth of the step)
    const ibdg_ctx::Images::Key key = c->img.key_for(*c, pa.t_base, (uint32_t)P.T_one, P.mx_counts, (int)P.ibd1, R.cur);
    const bool wt_cached = same_inputs && c->img.fresh(key) && !P.dispatch_events;
    // a new individual's images: on stream3 with its weights (under the --LD kernel of the run before) unless the
    // launch carries the run's start event (dispatch_events: that belongs on the main stream)
    const bool wt_ahead = R.unsettled && !P.dispatch_events;
    const hipStream_t is = wt_ahead ? c->stream3 : c->stream;
    if (!wt_ahead && ring_settle(c)) return 1;
    if (wt_ahead && R.s3_gen != c->sites_gen) {
        // once per upload / change of layout: stream3's kernel reads the prepared sites (segments, window constants),
        // whose kernels were queued on the main stream
        HIP_TRY(c, hipEventRecord(R.ev_s3sync, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream3, R.ev_s3sync, 0));
        R.s3_gen = c->sites_gen;
    }
    if (P.ibd1) {
        if (!c->fb.fresh(*c)) {
            // once per site list (and layout): the three fragments per segment an individual's images select between
            if (ensure(c, c->fb.fragb, (size_t)c->lay.n_segs * 72)) return 1;
            if (!c->fb.ev_fb)
                HIP_TRY(c, hipEventCreateWithFlags(&c->fb.ev_fb, hipEventDisableTiming));
            ibdg::launch_frag_base(pa, (uint32_t *)c->fb.fragb.p, is);
            HIP_TRY(c, hipEventRecord(c->fb.ev_fb, is));
            HIP_TRY(c, hipStreamWaitEvent(wt_ahead ? c->stream : c->stream3, c->fb.ev_fb, 0));   // (whichever makes the next images)
            c->fb.made(*c);
        }
        pa.frag_base = (const uint32_t *)c->fb.fragb.p;
    }
    if (!wt_cached)
        ibdg::launch_win_target(pa, (unsigned)P.T_one, is, first);
    if (ring_settle(c)) return 1;
    c->img.made(key);
    if (P.end_in_dispatch)
        dominant.stop = E.ld_end;
    if (ibdg::launch_ld_popcount(pa, (unsigned)P.T_one, c->lay.planes, c->stream, dominant))
        return fail(c, "[::] ERROR in ibdg_run: unsupported number of weight bit-planes %d", c->lay.planes);
    return 0;
}

// LIBD0 / LIBD1 of the counting kernels' individuals [T_g, T) from their partial sums.  Queued runs of single individuals
// (the timed steps of a shard, a caller's loop over the same comparison): this run's finalising step -- one wave per
// window, 5 us, but a launch of its own with its gap and the event packet behind it: a tenth of a step on an eighth of a
// chromosome -- is left to the NEXT run's --LD launch, whose first workgroups do it on the way (the kernel boundary between
// the two launches is all the ordering it needs), and this run's launch does the same for its predecessor.  The partial
// sums alternate between two halves of their buffer.
int finalise(ibdg_ctx *c, const RunPlan &P, const ibdg::PopArgs &pa, ibdg::KernelEvents last, EvSet &E)
{
    if (!P.T_cnt) return 0;
    const int *d_nref = ring_slot<const int>(c->nrefpanel, c->ring.nref, Ring::NREF_SLOTS);
    ibdg::PopFinalArgs fa;
    fa.wconst = pa.wconst; fa.n_win = c->sites.n_win; fa.n_chunks = c->pan.n_chunks;
    fa.n_refpanel = d_nref; fa.win_ll = (double *)c->win_ll.p;
    fa.partial = pa.partial; fa.t_base = (uint32_t)P.T_g; fa.halves = 0;
    if (P.ibd1) {                      // (whatever kernel made an individual's IBD1 sums)
        fa.p2c = (const double *)c->p2.p2c.p; fa.p2w = (const double *)c->p2.p2w.p; fa.lanes = (uint32_t)P.lanes;
        fa.targets = (const uint32_t *)(d_nref + P.T);      // (this run's individuals, from the longer ring: k_target_weights)
    }
    if (!P.fin_in_next) {
        ibdg::launch_ld_finalize(fa, (unsigned)P.T_cnt, c->stream, last);
        return 0;
    }
    c->fin = {true, fa, (unsigned)P.T_cnt, c->sites_gen, c->fin.half ^ 1};
    if (P.dispatch_events)         // (no finalising launch to carry the run's end in its dispatch packet)
        HIP_TRY(c, hipEventRecord(E.ld_end, c->stream));
    return 0;
}

// the exponent-counting --LD path: k_ld_mfma groups, k_ld_popcount_mt groups, single individuals, the finalising step
int launch_pop(ibdg_ctx *c, const RunPlan &P, EvSet &E, bool same_inputs)
{
    // (the single individuals' images in ring slots like the other per-individual data)
    const size_t img_slots = P.T <= Ring::AHEAD_MAX_T ? Ring::SLOTS : 1;
    if (ensure(c, c->img.wtarget, img_slots * P.T_one * (size_t)c->sites.n_win * 32) ||
        ensure(c, c->img.twords, img_slots * P.T_one * (size_t)c->lay.n_segs * ibdg::ld_popcount_rec_bytes(P.mx_counts)) ||
        ensure(c, c->wtarget_mt, P.n_grp * (size_t)c->sites.n_win * ibdg::ld_popcount_mt_wc_bytes()) ||
        ensure(c, c->twords_mt, P.n_grp * (size_t)c->lay.n_segs * ibdg::ld_popcount_mt_rec_bytes()) ||
        ensure(c, c->partial, P.T_cnt ? 2 * P.part_bytes : 0) ||
        ensure(c, c->aimg, P.gg_batch * (size_t)c->lay.n_segs * 1024) ||
        ensure(c, c->wc_slot, P.gg_batch * (size_t)c->sites.n_win * 512) ||
        ensure(c, c->partial_h, P.gg_batch * P.ph_group))
        return 1;
    ibdg::PopArgs pa = pop_args(c, P);
    if (P.ibd0_pass && ibd0_pass(c, P, pa)) return 1;
    if (c->fin.pending) {                 // the finalising step the run before left to this run's launch
        pa.fin_prev = c->fin.args.partial; pa.win_ll = (double *)c->win_ll.p;
        pa.n_refpanel = c->fin.args.n_refpanel;      // (of the run that left it: its entry of the ring)
        pa.fin_p2c = c->fin.args.p2c; pa.fin_p2w = c->fin.args.p2w;   // (non-null: that run was of the IBD1 form)
        pa.fin_targets = c->fin.args.targets;
        c->fin.pending = false;
    }
    ibdg::KernelEvents first, dominant, last;  // all null unless dispatch_events
    if (P.dispatch_events) {
        first.start = E.start_own; last.stop = E.ld_end;
        dominant.start = E.k_start; dominant.stop = E.k_stop;
    }
    if ((P.n_gg && launch_mfma_groups(c, P, E)) || (P.n_grp && launch_mt_groups(c, P, pa, first, dominant)) ||
        (P.T_one && launch_singles(c, P, pa, first, dominant, same_inputs, E)))
        return 1;
    return finalise(c, P, pa, last, E);
}

// the background list in the reference's order: ibdg_set_background_order's (checked against bg_count), or every
// individual bg_count times in the panel's order
int background_order(ibdg_ctx *c, const uint8_t *bg_count, std::vector<uint32_t> &order)
{
    if (c->opt.bg_order.empty()) {
        for (unsigned n = 0; n < c->pan.n_ids; ++n)
            for (unsigned k = bg_count ? bg_count[n] : 1u; k > 0; --k)
                order.push_back(n);
        return 0;
    }
    order = c->opt.bg_order;
    std::vector<unsigned> cnt(c->pan.n_ids, 0);
    for (uint32_t n : order) {
        if (n >= c->pan.n_ids)
            return fail(c, "[::] ERROR in ibdg_run: background order names individual %u of %u", n, c->pan.n_ids);
        cnt[n]++;
    }
    for (unsigned n = 0; n < c->pan.n_ids; ++n)
        if (cnt[n] != (bg_count ? bg_count[n] : 1u))
            return fail(c, "[::] ERROR in ibdg_run: background order and bg_count disagree for individual %u", n);
    return 0;
}

// the strict --LD kernels; option ld_variant 3: per comparison individual, the per-individual products of every window,
// then serial sums over the background list in the reference's order
int launch_strict(ibdg_ctx *c, const RunPlan &P, const uint32_t *targets, const uint8_t *bg_count, int pu_id)
{
    if (ring_settle(c)) return 1;
    ibdg::LdArgs la{};
    la.panel = (const uint64_t *)c->pan.panel.p; la.stride = c->pan.stride; la.n_groups = c->pan.n_groups;
    la.rec_cov = (const uint2 *)c->sites.rec_cov.p; la.n_cov = c->sites.n_cov; la.window = c->sites.window; la.n_win = c->sites.n_win;
    la.lut = (const double *)c->tab.lut.p; la.win_ll = (double *)c->win_ll.p;
    la.targets = ring_slot<const uint32_t>(c->targets, c->ring.cur, Ring::SLOTS);
    la.weight = ring_slot<const double>(c->weight, c->ring.cur, Ring::SLOTS);
    la.n_refpanel = ring_slot<const int>(c->nrefpanel, c->ring.nref, Ring::NREF_SLOTS);
    if (c->opt.variant != 3) {
        if (ibdg::launch_ld(la, (unsigned)P.T, c->pan.cpw, (unsigned)c->opt.waves, c->stream))
            return fail(c, "[::] ERROR in ibdg_run: unsupported chunks_per_wave %d", c->pan.cpw);
        return 0;
    }
    std::vector<uint32_t> order;
    if (background_order(c, bg_count, order)) return 1;
    if (ensure(c, c->vals, (size_t)c->sites.n_win * P.lanes * 16) || ensure(c, c->order, order.size() * 4)) return 1;
    HIP_TRY(c, hipMemcpyAsync(c->order.p, order.data(), order.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // `order` is a local
    la.vals = (double2 *)c->vals.p;
    ibdg::OrdArgs oa;
    oa.vals = la.vals; oa.lanes = (uint32_t)P.lanes; oa.n_win = c->sites.n_win; oa.pu_id = pu_id;
    oa.order = (const uint32_t *)c->order.p; oa.n_order = (uint32_t)order.size();
    for (size_t t = 0; t < P.T; ++t) {
        la.t_base = (uint32_t)t;
        if (ibdg::launch_ld(la, 1, c->pan.cpw, (unsigned)c->opt.waves, c->stream))
            return fail(c, "[::] ERROR in ibdg_run: unsupported chunks_per_wave %d", c->pan.cpw);
        oa.target = targets[t];
        oa.win_ll = (double *)c->win_ll.p + t * (size_t)c->sites.n_win * 3;
        ibdg::launch_ld_ordered_sum(oa, c->stream);
    }
    return 0;
}

// Option "log_windows", the --LD columns of the log table: why the exponent-counting form cannot serve this site list (the
// conditions under which "ld_variant" 2 is refused), or null.  The strict and reference-order variants of the linear columns
// do not stop it: k_ld_log reads the layout, not their results.
const char *ld_log_refused(const ibdg_ctx *c)
{
    if (c->tab.max_cov > 50)
        return "max_cov > 50";
    if (!c->tab.pop_lut_ok)
        return "a clamped P(D|G) table (or epsilon outside (0,1))";
    if (!c->lay.pop_sites_ok || !(c->lay.compact ? c->lay.t32c.p : c->pan.t32.p))
        return "no prepared segments for this site list (rows out of file order or too far apart)";
    if (ibdg::ld_log_lds_bytes(c->pan.n_chunks) > 64 * 1024)
        return "more individuals than its workgroup's LDS holds chunk sums for";
    return nullptr;
}

// k_ld_log on the main stream, in front of the run's --LD launches (ibdg_ctx::WinLog)
int launch_log_windows(ibdg_ctx *c, const RunPlan &P)
{
    if (ring_settle(c)) return 1;
    ibdg::LdLogArgs la{};
    const ibdg_ctx::Layout &L = c->lay;
    la.t32 = (const uint4 *)(L.compact ? L.t32c.p : c->pan.t32.p); la.n_pairs = L.compact ? L.n_pairs_c : c->pan.n_pairs;
    la.n_chunks = c->pan.n_chunks;
    la.segs = (const ibdg::Seg *)L.segs.p; la.n_segs = L.n_segs;
    la.wconst = (const ibdg::WinConst *)L.wconst.p; la.n_win = c->sites.n_win;
    la.pow_rho = (const ibdg::PowEntry *)c->tab.pow1.p; la.pow_sigma = (const ibdg::PowEntry *)c->tab.pow2.p; la.tab_len = L.ct_max + 1;
    la.targets = ring_slot<const uint32_t>(c->targets, c->ring.cur, Ring::SLOTS);
    la.base_w = (const double *)c->bg.base_w.p; la.lanes = (uint32_t)P.lanes; la.base_sum = c->bg.base_sum;
    la.win_log2 = (double *)c->wlog.win_log2.p;
    ibdg::launch_ld_log(la, (unsigned)P.T, c->stream);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

// stream2's share of the run, queued after the critical path so that the --LD launches reach the device first: the
// recount of the alt counts, the per-row values and the window products
int queue_stream2(ibdg_ctx *c, const RunPlan &P, const ibdg::RowsArgs &sa, EvSet &E)
{
    if (P.n_gg)                        // (behind the matrix-core groups' operands, launch_mfma_groups)
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, E.prep, 0));
    HIP_TRY(c, hipEventRecord(E.s2_start, c->stream2));
    if (P.recount) {
        // beside the --LD kernel: few long-lived waves (opt.recount_blocks per CU), so that the recount does not
        // take the wave slots the --LD workgroups need -- it is bound by HBM, they by instruction issue
        ibdg::launch_alt_count((const uint64_t *)c->pan.panel.p, c->pan.stride, c->pan.n_rows, (uint32_t *)c->pan.alt_count.p,
                               c->stream2, P.ld ? (unsigned)(c->n_cu * c->opt.recount_blocks) : 0u);
        c->pan.counts_valid = true;
        HIP_TRY(c, hipEventRecord(E.s2_count, c->stream2));
    }
    // The site list's row table, when stale: one comparison individual's run makes it in the launch it makes anyway
    // (its rows' values are all computed there: 32 B per row stored instead of the per-site triple's 24), a run over
    // several with k_row_table first.  Every other --LD run takes the LIBD2 window products of the covered rows only.
    // (stream2, behind this run's recount of the alt counts; readers: see ibdg_ctx::row_tab)
    ibdg::RowsArgs ra = sa;
    if (P.rt_build) {
        ra.row_tab = (double *)c->rt.row_tab.p;
        if (P.T > 1) {
            ibdg::launch_row_table(ra, c->stream2);
            ra.row_tab = nullptr;
        }
    }
    ibdg::launch_rows_windows(ra, (unsigned)P.T, c->stream2, P.row_blocks);
    if (c->opt.log_windows)            // (the row-sum columns of the log table: ibdg_ctx::WinLog)
        ibdg::launch_win_log_rows(sa, (unsigned)P.T, (double *)c->wlog.win_log2.p, c->stream2);
    HIP_TRY(c, hipEventRecord(E.s2_end, c->stream2));
    c->tl.last_s2 = E.s2_end;
    c->tl.s2_pending = true;
    return 0;
}

}  // namespace

extern "C" {

int ibdg_run(ibdg_ctx *c, const uint32_t *targets, size_t T, const uint8_t *bg_count, int pu_id, int ld_mode)
{
    if (!c) return 1;
    if (!c->pan.panel.p || c->pan.n_ids == 0) return fail(c, "[::] ERROR in ibdg_run: no panel uploaded");
    if (!c->sites.sites_valid) return fail(c, "[::] ERROR in ibdg_run: no sites uploaded");
    if (T == 0 || !targets) return fail(c, "[::] ERROR in ibdg_run: no targets");
    if (T > 65535) return fail(c, "[::] ERROR in ibdg_run: at most 65535 targets per call");
    c->ls.drop();                            // (the paths, posteriors and records belong to the run before)
    for (size_t t = 0; t < T; ++t)
        if (targets[t] >= c->pan.n_ids)
            return fail(c, "[::] ERROR in ibdg_run: target %u is not a panel individual (n_ids=%u)", targets[t],
                        c->pan.n_ids);
    HIP_TRY(c, hipSetDevice(c->device));

    const size_t lanes = (size_t)c->pan.n_groups * c->pan.cpw * 64;
    const bool want_ll = c->opt.site_results != 0;
    // --LD: the per-site values come from the site list's row table (one for every comparison individual: they differ by the
    // genotype picked), made once per upload; an individual's per-site table is put together when it is fetched (k_site_expand)
    const bool row_table = want_ll && ld_mode;
    if (ensure(c, c->targets, Ring::SLOTS * T * 4) || (want_ll && ensure(c, c->site_ll, (row_table ? 1 : T) * c->sites.n_sites * 24)) ||
        (row_table && ensure(c, c->rt.row_tab, c->sites.n_sites * 32)) || ensure(c, c->win_ll, T * (size_t)c->sites.n_win * 24) ||
        (c->opt.log_windows && ensure(c, c->wlog.win_log2, T * (size_t)c->sites.n_win * 24)))
        return 1;
    // targets / background weights change rarely between calls (a loop over windows sizes, repeated
    // timing steps): their device copies are rebuilt only when the inputs differ
    const bool same_bg = c->bg.prev_pu == pu_id && c->bg.prev_has_bg == (bg_count ? 1 : 0) && c->bg.prev_lanes == lanes &&
                         (!bg_count || (c->bg.prev_bg.size() == c->pan.n_ids &&
                                        std::equal(bg_count, bg_count + c->pan.n_ids, c->bg.prev_bg.begin()))) &&
                         c->bg.base_w.p;
    const bool same_inputs = same_bg && c->prev_targets.size() == T && std::equal(targets, targets + T, c->prev_targets.begin()) &&
                             c->weight.p;
    if (!same_bg && set_background(c, bg_count, pu_id, lanes)) return 1;
    if (ring_settle(c) || (!same_inputs && ring_prepare(c, targets, T, lanes))) return 1;   // (settles what a failed run left)
    if (ld_mode && relayout_when_paid(c, T)) return 1;
    RunPlan P;
    if (plan_run(c, T, lanes, ld_mode, row_table, P)) return 1;
    const bool ld_log = c->opt.log_windows && ld_mode && c->sites.n_win > 0;
    if (ld_log && ld_log_refused(c))
        return fail(c, "[::] ERROR in ibdg_run: log_windows cannot give the --LD columns here: %s", ld_log_refused(c));
    c->last_variant = P.variant;
    c->last_count_unit = P.count_unit;
    c->last_window_end = P.window_end;
    // A finalising step left by the run before rides in this run's k_ld_popcount launch only where this run is of the same
    // shape over the same background and prepared sites (it reads the windows' constants and its own run's background sizes)
    // and no IBD0 pass rewrites its sums first; the strict and non-LD kernels write the same win_ll entries themselves, and
    // the stale sums must not land behind them.  Otherwise it is made up for here, before the run's first launch.
    const bool flush = c->fin.pending && (!same_bg || c->fin.sites_gen != c->sites_gen || !P.use_pop || P.ibd0_pass ||
                                          !P.fin_in_next || c->fin.count != (unsigned)P.T_cnt || c->fin.args.t_base != (uint32_t)P.T_g);
    if (flush && flush_finalize(c)) return 1;
    const int ev_slot = (c->tl.ev_head + 1) % ibdg_ctx::Timeline::EV_RING;      // becomes the head once the run is queued
    EvSet &E = c->tl.evs[ev_slot];
    if (start_run(c, P, E, flush)) return 1;

    const ibdg::RowsArgs sa = rows_args(c, ld_mode, row_table);
    if (ld_log && launch_log_windows(c, P)) return 1;
    if (P.use_pop ? launch_pop(c, P, E, same_inputs) : ld_mode && launch_strict(c, P, targets, bg_count, pu_id)) return 1;
    if (ring_settle(c)) return 1;
    if (P.rows_on_main) {
        if (join_streams(c)) return 1;           // an earlier run's kernel on stream2 may still write the results
        // alone on the chip: a wave per pair of windows (the default).  A resident grid whose waves walk over several windows -- even
        // with the next window's records kept in flight -- measured slower at every size (rows_blocks_per_cu 4..28:
        // 0.048-0.041 ms against 0.040)
        unsigned blocks = 0;
        if (c->opt.rows_blocks > 0)
            blocks = std::max<unsigned>(1u, (unsigned)((size_t)c->n_cu * c->opt.rows_blocks / T));
        ibdg::launch_rows_windows(sa, (unsigned)T, c->stream, blocks);
        if (c->opt.log_windows)
            ibdg::launch_win_log_rows(sa, (unsigned)T, (double *)c->wlog.win_log2.p, c->stream);
    }
    if (!P.dispatch_events && !P.end_in_dispatch)
        HIP_TRY(c, hipEventRecord(E.ld_end, c->stream));
    if (!P.rows_on_main && queue_stream2(c, P, sa, E)) return 1;
    ring_mark_readers(c, T, E.ld_end, P.rows_on_main ? nullptr : E.s2_end);
    HIP_TRY(c, hipGetLastError());
    if (P.rt_build)
        c->rt.made(*c);
    c->tl.ev_head = ev_slot; ++c->tl.runs_done; c->tl.chain_ok = true;
    if (!c->opt.async && quiesce(c)) return 1;
    c->n_targets = T; c->have_results = true;
    c->res_site_mode = row_table ? 2 : (int)c->opt.site_results;
    c->wlog.valid = c->opt.log_windows != 0;
    return 0;
}

static int fetch(ibdg_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    if (join_streams(c)) return 1;
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return quiesce(c);
}

int ibdg_get_site_af(ibdg_ctx *c, double *af)
{
    if (!c) return 1;
    if (!c->have_results) return fail(c, "[::] ERROR in ibdg_get_site_af: no results (call ibdg_run)");
    if (!c->pan.counts_valid) return fail(c, "[::] ERROR in ibdg_get_site_af: alt counts not computed yet");
    // made when asked for: it depends on the panel row (or the -A value) only, and no run needs it
    HIP_TRY(c, hipSetDevice(c->device));
    if (ensure(c, c->af, c->sites.n_sites * 8)) return 1;
    if (join_streams(c)) return 1;
    ibdg::RowsArgs ra = {};
    ra.rec_all = (const uint2 *)c->sites.rec_all.p;
    ra.n_sites = c->sites.n_sites;
    ra.n_ids = c->pan.n_ids;
    ra.alt_count = (const uint32_t *)c->pan.alt_count.p;
    ra.fo = c->sites.have_fo ? (const double *)c->sites.fo.p : nullptr;
    ra.af = (double *)c->af.p;
    ibdg::launch_site_af(ra, c->stream);
    HIP_TRY(c, hipGetLastError());
    return fetch(c, af, c->af.p, c->sites.n_sites * 8);
}

int ibdg_get_site_ll(ibdg_ctx *c, size_t t, double *out)
{
    if (!c) return 1;
    if (!c->have_results || t >= c->n_targets) return fail(c, "[::] ERROR in ibdg_get_site_ll: no results for target %zu", t);
    if (c->res_site_mode == 0) return fail(c, "[::] ERROR in ibdg_get_site_ll: the run kept no per-site results (option site_results)");
    if (c->res_site_mode == 2) {
        // the site list's row table (ibdg_ctx::row_tab): the per-site table of the last run's individual t from it
        if (t >= c->prev_targets.size()) return fail(c, "[::] ERROR in ibdg_get_site_ll: no results for target %zu", t);
        HIP_TRY(c, hipSetDevice(c->device));
        if (join_streams(c)) return 1;
        ibdg::RowsArgs ra = {};
        ra.panel = (const uint64_t *)c->pan.panel.p;
        ra.stride = c->pan.stride;
        ra.n_ids = c->pan.n_ids;
        ra.rec_all = (const uint2 *)c->sites.rec_all.p;
        ra.n_sites = c->sites.n_sites;
        ra.lut = (const double *)c->tab.lut.p;
        ra.t32 = c->tab.pop_lut_ok ? (const uint4 *)c->pan.t32.p : nullptr;
        ra.n_pairs = c->pan.n_pairs;
        ra.row_tab = (double *)c->rt.row_tab.p;
        ibdg::launch_site_expand(ra, c->prev_targets[t], (double *)c->site_ll.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        return fetch(c, out, c->site_ll.p, c->sites.n_sites * 24);
    }
    return fetch(c, out, (const char *)c->site_ll.p + t * c->sites.n_sites * 24, c->sites.n_sites * 24);
}

int ibdg_get_window_ll(ibdg_ctx *c, size_t t, double *out)
{
    if (!c) return 1;
    if (!c->have_results || t >= c->n_targets) return fail(c, "[::] ERROR in ibdg_get_window_ll: no results for target %zu", t);
    return fetch(c, out, (const char *)c->win_ll.p + t * (size_t)c->sites.n_win * 24, (size_t)c->sites.n_win * 24);
}

int ibdg_get_window_ll_all(ibdg_ctx *c, double *out)
{
    if (!c) return 1;
    if (!c->have_results) return fail(c, "[::] ERROR in ibdg_get_window_ll_all: no results (call ibdg_run)");
    return fetch(c, out, c->win_ll.p, c->n_targets * (size_t)c->sites.n_win * 24);
}

int ibdg_get_window_log2(ibdg_ctx *c, size_t t, double *out)
{
    if (!c) return 1;
    if (!c->have_results || t >= c->n_targets) return fail(c, "[::] ERROR in ibdg_get_window_log2: no results for target %zu", t);
    if (!c->wlog.valid) return fail(c, "[::] ERROR in ibdg_get_window_log2: the last run kept no window logs (option log_windows)");
    return fetch(c, out, (const char *)c->wlog.win_log2.p + t * (size_t)c->sites.n_win * 24, (size_t)c->sites.n_win * 24);
}

int ibdg_get_window_log2_all(ibdg_ctx *c, double *out)
{
    if (!c) return 1;
    if (!c->have_results) return fail(c, "[::] ERROR in ibdg_get_window_log2_all: no results (call ibdg_run)");
    if (!c->wlog.valid) return fail(c, "[::] ERROR in ibdg_get_window_log2_all: the last run kept no window logs (option log_windows)");
    return fetch(c, out, c->wlog.win_log2.p, c->n_targets * (size_t)c->sites.n_win * 24);
}

// The caller's table in place of the last run's (tests, and callers that gathered a table elsewhere).  The copy is queued on the
// main stream behind join_streams -- the run's own writers of the table are in front of it -- and waited for on the host: tab may
// go once this returns.  Everything the log-domain state calls keep is a function of the table: drop().  Nothing else of the
// run is touched; the next ibdg_run writes the whole table again.  A refused call changes nothing.
int ibdg_set_window_log2(ibdg_ctx *c, const double *tab, size_t n_targets)
{
    if (!c) return 1;
    if (!c->have_results) return fail(c, "[::] ERROR in ibdg_set_window_log2: no results (call ibdg_run)");
    if (!c->wlog.valid) return fail(c, "[::] ERROR in ibdg_set_window_log2: the last run kept no window logs (option log_windows)");
    if (n_targets != c->n_targets)
        return fail(c, "[::] ERROR in ibdg_set_window_log2: %zu tables for the %zu comparison individuals of the last run", n_targets, c->n_targets);
    if (!tab) return fail(c, "[::] ERROR in ibdg_set_window_log2: NULL tab");
    const size_t bytes = c->n_targets * (size_t)c->sites.n_win * 24;
    HIP_TRY(c, hipSetDevice(c->device));
    if (join_streams(c)) return 1;
    if (bytes)
        HIP_TRY(c, hipMemcpyAsync(c->wlog.win_log2.p, tab, bytes, hipMemcpyHostToDevice, c->stream));
    if (quiesce(c)) return 1;
    c->ls.drop();
    return 0;
}

// Segmented sums over the window table of the last run (ibdg_llr.hip).  On the main stream behind join_streams: LIBD2 comes
// from stream2, LIBD0/LIBD1 may come from a finalising launch still pending for the next run.  The segments go in chunks
// whose slab of partials stays under LLR_SLAB items (one segment per chunk at least: its slab is then ~1/1500 of win_ll).
static int llr_sums(ibdg_ctx *c, const char *fn, bool from_log, const uint32_t *first, const uint32_t *end, size_t n_seg, double *out)
{
    if (!c) return 1;
    if (!c->have_results) return fail(c, "[::] ERROR in %s: no results (call ibdg_run)", fn);
    if (n_seg && (!first || !end || !out)) return fail(c, "[::] ERROR in %s: NULL array", fn);
    if (from_log && !c->wlog.valid) return fail(c, "[::] ERROR in %s: the last run kept no window logs (option log_windows)", fn);
    for (size_t s = 0; s < n_seg; ++s) {
        if (end[s] < first[s])
            return fail(c, "[::] ERROR in %s: range %zu is reversed ([%u, %u))", fn, s, first[s], end[s]);
        if (end[s] > c->sites.n_win)
            return fail(c, "[::] ERROR in %s: range %zu ends at %u, past the %u windows", fn, s, end[s], c->sites.n_win);
    }
    if (n_seg == 0 || c->n_targets == 0) return 0;
    constexpr size_t LLR_SLAB = (size_t)1 << 22;
    const size_t T = c->n_targets;
    std::vector<uint32_t> seg(2 * n_seg);
    uint32_t nb = 1;
    for (size_t s = 0; s < n_seg; ++s) {
        seg[2 * s] = first[s];
        seg[2 * s + 1] = end[s];
        nb = std::max<uint32_t>(nb, (uint32_t)(((uint64_t)end[s] - first[s] + ibdg::LLR_BLK - 1) / ibdg::LLR_BLK));
    }
    const size_t chunk = std::max<size_t>(1, std::min(n_seg, LLR_SLAB / (T * nb)));
    HIP_TRY(c, hipSetDevice(c->device));
    if (ensure(c, c->llr_seg, chunk * 8) || ensure(c, c->llr_part, T * chunk * nb * 32) || ensure(c, c->llr_out, T * chunk * 32))
        return 1;
    if (join_streams(c)) return 1;
    for (size_t s0 = 0; s0 < n_seg; s0 += chunk) {
        const size_t m = std::min(chunk, n_seg - s0);
        HIP_TRY(c, hipMemcpyAsync(c->llr_seg.p, seg.data() + 2 * s0, m * 8, hipMemcpyHostToDevice, c->stream));
        ibdg::launch_llr_sums((const double *)(from_log ? c->wlog.win_log2.p : c->win_ll.p), c->sites.n_win, (uint32_t)T, (const uint32_t *)c->llr_seg.p, (uint32_t)m,
                              nb, (double *)c->llr_part.p, (double *)c->llr_out.p, c->stream, from_log);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpy2DAsync(out + s0 * 4, n_seg * 32, c->llr_out.p, m * 32, m * 32, T, hipMemcpyDeviceToHost, c->stream));
        if (s0 + m < n_seg)                              // (the next chunk reuses the device buffers)
            HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return quiesce(c);
}

int ibdg_window_llr_sums(ibdg_ctx *c, const uint32_t *first, const uint32_t *end, size_t n_seg, double *out)
{
    return llr_sums(c, __func__, false, first, end, n_seg, out);
}

// The same over win_log2, whose entries are the terms (its writers are covered by join_streams like win_ll's: WinLog in ibdg_ctx.h)
int ibdg_window_log2_llr_sums(ibdg_ctx *c, const uint32_t *first, const uint32_t *end, size_t n_seg, double *out)
{
    return llr_sums(c, __func__, true, first, end, n_seg, out);
}

int ibdg_log2_states_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, uint8_t *path, int64_t *score,
                          uint64_t count[3])
{
    char msg[256];
    if (ibdg::log2_states_host(__func__, log2_tab, n_win, p01, p02, p12, nullptr, 0, nullptr, path, score, count, msg, sizeof msg))
        return fail(nullptr, "%s", msg);
    return 0;
}

int ibdg_log2_states_chains_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, uint8_t *path, int64_t *score,
                                 uint64_t count[3], const uint32_t *starts, size_t n_starts)
{
    char msg[256];
    if (ibdg::log2_states_host(__func__, log2_tab, n_win, p01, p02, p12, starts, n_starts, nullptr, path, score, count, msg, sizeof msg))
        return fail(nullptr, "%s", msg);
    return 0;
}

int ibdg_log2_states_steps_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, uint8_t *path, int64_t *score,
                                uint64_t count[3], const uint32_t *starts, size_t n_starts, const int32_t *shift)
{
    char msg[256];
    if (ibdg::log2_states_host(__func__, log2_tab, n_win, p01, p02, p12, starts, n_starts, shift, path, score, count, msg, sizeof msg))
        return fail(nullptr, "%s", msg);
    return 0;
}

// ---- the log-domain state calls over win_log2 of the last run (ibdg_states.hip; LogStates in ibdg_ctx.h has the rule) ----
// Each public call is: log_call_begin, join_streams (the table's writers: WinLog in ibdg_ctx.h), the stages it needs, its
// copies out, quiesce -- no reader of the table and no kernel of the group outlives the call.
struct LogCall {                     // an accepted call: the penalties in quanta, their weights, the size of the run
    int64_t P[3];
    double a[3];
    size_t T, n_win;
};

// Every check the three calls share, in the order and with the text each had.  own: the caller's complaint about its own
// arguments, or NULL; max_tail: how its refusal of too many windows ends.
static int log_call_begin(ibdg_ctx *c, const char *fn, const char *own, const char *max_tail, double p01, double p02, double p12,
                          LogCall &L)
{
    if (!c->have_results) return fail(c, "[::] ERROR in %s: no results (call ibdg_run)", fn);
    if (!c->wlog.valid) return fail(c, "[::] ERROR in %s: the last run kept no window logs (option log_windows)", fn);
    if (own) return fail(c, "[::] ERROR in %s: %s", fn, own);
    int bad = 0;
    if (ibdg::states_penalties(p01, p02, p12, L.P, &bad)) {
        static const char *const name[3] = {"p01", "p02", "p12"};
        return fail(c, "[::] ERROR in %s: %s = %g is not in (0, 1]", fn, name[bad], bad == 0 ? p01 : bad == 1 ? p02 : p12);
    }
    ibdg::post_penalty_weights(L.P, L.a);
    L.T = c->n_targets, L.n_win = c->sites.n_win;
    if (L.n_win > ibdg::STATES_MAX_WIN)
        return fail(c, "[::] ERROR in %s: %zu windows, more than the %zu (2^21) %s", fn, L.n_win, ibdg::STATES_MAX_WIN, max_tail);
    return 0;
}

// The stages: each makes sure of its buffers and queues its launch on the main stream, behind the caller's join_streams; none
// waits on the host.  A product that is fresh for L.P is not made again; the scores are not kept, so want_score launches.
static int enqueue_states(ibdg_ctx *c, const LogCall &L, bool want_score)
{
    ibdg_ctx::LogStates &S = c->ls;
    if (ensure(c, S.path, L.T * L.n_win) || ensure(c, S.count, L.T * 24) || (want_score && ensure(c, S.score, L.T * L.n_win * 24)))
        return 1;
    if (S.fresh(S.PATH, L.P) && !want_score) return 0;
    ibdg::launch_log2_states((const double *)c->wlog.win_log2.p, (uint32_t)L.n_win, (uint32_t)L.T, L.P, S.mask(), S.shift(), (uint8_t *)S.path.p,
                             want_score ? (int64_t *)S.score.p : nullptr, (uint64_t *)S.count.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    S.made(S.PATH, L.P);
    return 0;
}

static int enqueue_posteriors(ibdg_ctx *c, const LogCall &L)
{
    ibdg_ctx::LogStates &S = c->ls;
    if (ensure(c, S.post, L.T * L.n_win * 24) || ensure(c, S.pout, L.T * 40) || ensure(c, S.ptab, 4096))
        return 1;
    if (S.fresh(S.POST, L.P)) return 0;
    HIP_TRY(c, hipMemcpyAsync(S.ptab.p, ibdg::post_tables(), 4096, hipMemcpyHostToDevice, c->stream));
    ibdg::launch_log2_posteriors((const double *)c->wlog.win_log2.p, (uint32_t)L.n_win, (uint32_t)L.T, L.P, L.a, (const double *)S.ptab.p,
                                 S.mask(), S.shift(), (double *)S.post.p, (double *)S.pout.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    S.made(S.POST, L.P);
    return 0;
}

// (behind enqueue_states: it reads the path; d_first, d_last: the windows' positions on the device, or both NULL)
static int enqueue_segments_count(ibdg_ctx *c, const LogCall &L, const uint64_t *d_first, const uint64_t *d_last)
{
    if (ensure(c, c->ls.sout, L.T * 104)) return 1;
    ibdg::launch_log2_segments_count((const uint8_t *)c->ls.path.p, (uint32_t)L.n_win, (uint32_t)L.T, d_first, d_last,
                                     c->ls.mask(), (uint64_t *)c->ls.sout.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

// IBD-state paths: the states stage, the counts (and what else is asked for) out
int ibdg_window_log2_states(ibdg_ctx *c, double p01, double p02, double p12, uint8_t *path, int64_t *score, uint64_t *count)
{
    if (!c) return 1;
    LogCall L;
    if (log_call_begin(c, __func__, count ? nullptr : "NULL count", "the integer scores allow", p01, p02, p12, L)) return 1;
    if (L.T == 0) return 0;
    if (L.n_win == 0) {
        memset(count, 0, L.T * 3 * sizeof *count);
        return 0;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    c->ls.records_drop();
    if (join_streams(c) || enqueue_states(c, L, score != nullptr)) return 1;
    HIP_TRY(c, hipMemcpyAsync(count, c->ls.count.p, L.T * 24, hipMemcpyDeviceToHost, c->stream));
    if (path) HIP_TRY(c, hipMemcpyAsync(path, c->ls.path.p, L.T * L.n_win, hipMemcpyDeviceToHost, c->stream));
    if (score) HIP_TRY(c, hipMemcpyAsync(score, c->ls.score.p, L.T * L.n_win * 24, hipMemcpyDeviceToHost, c->stream));
    return quiesce(c);
}

static int posteriors_twin(const char *fn, const double *log2_tab, size_t n_win, double p01, double p02, double p12, double *post,
                           double expect[3], double *log2_z, const uint32_t *starts, size_t n_starts, const int32_t *shift)
{
    char msg[256];
    double zm = 1.0;
    int ze = 0;
    if (!log2_z) return fail(nullptr, "[::] ERROR in %s: NULL log2_z", fn);
    if (ibdg::log2_posteriors_host(fn, log2_tab, n_win, p01, p02, p12, starts, n_starts, shift, post, expect, &zm, &ze, msg, sizeof msg))
        return fail(nullptr, "%s", msg);
    *log2_z = std::log2(zm) + (double)ze;
    return 0;
}

int ibdg_log2_posteriors_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, double *post,
                              double expect[3], double *log2_z)
{
    return posteriors_twin(__func__, log2_tab, n_win, p01, p02, p12, post, expect, log2_z, nullptr, 0, nullptr);
}

int ibdg_log2_posteriors_chains_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, double *post,
                                     double expect[3], double *log2_z, const uint32_t *starts, size_t n_starts)
{
    return posteriors_twin(__func__, log2_tab, n_win, p01, p02, p12, post, expect, log2_z, starts, n_starts, nullptr);
}

int ibdg_log2_posteriors_steps_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, double *post,
                                    double expect[3], double *log2_z, const uint32_t *starts, size_t n_starts, const int32_t *shift)
{
    return posteriors_twin(__func__, log2_tab, n_win, p01, p02, p12, post, expect, log2_z, starts, n_starts, shift);
}

// IBD-state posteriors (k_log2_posteriors): the posteriors stage, expect and Z (and the gammas when asked for) out
int ibdg_window_log2_posteriors(ibdg_ctx *c, double p01, double p02, double p12, double *post, double *expect, double *log2_z)
{
    if (!c) return 1;
    LogCall L;
    if (log_call_begin(c, __func__, !expect ? "NULL expect" : !log2_z ? "NULL log2_z" : nullptr, "of the path", p01, p02, p12, L))
        return 1;
    const size_t T = L.T;
    if (T == 0) return 0;
    if (L.n_win == 0) {
        memset(expect, 0, T * 3 * sizeof *expect);
        memset(log2_z, 0, T * sizeof *log2_z);
        return 0;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    c->ls.records_drop();
    if (join_streams(c) || enqueue_posteriors(c, L)) return 1;
    std::vector<double> o(T * 5);
    HIP_TRY(c, hipMemcpyAsync(o.data(), c->ls.pout.p, T * 40, hipMemcpyDeviceToHost, c->stream));
    if (post) HIP_TRY(c, hipMemcpyAsync(post, c->ls.post.p, T * L.n_win * 24, hipMemcpyDeviceToHost, c->stream));
    if (quiesce(c)) return 1;
    for (size_t t = 0; t < T; ++t) {
        expect[3 * t] = o[5 * t], expect[3 * t + 1] = o[5 * t + 1], expect[3 * t + 2] = o[5 * t + 2];
        log2_z[t] = std::log2(o[5 * t + 3]) + o[5 * t + 4];
    }
    return 0;
}

int ibdg_log2_switches_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                            size_t n_starts, const int32_t *shift, double *sw, double expect[3], uint64_t counted[3])
{
    char msg[256];
    if (ibdg::log2_switches_host(__func__, log2_tab, n_win, p01, p02, p12, starts, n_starts, shift, sw, expect, counted, msg, sizeof msg))
        return fail(nullptr, "%s", msg);
    return 0;
}

int ibdg_switch_penalty_update(const double p[3], const double total[3], size_t n_individuals, const double prior[3], double next[3])
{
    if (!p || !total || !prior || !next)
        return fail(nullptr, "[::] ERROR in %s: NULL %s", __func__, !p ? "p" : !total ? "total" : !prior ? "prior" : "next");
    ibdg::switch_penalty_update(p, total, n_individuals, prior, next);
    return 0;
}

// the prior under the context's chains and steps: the twin on the NULL table, no device work
int ibdg_window_log2_switches_prior(ibdg_ctx *c, double p01, double p02, double p12, double expect[3], uint64_t counted[3])
{
    if (!c) return 1;
    if (!c->sites.sites_valid) return fail(c, "[::] ERROR in %s: no valid site list (call ibdg_upload_sites)", __func__);
    const ibdg_ctx::LogStates &S = c->ls;
    char msg[256];
    if (ibdg::log2_switches_host(__func__, nullptr, c->sites.n_win, p01, p02, p12, S.chains.data(), S.chains.size(),
                                 S.steps.empty() ? nullptr : S.steps.data(), nullptr, expect, counted, msg, sizeof msg))
        return fail(c, "%s", msg);
    return 0;
}

// Switches (k_log2_switches): one launch over the posteriors' scratch, which it leaves holding beta or sw -- the posteriors kept
// there and the records cut from them go stale --, the expectations (and the rows when asked for) out
int ibdg_window_log2_switches(ibdg_ctx *c, double p01, double p02, double p12, double *sw, double *expect)
{
    if (!c) return 1;
    LogCall L;
    if (log_call_begin(c, __func__, !expect ? "NULL expect" : nullptr, "of the path", p01, p02, p12, L)) return 1;
    const size_t T = L.T;
    if (T == 0) return 0;
    if (L.n_win == 0) {
        memset(expect, 0, T * 3 * sizeof *expect);
        return 0;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    ibdg_ctx::LogStates &S = c->ls;
    S.records_drop();
    if (ensure(c, S.post, T * L.n_win * 24) || ensure(c, S.pout, T * 40) || ensure(c, S.ptab, 4096)) return 1;
    if (join_streams(c)) return 1;
    S.have[S.POST] = false;
    HIP_TRY(c, hipMemcpyAsync(S.ptab.p, ibdg::post_tables(), 4096, hipMemcpyHostToDevice, c->stream));
    ibdg::launch_log2_switches((const double *)c->wlog.win_log2.p, (uint32_t)L.n_win, (uint32_t)T, L.P, L.a, (const double *)S.ptab.p, S.mask(),
                               S.shift(), sw != nullptr, (double *)S.post.p, (double *)S.pout.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(expect, S.pout.p, T * 24, hipMemcpyDeviceToHost, c->stream));
    if (sw) HIP_TRY(c, hipMemcpyAsync(sw, S.post.p, T * L.n_win * 24, hipMemcpyDeviceToHost, c->stream));
    return quiesce(c);
}

// ---- the fit of the switch penalties: one step, the twin's loop, the table store and the loop over it ----

int ibdg_switch_fit_step(const double p[3], const double total[3], size_t n_individuals, const double prior[3],
                         const uint64_t counted[3], ibdg_fit_row *row, double next[3], int *stood)
{
    static const char *const name[3] = {"p01", "p02", "p12"};
    const char *null_arg = !p ? "p" : !total ? "total" : !prior ? "prior" : !counted ? "counted" : !row ? "row" : !next ? "next" :
                           !stood ? "stood" : nullptr;
    if (null_arg)
        return fail(nullptr, "[::] ERROR in %s: NULL %s", __func__, null_arg);
    const int bad = ibdg::switch_fit_step(p, total, n_individuals, prior, counted, row, next, stood);
    if (bad)
        return fail(nullptr, "[::] ERROR in %s: %s = %g is not in (0, 1]", __func__, name[bad - 1], p[bad - 1]);
    return 0;
}

int ibdg_log2_fit_host(const double *const *tabs, size_t n_individuals, size_t n_win, const double p[3], const uint32_t *starts,
                       size_t n_starts, const int32_t *shift, size_t max_iter, ibdg_fit_row *rows, size_t *n_rows, int *stood,
                       double fitted[3])
{
    char msg[256];
    if (ibdg::log2_fit_host(__func__, tabs, n_individuals, n_win, p, starts, n_starts, shift, max_iter, rows, n_rows, stood, fitted, msg,
                            sizeof msg))
        return fail(nullptr, "%s", msg);
    return 0;
}

// The store (LogStore in ibdg_ctx.h has the rule).  A device buffer of `bytes` for it, kept when large enough; a failure names
// the bytes asked for.  (ensure()'s wait for queued runs: the buffer may be read by a launch of an earlier call only, and every
// such call ends in a host wait.)
static int store_buffer(ibdg_ctx *c, const char *fn, DevBuf &b, size_t bytes, const char *what)
{
    if (bytes == 0)
        bytes = 16;
    if (b.cap >= bytes)
        return 0;
    b.release();
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(c, "[::] ERROR in %s: cannot allocate %zu bytes of device memory for %s: %s", fn, bytes, what, hipGetErrorString(e));
    }
    b.cap = bytes;
    ++b.allocs;
    return 0;
}

int ibdg_log2_store_reserve(ibdg_ctx *c, size_t n_individuals)
{
    if (!c) return 1;
    if (!c->sites.sites_valid) return fail(c, "[::] ERROR in %s: no valid site list (call ibdg_upload_sites)", __func__);
    if (n_individuals > 0x7fffffffu)
        return fail(c, "[::] ERROR in %s: %zu individuals, more than the 2^31 - 1 a store holds", __func__, n_individuals);
    c->lstore.empty();
    c->lstore.cap = n_individuals;
    c->lstore.reserved = true;
    return 0;
}

size_t ibdg_log2_store_count(ibdg_ctx *c) { return c ? c->lstore.count : 0; }

int ibdg_log2_store_append(ibdg_ctx *c)
{
    if (!c) return 1;
    if (!c->have_results) return fail(c, "[::] ERROR in %s: no results (call ibdg_run)", __func__);
    if (!c->wlog.valid) return fail(c, "[::] ERROR in %s: the last run kept no window logs (option log_windows)", __func__);
    ibdg_ctx::LogStore &R = c->lstore;
    if (!R.reserved) return fail(c, "[::] ERROR in %s: no store (call ibdg_log2_store_reserve)", __func__);
    const size_t T = c->n_targets, row = (size_t)c->sites.n_win * 24;
    if (T > R.cap - R.count)
        return fail(c, "[::] ERROR in %s: %zu individuals stored and %zu more, beyond the reserve of %zu", __func__, R.count, T, R.cap);
    HIP_TRY(c, hipSetDevice(c->device));
    if (store_buffer(c, __func__, R.tabs, R.cap * row, "the table store")) return 1;
    if (join_streams(c)) return 1;
    if (T * row)
        HIP_TRY(c, hipMemcpyAsync((char *)R.tabs.p + R.count * row, c->wlog.win_log2.p, T * row, hipMemcpyDeviceToDevice, c->stream));
    if (quiesce(c)) return 1;
    R.count += T;
    return 0;
}

// what ibdg_log2_store_switches and ibdg_log2_store_fit refuse alike, and the launch with its copy out and host wait
static int store_begin(ibdg_ctx *c, const char *fn, const char *own, double p01, double p02, double p12, LogCall &L)
{
    if (log_call_begin(c, fn, own, "of the path", p01, p02, p12, L)) return 1;
    if (!c->lstore.reserved) return fail(c, "[::] ERROR in %s: no store (call ibdg_log2_store_reserve)", fn);
    return 0;
}

// (tables: the 4 KB of post_tables go up in front of the launch -- a fit's iterations after the first find them there: every
// one ends in a host wait, and nothing else runs on the context inside the call)
static int store_expect(ibdg_ctx *c, const char *fn, const LogCall &L, bool tables, double *expect)
{
    ibdg_ctx::LogStore &R = c->lstore;
    ibdg_ctx::LogStates &S = c->ls;
    const size_t n = R.count;
    if (n == 0) return 0;
    if (L.n_win == 0) {
        memset(expect, 0, n * 3 * sizeof *expect);
        return 0;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t grid = ibdg::switch_expect_grid(n, c->n_cu);
    if (store_buffer(c, fn, R.scr, (size_t)grid * L.n_win * 24, "the workgroups' scratch") || store_buffer(c, fn, R.out, n * 24, "the expectations") ||
        ensure(c, S.ptab, 4096))
        return 1;
    if (join_streams(c)) return 1;
    if (tables)
        HIP_TRY(c, hipMemcpyAsync(S.ptab.p, ibdg::post_tables(), 4096, hipMemcpyHostToDevice, c->stream));
    ibdg::launch_log2_switch_expect((const double *)R.tabs.p, (uint32_t)L.n_win, (uint32_t)n, grid, L.P, L.a, (const double *)S.ptab.p, S.mask(),
                                    S.shift(), (double *)R.scr.p, (double *)R.out.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(expect, R.out.p, n * 24, hipMemcpyDeviceToHost, c->stream));
    return quiesce(c);
}

int ibdg_log2_store_switches(ibdg_ctx *c, double p01, double p02, double p12, double *expect)
{
    if (!c) return 1;
    LogCall L;
    if (store_begin(c, __func__, !expect ? "NULL expect" : nullptr, p01, p02, p12, L)) return 1;
    return store_expect(c, __func__, L, true, expect);
}

int ibdg_log2_store_fit(ibdg_ctx *c, const double p[3], size_t max_iter, ibdg_fit_row *rows, size_t *n_rows, int *stood, double fitted[3])
{
    if (!c) return 1;
    LogCall L;
    const char *own = !p ? "NULL p" : !n_rows ? "NULL n_rows" : !stood ? "NULL stood" : !fitted ? "NULL fitted" :
                      max_iter && !rows ? "NULL rows" : nullptr;
    if (store_begin(c, __func__, own, p ? p[0] : 1.0, p ? p[1] : 1.0, p ? p[2] : 1.0, L)) return 1;
    const ibdg_ctx::LogStates &S = c->ls;
    const size_t T = c->lstore.count;
    double cur[3] = {p[0], p[1], p[2]};
    *n_rows = 0, *stood = 0;
    fitted[0] = cur[0], fitted[1] = cur[1], fitted[2] = cur[2];
    std::vector<double> expect(T * 3);
    for (size_t it = 0; T && it < max_iter && !*stood; ++it) {
        double total[3] = {0.0, 0.0, 0.0}, prior[3], next[3];
        uint64_t counted[3];
        char msg[256];
        (void)ibdg::states_penalties(cur[0], cur[1], cur[2], L.P, nullptr);     // (checked: p above, then the update's range)
        ibdg::post_penalty_weights(L.P, L.a);
        if (store_expect(c, __func__, L, it == 0, expect.data())) return 1;
        for (size_t t = 0; t < T; ++t)              // the round trip of 24 T bytes and this sum stay on the host: microseconds
            for (int k = 0; k < 3; ++k)              // beside the launch, and the order of the additions is the twin's
                total[k] = total[k] + expect[3 * t + k];
        if (ibdg::log2_switches_host(__func__, nullptr, L.n_win, cur[0], cur[1], cur[2], S.chains.data(), S.chains.size(),
                                     S.steps.empty() ? nullptr : S.steps.data(), nullptr, prior, counted, msg, sizeof msg))
            return fail(c, "%s", msg);
        (void)ibdg::switch_fit_step(cur, total, T, prior, counted, &rows[it], next, stood);
        *n_rows = it + 1;
        for (int k = 0; k < 3; ++k)
            cur[k] = fitted[k] = next[k];
    }
    return 0;
}

int ibdg_log2_segments_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, int with_post,
                            const uint64_t *pos_first, const uint64_t *pos_last, ibdg_segment *seg, size_t seg_cap, uint64_t *n_seg,
                            uint64_t summary[12])
{
    char msg[256];
    if (ibdg::log2_segments_host(__func__, log2_tab, n_win, p01, p02, p12, nullptr, 0, nullptr, with_post, pos_first, pos_last, seg, seg_cap,
                                 n_seg, summary, msg, sizeof msg))
        return fail(nullptr, "%s", msg);
    return 0;
}

int ibdg_log2_segments_chains_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, int with_post,
                                   const uint64_t *pos_first, const uint64_t *pos_last, ibdg_segment *seg, size_t seg_cap,
                                   uint64_t *n_seg, uint64_t summary[12], const uint32_t *starts, size_t n_starts)
{
    char msg[256];
    if (ibdg::log2_segments_host(__func__, log2_tab, n_win, p01, p02, p12, starts, n_starts, nullptr, with_post, pos_first, pos_last,
                                 seg, seg_cap, n_seg, summary, msg, sizeof msg))
        return fail(nullptr, "%s", msg);
    return 0;
}

int ibdg_log2_segments_steps_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, int with_post,
                                  const uint64_t *pos_first, const uint64_t *pos_last, ibdg_segment *seg, size_t seg_cap,
                                  uint64_t *n_seg, uint64_t summary[12], const uint32_t *starts, size_t n_starts, const int32_t *shift)
{
    char msg[256];
    if (ibdg::log2_segments_host(__func__, log2_tab, n_win, p01, p02, p12, starts, n_starts, shift, with_post, pos_first, pos_last,
                                 seg, seg_cap, n_seg, summary, msg, sizeof msg))
        return fail(nullptr, "%s", msg);
    return 0;
}

// The window chains of the current site list (LogStates in ibdg_ctx.h has the rule): checked, then kept on the
// host and as a mask on the device for the four kernels.  The upload waits on the host: no call of the group is in flight
// (each ends with quiesce), and the list it copies from may go once this returns.  A refused call changes nothing.
int ibdg_set_window_chains(ibdg_ctx *c, const uint32_t *starts, size_t n_starts)
{
    if (!c) return 1;
    if (!c->sites.sites_valid) return fail(c, "[::] ERROR in ibdg_set_window_chains: no valid site list (call ibdg_upload_sites)");
    ibdg_ctx::LogStates &S = c->ls;
    const size_t n_win = c->sites.n_win;
    std::vector<uint32_t> mask(n_starts ? (n_win + 31) / 32 : 0);
    char msg[256];
    if (ibdg::chain_mask(__func__, starts, n_starts, n_win, mask.data(), msg, sizeof msg))
        return fail(c, "%s", msg);
    if (n_starts) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (quiesce(c) || ensure(c, S.cmask, mask.size() * 4)) return 1;
        HIP_TRY(c, hipMemcpy(S.cmask.p, mask.data(), mask.size() * 4, hipMemcpyHostToDevice));
    }
    S.chains.assign(starts, starts + n_starts);
    ++S.chain_gen;
    S.drop();
    return 0;
}

// The step shifts of the current site list: the chains' rule in every respect -- checked, kept on the host and
// uploaded behind a host wait, the kept products stale; a refused call changes nothing.
int ibdg_set_window_steps(ibdg_ctx *c, const int32_t *shift, size_t n)
{
    if (!c) return 1;
    if (!c->sites.sites_valid) return fail(c, "[::] ERROR in ibdg_set_window_steps: no valid site list (call ibdg_upload_sites)");
    ibdg_ctx::LogStates &S = c->ls;
    const size_t n_win = c->sites.n_win;
    if (n && n != n_win)
        return fail(c, "[::] ERROR in ibdg_set_window_steps: %zu shifts for the %zu windows of the site list (n is that number, or 0 to clear)", n, n_win);
    if (n && !shift) return fail(c, "[::] ERROR in ibdg_set_window_steps: NULL shift with n = %zu", n);
    char msg[256];
    if (ibdg::shift_check(__func__, shift, n, msg, sizeof msg))
        return fail(c, "%s", msg);
    if (n) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (quiesce(c) || ensure(c, S.cshift, n * 4)) return 1;
        HIP_TRY(c, hipMemcpy(S.cshift.p, shift, n * 4, hipMemcpyHostToDevice));
    }
    S.steps.assign(shift, shift + n);
    ++S.chain_gen;
    S.drop();
    return 0;
}

int ibdg_has_window_steps(const ibdg_ctx *c)
{
    return c && c->sites.sites_valid && !c->ls.steps.empty();
}

size_t ibdg_num_window_chains(const ibdg_ctx *c)
{
    return c && c->sites.sites_valid && c->sites.n_win ? c->ls.chains.size() + 1 : 0;
}

// The segments of the paths (k_log2_segments_count): the states stage, with with_post the posteriors stage, the count stage
// -- the first two launch nothing where a states / posteriors call with these penalties went before on this run --, the
// summaries and counts out.  The path and the posteriors stay as they are for ibdg_get_log2_segments (records_made).
int ibdg_window_log2_segments(ibdg_ctx *c, double p01, double p02, double p12, int with_post, const uint64_t *pos_first,
                              const uint64_t *pos_last, uint64_t *n_seg, uint64_t *summary)
{
    if (!c) return 1;
    LogCall L;
    const char *own = !n_seg ? "NULL n_seg" : !summary ? "NULL summary" : pos_first && !pos_last ? "pos_first without pos_last"
                      : pos_last && !pos_first ? "pos_last without pos_first" : nullptr;
    if (log_call_begin(c, __func__, own, "of the path", p01, p02, p12, L)) return 1;
    const size_t T = L.T, n_win = L.n_win;
    for (size_t w = 0; pos_first && w < n_win; ++w)
        if (pos_last[w] < pos_first[w])
            return fail(c, "[::] ERROR in ibdg_window_log2_segments: window %zu ends at %llu, before its start %llu", w,
                        (unsigned long long)pos_last[w], (unsigned long long)pos_first[w]);
    ibdg_ctx::LogStates &S = c->ls;
    S.records_drop();
    S.with_post = with_post != 0;
    S.n_seg.assign(T, 0);
    if (T == 0) return 0;
    memset(n_seg, 0, T * sizeof *n_seg);
    memset(summary, 0, T * 12 * sizeof *summary);
    if (n_win == 0) {
        S.records_made();
        return 0;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if ((pos_first && ensure(c, S.spos, n_win * 16)) || join_streams(c)) return 1;
    const uint64_t *d_first = nullptr, *d_last = nullptr;
    if (pos_first) {
        d_first = (const uint64_t *)S.spos.p, d_last = d_first + n_win;
        HIP_TRY(c, hipMemcpyAsync(S.spos.p, pos_first, n_win * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync((char *)S.spos.p + n_win * 8, pos_last, n_win * 8, hipMemcpyHostToDevice, c->stream));
    }
    if (enqueue_states(c, L, false) || (with_post && enqueue_posteriors(c, L)) || enqueue_segments_count(c, L, d_first, d_last))
        return 1;
    std::vector<uint64_t> o(T * 13);
    HIP_TRY(c, hipMemcpyAsync(o.data(), S.sout.p, T * 104, hipMemcpyDeviceToHost, c->stream));
    if (quiesce(c)) return 1;
    for (size_t t = 0; t < T; ++t) {
        memcpy(summary + 12 * t, &o[13 * t], 96);
        S.n_seg[t] = n_seg[t] = o[13 * t + 12];
        if (n_seg[t] == 0 || n_seg[t] > n_win)          // (what sizes the record buffer: never taken on trust)
            return fail(c, "[::] ERROR in ibdg_window_log2_segments: individual %zu has %llu segments in %zu windows", t,
                        (unsigned long long)n_seg[t], n_win);
    }
    S.records_made();
    return 0;
}

// The records of that call (k_log2_segments_write): the offsets go up, the kernel writes the individuals' records back to
// back into a buffer of their total, one copy out and a host wait.
int ibdg_get_log2_segments(ibdg_ctx *c, ibdg_segment *seg, size_t cap)
{
    if (!c) return 1;
    ibdg_ctx::LogStates &S = c->ls;
    if (!c->have_results || !S.records_fresh())
        return fail(c, "[::] ERROR in ibdg_get_log2_segments: no ibdg_window_log2_segments call since the last ibdg_run");
    const size_t T = S.n_seg.size(), n_win = c->sites.n_win;
    std::vector<uint64_t> off(T ? T : 1);
    uint64_t total = 0;
    for (size_t t = 0; t < T; ++t) {
        off[t] = total;
        total += S.n_seg[t];
    }
    if (cap < total)
        return fail(c, "[::] ERROR in ibdg_get_log2_segments: room for %zu records, %llu are there", cap, (unsigned long long)total);
    if (total == 0) return 0;
    if (!seg) return fail(c, "[::] ERROR in ibdg_get_log2_segments: NULL seg");
    HIP_TRY(c, hipSetDevice(c->device));
    if (ensure(c, S.soff, T * 8) || ensure(c, S.recs, total * sizeof(ibdg_segment)))
        return 1;
    if (join_streams(c)) return 1;
    HIP_TRY(c, hipMemcpyAsync(S.soff.p, off.data(), T * 8, hipMemcpyHostToDevice, c->stream));
    ibdg::launch_log2_segments_write((const double *)c->wlog.win_log2.p, (const uint8_t *)S.path.p,
                                     S.with_post ? (const double *)S.post.p : nullptr, (uint32_t)n_win, (uint32_t)T,
                                     (const uint64_t *)S.soff.p, S.mask(), (ibdg_segment *)S.recs.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(seg, S.recs.p, total * sizeof(ibdg_segment), hipMemcpyDeviceToHost, c->stream));
    return quiesce(c);
}

int ibdg_log2_samples_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                           size_t n_starts, const int32_t *shift, size_t n_samples, uint64_t seed, uint64_t stream,
                           const uint64_t *pos_first, const uint64_t *pos_last, uint8_t *paths, uint64_t *out)
{
    char msg[256];
    if (ibdg::log2_samples_host(__func__, log2_tab, n_win, p01, p02, p12, starts, n_starts, shift, n_samples, seed, stream, pos_first,
                                pos_last, paths, out, msg, sizeof msg))
        return fail(nullptr, "%s", msg);
    return 0;
}

// The draws' scratch bound: the paths, records and summaries of the pairs in flight stay under this many bytes.
// IBDG_SAMPLE_SCRATCH_BYTES is for tests that want more than one chunk on a small shape; ibdg_window_log2_samples alone reads it.
static size_t sample_scratch_bytes()
{
    const char *e = getenv("IBDG_SAMPLE_SCRATCH_BYTES");
    const unsigned long long v = e ? strtoull(e, nullptr, 10) : 0;
    return v ? (size_t)v : (size_t)256 << 20;
}

// the alpha stage, under the stages' rule (enqueue_posteriors)
static int enqueue_alpha(ibdg_ctx *c, const LogCall &L)
{
    ibdg_ctx::LogStates &S = c->ls;
    if (ensure(c, S.alpha, L.T * L.n_win * 24) || ensure(c, S.ptab, 4096))
        return 1;
    if (S.fresh(S.ALPHA, L.P)) return 0;
    HIP_TRY(c, hipMemcpyAsync(S.ptab.p, ibdg::post_tables(), 4096, hipMemcpyHostToDevice, c->stream));
    ibdg::launch_log2_alpha((const double *)c->wlog.win_log2.p, (uint32_t)L.n_win, (uint32_t)L.T, L.P, L.a, (const double *)S.ptab.p,
                            S.mask(), S.shift(), (double *)S.alpha.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    S.made(S.ALPHA, L.P);
    return 0;
}

// the draws of pairs p0 .. p0 + n - 1 (pair p: individual p / K, draw p % K) into `spath` and words 0..2 of `srec`, behind
// enqueue_alpha and the streams' upload
static int enqueue_sample_paths(ibdg_ctx *c, size_t n_win, uint64_t p0, size_t n)
{
    ibdg_ctx::LogStates &S = c->ls;
    ibdg::launch_log2_sample_paths((const double *)S.alpha.p, (uint32_t)n_win, p0, (uint32_t)n, (uint32_t)S.smp.K, S.smp.P, S.smp.a,
                                   (const double *)S.ptab.p, S.mask(), S.shift(), S.smp.seed, (const uint64_t *)S.sstream.p,
                                   (uint8_t *)S.spath.p, (uint64_t *)S.srec.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

// Sampled paths (k_log2_alpha, k_log2_sample_paths, k_log2_segments_count over the drawn paths, k_log2_sample_records): the
// alpha stage, then chunks of pairs under the scratch bound, each chunk's records out behind it.
int ibdg_window_log2_samples(ibdg_ctx *c, double p01, double p02, double p12, size_t n_samples, uint64_t seed, const uint64_t *stream,
                             const uint64_t *pos_first, const uint64_t *pos_last, uint64_t *out)
{
    if (!c) return 1;
    LogCall L;
    const char *own = !out ? "NULL out" : !stream ? "NULL stream" : pos_first && !pos_last ? "pos_first without pos_last"
                      : pos_last && !pos_first ? "pos_last without pos_first" : nullptr;
    if (log_call_begin(c, __func__, own, "of the path", p01, p02, p12, L)) return 1;
    const size_t T = L.T, n_win = L.n_win, K = n_samples;
    if (K < 1 || K > ibdg::SAMPLE_MAX_DRAWS)
        return fail(c, "[::] ERROR in ibdg_window_log2_samples: n_samples = %zu is not in 1 .. %zu", K, ibdg::SAMPLE_MAX_DRAWS);
    for (size_t w = 0; pos_first && w < n_win; ++w)
        if (pos_last[w] < pos_first[w])
            return fail(c, "[::] ERROR in ibdg_window_log2_samples: window %zu ends at %llu, before its start %llu", w,
                        (unsigned long long)pos_last[w], (unsigned long long)pos_first[w]);
    ibdg_ctx::LogStates &S = c->ls;
    S.smp.ok = false;
    if (T == 0) return 0;
    if (n_win == 0) {
        memset(out, 0, T * K * ibdg::SAMPLE_RECORD * sizeof *out);
        return 0;
    }
    const size_t pairs = T * K, per_pair = n_win + 8 * (ibdg::SAMPLE_RECORD + 13);
    size_t chunk = sample_scratch_bytes() / per_pair;
    chunk = chunk < 1 ? 1 : chunk > pairs ? pairs : chunk;
    chunk = chunk > ((size_t)1 << 30) ? (size_t)1 << 30 : chunk;       // (a launch counts its pairs in 32 bits)
    HIP_TRY(c, hipSetDevice(c->device));
    if ((pos_first && ensure(c, S.spos, n_win * 16)) || ensure(c, S.sstream, T * 8) || ensure(c, S.spath, chunk * n_win) ||
        ensure(c, S.srec, chunk * 8 * ibdg::SAMPLE_RECORD) || ensure(c, S.ssum, chunk * 104) || join_streams(c))
        return 1;
    const uint64_t *d_first = nullptr, *d_last = nullptr;
    if (pos_first) {
        d_first = (const uint64_t *)S.spos.p, d_last = d_first + n_win;
        HIP_TRY(c, hipMemcpyAsync(S.spos.p, pos_first, n_win * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync((char *)S.spos.p + n_win * 8, pos_last, n_win * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(S.sstream.p, stream, T * 8, hipMemcpyHostToDevice, c->stream));
    if (enqueue_alpha(c, L)) return 1;
    S.smp.K = K, S.smp.seed = seed;
    S.smp.stream.assign(stream, stream + T);
    for (int i = 0; i < 3; ++i)
        S.smp.P[i] = L.P[i], S.smp.a[i] = L.a[i];
    for (size_t p0 = 0; p0 < pairs; p0 += chunk) {
        const size_t n = pairs - p0 < chunk ? pairs - p0 : chunk;
        if (enqueue_sample_paths(c, n_win, p0, n)) return 1;
        ibdg::launch_log2_segments_count((const uint8_t *)S.spath.p, (uint32_t)n_win, (uint32_t)n, d_first, d_last, S.mask(),
                                         (uint64_t *)S.ssum.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        ibdg::launch_log2_sample_records((const uint64_t *)S.ssum.p, (uint32_t)n, (uint64_t *)S.srec.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(out + p0 * ibdg::SAMPLE_RECORD, S.srec.p, n * 8 * ibdg::SAMPLE_RECORD, hipMemcpyDeviceToHost, c->stream));
    }
    if (quiesce(c)) return 1;
    S.smp.ok = true;
    return 0;
}

// One draw again: the pair's workgroup alone, its path out.  The streams on the device are the call's own still (`sstream` has
// no other writer), alpha is fresh as long as smp.ok stands (drop() clears both).
int ibdg_get_log2_sample_path(ibdg_ctx *c, size_t t, size_t k, uint8_t *path)
{
    if (!c) return 1;
    ibdg_ctx::LogStates &S = c->ls;
    if (!c->have_results || !S.smp.ok || !S.fresh(S.ALPHA, S.smp.P))
        return fail(c, "[::] ERROR in ibdg_get_log2_sample_path: no ibdg_window_log2_samples call since the last ibdg_run or change of chains or steps");
    const size_t T = S.smp.stream.size(), n_win = c->sites.n_win;
    if (t >= T) return fail(c, "[::] ERROR in ibdg_get_log2_sample_path: individual %zu of %zu", t, T);
    if (k >= S.smp.K) return fail(c, "[::] ERROR in ibdg_get_log2_sample_path: draw %zu of %zu", k, S.smp.K);
    if (!path) return fail(c, "[::] ERROR in ibdg_get_log2_sample_path: NULL path");
    HIP_TRY(c, hipSetDevice(c->device));
    if (join_streams(c) || enqueue_sample_paths(c, n_win, (uint64_t)t * S.smp.K + k, 1)) return 1;
    HIP_TRY(c, hipMemcpyAsync(path, S.spath.p, n_win, hipMemcpyDeviceToHost, c->stream));
    return quiesce(c);
}

int ibdg_get_alt_counts(ibdg_ctx *c, size_t first_row, size_t n, uint32_t *out)
{
    if (!c) return 1;
    if (!c->pan.counts_valid) return fail(c, "[::] ERROR in ibdg_get_alt_counts: counts not computed yet");
    if (first_row + n > c->pan.n_rows) return fail(c, "[::] ERROR in ibdg_get_alt_counts: range outside the panel");
    return fetch(c, out, (const char *)c->pan.alt_count.p + first_row * 4, n * 4);
}

int ibdg_run_ms(ibdg_ctx *c, unsigned back, float out[5])
{
    if (!c || !out) return 1;
    if (back + 1 >= (unsigned)ibdg_ctx::Timeline::EV_RING || (long)back >= c->tl.runs_done)
        return fail(c, "[::] ERROR in ibdg_run_ms: no timing kept for the run %u calls back", back);
    const EvSet &E = c->tl.evs[(c->tl.ev_head + ibdg_ctx::Timeline::EV_RING - (int)back) % ibdg_ctx::Timeline::EV_RING];
    if (quiesce(c)) return 1;
    float v, w;
    HIP_TRY(c, hipEventElapsedTime(&v, E.start, E.ld_end));
    out[1] = out[4] = 0.f;
    if (E.rows_on_main) {                        // non-LD: one kernel between the two events of the main stream
        out[0] = out[2] = v;
        out[3] = 0.f;
        return 0;
    }
    HIP_TRY(c, hipEventElapsedTime(&w, E.start, E.s2_end));
    out[0] = v > w ? v : w;                  // the run ends when both streams are done
    out[3] = E.ld ? v : 0.f;
    if (E.recount)
        HIP_TRY(c, hipEventElapsedTime(&out[1], E.s2_start, E.s2_count));
    HIP_TRY(c, hipEventElapsedTime(&v, E.recount ? E.s2_count : E.s2_start, E.s2_end));
    out[2] = v;                              // per-row values and window products are one kernel
    return 0;
}

int ibdg_run_kernel_ms(ibdg_ctx *c, unsigned back, float *ms)
{
    if (!c || !ms) return 1;
    if (back + 1 >= (unsigned)ibdg_ctx::Timeline::EV_RING || (long)back >= c->tl.runs_done)
        return fail(c, "[::] ERROR in ibdg_run_kernel_ms: no timing kept for the run %u calls back", back);
    const EvSet &E = c->tl.evs[(c->tl.ev_head + ibdg_ctx::Timeline::EV_RING - (int)back) % ibdg_ctx::Timeline::EV_RING];
    if (!E.has_kernel_times)
        return fail(c, "[::] ERROR in ibdg_run_kernel_ms: that run did not use the exponent-counting --LD kernel");
    if (quiesce(c)) return 1;
    HIP_TRY(c, hipEventElapsedTime(ms, E.k_start, E.k_stop));
    return 0;
}

int ibdg_last_run_ms(ibdg_ctx *c, float out[5])
{
    if (!c || !out) return 1;
    if (c->tl.runs_done == 0) {
        for (int i = 0; i < 5; ++i) out[i] = 0.f;
        return 0;
    }
    return ibdg_run_ms(c, 0, out);
}

int ibdg_last_ld_variant(const ibdg_ctx *c) { return c ? c->last_variant : 0; }

int ibdg_last_count_unit(const ibdg_ctx *c) { return c ? c->last_count_unit : 0; }
int ibdg_last_window_end(const ibdg_ctx *c) { return c ? c->last_window_end : 0; }

int ibdg_ld_layout(const ibdg_ctx *c)
{
    if (!c || !c->sites.sites_valid || !c->lay.pop_sites_ok)
        return 0;
    return c->lay.compact ? 2 : 1;
}

int ibdg_set_option(ibdg_ctx *c, const char *name, long value)
{
    if (!c || !name) return 1;
    for (const OptionRow &o : OPTION_TABLE) {
        if (strcmp(name, o.name))
            continue;
        const bool in_set = o.kind == OptionRow::SET && value >= 0 && value < 63 && ((o.lo >> value) & 1);
        if ((o.kind == OptionRow::RANGE && (value < o.lo || value > o.hi)) || (o.kind == OptionRow::SET && !in_set)) {
            if (o.text)
                return fail(c, "[::] ERROR in ibdg_set_option: %s must be %s", o.name, o.text);
            return fail(c, "[::] ERROR in ibdg_set_option: %s must be %ld..%ld", o.name, o.lo, o.hi);
        }
        if (o.effect == OptionRow::JOIN_STREAMS && join_streams(c)) return 1;
        if (o.effect == OptionRow::FIX_WPG) c->opt.wpg_fixed = true;
        c->opt.*o.member = o.kind == OptionRow::BOOL ? value != 0 : o.kind == OptionRow::CLAMP ? std::min(std::max(value, o.lo), o.hi) : value;
        return 0;
    }
    return fail(c, "[::] ERROR in ibdg_set_option: unknown option '%s'", name);
}

int ibdg_set_background_order(ibdg_ctx *c, const uint32_t *ids, size_t n)
{
    if (!c) return 1;
    if (n && !ids) return fail(c, "[::] ERROR in ibdg_set_background_order: ids is NULL");
    c->opt.bg_order.assign(ids, ids + n);
    return 0;
}

int ibdg_selftest(const char *what)
{
    if (!what)
        return 1;
    if (!strcmp(what, "wait_info")) {
        // the three ways the bounded poll ends, without a device: the word arrives (from another thread); the producer
        // reports completion / failure without having written it; neither -- the wall-clock bound
        volatile uint32_t flag = 0;
        std::thread setter([&]() {
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
            flag = 7;
        });
        const int arrived = poll_seq(&flag, 7u, 5.0, []() { return 0; });
        setter.join();
        flag = 0;
        const int done = poll_seq(&flag, 9u, 5.0, []() { return 1; });
        const int failed = poll_seq(&flag, 9u, 5.0, []() { return 5; });
        const auto t0 = std::chrono::steady_clock::now();
        const int timed_out = poll_seq(&flag, 9u, 0.05, []() { return 0; });
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return (arrived == 0 && done == 1 && failed == -5 && timed_out == 2 && waited >= 0.05 && waited < 2.0) ? 0 : 2;
    }
    return 1;
}

int ibdg_sync(ibdg_ctx *c)
{
    if (!c) return 1;
    return quiesce(c);
}

}  // extern "C"
