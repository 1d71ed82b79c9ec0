/* A recording stand-in for the engine library (include/ibdgem_hip.h), for the CPU tier: the functions the host program calls,
 * with no device behind them.  Every call on a context appends one line to IBDG_STUB_TRACE/ctx<k>.trace (k: the order of
 * ibdg_create): the function, its scalar arguments, length:FNV-1a-64 of every input array, and the targets of a run.  What
 * comes back means nothing but is a fixed function of (individual, window or site, column), so every individual's files
 * differ and a table that reaches the wrong file shows.  The windows are the engine's (and the host's host_windows()).
 * tests/test_host_conversation.py compares traces and output files with the ones recorded before a change to the host program. */
#include <math.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "../../include/ibdgem_hip.h"

struct ibdg_ctx {
    FILE *tr;
    uint64_t *panel;                     /* a copy, for ibdg_select_variable_sites */
    size_t n_rows, rw;
    unsigned n_ids;
    uint32_t *c_row, *s_cand, *cov_idx;  /* candidates' rows; the list's candidates (selection); its rows with reads */
    uint8_t *c_cov;
    size_t n_cand, n_sites, n_cov, n_win, n_targets;
    unsigned window;
    int selected;
    uint32_t *targets;
};

static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;
static int g_created;

static uint64_t fnv(const void *p, size_t bytes)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; ++i)
        h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
    return h;
}

/* one line: the format's %H takes (pointer, bytes) and prints length:hash, or - for NULL; the rest is printf's */
static void tr(const ibdg_ctx *c, const char *fmt, ...)
{
    char piece[64];
    va_list ap;
    if (!c || !c->tr)
        return;
    va_start(ap, fmt);
    for (const char *f = fmt; *f; ++f) {
        if (*f != '%') { fputc(*f, c->tr); continue; }
        const char k = *++f;
        if (k == 'H') {
            const void *p = va_arg(ap, const void *);
            const size_t bytes = va_arg(ap, size_t);
            if (p) fprintf(c->tr, "%zu:%016llx", bytes, (unsigned long long)fnv(p, bytes)); else fputc('-', c->tr);
        } else if (k == 'z') fprintf(c->tr, "%zu", va_arg(ap, size_t));
        else if (k == 'd') fprintf(c->tr, "%ld", va_arg(ap, long));
        else if (k == 'a') { snprintf(piece, sizeof piece, "%a", va_arg(ap, double)); fputs(piece, c->tr); }
        else if (k == 's') fputs(va_arg(ap, const char *), c->tr);
    }
    va_end(ap);
    fputc('\n', c->tr);
    fflush(c->tr);
}

/* finite, normal, below 1: the value of (individual, index, column) in table `salt` */
static double val(uint32_t id, size_t i, int col, int salt)
{
    const uint64_t h = ((uint64_t)id * 1315423911u) ^ ((uint64_t)i * 2654435761u) ^ ((uint64_t)(col + 3 * salt) * 40503u);
    return ldexp(1.0 + (double)(h % 4096) / 4096.0, -1 - (int)((h >> 12) % 60));
}

int ibdg_device_count(void) { return 1; }
void *ibdg_host_alloc(size_t bytes) { return malloc(bytes); }
void ibdg_host_free(void *p) { free(p); }
const char *ibdg_last_error(const ibdg_ctx *c) { tr(c, "last_error"); return ""; }
int ibdg_pdg_table(double eps, unsigned max_cov, double *out) { return 1; }              /* (a device is always "found") */
double ibdg_pdg_ibd0(double f, double p00, double p01, double p11) { return p00; }
double ibdg_pdg_ibd1(unsigned a0, unsigned a1, double f, double p00, double p01, double p11) { return p01; }
size_t ibdg_row_words(unsigned n_ids) { return 2 * (((size_t)n_ids + 63) / 64); }

void ibdg_pack_alleles(const uint8_t *alleles, unsigned n_ids, uint64_t *row)
{
    memset(row, 0, ibdg_row_words(n_ids) * 8);
    for (unsigned n = 0; n < n_ids; ++n) {
        if (alleles[2 * n] == 1) row[2 * (n >> 6)] |= 1ull << (n & 63);
        if (alleles[2 * n + 1] == 1) row[2 * (n >> 6) + 1] |= 1ull << (n & 63);
    }
}

ibdg_ctx *ibdg_create(int device, double epsilon, unsigned max_cov)
{
    ibdg_ctx *c = calloc(1, sizeof *c);
    const char *dir = getenv("IBDG_STUB_TRACE");
    char fn[4096];
    if (!c)
        return NULL;
    pthread_mutex_lock(&g_mu);
    const int k = g_created++;
    pthread_mutex_unlock(&g_mu);
    if (dir && snprintf(fn, sizeof fn, "%s/ctx%d.trace", dir, k) < (int)sizeof fn)
        c->tr = fopen(fn, "w");
    tr(c, "create device=%d eps=%a max_cov=%d", (long)device, epsilon, (long)max_cov);
    return c;
}

void ibdg_destroy(ibdg_ctx *c)
{
    if (!c)
        return;
    tr(c, "destroy");
    if (c->tr)
        fclose(c->tr);
    free(c->panel); free(c->c_row); free(c->c_cov); free(c->s_cand); free(c->cov_idx); free(c->targets);
    free(c);
}

int ibdg_set_option(ibdg_ctx *c, const char *name, long value) { tr(c, "set_option %s=%d", name, value); return 0; }
int ibdg_sync(ibdg_ctx *c) { tr(c, "sync"); return 0; }
size_t ibdg_num_sites(const ibdg_ctx *c) { tr(c, "num_sites"); return c->n_sites; }
size_t ibdg_num_windows(const ibdg_ctx *c) { tr(c, "num_windows"); return c->n_win; }
size_t ibdg_num_targets(const ibdg_ctx *c) { tr(c, "num_targets"); return c->n_targets; }

int ibdg_set_background_order(ibdg_ctx *c, const uint32_t *ids, size_t n) { tr(c, "set_background_order ids=%H", ids, n * 4); return 0; }

static int panel_keep(ibdg_ctx *c, size_t n_rows, unsigned n_ids)
{
    free(c->panel);
    c->n_rows = n_rows; c->n_ids = n_ids; c->rw = ibdg_row_words(n_ids);
    c->panel = malloc(n_rows * c->rw * 8 + 8);
    return !c->panel;
}

int ibdg_upload_panel(ibdg_ctx *c, const uint64_t *rows, size_t n_rows, unsigned n_ids)
{
    if (panel_keep(c, n_rows, n_ids))
        return 1;
    memcpy(c->panel, rows, n_rows * c->rw * 8);
    tr(c, "upload_panel n_ids=%d rows=%H", (long)n_ids, c->panel, n_rows * c->rw * 8);
    return 0;
}

int ibdg_upload_panel_fd(ibdg_ctx *c, int fd, uint64_t offset, size_t n_rows, unsigned n_ids)
{
    tr(c, "upload_panel_fd n_ids=%d n_rows=%z", (long)n_ids, n_rows);
    return panel_keep(c, n_rows, n_ids) || pread(fd, c->panel, n_rows * c->rw * 8, (off_t)offset) != (ssize_t)(n_rows * c->rw * 8);
}

/* the list's windows: runs of `window` rows with reads (cov[i] != 0), the last one shorter */
static int sites_keep(ibdg_ctx *c, const uint8_t *nr, const uint8_t *na, const uint32_t *pick, size_t n, unsigned window)
{
    free(c->cov_idx);
    c->cov_idx = malloc((n + 1) * 4);
    if (!c->cov_idx || window == 0)
        return 1;
    c->n_cov = 0;
    for (size_t i = 0; i < n; ++i)
        if (pick ? c->c_cov[pick[i]] : (nr[i] + na[i]) > 0)
            c->cov_idx[c->n_cov++] = (uint32_t)i;
    c->n_sites = n; c->window = window; c->n_win = (c->n_cov + window - 1) / window;
    c->n_targets = 0;
    return 0;
}

int ibdg_upload_sites(ibdg_ctx *c, const uint32_t *row, const uint8_t *nr, const uint8_t *na, const double *fo, size_t n, unsigned window)
{
    tr(c, "upload_sites n=%z window=%d row=%H nr=%H na=%H fo=%H", n, (long)window, row, n * 4, nr, n, na, n, fo, n * 8);
    c->selected = 0;
    return sites_keep(c, nr, na, NULL, n, window);
}

int ibdg_upload_candidates(ibdg_ctx *c, const uint32_t *row, const uint8_t *nr, const uint8_t *na, const double *fo, size_t n)
{
    tr(c, "upload_candidates n=%z row=%H nr=%H na=%H fo=%H", n, row, n * 4, nr, n, na, n, fo, n * 8);
    free(c->c_row); free(c->c_cov); free(c->s_cand);
    c->c_row = malloc((n + 1) * 4); c->c_cov = malloc(n + 1); c->s_cand = malloc((n + 1) * 4);
    if (!c->c_row || !c->c_cov || !c->s_cand)
        return 1;
    for (size_t i = 0; i < n; ++i) {
        c->c_row[i] = row[i];
        c->c_cov[i] = (nr[i] + na[i]) > 0;
    }
    c->n_cand = n;
    return 0;
}

int ibdg_select_variable_sites(ibdg_ctx *c, uint32_t target, unsigned window)
{
    size_t n = 0;
    tr(c, "select_variable_sites target=%d window=%d", (long)target, (long)window);
    if (!c->panel || !c->s_cand || target >= c->n_ids)
        return 1;
    for (size_t i = 0; i < c->n_cand; ++i) {
        if (c->c_row[i] >= c->n_rows)
            return 1;
        const uint64_t *r = c->panel + c->c_row[i] * c->rw + 2 * (target >> 6);
        if (((r[0] | r[1]) >> (target & 63)) & 1)
            c->s_cand[n++] = (uint32_t)i;
    }
    c->selected = 1;
    return sites_keep(c, NULL, NULL, c->s_cand, n, window);
}

int ibdg_get_site_candidates(ibdg_ctx *c, uint32_t *out)
{
    tr(c, "get_site_candidates");
    if (c->selected)
        memcpy(out, c->s_cand, c->n_sites * 4);
    return !c->selected;
}

int ibdg_get_windows(ibdg_ctx *c, uint32_t *first, uint32_t *last, uint32_t *ncov)
{
    tr(c, "get_windows");
    for (size_t w = 0; w < c->n_win; ++w) {
        const size_t a = w * c->window, b = (w + 1) * c->window < c->n_cov ? (w + 1) * c->window : c->n_cov;
        if (first) first[w] = c->cov_idx[a];
        if (last) last[w] = c->cov_idx[b - 1];
        if (ncov) ncov[w] = (uint32_t)(b - a);
    }
    return 0;
}

int ibdg_run(ibdg_ctx *c, const uint32_t *targets, size_t T, const uint8_t *bg, int pu_id, int ld)
{
    if (c->tr) {
        fprintf(c->tr, "run targets=");
        for (size_t t = 0; t < T; ++t)
            fprintf(c->tr, "%s%u", t ? "," : "", targets[t]);
        fputc(' ', c->tr);
    }
    tr(c, "bg=%H pu_id=%d ld=%d", bg, (size_t)c->n_ids, (long)pu_id, (long)ld);
    free(c->targets);
    c->targets = malloc((T + 1) * 4);
    if (!c->targets)
        return 1;
    memcpy(c->targets, targets, T * 4);
    c->n_targets = T;
    return 0;
}

static int table(ibdg_ctx *c, const char *what, size_t t0, size_t t1, size_t n, int salt, double *out)
{
    if (t1 == t0 + 1) tr(c, "%s t=%z", what, t0); else tr(c, "%s", what);
    if (t1 > c->n_targets)
        return 1;
    for (size_t t = t0; t < t1; ++t)
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) {
                const double v = val(c->targets[t], i, k, salt);
                *out++ = salt == 1 ? -1000.0 * v - (double)k : v;          /* (1: a log2 table) */
            }
    return 0;
}

int ibdg_get_site_ll(ibdg_ctx *c, size_t t, double *out) { return table(c, "get_site_ll", t, t + 1, c->n_sites, 2, out); }
int ibdg_get_window_ll(ibdg_ctx *c, size_t t, double *out) { return table(c, "get_window_ll", t, t + 1, c->n_win, 0, out); }
int ibdg_get_window_ll_all(ibdg_ctx *c, double *out) { return table(c, "get_window_ll_all", 0, c->n_targets, c->n_win, 0, out); }
int ibdg_get_window_log2(ibdg_ctx *c, size_t t, double *out) { return table(c, "get_window_log2", t, t + 1, c->n_win, 1, out); }
int ibdg_get_window_log2_all(ibdg_ctx *c, double *out) { return table(c, "get_window_log2_all", 0, c->n_targets, c->n_win, 1, out); }
/* (the host program never sets a table; the stand-in's tables are functions of the individuals and stay so) */
int ibdg_set_window_log2(ibdg_ctx *c, const double *tab, size_t n_targets)
{
    tr(c, "set_window_log2 n_targets=%z", n_targets);
    return !tab || n_targets != c->n_targets;
}

static int llr_sums(ibdg_ctx *c, const char *what, const uint32_t *first, const uint32_t *end, size_t n_seg, double *out)
{
    tr(c, "%s n_seg=%z first=%H end=%H", what, n_seg, first, n_seg * 4, end, n_seg * 4);
    for (size_t t = 0; t < c->n_targets; ++t)
        for (size_t s = 0; s < n_seg; ++s)
            for (int k = 0; k < 4; ++k) {
                const double len = (double)(end[s] - first[s]);
                *out++ = k & 1 ? ldexp(len, -60) : len * (val(c->targets[t], first[s], k, 3) - 0.25);
            }
    return 0;
}

int ibdg_window_llr_sums(ibdg_ctx *c, const uint32_t *first, const uint32_t *end, size_t n_seg, double *out)
{ return llr_sums(c, "window_llr_sums", first, end, n_seg, out); }
int ibdg_window_log2_llr_sums(ibdg_ctx *c, const uint32_t *first, const uint32_t *end, size_t n_seg, double *out)
{ return llr_sums(c, "window_log2_llr_sums", first, end, n_seg, out); }

/* the host twins: the path of a table is ((w / 3 + its hash) % 3), everything else follows from it by fixed rules */
static unsigned path_of(const double *tab, size_t n, size_t w) { return (unsigned)((w / 3 + fnv(tab, n * 24) % 3) % 3); }

int ibdg_log2_states_host(const double *tab, size_t n, double p01, double p02, double p12, uint8_t *path, int64_t *score, uint64_t count[3])
{
    count[0] = count[1] = count[2] = 0;
    for (size_t w = 0; w < n; ++w) {
        const unsigned s = path_of(tab, n, w);
        count[s]++;
        if (path) path[w] = (uint8_t)s;
        for (int k = 0; score && k < 3; ++k)
            score[3 * w + k] = -(int64_t)(16384 * (w + 1) + 4096 * ((s + k) % 3));
    }
    return 0;
}

int ibdg_log2_posteriors_host(const double *tab, size_t n, double p01, double p02, double p12, double *post, double expect[3], double *log2_z)
{
    static const double g[3] = {0.625, 0.25, 0.125};
    expect[0] = expect[1] = expect[2] = 0.0;
    for (size_t w = 0; w < n; ++w)
        for (unsigned k = 0; k < 3; ++k) {
            const double v = g[(k + 3 - path_of(tab, n, w)) % 3];
            expect[k] += v;
            if (post) post[3 * w + k] = v;
        }
    *log2_z = -(double)n * 1.5 - (double)(fnv(tab, n * 24) % 1024) / 1024.0;
    return 0;
}

int ibdg_log2_segments_host(const double *tab, size_t n, double p01, double p02, double p12, int with_post, const uint64_t *pf,
                            const uint64_t *pl, ibdg_segment *seg, size_t cap, uint64_t *n_seg, uint64_t sum[12])
{
    memset(sum, 0, 12 * sizeof *sum);
    *n_seg = 0;
    for (size_t a = 0, b; a < n; a = b) {
        const unsigned s = path_of(tab, n, a);
        for (b = a + 1; b < n && path_of(tab, n, b) == s; ++b)
            ;
        const uint64_t bp = pf ? pl[b - 1] - pf[a] + 1 : 0;
        sum[s]++; sum[6 + s] += bp;
        if (b - a > sum[3 + s]) sum[3 + s] = b - a;
        if (bp > sum[9 + s]) sum[9 + s] = bp;
        if (seg && *n_seg < cap) {
            ibdg_segment *g = &seg[*n_seg];
            memset(g, 0, sizeof *g);
            g->first = (uint32_t)a; g->n_win = (uint32_t)(b - a); g->state = s;
            for (unsigned k = 0; k < 3; ++k)
                g->e[k] = -(int64_t)((b - a) * 65536 * (1 + (k + 3 - s) % 3));
            g->post_q = with_post ? (uint64_t)(b - a) << 31 : 0;
            g->post_min = with_post ? 0.375 : 0.0;
        }
        ++*n_seg;
    }
    return 0;
}

/* ... and the device's calls: per individual of the last run, a fixed split of the windows and numbers made from its id */
int ibdg_window_log2_states(ibdg_ctx *c, double p01, double p02, double p12, uint8_t *path, int64_t *score, uint64_t *count)
{
    tr(c, "window_log2_states p01=%a p02=%a p12=%a path=%d score=%d", p01, p02, p12, (long)(path != NULL), (long)(score != NULL));
    for (size_t t = 0; t < c->n_targets; ++t) {
        const uint64_t n = c->n_win, c0 = (c->targets[t] * 7u) % (n + 1), c1 = (n - c0) / 2;
        count[3 * t] = c0; count[3 * t + 1] = c1; count[3 * t + 2] = n - c0 - c1;
        if (path) memset(path + t * n, 0, n);
        if (score) memset(score + 3 * t * n, 0, 3 * n * sizeof *score);
    }
    return 0;
}

int ibdg_window_log2_posteriors(ibdg_ctx *c, double p01, double p02, double p12, double *post, double *expect, double *log2_z)
{
    tr(c, "window_log2_posteriors p01=%a p02=%a p12=%a post=%d", p01, p02, p12, (long)(post != NULL));
    for (size_t t = 0; t < c->n_targets; ++t) {
        for (int k = 0; k < 3; ++k)
            expect[3 * t + k] = (double)c->n_win * val(c->targets[t], 0, k, 4);
        log2_z[t] = -1000.0 * val(c->targets[t], 1, 0, 4);
        if (post) memset(post + 3 * t * c->n_win, 0, 24 * c->n_win);
    }
    return 0;
}

int ibdg_window_log2_segments(ibdg_ctx *c, double p01, double p02, double p12, int with_post, const uint64_t *pf, const uint64_t *pl,
                              uint64_t *n_seg, uint64_t *sum)
{
    tr(c, "window_log2_segments p01=%a p02=%a p12=%a with_post=%d pos_first=%H pos_last=%H", p01, p02, p12, (long)with_post, pf,
       c->n_win * 8, pl, c->n_win * 8);
    for (size_t t = 0; t < c->n_targets; ++t) {
        n_seg[t] = 1 + c->targets[t] % 5;
        for (uint32_t k = 0; k < 12; ++k)
            sum[12 * t + k] = (c->targets[t] + 1) * (k + 1) + (pf && c->n_win ? pl[c->n_win - 1] - pf[0] : 0);
    }
    return 0;
}
