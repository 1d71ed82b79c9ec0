// ibdg_states_host.cpp -- the host twin of the log-domain IBD-state path, posteriors, segments, sampled paths and switches: the serial caller of the steps
// that ibdg_states.h defines (the kernels of ibdg_states.hip are the parallel one), one window after the other.  Host only;
// built with -ffp-contract=off like the rest.
#include "ibdg_states.h"

#include <cmath>
#include <cstdio>
#include <vector>

namespace ibdg {

int states_penalties(double p01, double p02, double p12, int64_t P[3], int *bad)
{
    const double p[3] = {p01, p02, p12};
    for (int k = 0; k < 3; ++k) {
        if (!(p[k] > 0.0 && p[k] <= 1.0)) {         // (NaN fails both)
            if (bad) *bad = k;
            return 1;
        }
        const double q = std::log2(p[k]) * STATES_QUANTA;
        P[k] = q < (double)STATES_PEN_MIN ? STATES_PEN_MIN : (int64_t)std::llrint(q);
    }
    return 0;
}

// What the three twins check alike, with the text each had.  own: the caller's complaint about its own pointers, or NULL;
// max_tail: how its refusal of too many windows ends.  P: the penalties in quanta.
static int check_log_args(const char *fn, const char *own, const double *tab, size_t n_win, double p01, double p02, double p12,
                          const char *max_tail, int64_t P[3], char *err, size_t err_len)
{
    static const char *const name[3] = {"p01", "p02", "p12"};
    int bad = 0;
    if (own)
        snprintf(err, err_len, "[::] ERROR in %s: NULL %s", fn, own);
    else if (n_win && !tab)
        snprintf(err, err_len, "[::] ERROR in %s: NULL table", fn);
    else if (states_penalties(p01, p02, p12, P, &bad))
        snprintf(err, err_len, "[::] ERROR in %s: %s = %g is not in (0, 1]", fn, name[bad], bad == 0 ? p01 : bad == 1 ? p02 : p12);
    else if (n_win > STATES_MAX_WIN)
        snprintf(err, err_len, "[::] ERROR in %s: %zu windows, more than the %zu (2^21) %s", fn, n_win, STATES_MAX_WIN, max_tail);
    else
        return 0;
    return 1;
}

int chain_mask(const char *fn, const uint32_t *starts, size_t n_starts, size_t n_win, uint32_t *mask, char *err, size_t err_len)
{
    if (n_starts && !starts) {
        snprintf(err, err_len, "[::] ERROR in %s: NULL starts with n_starts = %zu", fn, n_starts);
        return 1;
    }
    for (size_t i = 0; i < n_starts; ++i) {
        if (starts[i] == 0)
            snprintf(err, err_len, "[::] ERROR in %s: starts[%zu] = 0 (window 0 always starts a chain; the entries are 1 .. n_win - 1)", fn, i);
        else if (starts[i] >= n_win)
            snprintf(err, err_len, "[::] ERROR in %s: starts[%zu] = %u is not below the %zu windows", fn, i, starts[i], n_win);
        else if (i && starts[i] <= starts[i - 1])
            snprintf(err, err_len, "[::] ERROR in %s: starts[%zu] = %u does not lie above starts[%zu] = %u (strictly increasing)", fn, i,
                     starts[i], i - 1, starts[i - 1]);
        else
            continue;
        return 1;
    }
    for (size_t i = 0; n_starts && i < (n_win + 31) / 32; ++i)
        mask[i] = 0;
    for (size_t i = 0; i < n_starts; ++i)
        mask[starts[i] >> 5] |= 1u << (starts[i] & 31);
    return 0;
}

int shift_check(const char *fn, const int32_t *shift, size_t n_win, char *err, size_t err_len)
{
    for (size_t w = 1; shift && w < n_win; ++w)
        if (shift[w] > STATES_SHIFT_MAX || shift[w] < -STATES_SHIFT_MAX) {
            snprintf(err, err_len, "[::] ERROR in %s: shift[%zu] = %d is not within +-2^30", fn, w, shift[w]);
            return 1;
        }
    return 0;
}

// chain_mask into a vector of the twins' own; *mask: its words, or NULL for no starts
static int own_mask(const char *fn, const uint32_t *starts, size_t n_starts, size_t n_win, std::vector<uint32_t> &own,
                    const uint32_t **mask, char *err, size_t err_len)
{
    own.resize(n_starts ? (n_win + 31) / 32 : 0);
    *mask = n_starts ? own.data() : nullptr;
    return chain_mask(fn, starts, n_starts, n_win, own.data(), err, err_len);
}

// The cores take checked arguments and check nothing.  mask: the chain starts' bits (chain_start), or NULL; shift: the step
// shifts [n_win], or NULL.
// The states recurrence: path [n_win] or NULL, score [n_win][3] or NULL, count[3]
static void states_core(const double *tab, size_t n_win, const int64_t P[3], const uint32_t *mask, const int32_t *shift, uint8_t *path,
                        int64_t *score, uint64_t count[3])
{
    count[0] = count[1] = count[2] = 0;
    if (n_win == 0)
        return;
    std::vector<uint8_t> from(n_win);            // from[i][s] in bits 2 s, 2 s + 1
    int64_t v[3], e[3];
    states_emission(tab, v);
    from[0] = (uint8_t)MAP_ID;
    if (score)
        score[0] = v[0], score[1] = v[1], score[2] = v[2];
    for (size_t i = 1; i < n_win; ++i) {
        states_emission(tab + 3 * i, e);
        from[i] = (uint8_t)states_shift_step(v, P, e, chain_start(mask, (uint32_t)i), shift != nullptr, step_shift(shift, (uint32_t)i));
        if (score)
            score[3 * i] = v[0], score[3 * i + 1] = v[1], score[3 * i + 2] = v[2];
    }
    unsigned st = (unsigned)argmax3(v);
    for (size_t i = n_win; i-- > 0;) {
        ++count[st];
        if (path)
            path[i] = (uint8_t)st;
        st = map_at(from[i], st);
    }
}

// err: room for a message
int log2_states_host(const char *fn, const double *tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                     size_t n_starts, const int32_t *shift, uint8_t *path, int64_t *score, uint64_t count[3], char *err, size_t err_len)
{
    int64_t P[3];
    std::vector<uint32_t> own;
    const uint32_t *mask;
    if (check_log_args(fn, count ? nullptr : "count", tab, n_win, p01, p02, p12, "the integer scores allow", P, err, err_len) ||
        own_mask(fn, starts, n_starts, n_win, own, &mask, err, err_len) || shift_check(fn, shift, n_win, err, err_len))
        return 1;
    states_core(tab, n_win, P, mask, shift, path, score, count);
    return 0;
}

const double *post_tables()
{
    static const struct Tab {
        double v[512];
        Tab()
        {
            for (int j = 0; j < 256; ++j) {
                v[j] = std::exp2(j / 256.0);
                v[256 + j] = std::exp2(j / 65536.0);
            }
        }
    } tab;
    return tab.v;
}

void post_penalty_weights(const int64_t P[3], double a[3])
{
    const double *T = post_tables();
    for (int k = 0; k < 3; ++k)
        a[k] = std::ldexp(T[P[k] >> 8 & 255] * T[256 + (P[k] & 255)], (int)(P[k] >> 16));
}

// The sum-product pass: steps 1 .. 4 are the functions of ibdg_states.h that the kernel's threads call, here in loops over b; step
// 5 is the same tree, serial.  post [n_win][3] or NULL.
static void posteriors_core(const double *tab, size_t n_win, const int64_t P[3], const uint32_t *mask, const int32_t *shift, double *post,
                            double expect[3], double *z_mant, int *z_exp)
{
    expect[0] = expect[1] = expect[2] = 0.0;
    *z_mant = 1.0, *z_exp = 0;
    if (n_win == 0)
        return;
    PostIn in = {tab, post_tables(), {}, mask, shift, {P[0], P[1], P[2]}};
    post_penalty_weights(P, in.a);
    std::vector<double> own;
    if (!post) {
        own.resize(n_win * 3);
        post = own.data();
    }
    const Blocks B((uint32_t)n_win);
    std::vector<double> mat(B.nbk * 9), fin(B.nbk * 3), gout(B.nbk * 3);
    std::vector<int> mexp(B.nbk), fexp(B.nbk);
    // 1
    for (uint32_t b = 0; b < B.nbk; ++b)
        post_block_matrix(in, B.begin(b), B.end(b), &mat[9 * b], &mexp[b]);
    // 2
    post_forward_walk(mat.data(), mexp.data(), B.nbk, fin.data(), fexp.data());
    post_backward_walk(mat.data(), B.nbk, gout.data());
    // 3, 4 (the last block's D and exponent are Z's)
    double part[STATES_BLOCKS][3] = {};
    for (uint32_t b = 0; b < B.nbk; ++b)
        post_block_gamma(in, B.begin(b), B.end(b), &gout[3 * b], &fin[3 * b], fexp[b], post, part[b], z_mant, z_exp);
    // 5
    for (int d = STATES_BLOCKS / 2; d > 0; d >>= 1)
        for (int b = 0; b < d; ++b)
            for (int s = 0; s < 3; ++s)
                part[b][s] = part[b][s] + part[b + d][s];
    expect[0] = part[0][0], expect[1] = part[0][1], expect[2] = part[0][2];
}

int log2_posteriors_host(const char *fn, const double *tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                         size_t n_starts, const int32_t *shift, double *post, double expect[3], double *z_mant, int *z_exp, char *err,
                         size_t err_len)
{
    int64_t P[3];
    std::vector<uint32_t> own;
    const uint32_t *mask;
    if (check_log_args(fn, !expect ? "expect" : !z_mant || !z_exp ? "log2_z" : nullptr, tab, n_win, p01, p02, p12, "of the path", P,
                       err, err_len) ||
        own_mask(fn, starts, n_starts, n_win, own, &mask, err, err_len) || shift_check(fn, shift, n_win, err, err_len))
        return 1;
    posteriors_core(tab, n_win, P, mask, shift, post, expect, z_mant, z_exp);
    return 0;
}

void switch_counted_steps(size_t n_win, const int64_t P[3], const uint32_t *mask, const int32_t *shift, uint64_t counted[3])
{
    const PostIn in = {nullptr, nullptr, {}, mask, shift, {P[0], P[1], P[2]}};
    counted[0] = counted[1] = counted[2] = 0;
    for (size_t w = 1; w < n_win; ++w)
        for (int k = 0; k < 3; ++k)
            counted[k] += switch_counted(in, (uint32_t)w, k);
}

// The switches' pass: steps 1 and 2 as posteriors_core, then post_block_switches in a loop over b and step 5's
// tree.  tab may be NULL (post_emission_weights); sw [n_win][3] or NULL.
static void switches_core(const double *tab, size_t n_win, const int64_t P[3], const uint32_t *mask, const int32_t *shift, double *sw,
                          double expect[3])
{
    expect[0] = expect[1] = expect[2] = 0.0;
    if (n_win == 0)
        return;
    PostIn in = {tab, post_tables(), {}, mask, shift, {P[0], P[1], P[2]}};
    post_penalty_weights(P, in.a);
    std::vector<double> own;
    if (!sw) {
        own.resize(n_win * 3);
        sw = own.data();
    }
    const Blocks B((uint32_t)n_win);
    std::vector<double> mat(B.nbk * 9), fin(B.nbk * 3), gout(B.nbk * 3);
    std::vector<int> mexp(B.nbk), fexp(B.nbk);
    for (uint32_t b = 0; b < B.nbk; ++b)
        post_block_matrix(in, B.begin(b), B.end(b), &mat[9 * b], &mexp[b]);
    post_forward_walk(mat.data(), mexp.data(), B.nbk, fin.data(), fexp.data());
    post_backward_walk(mat.data(), B.nbk, gout.data());
    double part[STATES_BLOCKS][3] = {};
    for (uint32_t b = 0; b < B.nbk; ++b)
        post_block_switches<true>(in, B.begin(b), B.end(b), &gout[3 * b], &fin[3 * b], fexp[b], sw, part[b]);
    for (int d = STATES_BLOCKS / 2; d > 0; d >>= 1)
        for (int b = 0; b < d; ++b)
            for (int s = 0; s < 3; ++s)
                part[b][s] = part[b][s] + part[b + d][s];
    expect[0] = part[0][0], expect[1] = part[0][1], expect[2] = part[0][2];
}

int log2_switches_host(const char *fn, const double *tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                       size_t n_starts, const int32_t *shift, double *sw, double expect[3], uint64_t counted[3], char *err,
                       size_t err_len)
{
    int64_t P[3];
    std::vector<uint32_t> own;
    const uint32_t *mask;
    static const double none[3] = {0.0, 0.0, 0.0};       // (a NULL table is an input here: check_log_args sees a table)
    if (check_log_args(fn, !expect ? "expect" : !counted ? "counted" : nullptr, tab ? tab : none, n_win, p01, p02, p12, "of the path", P,
                       err, err_len) ||
        own_mask(fn, starts, n_starts, n_win, own, &mask, err, err_len) || shift_check(fn, shift, n_win, err, err_len))
        return 1;
    switches_core(tab, n_win, P, mask, shift, sw, expect);
    switch_counted_steps(n_win, P, mask, shift, counted);
    return 0;
}

void switch_penalty_update(const double p[3], const double total[3], size_t T, const double prior[3], double next[3])
{
    for (int k = 0; k < 3; ++k) {
        const bool ok = std::isfinite(total[k]) && std::isfinite(prior[k]) && total[k] > 0.0 && prior[k] > 0.0;
        double x = p[k];
        if (ok) {
            x = p[k] * total[k] / ((double)T * prior[k]);
            x = x < 1e-300 ? 1e-300 : x;
            x = x > 1.0 ? 1.0 : x;
        }
        next[k] = x;
    }
}

int switch_fit_step(const double p[3], const double total[3], size_t T, const double prior[3], const uint64_t counted[3],
                    ibdg_fit_row *row, double next[3], int *stood)
{
    int64_t Pp[3], Pn[3];
    int bad = 0;
    if (states_penalties(p[0], p[1], p[2], Pp, &bad))
        return 1 + bad;
    for (int k = 0; k < 3; ++k)
        row->p[k] = p[k], row->total[k] = total[k], row->prior[k] = prior[k], row->counted[k] = counted[k];
    switch_penalty_update(p, total, T, prior, next);
    (void)states_penalties(next[0], next[1], next[2], Pn, nullptr);      // (the update keeps next in [1e-300, 1])
    *stood = 1;
    for (int k = 0; k < 3; ++k)
        if (Pn[k] - Pp[k] > 1 || Pp[k] - Pn[k] > 1)
            *stood = 0;
    return 0;
}

// The fit's loop over the cores: the arguments are checked once, the mask is made once, and every iteration is switches_core on
// every table in order, on the NULL table for the prior, switch_counted_steps and switch_fit_step.
int log2_fit_host(const char *fn, const double *const *tabs, size_t T, size_t n_win, const double p[3], const uint32_t *starts,
                  size_t n_starts, const int32_t *shift, size_t max_iter, ibdg_fit_row *rows, size_t *n_rows, int *stood,
                  double fitted[3], char *err, size_t err_len)
{
    int64_t P[3];
    std::vector<uint32_t> own;
    const uint32_t *mask;
    static const double none[3] = {0.0, 0.0, 0.0};
    const char *null_arg = !p ? "p" : !n_rows ? "n_rows" : !stood ? "stood" : !fitted ? "fitted" : max_iter && !rows ? "rows" :
                           T && !tabs ? "tabs" : nullptr;
    if (check_log_args(fn, null_arg, none, n_win, p ? p[0] : 1.0, p ? p[1] : 1.0, p ? p[2] : 1.0, "of the path", P, err, err_len) ||
        own_mask(fn, starts, n_starts, n_win, own, &mask, err, err_len) || shift_check(fn, shift, n_win, err, err_len))
        return 1;
    for (size_t t = 0; t < T && n_win; ++t)
        if (!tabs[t]) {
            snprintf(err, err_len, "[::] ERROR in %s: NULL table of individual %zu", fn, t);
            return 1;
        }
    double cur[3] = {p[0], p[1], p[2]};
    *n_rows = 0, *stood = 0;
    fitted[0] = cur[0], fitted[1] = cur[1], fitted[2] = cur[2];
    if (T == 0)
        return 0;
    for (size_t it = 0; it < max_iter && !*stood; ++it) {
        double total[3] = {0.0, 0.0, 0.0}, expect[3], prior[3], next[3];
        uint64_t counted[3];
        (void)states_penalties(cur[0], cur[1], cur[2], P, nullptr);     // (checked: p above, then the update's range)
        for (size_t t = 0; t < T; ++t) {
            switches_core(tabs[t], n_win, P, mask, shift, nullptr, expect);
            for (int k = 0; k < 3; ++k)
                total[k] = total[k] + expect[k];
        }
        switches_core(nullptr, n_win, P, mask, shift, nullptr, prior);
        switch_counted_steps(n_win, P, mask, shift, counted);
        (void)switch_fit_step(cur, total, T, prior, counted, &rows[it], next, stood);
        *n_rows = it + 1;
        for (int k = 0; k < 3; ++k)
            cur[k] = fitted[k] = next[k];
    }
    return 0;
}

// The segment walk: one pass over the path in window order with the kernels' accumulator and summary functions (ibdg_states.h:
// every quantity is exact and associative, so this is the kernels' result whatever their blocks).  post: the gammas [n_win][3],
// or NULL for no support.
static void segments_core(const double *tab, size_t n_win, const uint8_t *path, const uint32_t *mask, const double *post,
                          const uint64_t *pos_first, const uint64_t *pos_last, ibdg_segment *seg, size_t seg_cap, uint64_t *n_seg, uint64_t summary[12])
{
    *n_seg = 0;
    for (int i = 0; i < 12; ++i)
        summary[i] = 0;
    for (size_t f = 0; f < n_win;) {
        const unsigned s = path[f];
        SegAcc a;
        seg_reset(a);
        size_t w = f;
        for (; w < n_win && (w == f || !seg_start(mask, (uint32_t)w, s, path[w])); ++w)
            seg_add_window(a, tab + 3 * w, post ? post + 3 * w : nullptr, s);
        if (seg && *n_seg < seg_cap)
            seg_record(seg + *n_seg, (uint32_t)f, (uint32_t)(w - f), s, a, post != nullptr);
        ++*n_seg;
        seg_summary_add(summary, s, w - f, pos_first ? pos_last[w - 1] - pos_first[f] + 1 : 0);
        f = w;
    }
}

// (the table and the penalties are refused in the words of ibdg_log2_states_host, whose checks they are)
int log2_segments_host(const char *fn, const double *tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                       size_t n_starts, const int32_t *shift, int with_post, const uint64_t *pos_first, const uint64_t *pos_last, ibdg_segment *seg,
                       size_t seg_cap, uint64_t *n_seg, uint64_t summary[12], char *err, size_t err_len)
{
    int64_t P[3];
    std::vector<uint32_t> own;
    const uint32_t *mask;
    if (!n_seg || !summary) {
        snprintf(err, err_len, "[::] ERROR in %s: NULL %s", fn, n_seg ? "summary" : "n_seg");
        return 1;
    }
    if (!pos_first != !pos_last) {
        snprintf(err, err_len, "[::] ERROR in %s: %s without %s", fn, pos_first ? "pos_first" : "pos_last",
                 pos_first ? "pos_last" : "pos_first");
        return 1;
    }
    if (check_log_args("ibdg_log2_states_host", nullptr, tab, n_win, p01, p02, p12, "the integer scores allow", P, err, err_len))
        return 1;
    for (size_t w = 0; pos_first && w < n_win; ++w)
        if (pos_last[w] < pos_first[w]) {
            snprintf(err, err_len, "[::] ERROR in %s: window %zu ends at %llu, before its start %llu", fn, w,
                     (unsigned long long)pos_last[w], (unsigned long long)pos_first[w]);
            return 1;
        }
    if (own_mask(fn, starts, n_starts, n_win, own, &mask, err, err_len) || shift_check(fn, shift, n_win, err, err_len))
        return 1;
    std::vector<uint8_t> path(n_win);
    std::vector<double> post(with_post ? n_win * 3 : 0);
    uint64_t count[3];
    double expect[3], zm;
    int ze;
    states_core(tab, n_win, P, mask, shift, path.data(), nullptr, count);
    if (with_post)
        posteriors_core(tab, n_win, P, mask, shift, post.data(), expect, &zm, &ze);
    segments_core(tab, n_win, path.data(), mask, with_post ? post.data() : nullptr, pos_first, pos_last, seg, seg_cap, n_seg, summary);
    return 0;
}

// alpha [n_win][3]: steps 1 and 2 (the forward walk) and the forward half of step 4, the kernel's calls in loops over b
static void alpha_core(const PostIn &in, size_t n_win, double *alpha)
{
    const Blocks B((uint32_t)n_win);
    std::vector<double> mat(B.nbk * 9), fin(B.nbk * 3);
    std::vector<int> mexp(B.nbk), fexp(B.nbk);
    for (uint32_t b = 0; b < B.nbk; ++b)
        post_block_matrix(in, B.begin(b), B.end(b), &mat[9 * b], &mexp[b]);
    post_forward_walk(mat.data(), mexp.data(), B.nbk, fin.data(), fexp.data());
    for (uint32_t b = 0; b < B.nbk; ++b)
        post_block_alpha(in, B.begin(b), B.end(b), &fin[3 * b], fexp[b], alpha);
}

// a draw's record from its path: the windows per state and the segments' summary, one pass in window order
static void sample_record(const uint8_t *path, size_t n_win, const uint32_t *mask, const uint64_t *pos_first, const uint64_t *pos_last,
                          uint64_t rec[SAMPLE_RECORD])
{
    for (int i = 0; i < SAMPLE_RECORD; ++i)
        rec[i] = 0;
    for (size_t f = 0; f < n_win;) {
        const unsigned s = path[f];
        size_t w = f + 1;
        while (w < n_win && !seg_start(mask, (uint32_t)w, s, path[w]))
            ++w;
        rec[s] += w - f;
        seg_summary_add(rec + 3, s, w - f, pos_first ? pos_last[w - 1] - pos_first[f] + 1 : 0);
        f = w;
    }
}

int log2_samples_host(const char *fn, const double *tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                      size_t n_starts, const int32_t *shift, size_t n_samples, uint64_t seed, uint64_t stream, const uint64_t *pos_first,
                      const uint64_t *pos_last, uint8_t *paths, uint64_t *out, char *err, size_t err_len)
{
    int64_t P[3];
    std::vector<uint32_t> own;
    const uint32_t *mask;
    if (check_log_args(fn, !out ? "out" : nullptr, tab, n_win, p01, p02, p12, "of the path", P, err, err_len))
        return 1;
    if (n_samples < 1 || n_samples > SAMPLE_MAX_DRAWS) {
        snprintf(err, err_len, "[::] ERROR in %s: n_samples = %zu is not in 1 .. %zu", fn, n_samples, SAMPLE_MAX_DRAWS);
        return 1;
    }
    if (!pos_first != !pos_last) {
        snprintf(err, err_len, "[::] ERROR in %s: %s without %s", fn, pos_first ? "pos_first" : "pos_last",
                 pos_first ? "pos_last" : "pos_first");
        return 1;
    }
    for (size_t w = 0; pos_first && w < n_win; ++w)
        if (pos_last[w] < pos_first[w]) {
            snprintf(err, err_len, "[::] ERROR in %s: window %zu ends at %llu, before its start %llu", fn, w,
                     (unsigned long long)pos_last[w], (unsigned long long)pos_first[w]);
            return 1;
        }
    if (own_mask(fn, starts, n_starts, n_win, own, &mask, err, err_len) || shift_check(fn, shift, n_win, err, err_len))
        return 1;
    if (n_win == 0) {
        for (size_t i = 0; i < n_samples * SAMPLE_RECORD; ++i)
            out[i] = 0;
        return 0;
    }
    PostIn in = {tab, post_tables(), {}, mask, shift, {P[0], P[1], P[2]}};
    post_penalty_weights(P, in.a);
    std::vector<double> alpha(n_win * 3);
    alpha_core(in, n_win, alpha.data());
    std::vector<uint8_t> one(paths ? 0 : n_win);
    for (size_t k = 0; k < n_samples; ++k) {
        uint8_t *path = paths ? paths + k * n_win : one.data();
        const uint64_t key = sample_key(seed, stream, k);
        unsigned st = 0;                              // (the last window's map takes anything)
        for (size_t w = n_win; w-- > 0;) {
            st = sample_window_state(in, alpha.data(), (uint32_t)n_win, (uint32_t)w, key, st);
            path[w] = (uint8_t)st;
        }
        sample_record(path, n_win, mask, pos_first, pos_last, out + k * SAMPLE_RECORD);
    }
    return 0;
}

}  // namespace ibdg
