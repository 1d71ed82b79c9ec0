// ibdg_states_host.cpp -- the host twin of the integer log-domain IBD-state path (ibdg_states.h has the definition): the
// sequential recurrence itself, one window after the other.  Host only; built with -ffp-contract=off like the rest.
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

static void emission(const double *l, int64_t e[3])
{
    e[0] = e[1] = e[2] = 0;
    if (l[0] != l[0] || l[1] != l[1] || l[2] != l[2])
        return;
    double m = l[0] > l[1] ? l[0] : l[1];
    m = m > l[2] ? m : l[2];
    if (!std::isfinite(m))
        return;
    for (int s = 0; s < 3; ++s) {
        double d = l[s] - m;
        d = d < STATES_D_MIN ? STATES_D_MIN : d;
        e[s] = (int64_t)std::llrint(d * STATES_QUANTA);
    }
}

static int argmax3(const int64_t v[3])
{
    int m = 0;
    for (int i = 0; i < 3; ++i)
        if (v[i] > v[m])
            m = i;
    return m;
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

// The cores take checked arguments and check nothing.
// The states recurrence: path [n_win] or NULL, score [n_win][3] or NULL, count[3]
static void states_core(const double *tab, size_t n_win, const int64_t P[3], uint8_t *path, int64_t *score, uint64_t count[3])
{
    count[0] = count[1] = count[2] = 0;
    if (n_win == 0)
        return;
    const int64_t pen[3][3] = {{0, P[0], P[1]}, {P[0], 0, P[2]}, {P[1], P[2], 0}};
    std::vector<uint8_t> from(n_win);            // from[i][s] in bits 2 s, 2 s + 1
    int64_t v[3];
    emission(tab, v);
    from[0] = 0 | 1 << 2 | 2 << 4;
    if (score)
        score[0] = v[0], score[1] = v[1], score[2] = v[2];
    for (size_t i = 1; i < n_win; ++i) {
        int64_t e[3], nv[3];
        emission(tab + 3 * i, e);
        unsigned f = 0;
        for (int s = 0; s < 3; ++s) {
            int64_t cand[3];
            for (int q = 0; q < 3; ++q)
                cand[q] = v[q] + pen[q][s];
            const int m = argmax3(cand);
            nv[s] = cand[m] + e[s];
            f |= (unsigned)m << (2 * s);
        }
        from[i] = (uint8_t)f;
        for (int s = 0; s < 3; ++s) {
            v[s] = nv[s];
            if (score)
                score[3 * i + s] = nv[s];
        }
    }
    int st = argmax3(v);
    for (size_t i = n_win; i-- > 0;) {
        ++count[st];
        if (path)
            path[i] = (uint8_t)st;
        st = from[i] >> (2 * st) & 3;
    }
}

// err: room for a message
int log2_states_host(const double *tab, size_t n_win, double p01, double p02, double p12, uint8_t *path, int64_t *score,
                     uint64_t count[3], char *err, size_t err_len)
{
    int64_t P[3];
    if (check_log_args("ibdg_log2_states_host", count ? nullptr : "count", tab, n_win, p01, p02, p12, "the integer scores allow", P,
                       err, err_len))
        return 1;
    states_core(tab, n_win, P, path, score, count);
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

static void emission_weights(const double *l, const double *T, double b[3])
{
    int64_t e[3];
    emission(l, e);
    for (int s = 0; s < 3; ++s)
        b[s] = post_weight(e[s], T, T + 256);
}

// The sum-product pass: the sequence of ibdg_states.h, step for step (its numbers are in the comments); the kernel's threads are
// the loops over b.  post [n_win][3] or NULL.
static void posteriors_core(const double *tab, size_t n_win, const int64_t P[3], double *post, double expect[3], double *z_mant,
                            int *z_exp)
{
    expect[0] = expect[1] = expect[2] = 0.0;
    *z_mant = 1.0, *z_exp = 0;
    if (n_win == 0)
        return;
    const double *T = post_tables();
    double a[3];
    post_penalty_weights(P, a);
    std::vector<double> own;
    if (!post) {
        own.resize(n_win * 3);
        post = own.data();
    }
    const size_t C = (n_win + POST_BLOCKS - 1) / POST_BLOCKS;
    const size_t nbk = (n_win + C - 1) / C;
    std::vector<double> mat(nbk * 9), fin(nbk * 3), gout(nbk * 3);
    std::vector<int> mexp(nbk), fexp(nbk);
    // 1
    for (size_t b = 0; b < nbk; ++b) {
        const size_t w0 = b * C, w1 = w0 + C < n_win ? w0 + C : n_win;
        double *R = &mat[9 * b], bw[3], M[9];
        int e = 0;
        emission_weights(tab + 3 * w0, T, bw);
        if (b == 0)
            for (int q = 0; q < 3; ++q)
                R[3 * q] = bw[0], R[3 * q + 1] = bw[1], R[3 * q + 2] = bw[2];
        else
            post_step_matrix(a, bw, R);
        for (size_t w = w0 + 1; w < w1; ++w) {
            emission_weights(tab + 3 * w, T, bw);
            post_step_matrix(a, bw, M);
            for (int q = 0; q < 3; ++q)
                post_vec_mat(R + 3 * q, M);
            post_rescale<9>(R, e);
        }
        mexp[b] = e;
    }
    // 2
    {
        double v[3] = {mat[0], mat[1], mat[2]};
        int e = mexp[0];
        for (size_t k = 1; k < nbk; ++k) {
            fin[3 * k] = v[0], fin[3 * k + 1] = v[1], fin[3 * k + 2] = v[2];
            fexp[k] = e;
            if (k + 1 < nbk) {
                post_vec_mat(v, &mat[9 * k]);
                e += mexp[k];
                post_rescale<3>(v, e);
            }
        }
        double g[3] = {1.0, 1.0, 1.0};
        int ge = 0;
        for (size_t k = nbk; k-- > 0;) {
            gout[3 * k] = g[0], gout[3 * k + 1] = g[1], gout[3 * k + 2] = g[2];
            if (k > 0) {
                post_mat_vec(&mat[9 * k], g);
                post_rescale<3>(g, ge);
            }
        }
    }
    double part[POST_BLOCKS][3] = {};
    for (size_t b = 0; b < nbk; ++b) {
        const size_t w0 = b * C, w1 = w0 + C < n_win ? w0 + C : n_win;
        double bw[3], M[9];
        // 3
        double be[3] = {gout[3 * b], gout[3 * b + 1], gout[3 * b + 2]};
        int ge = 0;
        for (size_t w = w1; w-- > w0;) {
            post[3 * w] = be[0], post[3 * w + 1] = be[1], post[3 * w + 2] = be[2];
            if (w > w0) {
                emission_weights(tab + 3 * w, T, bw);
                post_step_matrix(a, bw, M);
                post_mat_vec(M, be);
                post_rescale<3>(be, ge);
            }
        }
        // 4
        double v[3] = {fin[3 * b], fin[3 * b + 1], fin[3 * b + 2]}, acc[3] = {0.0, 0.0, 0.0};
        int e = fexp[b];
        for (size_t w = w0; w < w1; ++w) {
            emission_weights(tab + 3 * w, T, bw);
            if (w == 0) {
                v[0] = bw[0], v[1] = bw[1], v[2] = bw[2];
                e = 0;
            } else {
                post_step_matrix(a, bw, M);
                post_vec_mat(v, M);
                post_rescale<3>(v, e);
            }
            const double p0 = v[0] * post[3 * w], p1 = v[1] * post[3 * w + 1], p2 = v[2] * post[3 * w + 2];
            const double D = (p0 + p1) + p2;
            const double g0 = p0 / D, g1 = p1 / D, g2 = p2 / D;
            post[3 * w] = g0, post[3 * w + 1] = g1, post[3 * w + 2] = g2;
            acc[0] += g0, acc[1] += g1, acc[2] += g2;
            if (w + 1 == n_win)
                *z_mant = D, *z_exp = e;
        }
        part[b][0] = acc[0], part[b][1] = acc[1], part[b][2] = acc[2];
    }
    // 5
    for (int d = POST_BLOCKS / 2; d > 0; d >>= 1)
        for (int b = 0; b < d; ++b)
            for (int s = 0; s < 3; ++s)
                part[b][s] = part[b][s] + part[b + d][s];
    expect[0] = part[0][0], expect[1] = part[0][1], expect[2] = part[0][2];
}

int log2_posteriors_host(const double *tab, size_t n_win, double p01, double p02, double p12, double *post, double expect[3],
                         double *z_mant, int *z_exp, char *err, size_t err_len)
{
    int64_t P[3];
    if (check_log_args("ibdg_log2_posteriors_host", !expect ? "expect" : !z_mant || !z_exp ? "log2_z" : nullptr, tab, n_win, p01, p02,
                       p12, "of the path", P, err, err_len))
        return 1;
    posteriors_core(tab, n_win, P, post, expect, z_mant, z_exp);
    return 0;
}

// The segment walk: one pass over the path in window order (ibdg_states.h: every quantity is exact and associative, so this is
// the kernels' result whatever their blocks).  post: the gammas [n_win][3], or NULL for no support.
static void segments_core(const double *tab, size_t n_win, const uint8_t *path, const double *post, const uint64_t *pos_first,
                          const uint64_t *pos_last, ibdg_segment *seg, size_t seg_cap, uint64_t *n_seg, uint64_t summary[12])
{
    *n_seg = 0;
    for (int i = 0; i < 12; ++i)
        summary[i] = 0;
    for (size_t f = 0; f < n_win;) {
        const unsigned s = path[f];
        ibdg_segment r = {(uint32_t)f, 0, s, 0, {0, 0, 0}, 0, 0.0};
        double mn = INFINITY;
        size_t w = f;
        for (; w < n_win && path[w] == s; ++w) {
            int64_t e[3];
            emission(tab + 3 * w, e);
            r.e[0] += e[0], r.e[1] += e[1], r.e[2] += e[2];
            if (post) {
                const double g = post[3 * w + s];
                r.post_q += (uint64_t)std::llrint(g * SEG_POST_Q);
                mn = g < mn ? g : mn;
            }
        }
        r.n_win = (uint32_t)(w - f);
        r.post_min = post ? mn : 0.0;
        if (seg && *n_seg < seg_cap)
            seg[*n_seg] = r;
        ++*n_seg;
        ++summary[s];
        summary[3 + s] = r.n_win > summary[3 + s] ? r.n_win : summary[3 + s];
        if (pos_first) {
            const uint64_t span = pos_last[w - 1] - pos_first[f] + 1;
            summary[6 + s] += span;
            summary[9 + s] = span > summary[9 + s] ? span : summary[9 + s];
        }
        f = w;
    }
}

// (the table and the penalties are refused in the words of ibdg_log2_states_host, whose checks they are)
int log2_segments_host(const double *tab, size_t n_win, double p01, double p02, double p12, int with_post, const uint64_t *pos_first,
                       const uint64_t *pos_last, ibdg_segment *seg, size_t seg_cap, uint64_t *n_seg, uint64_t summary[12], char *err,
                       size_t err_len)
{
    int64_t P[3];
    if (!n_seg || !summary) {
        snprintf(err, err_len, "[::] ERROR in ibdg_log2_segments_host: NULL %s", n_seg ? "summary" : "n_seg");
        return 1;
    }
    if (!pos_first != !pos_last) {
        snprintf(err, err_len, "[::] ERROR in ibdg_log2_segments_host: %s without %s", pos_first ? "pos_first" : "pos_last",
                 pos_first ? "pos_last" : "pos_first");
        return 1;
    }
    if (check_log_args("ibdg_log2_states_host", nullptr, tab, n_win, p01, p02, p12, "the integer scores allow", P, err, err_len))
        return 1;
    for (size_t w = 0; pos_first && w < n_win; ++w)
        if (pos_last[w] < pos_first[w]) {
            snprintf(err, err_len, "[::] ERROR in ibdg_log2_segments_host: window %zu ends at %llu, before its start %llu", w,
                     (unsigned long long)pos_last[w], (unsigned long long)pos_first[w]);
            return 1;
        }
    std::vector<uint8_t> path(n_win);
    std::vector<double> post(with_post ? n_win * 3 : 0);
    uint64_t count[3];
    double expect[3], zm;
    int ze;
    states_core(tab, n_win, P, path.data(), nullptr, count);
    if (with_post)
        posteriors_core(tab, n_win, P, post.data(), expect, &zm, &ze);
    segments_core(tab, n_win, path.data(), with_post ? post.data() : nullptr, pos_first, pos_last, seg, seg_cap, n_seg, summary);
    return 0;
}

}  // namespace ibdg
