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

// path [n_win] or NULL, score [n_win][3] or NULL, count[3]; err: room for a message
int log2_states_host(const double *tab, size_t n_win, double p01, double p02, double p12, uint8_t *path, int64_t *score,
                     uint64_t count[3], char *err, size_t err_len)
{
    int64_t P[3];
    int bad = 0;
    if (!count) {
        snprintf(err, err_len, "[::] ERROR in ibdg_log2_states_host: NULL count");
        return 1;
    }
    if (n_win && !tab) {
        snprintf(err, err_len, "[::] ERROR in ibdg_log2_states_host: NULL table");
        return 1;
    }
    if (states_penalties(p01, p02, p12, P, &bad)) {
        static const char *const name[3] = {"p01", "p02", "p12"};
        snprintf(err, err_len, "[::] ERROR in ibdg_log2_states_host: %s = %g is not in (0, 1]", name[bad],
                 bad == 0 ? p01 : bad == 1 ? p02 : p12);
        return 1;
    }
    if (n_win > STATES_MAX_WIN) {
        snprintf(err, err_len, "[::] ERROR in ibdg_log2_states_host: %zu windows, more than the %zu (2^21) the integer scores allow",
                 n_win, STATES_MAX_WIN);
        return 1;
    }
    count[0] = count[1] = count[2] = 0;
    if (n_win == 0)
        return 0;
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
    return 0;
}

}  // namespace ibdg
