// log_fit_asan.cpp -- the host twin of the fit (ibdg::log2_fit_host, ibdg::switch_fit_step) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a program of its own: no device, no Python.  From the repository root:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -static-libasan -static-libubsan -o log_fit_asan tools/log_fit_asan.cpp ibdgem_amd/csrc/ibdg_states_host.cpp && ./log_fit_asan
// The shapes 1, 2, 257 (C = 2, a last block of one window) and 1279 (C = 5), four tables each: with and without chain starts (at
// 1, at a block's first window and at n - 1) and shifts on both sides of a penalty's cap; a limit the fit reaches and none; no
// iterations and no individuals; the step at a fixed point, at the clamps and with a penalty out of range.  Every row must repeat
// what the twin of the switches gives for its penalties, nothing may land behind the rows asked for, and the fitted penalties
// must lie in [1e-300, 1].  Exits 0 and prints a checksum per shape; a sanitizer report aborts.
#include "../ibdgem_amd/csrc/ibdg_states.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static const double PEN[3] = {0.5, 0.25, 0.5};

static int fit(size_t n, const std::vector<const double *> &tabs, const uint32_t *starts, size_t n_starts, const int32_t *shift,
               size_t max_iter, uint64_t *sum)
{
    const size_t T = tabs.size();
    std::vector<ibdg_fit_row> rows(max_iter + 1);
    memset(rows.data(), 0x5a, rows.size() * sizeof rows[0]);          // (one more: nothing may land behind the rows)
    const ibdg_fit_row guard = rows[max_iter];
    size_t n_rows = 99;
    int stood = 99;
    double fitted[3];
    char err[256];
    if (ibdg::log2_fit_host("log_fit_asan", tabs.data(), T, n, PEN, starts, n_starts, shift, max_iter, rows.data(), &n_rows, &stood, fitted,
                            err, sizeof err))
        return fprintf(stderr, "%s\n", err), 1;
    if (memcmp(&guard, &rows[max_iter], sizeof guard) || n_rows > max_iter || (stood != 0 && stood != 1))
        return fprintf(stderr, "%zu windows: a write behind the rows, or %zu rows of %zu\n", n, n_rows, max_iter), 1;
    if ((T == 0 || max_iter == 0) && (n_rows || stood || memcmp(fitted, PEN, sizeof PEN)))
        return fprintf(stderr, "%zu windows: an empty fit gave rows\n", n), 1;
    if (T && !stood && n_rows != max_iter)
        return fprintf(stderr, "%zu windows: ended after %zu of %zu iterations without standing\n", n, n_rows, max_iter), 1;
    for (size_t i = 0; i < n_rows; ++i) {
        const ibdg_fit_row &r = rows[i];
        double total[3] = {0.0, 0.0, 0.0}, expect[3], prior[3], next[3];
        uint64_t counted[3], cp[3];
        ibdg_fit_row again;
        int st;
        for (size_t t = 0; t < T; ++t) {
            if (ibdg::log2_switches_host("log_fit_asan", tabs[t], n, r.p[0], r.p[1], r.p[2], starts, n_starts, shift, nullptr, expect, counted,
                                         err, sizeof err))
                return fprintf(stderr, "%s\n", err), 1;
            for (int k = 0; k < 3; ++k)
                total[k] = total[k] + expect[k];
        }
        if (ibdg::log2_switches_host("log_fit_asan", nullptr, n, r.p[0], r.p[1], r.p[2], starts, n_starts, shift, nullptr, prior, cp, err,
                                     sizeof err))
            return fprintf(stderr, "%s\n", err), 1;
        if (memcmp(total, r.total, sizeof total) || memcmp(prior, r.prior, sizeof prior) || memcmp(cp, r.counted, sizeof cp))
            return fprintf(stderr, "%zu windows, iteration %zu: the row is not the twin's\n", n, i + 1), 1;
        if (ibdg::switch_fit_step(r.p, r.total, T, r.prior, r.counted, &again, next, &st) || memcmp(&again, &r, sizeof r))
            return fprintf(stderr, "%zu windows, iteration %zu: the step does not repeat the row\n", n, i + 1), 1;
        const double *after = i + 1 < n_rows ? rows[i + 1].p : fitted;
        if (memcmp(next, after, sizeof next) || st != (i + 1 == n_rows ? stood : 0))
            return fprintf(stderr, "%zu windows, iteration %zu: the step's next or verdict is not the fit's\n", n, i + 1), 1;
        for (int k = 0; k < 3; ++k) {
            uint64_t bits;
            memcpy(&bits, &next[k], sizeof bits);
            *sum = ibdg::sm64(*sum ^ bits);
        }
    }
    for (int k = 0; k < 3; ++k)
        if (!(fitted[k] >= 1e-300 && fitted[k] <= 1.0))
            return fprintf(stderr, "%zu windows: fitted[%d] = %g\n", n, k, fitted[k]), 1;
    return 0;
}

static int shape(size_t n)
{
    const size_t T = 4;
    std::vector<std::vector<double>> tab(T, std::vector<double>(n * 3));
    std::vector<int32_t> shift(n);
    uint64_t z = 7 * n;
    for (size_t t = 0; t < T; ++t)
        for (size_t w = 0; w < n; ++w) {
            const int live = (int)((w / 40 + t) % 3);               // runs of 40 windows in one state: penalties worth fitting
            for (int s = 0; s < 3; ++s)
                tab[t][3 * w + s] = -3000.0 + (double)(ibdg::sm64(z++) % 4000) / 1000.0 + (s == live ? 6.0 : 0.0);
        }
    tab[1][3 * (n / 2) + 1] = NAN;
    for (size_t w = 0; w < n; ++w)
        shift[w] = (int32_t)(ibdg::sm64(z++) % (6 * 65536)) - 3 * 65536;
    const uint32_t C = (uint32_t)((n + 255) / 256), all[3] = {1, C > 1 ? C : 2, (uint32_t)n - 1};
    const size_t n_starts = n >= 4 ? 3 : n >= 2 ? 1 : 0;
    std::vector<const double *> tabs;
    for (size_t t = 0; t < T; ++t)
        tabs.push_back(tab[t].data());
    uint64_t sum = 0;
    for (int form = 0; form < 4; ++form) {
        const uint32_t *st = form & 1 ? all : nullptr;
        const int32_t *sh = form & 2 ? shift.data() : nullptr;
        if (fit(n, tabs, st, form & 1 ? n_starts : 0, sh, 3, &sum) || fit(n, tabs, st, form & 1 ? n_starts : 0, sh, 40, &sum))
            return 1;
    }
    if (fit(n, tabs, nullptr, 0, nullptr, 0, &sum) || fit(n, std::vector<const double *>(), nullptr, 0, nullptr, 5, &sum))
        return 1;
    printf("%zu windows: %016llx\n", n, (unsigned long long)sum);
    return 0;
}

static int steps()
{
    const double prior[3] = {4.0, 0.25, 0.125}, fixed[3] = {40.0, 2.5, 1.25}, p[3] = {0.5, 0.01, 1e-5};
    const uint64_t counted[3] = {9, 8, 7};
    ibdg_fit_row row;
    double next[3];
    int stood = 0;
    if (ibdg::switch_fit_step(p, fixed, 10, prior, counted, &row, next, &stood) || !stood || memcmp(next, p, sizeof p))
        return fprintf(stderr, "the step at a fixed point\n"), 1;
    const double lo[3] = {0.5, 1e-299, 1.0}, tot[3] = {1000.0, 1e-9, 3.0}, one[3] = {1.0, 1.0, 1.0};
    if (ibdg::switch_fit_step(lo, tot, 1, one, counted, &row, next, &stood) || stood || next[0] != 1.0 || next[1] != 1e-300 || next[2] != 1.0)
        return fprintf(stderr, "the step at the clamps\n"), 1;
    const double bad[3] = {0.5, 0.0, 0.5};
    if (ibdg::switch_fit_step(bad, tot, 1, one, counted, &row, next, &stood) != 2)
        return fprintf(stderr, "the step with a penalty out of range\n"), 1;
    return 0;
}

int main()
{
    return steps() || shape(1) || shape(2) || shape(257) || shape(1279);
}
