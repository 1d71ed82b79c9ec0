// log_switches_asan.cpp -- the host twin of the switches (ibdg::log2_switches_host, ibdg::switch_penalty_update) under
// AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own: no device, no Python.  From the repository root:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -static-libasan -static-libubsan -o log_switches_asan tools/log_switches_asan.cpp ibdgem_amd/csrc/ibdg_states_host.cpp && ./log_switches_asan
// The shapes 1, 2, 257 (C = 2, a last block of one window) and 1279 (C = 5): a table with a NaN window and an emission below
// 2^-1000, chain starts at 1, at a block's first window and at n - 1, shifts that reach both caps; with and without the rows,
// with and without chains and shifts; the table that says nothing (NULL) under the same chains and shifts; a dead table (DESIGN
// 4.9); one update from the sums.  The rows must hold no NaN and nothing negative, the sums must not exceed the counted steps,
// and sw of window 0 is 0.  Exits 0 and prints a checksum per shape; a sanitizer report aborts.
#include "../ibdgem_amd/csrc/ibdg_states.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static const double PEN[3] = {0.05, 0.01, 0.05};

static int one(const char *what, const double *tab, size_t n, const uint32_t *starts, size_t n_starts, const int32_t *shift, bool dead,
               double expect[3], uint64_t counted[3], uint64_t *sum)
{
    std::vector<double> sw(n * 3 + 3, -1.0);            // (three more: nothing may land behind the rows)
    double bare[3];
    uint64_t cb[3];
    char err[256];
    if (ibdg::log2_switches_host("log_switches_asan", tab, n, PEN[0], PEN[1], PEN[2], starts, n_starts, shift, sw.data(), expect, counted, err,
                                 sizeof err) ||
        ibdg::log2_switches_host("log_switches_asan", tab, n, PEN[0], PEN[1], PEN[2], starts, n_starts, shift, nullptr, bare, cb, err, sizeof err))
        return fprintf(stderr, "%s\n", err), 1;
    if (memcmp(bare, expect, sizeof bare) || memcmp(cb, counted, sizeof cb))
        return fprintf(stderr, "%s, %zu windows: the sums without the rows differ\n", what, n), 1;
    if (sw[3 * n] != -1.0 || sw[3 * n + 1] != -1.0 || sw[3 * n + 2] != -1.0)
        return fprintf(stderr, "%s, %zu windows: a write behind the rows\n", what, n), 1;
    for (size_t w = 0; w < n; ++w)
        for (int k = 0; k < 3; ++k) {
            const double x = sw[3 * w + k];
            if (!(x >= 0.0 && x <= 1.0 + 1e-9) || (w == 0 && x != 0.0) || (dead && x != 0.0))
                return fprintf(stderr, "%s, %zu windows: sw[%zu][%d] = %g\n", what, n, w, k, x), 1;
            uint64_t bits;
            memcpy(&bits, &x, sizeof bits);
            *sum = ibdg::sm64(*sum ^ bits);
        }
    for (int k = 0; k < 3; ++k)
        if (!(expect[k] >= 0.0 && expect[k] <= (double)counted[k] * (1.0 + 1e-9)) || counted[k] > (n ? n - 1 : 0))
            return fprintf(stderr, "%s, %zu windows: expect[%d] = %g of %llu counted steps\n", what, n, k, expect[k],
                           (unsigned long long)counted[k]), 1;
    return 0;
}

static int shape(size_t n)
{
    std::vector<double> tab(n * 3);
    std::vector<int32_t> shift(n);
    uint64_t z = n;
    for (size_t w = 0; w < n; ++w) {
        for (int s = 0; s < 3; ++s)
            tab[3 * w + s] = -3000.0 + (double)(ibdg::sm64(z++) % 6000) / 1000.0;
        shift[w] = (int32_t)(ibdg::sm64(z++) % (6 * 65536)) - 3 * 65536;
    }
    tab[3 * (n / 2) + 1] = NAN;
    tab[3 * (n / 3)] = tab[3 * (n / 3) + 2] - 2000.0;
    std::vector<int32_t> mild(shift);                  // (no cap at 0: with it, any table might die)
    shift[n / 4] = -(1 << 30), shift[n / 5] = 1 << 30;
    const uint32_t C = (uint32_t)((n + 255) / 256), all[3] = {1, C > 1 ? C : 2, (uint32_t)n - 1};
    const size_t n_starts = n >= 4 ? 3 : n >= 2 ? 1 : 0;          // (1, 2 and n - 1 are three windows from n = 4 on)
    uint64_t sum = 0, counted[3], cp[3];
    double expect[3], total[3] = {0.0, 0.0, 0.0}, prior[3], next[3];
    for (int form = 0; form < 4; ++form) {
        const uint32_t *st = form & 1 ? all : nullptr;
        const int32_t *sh = form & 2 ? mild.data() : nullptr;
        if (one("table", tab.data(), n, st, form & 1 ? n_starts : 0, sh, false, expect, counted, &sum) ||
            one("nothing", nullptr, n, st, form & 1 ? n_starts : 0, sh, false, prior, cp, &sum))
            return 1;
        if (memcmp(counted, cp, sizeof cp))
            return fprintf(stderr, "%zu windows, form %d: the counted steps of the table and of the prior differ\n", n, form), 1;
        for (int k = 0; k < 3; ++k)
            total[k] += expect[k];
        ibdg::switch_penalty_update(PEN, total, (size_t)form + 1, prior, next);
        for (int k = 0; k < 3; ++k)
            if (!(next[k] >= 1e-300 && next[k] <= 1.0))
                return fprintf(stderr, "%zu windows, form %d: next[%d] = %g\n", n, form, k, next[k]), 1;
    }
    if (one("caps", tab.data(), n, all, n_starts, shift.data(), false, expect, counted, &sum))
        return 1;
    if (n >= 2) {
        std::vector<double> deadtab(tab);
        const size_t p = C > 1 ? (n / 2 / C) * C : 0;             // the pair inside a block where a block has two windows
        deadtab[3 * p] = -10.0, deadtab[3 * p + 1] = deadtab[3 * p + 2] = -5000.0;
        deadtab[3 * p + 3] = deadtab[3 * p + 5] = -5000.0, deadtab[3 * p + 4] = -10.0;
        std::vector<int32_t> kill(mild);
        kill[p + 1] = -(1 << 30);
        if (one("dead", deadtab.data(), n, nullptr, 0, kill.data(), true, expect, counted, &sum))
            return 1;
    }
    printf("%zu windows: %016llx\n", n, (unsigned long long)sum);
    return 0;
}

int main()
{
    return shape(1) || shape(2) || shape(257) || shape(1279);
}
