// log_samples_asan.cpp -- the host twin of the sampled paths (ibdg::log2_samples_host) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a program of its own: no device, no Python.  From the repository root:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -static-libasan -static-libubsan -o log_samples_asan tools/log_samples_asan.cpp ibdgem_amd/csrc/ibdg_states_host.cpp && ./log_samples_asan
// Two shapes of the tests -- 257 windows (C = 2, a last block of one window) and 1279 (C = 5) -- with chain starts at 1, at a
// block's first window and at n - 1, shifts that reach both caps, NaN windows, emissions below 2^-1000 and positions; with and
// without the paths.  Beside that table each shape walks two more (hard): one with NaN, +-inf, all-NaN and all -inf windows at its
// first, middle and last windows and at a block's border, and a dead one (a window with state 0 alone alive, then one
// with state 1 alone alive behind a shift of -2^30, so that no path has weight) -- the draws, the posteriors and the records with
// their support, where gamma must hold no NaN and, for the dead table, nothing but 0.  Exits 0 and prints a checksum per shape; a
// sanitizer report aborts.  On the same tables post_window_matrix is held against the step matrix of post_window_weights
// (weights_agree).
#include "../ibdgem_amd/csrc/ibdg_states.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// post_window_matrix against post_step_matrix over post_window_weights, which ibdg_states.h writes out twice (the posteriors' kernel
// keeps its instructions that way): every window, with and without the chains' mask and the shifts.  Returns the windows compared,
// 0 for a difference.
static size_t weights_agree(const double *tab, size_t n, const uint32_t *starts, size_t n_starts, const int32_t *shift)
{
    int64_t P[3];
    char err[256];
    std::vector<uint32_t> mask((n + 31) / 32);
    if (ibdg::states_penalties(0.05, 0.01, 0.05, P, nullptr) || ibdg::chain_mask("log_samples_asan", starts, n_starts, n, mask.data(), err, sizeof err))
        return 0;
    size_t done = 0;
    for (int form = 0; form < 4; ++form) {
        ibdg::PostIn in = {tab, ibdg::post_tables(), {}, form & 1 ? mask.data() : nullptr, form & 2 ? shift : nullptr, {P[0], P[1], P[2]}};
        ibdg::post_penalty_weights(P, in.a);
        for (size_t w = 1; w < n; ++w, ++done) {
            double b[3], a[3], M1[9], M2[9];
            ibdg::post_emission_weights(in, (uint32_t)w, b);
            ibdg::post_window_matrix(in, (uint32_t)w, b, M1);
            ibdg::post_window_weights(in, (uint32_t)w, a);
            ibdg::post_step_matrix(a, b, M2);
            if (memcmp(M1, M2, sizeof M1))
                return fprintf(stderr, "window %zu, form %d: post_window_matrix and post_window_weights differ\n", w, form), 0;
        }
    }
    return done;
}

// One hard table through the draws, the posteriors and the records with their support.  dead: gamma is 0 at every window, expect (0, 0,
// 0), Z = 0, every record's post_q 0 and post_min 0.0; else no NaN and rows of gamma that are not all 0.  Folds what it saw into *sum.
static int hard(const char *what, const std::vector<double> &tab, size_t n, size_t K, const uint32_t *starts, size_t n_starts,
                const int32_t *shift, bool dead, uint64_t *sum)
{
    std::vector<uint8_t> paths(K * n);
    std::vector<uint64_t> out(K * 15);
    std::vector<double> post(n * 3);
    std::vector<ibdg_segment> seg(n);
    double expect[3], zm;
    int ze;
    uint64_t n_seg, summary[12];
    char err[256];
    if (ibdg::log2_samples_host("log_samples_asan", tab.data(), n, 0.05, 0.01, 0.05, starts, n_starts, shift, K, 7, 3, nullptr, nullptr,
                                paths.data(), out.data(), err, sizeof err) ||
        ibdg::log2_posteriors_host("log_samples_asan", tab.data(), n, 0.05, 0.01, 0.05, starts, n_starts, shift, post.data(), expect, &zm,
                                   &ze, err, sizeof err) ||
        ibdg::log2_segments_host("log_samples_asan", tab.data(), n, 0.05, 0.01, 0.05, starts, n_starts, shift, 1, nullptr, nullptr,
                                 seg.data(), n, &n_seg, summary, err, sizeof err))
        return fprintf(stderr, "%s\n", err), 1;
    for (size_t w = 0; w < n; ++w) {
        const double *g = &post[3 * w];
        if (g[0] != g[0] || g[1] != g[1] || g[2] != g[2])
            return fprintf(stderr, "%s table, %zu windows: gamma of window %zu is NaN\n", what, n, w), 1;
        if (dead != (g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0))
            return fprintf(stderr, "%s table, %zu windows: gamma of window %zu is %s\n", what, n, w, dead ? "not 0" : "0"), 1;
    }
    if (dead && (expect[0] != 0.0 || expect[1] != 0.0 || expect[2] != 0.0 || zm != 0.0))
        return fprintf(stderr, "%s table, %zu windows: expect or Z is not 0\n", what, n), 1;
    for (uint64_t i = 0; i < n_seg; ++i) {
        if (seg[i].post_min != seg[i].post_min || (dead && (seg[i].post_q != 0 || seg[i].post_min != 0.0)))
            return fprintf(stderr, "%s table, %zu windows: the support of record %llu\n", what, n, (unsigned long long)i), 1;
        *sum = ibdg::sm64(*sum ^ seg[i].post_q ^ seg[i].first);
    }
    for (size_t k = 0; k < K; ++k) {
        if (out[15 * k] + out[15 * k + 1] + out[15 * k + 2] != n)
            return fprintf(stderr, "%s table, draw %zu of %zu windows: the states' windows do not add up\n", what, k, n), 1;
        for (int i = 0; i < 15; ++i)
            *sum = ibdg::sm64(*sum ^ out[15 * k + i]);
    }
    for (uint8_t s : paths)
        if (s > 2)
            return fprintf(stderr, "a state above 2\n"), 1;
    return weights_agree(tab.data(), n, starts, n_starts, shift) ? 0 : 1;
}

static int shape(size_t n, size_t K)
{
    std::vector<double> tab(n * 3);
    std::vector<int32_t> shift(n);
    std::vector<uint64_t> first(n), last(n);
    uint64_t z = n;
    for (size_t w = 0; w < n; ++w) {
        for (int s = 0; s < 3; ++s)
            tab[3 * w + s] = -3000.0 + (double)(ibdg::sm64(z++) % 6000) / 1000.0;
        shift[w] = (int32_t)(ibdg::sm64(z++) % (6 * 65536)) - 3 * 65536;
        first[w] = 1000 * w + 1, last[w] = 1000 * w + 1 + ibdg::sm64(z++) % 900;
    }
    tab[3 * (n / 2) + 1] = NAN;
    tab[3 * (n / 3)] = tab[3 * (n / 3) + 2] - 2000.0;
    shift[n / 4] = -(1 << 30), shift[n / 5] = 1 << 30;
    const uint32_t C = (uint32_t)((n + 255) / 256), starts[3] = {1, C > 1 ? C : 2, (uint32_t)n - 1};
    std::vector<uint8_t> paths(K * n);
    std::vector<uint64_t> out(K * 15), bare(K * 15);
    char err[256];
    if (ibdg::log2_samples_host("log_samples_asan", tab.data(), n, 0.05, 0.01, 0.05, starts, 3, shift.data(), K, 7, 3, first.data(),
                                last.data(), paths.data(), out.data(), err, sizeof err) ||
        ibdg::log2_samples_host("log_samples_asan", tab.data(), n, 0.05, 0.01, 0.05, nullptr, 0, nullptr, K, 7, 3, nullptr, nullptr,
                                nullptr, bare.data(), err, sizeof err)) {
        fprintf(stderr, "%s\n", err);
        return 1;
    }
    uint64_t sum = 0;
    for (size_t k = 0; k < K; ++k) {
        if (out[15 * k] + out[15 * k + 1] + out[15 * k + 2] != n || bare[15 * k] + bare[15 * k + 1] + bare[15 * k + 2] != n)
            return fprintf(stderr, "draw %zu of %zu windows: the states' windows do not add up\n", k, n), 1;
        for (int i = 0; i < 15; ++i)
            sum = ibdg::sm64(sum ^ out[15 * k + i] ^ bare[15 * k + i]);
    }
    for (uint8_t s : paths)
        if (s > 2)
            return fprintf(stderr, "a state above 2\n"), 1;
    const size_t held = weights_agree(tab.data(), n, starts, 3, shift.data());
    if (!held)
        return 1;
    // the two hard tables: on the moderate shifts alone (no cap: with the caps, any table might die), without the start at C
    std::vector<double> nantab(tab), deadtab(tab);
    std::vector<int32_t> mild(shift);
    mild[n / 4] = mild[n / 5] = 0;
    const size_t at[5] = {0, C - 1, C, n / 2, n - 1};
    for (int i = 0; i < 5; ++i) {
        double *r = &nantab[3 * at[i]];
        if (i == 0) r[2] = NAN;
        else if (i == 1) r[0] = r[1] = r[2] = NAN;
        else if (i == 2) r[1] = -INFINITY;
        else if (i == 3) r[0] = INFINITY;
        else r[0] = r[1] = r[2] = -INFINITY;
    }
    const size_t p = (n / 2 / C) * C;             // the pair inside a block: windows p and p + 1 (C >= 2 at both shapes)
    deadtab[3 * p] = -10.0, deadtab[3 * p + 1] = deadtab[3 * p + 2] = -5000.0;
    deadtab[3 * p + 3] = deadtab[3 * p + 5] = -5000.0, deadtab[3 * p + 4] = -10.0;
    std::vector<int32_t> kill(mild);
    kill[p + 1] = -(1 << 30);
    const uint32_t ends[2] = {1, (uint32_t)n - 1};
    if (hard("NaN", nantab, n, K, ends, 2, mild.data(), false, &sum) || hard("NaN", nantab, n, K, nullptr, 0, nullptr, false, &sum) ||
        hard("dead", deadtab, n, K, ends, 2, kill.data(), true, &sum) || hard("dead", deadtab, n, K, nullptr, 0, kill.data(), true, &sum))
        return 1;
    printf("%zu windows, %zu draws: %016llx; %zu windows hold the weights' two copies together\n", n, K, (unsigned long long)sum, held);
    return 0;
}

int main()
{
    return shape(257, 3) || shape(1279, 3);
}
