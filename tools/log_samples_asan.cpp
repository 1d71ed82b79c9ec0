// log_samples_asan.cpp -- the host twin of the sampled paths (ibdg::log2_samples_host) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a program of its own: no device, no Python.  From the repository root:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -static-libasan -static-libubsan -o log_samples_asan tools/log_samples_asan.cpp ibdgem_amd/csrc/ibdg_states_host.cpp && ./log_samples_asan
// Two shapes of the tests -- 257 windows (C = 2, a last block of one window) and 1279 (C = 5) -- with chain starts at 1, at a
// block's first window and at n - 1, shifts that reach both caps, NaN windows, emissions below 2^-1000 and positions; with and
// without the paths.  Exits 0 and prints a checksum per shape; a sanitizer report aborts.  On the same tables post_window_matrix is
// held against the step matrix of post_window_weights (weights_agree).
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
    printf("%zu windows, %zu draws: %016llx; %zu windows hold the weights' two copies together\n", n, K, (unsigned long long)sum, held);
    return 0;
}

int main()
{
    return shape(257, 3) || shape(1279, 3);
}
