// ibdg_states.h -- the integer log-domain IBD-state path, its posteriors (4.9) and segments (4.10), chains (4.11), step shifts (4.12),
// sampled paths (4.13) and switches (4.14): the definition,
// and every step of it as one inline function that the kernels' threads (ibdg_states.hip) and the host twin's loops
// (ibdg_states_host.cpp) both call.  No HIP type in here: the host twin needs no device.
//
// Input l[w][0..2] = log2 LIBD0/1/2 of window w and the switch penalties p01, p02, p12.  In quanta of 2^-16 bit:
//   emission   a NaN column, or a maximum that is not finite: e = (0, 0, 0) (the window says nothing).  Otherwise
//              d_s = l_s - max(l) (one fp64 subtraction), clamped below at -2^24, e_s = (int64) rint(d_s * 65536), ties to
//              even: the product is exact, so e_s is the same integer wherever it is formed (states_emission)
//   penalties  P_xy = llrint(log2(p_xy) * 65536) by the host's libm, clamped below at -2^40; 0 on the diagonal
//   recurrence score[0][s] = e_0[s], from[0][s] = s; score[i][s] = max_q(score[i-1][q] + pen[q][s]) + e_i[s], q = 0, 1, 2
//              with strict >: the lowest state wins a tie (argmax3 of hgpath.c; states_step)
//   traceback  from argmax3(score[n-1]), as hg_solve
// (max, +) over integers is exact and associative: the scores, hence the `from` entries, hence the path are the same
// integers for any blocking of the windows.  n_win <= 2^21 keeps |score| < 2^62 (a step moves a score by at most 2^40
// down -- its own state's emission -- and never up).
//
// Chains.  A chain start is a window that is treated the way window 0 is: uniform entry, no penalty into it.  The
// starts are a mask of ceil(n_win / 32) words, bit w & 31 of word w >> 5 set iff window w >= 1 starts a chain; window 0 always
// starts one, and a NULL mask means no further start (chain_start).  Everything else accumulates as before:
//   path        at a start the step takes pen[q][s] = 0 for all q, s (states_shift_step): score[w][s] = max_q score[w-1][q] +
//               e_w[s], from[w][s] = the lowest q of that maximum, the same for every s.  The scores are not reset, and a step
//               still never moves a score up: the bound above holds.  Inside a chain [c0, c1) the scores are the chain's own
//               plus one constant K = max_q score[c0-1][q], so `from`, the traceback and the path are what a call on the slice
//               gives.
//   posteriors  at a start M_w[q][s] = b_w[s] -- post_step_matrix with a = (1, 1, 1), products with 1.0, which are exact --
//               in steps 1, 3 and 4 alike (post_window_matrix); "the first matrix of a block" is that of w0 == 0 or a start.
//               Z is the product of the chains' Z, gamma inside a chain the chain's own.  No operation is added.
//   segments    window w starts a segment iff w == 0, path[w] != path[w-1] or w starts a chain: no segment crosses a border.
//
// Step shifts.  A step shift is one int32 per window: shift[w] in quanta of 2^-16 bit, |shift| <= 2^30
// (STATES_SHIFT_MAX); shift[0] is ignored.  For a window w >= 1 that does not start a chain the step into w uses
//   P_xy(w) = min(0, max(STATES_PEN_MIN, P_xy + shift[w]))      xy = 01, 02, 12; the diagonal stays 0
// (states_shift_penalty).  A chain start keeps its meaning and wins over the shift: penalty 0 into the window, and a segment
// begins; a shift alone never begins a segment.  A NULL shift array gives the bytes of everything above.
//   path        states_step with the window's own matrix (states_shift_step).  A penalty stays <= 0, so a step still never
//               moves a score up and the bound on |score| stands; integer (max, +) is exact for any blocking.
//   posteriors  a_xy(w) = post_weight(P_xy(w), T1, T2) -- the emissions' rule, so a switch weight below 2^-1000 is 0 --, the
//               diagonal 1; M_w = post_step_matrix(a(w), b_w) in steps 1, 3 and 4 alike (post_window_matrix), the order of
//               operations unchanged.  The weights are inputs, the same doubles on either side: the count of roundings per
//               window stands.  A constant penalty's weight is never 0 (the host's ldexp), a window's own is 0 below 2^-1000:
//               "all shifts 0" gives the bytes of "no shifts" for p >= 2^-1000.
//   segments    seg_start does not change; the records change through the path and gamma only.
#pragma once
#include "../../include/ibdgem_hip.h"      // ibdg_segment

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define IBDG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define IBDG_HD inline
#endif

namespace ibdg {

constexpr size_t STATES_MAX_WIN = (size_t)1 << 21;
constexpr double STATES_QUANTA = 65536.0;               // per bit
constexpr double STATES_D_MIN = -16777216.0;            // clamp of l_s - max(l), bits
constexpr int64_t STATES_PEN_MIN = -((int64_t)1 << 40); // clamp of a penalty, quanta
constexpr int32_t STATES_SHIFT_MAX = (int32_t)1 << 30;  // the largest |shift[w]|, quanta

// the nearest integer, ties to even (the default rounding mode on the host; v_rndne_f64 and a conversion on the device)
IBDG_HD int64_t states_rint(double x)
{
    return (int64_t)__builtin_llrint(x);
}

// e[0..2] of the window whose row is l[0..2]
IBDG_HD void states_emission(const double *__restrict__ l, int64_t e[3])
{
    const double v[3] = {l[0], l[1], l[2]};
    e[0] = e[1] = e[2] = 0;
    if (v[0] != v[0] || v[1] != v[1] || v[2] != v[2])
        return;
    double m = v[0] > v[1] ? v[0] : v[1];
    m = m > v[2] ? m : v[2];
    if (!(m - m == 0.0))                       // +-inf
        return;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        double d = v[s] - m;
        d = d < STATES_D_MIN ? STATES_D_MIN : d;
        e[s] = states_rint(d * STATES_QUANTA);
    }
}

// v'[s] = max_q(v[q] + pen[q][s]) + e[s], lowest q on a tie; returns from[s] in bits 2 s, 2 s + 1
IBDG_HD unsigned states_step(int64_t v[3], const int64_t pen[3][3], const int64_t e[3])
{
    int64_t nv[3];
    unsigned f = 0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        int64_t best = v[0] + pen[0][s];
        unsigned m = 0;
#pragma unroll
        for (int q = 1; q < 3; ++q) {
            const int64_t c = v[q] + pen[q][s];
            const bool gt = c > best;
            best = gt ? c : best;
            m = gt ? q : m;
        }
        nv[s] = best + e[s];
        f |= m << (2 * s);
    }
    v[0] = nv[0], v[1] = nv[1], v[2] = nv[2];
    return f;
}

// whether window w >= 1 starts a chain; mask: the starts' bits, or NULL for none
IBDG_HD bool chain_start(const uint32_t *__restrict__ mask, uint32_t w)
{
    return mask && (mask[w >> 5] >> (w & 31) & 1);
}

// P_xy(w): the penalty P of the step into a window whose shift is sh
IBDG_HD int64_t states_shift_penalty(int64_t P, int32_t sh)
{
    int64_t x = P + sh;
    x = x < STATES_PEN_MIN ? STATES_PEN_MIN : x;
    return x > 0 ? 0 : x;
}

// the three penalties of the step into a window: 0 at a chain start, else P_xy(w) where the windows have shifts (shifted; sh: the
// window's), else P_xy.  P = {P_01, P_02, P_12}
IBDG_HD void states_window_penalties(const int64_t P[3], bool start, bool shifted, int32_t sh, int64_t Pw[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k)
        Pw[k] = start ? 0 : shifted ? states_shift_penalty(P[k], sh) : P[k];
}

// states_step of a window that starts a chain (start) or not, with its own penalties (states_window_penalties): one matrix, by
// selects
IBDG_HD unsigned states_shift_step(int64_t v[3], const int64_t P[3], const int64_t e[3], bool start, bool shifted, int32_t sh)
{
    int64_t Pw[3];
    states_window_penalties(P, start, shifted, sh, Pw);
    const int64_t pw[3][3] = {{0, Pw[0], Pw[1]}, {Pw[0], 0, Pw[2]}, {Pw[1], Pw[2], 0}};
    return states_step(v, pw, e);
}

// shift[w] of a window w >= 1, or 0 without shifts (the caller says "shifted" beside it)
IBDG_HD int32_t step_shift(const int32_t *__restrict__ shift, uint32_t w)
{
    return shift ? shift[w] : 0;
}

IBDG_HD int argmax3(const int64_t v[3])
{
    const int m = v[1] > v[0] ? 1 : 0;
    return v[2] > v[m] ? 2 : m;
}

// a map of the three states as 6 bits (state s -> bits 2 s, 2 s + 1), the form of `from`; (a after b)(s) = a(b(s))
constexpr unsigned MAP_ID = 0 | 1 << 2 | 2 << 4;
IBDG_HD unsigned map_at(unsigned a, unsigned s)
{
    return a >> (2 * s) & 3;
}
IBDG_HD unsigned map_after(unsigned a, unsigned b)
{
    return map_at(a, map_at(b, 0)) | map_at(a, map_at(b, 1)) << 2 | map_at(a, map_at(b, 2)) << 4;
}

// The blocking of all four kernels and of the posteriors' order: STATES_BLOCKS blocks of C = ceil(n_win / STATES_BLOCKS)
// windows, block b owns [begin(b), end(b)); the first nbk = ceil(n_win / C) own windows, a b >= nbk owns nothing (begin = end
// = n_win).  n_win <= 2^21, so windows are uint32_t; index the tables with size_t.
constexpr int STATES_BLOCKS = 256;
struct Blocks {
    uint32_t n_win, C, nbk;
    IBDG_HD explicit Blocks(uint32_t n) : n_win(n), C((n + STATES_BLOCKS - 1) / STATES_BLOCKS), nbk(C ? (n + C - 1) / C : 0) {}
    IBDG_HD uint32_t begin(uint32_t b) const { return b * C < n_win ? b * C : n_win; }
    IBDG_HD uint32_t end(uint32_t b) const { return begin(b) + C < n_win ? begin(b) + C : n_win; }
};

// P[0..2] = P_01, P_02, P_12; 1 if a p is NaN or outside (0, 1] (bad: its index 0..2)
int states_penalties(double p01, double p02, double p12, int64_t P[3], int *bad);

// The chain starts as callers give them: a strictly increasing list with every entry in [1, n_win).  1 and a message in err
// (fn: who refuses) for anything else; else mask holds the ceil(n_win / 32) words (none for an empty list).
int chain_mask(const char *fn, const uint32_t *starts, size_t n_starts, size_t n_win, uint32_t *mask, char *err, size_t err_len);

// The step shifts as callers give them: NULL, or n_win entries with |shift[w]| <= 2^30, w >= 1 (shift[0] is ignored).  1 and a
// message in err (fn: who refuses) for anything else.
int shift_check(const char *fn, const int32_t *shift, size_t n_win, char *err, size_t err_len);

// the host twin (ibdg_log2_states[_chains|_steps]_host): path [n_win] or NULL, score [n_win][3] or NULL, count[3]; starts
// [n_starts]: the chain starts (chain_mask's rules); shift: the step shifts (shift_check's rules); fn: the public name, for
// messages; err: room for a message
int log2_states_host(const char *fn, const double *tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                     size_t n_starts, const int32_t *shift, uint8_t *path, int64_t *score, uint64_t count[3], char *err, size_t err_len);

// ---- posteriors: the sum-product pass over the weights whose max-product the path takes ---------------------
//
// Weights.  An integer x <= 0 of the path (an emission e_w[s] or a penalty P_xy, in quanta) splits as x = 65536 k + 256 j + i,
// 0 <= j, i < 256 (k = x >> 16, j = x >> 8 & 255, i = x & 255); its weight is ldexp(T1[j] * T2[i], k) with T1[j] = exp2(j /
// 256), T2[i] = exp2(i / 65536): two tables of 256 doubles made once by the host's libm (post_tables), one rounded product in
// [1, 2) and an exact scaling.  An emission weight with k < -1000 is 0, so none is subnormal; x = 0 gives exactly 1, so the
// window's best state weighs 1.  The three penalty weights a01, a02, a12 are formed on the host by the same formula with
// libm's ldexp (never 0 for a p > 0) and passed as doubles; a[q][q] = 1.  b_w[s] is the weight of e_w[s].
//
// Model.  weight(path) = prod_w b_w[path_w] * prod_{w >= 1} a[path_{w-1}][path_w] (uniform start: score[0][s] = e_0[s]),
// Z = sum over paths, gamma_w[s] = (sum over paths with path_w = s) / Z.  With alpha_0 = b_0, alpha_w = alpha_{w-1} M_w (row
// vector, M_w[q][s] = a[q][s] b_w[s]), beta_{n-1} = (1, 1, 1), beta_{w-1} = M_w beta_w (column vector): gamma_w[s] = alpha_w[s]
// beta_w[s] / sum_s alpha_w[s] beta_w[s] and Z = sum_s alpha_{n-1}[s].
//
// Arithmetic.  fp64, no contraction; +, * and multiplications by a power of two only, and one division per (window, state).
// Every matrix and vector is kept as doubles with one integer exponent (value = stored * 2^e); after every product it is
// rescaled (post_rescale): with E the exponent field of its largest entry, every entry times 2^-E and e += E.  That is exact
// unless an entry falls below 2^-1022 of the largest, where it is rounded like any subnormal (the 2^-1000 of the tests' bar).
// The exponents of the backward vectors cancel in gamma and are not carried.
//
// Order (part of the definition: floating-point products are not associative).  Blocks above: C = ceil(n_win / 256), block b owns
// windows [b C, (b + 1) C) (w0 .. w1 - 1), nbk = ceil(n_win / C) blocks own windows.  Steps 1 .. 4 are post_block_matrix,
// post_forward_walk, post_backward_walk and post_block_gamma below: the kernel calls them per thread, the twin in loops over b.
//   1  block matrix   B_b = M_w0, then for w = w0 + 1 .. w1 - 1: M = post_step_matrix(b_w); each row r of B_b <- post_vec_mat(row,
//                     M); post_rescale of the 9 entries.  M_0[q][s] = b_0[s] for every q (the uniform start): block 0's rows are
//                     three copies of alpha at its end.  The first matrix of a block is not rescaled (its largest entry is 1).
//   2  forward walk   F_1 = row 0 of B_0 with its exponent; F_{k+1} = post_vec_mat(F_k, B_k), exponent + B_k's, post_rescale; k
//                     = 1 .. nbk - 2.  F_k is alpha at the last window of block k - 1.
//      backward walk  G_{nbk-1} = (1, 1, 1); G_{k-1} = post_mat_vec(B_k, G_k), post_rescale; k = nbk - 1 .. 1.  G_k is beta at
//                     the last window of block k.  The two walks share nothing but the B_k.
//   3  block, backward  beta = G_b; for w = w1 - 1 .. w0: keep beta as beta_w; if w > w0: beta <- post_mat_vec(M_w, beta),
//                     post_rescale.
//   4  block, forward   v = F_b (block 0: none); for w = w0 .. w1 - 1: w = 0: v = b_0, exponent 0; else v <- post_vec_mat(v,
//                     M_w), post_rescale.  p_s = v[s] * beta_w[s]; D = (p_0 + p_1) + p_2; gamma_w[s] = p_s / D, or 0 if D ==
//                     0 (the dead-chain rule below); acc[s] += gamma_w[s] (acc starts at 0: the block's sum in window order).
//                     At w = n_win - 1: Z = D * 2^(v's exponent).
//   5  expect         part[b] = acc (0 for a b that owns no window), b = 0 .. 255; for d = 128, 64, .. 1: part[b] = part[b] +
//                     part[b + d] for b < d; expect = part[0].
// log2_z = log2(D) + exponent: one libm log2 and one addition on the host, in the device route too.
// Roundings on the way to one gamma, counted as hp_post_ref.R counts them: at most 14 per window.
//
// The dead-chain rule.  A switch weight of a window with a shift can be exactly 0 (below 2^-1000), and a product a * b of two tiny
// weights can underflow to 0 (two switch weights of 2^-997 in one block matrix): legal inputs can leave every path of an
// individual with weight 0.  alpha then becomes (0, 0, 0) at some window and stays so to the end, beta does the same towards
// the front, and D = 0 at every window (after an underflow: at most of them, see below) -- a dead stretch kills the individual's posteriors across chain starts too (Z is the
// product of the chains' Z).  v and beta are finite and non-negative, so D is never NaN, and D == 0 is the only case without
// a quotient: there gamma_w = (0, 0, 0).  Nothing else needs a rule: expect omits the window, a segment's post_q adds 0 and
// its post_min is 0.0, Z = 0 gives log2_z = -inf from the host's log2, and no gamma is ever NaN.  A row of gamma that sums to
// 0 is the visible mark of an individual whose weights leave no path.  The path of 4.8 is not affected: its integers do not
// underflow.  Of the two causes the exact reference (tests/hp_post_ref.py, hp_steps_ref.py) shares the first -- a weight
// that is exactly 0 is an input, and its Z is 0 too --, not the second: an underflowing product is a rounding of this
// arithmetic (it happens before the rescale, to an entry that is far above 2^-1022 of its vector's largest), the exact Z is
// not 0, D may be 0 at some windows and not at others, and such an individual can only be held to "device == twin", not to
// the exact truth.  Penalties of 1e-300 beside windows with a single live state are what it takes.
constexpr int64_t POST_K_MIN = -1000;    // an emission weight below 2^-1000 is 0

IBDG_HD double post_pow2(int k)          // 2^k, -1022 <= k <= 1023
{
    return __builtin_bit_cast(double, (uint64_t)(k + 1023) << 52);
}

// T1, T2: the tables of post_tables
IBDG_HD double post_weight(int64_t x, const double *T1, const double *T2)
{
    const int64_t k = x >> 16;
    if (k < POST_K_MIN)
        return 0.0;
    const double m = T1[x >> 8 & 255] * T2[x & 255];
    return m * post_pow2((int)k);
}

// v[0..N) * 2^e stays what it is; the largest entry comes to [1, 2).  Nothing happens if that entry is 0 or subnormal (or in
// [1, 2) already): the factor is then exactly 1, which leaves every double as it is.  A wave takes that road without a branch;
// the host, which predicts the common case, leaves early (the same result, and 7 % of the twin's time).
template <int N>
IBDG_HD void post_rescale(double *v, int &e)
{
    double mx = v[0];
#pragma unroll
    for (int i = 1; i < N; ++i)
        mx = v[i] > mx ? v[i] : mx;
    const int E = (int)(__builtin_bit_cast(uint64_t, mx) >> 52 & 0x7ff) - 1023;
    const bool keep = E == 0 || E < -1022 || E > 1022;
#if !defined(__HIP_DEVICE_COMPILE__)
    if (keep)
        return;
#endif
    const double sc = keep ? 1.0 : post_pow2(-E);
#pragma unroll
    for (int i = 0; i < N; ++i)
        v[i] *= sc;
    e += keep ? 0 : E;
}

// M[3 q + s] = a[q][s] * b[s]; a = {a01, a02, a12}
IBDG_HD void post_step_matrix(const double a[3], const double b[3], double M[9])
{
    M[0] = b[0], M[1] = a[0] * b[1], M[2] = a[1] * b[2];
    M[3] = a[0] * b[0], M[4] = b[1], M[5] = a[2] * b[2];
    M[6] = a[1] * b[0], M[7] = a[2] * b[1], M[8] = b[2];
}

// row vector times matrix: v[s] <- (v[0] M[0][s] + v[1] M[1][s]) + v[2] M[2][s]
IBDG_HD void post_vec_mat(double v[3], const double M[9])
{
    double n[3];
#pragma unroll
    for (int s = 0; s < 3; ++s)
        n[s] = (v[0] * M[s] + v[1] * M[3 + s]) + v[2] * M[6 + s];
    v[0] = n[0], v[1] = n[1], v[2] = n[2];
}

// matrix times column vector: v[q] <- (M[q][0] v[0] + M[q][1] v[1]) + M[q][2] v[2]
IBDG_HD void post_mat_vec(const double M[9], double v[3])
{
    double n[3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
        n[q] = (M[3 * q] * v[0] + M[3 * q + 1] * v[1]) + M[3 * q + 2] * v[2];
    v[0] = n[0], v[1] = n[1], v[2] = n[2];
}

// what steps 1, 3 and 4 read: the individual's table [n_win][3], the penalty weights, the tables T1, T2 = T + 256, the chain
// starts' mask or NULL, the step shifts [n_win] or NULL and the penalties in quanta (read with shifts only)
struct PostIn {
    const double *__restrict__ tab;
    const double *T;
    double a[3];
    const uint32_t *__restrict__ starts;
    const int32_t *__restrict__ shift;
    int64_t P[3];
};

// b_w[0..2] of window w.  On the host a NULL table stands for "every window says nothing": e = (0, 0, 0), b = (1, 1, 1), the
// weights post_weight gives a 0 (the switches' prior, 4.14).  The kernels' tables are never NULL and their code does not ask.
IBDG_HD void post_emission_weights(const PostIn &in, uint32_t w, double b[3])
{
#if !defined(__HIP_DEVICE_COMPILE__)
    if (!in.tab) {
        b[0] = b[1] = b[2] = 1.0;
        return;
    }
#endif
    int64_t e[3];
    states_emission(in.tab + 3 * (size_t)w, e);
#pragma unroll
    for (int s = 0; s < 3; ++s)
        b[s] = post_weight(e[s], in.T, in.T + 256);
}

// a[0..2] = a01, a02, a12 of the step into window w >= 1: the penalty weights -- with shifts the weights of the window's own
// penalties P_xy(w), formed from the integers with the tables --, or (1, 1, 1) where w starts a chain, by selects
IBDG_HD void post_window_weights(const PostIn &in, uint32_t w, double a[3])
{
    const bool st = chain_start(in.starts, w);
    if (in.shift) {
        const int32_t sh = in.shift[w];        // (asked first: its address waits for nothing)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double aw = post_weight(states_shift_penalty(in.P[k], sh), in.T, in.T + 256);
            a[k] = st ? 1.0 : aw;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            a[k] = st ? 1.0 : in.a[k];
    }
}

// M_w of window w >= 1 from its b_w and those weights (formed here as there, not by a call: the posteriors' kernel keeps the
// instructions it had before the weights were asked for on their own; tools/log_samples_asan.cpp holds the two against each other
// at every window, with and without chains and shifts, and tests/test_log_samples_asan.py runs it)
IBDG_HD void post_window_matrix(const PostIn &in, uint32_t w, const double b[3], double M[9])
{
    const bool st = chain_start(in.starts, w);
    double a[3];
    if (in.shift) {
        const int32_t sh = in.shift[w];        // (asked first: its address waits for nothing)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double aw = post_weight(states_shift_penalty(in.P[k], sh), in.T, in.T + 256);
            a[k] = st ? 1.0 : aw;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            a[k] = st ? 1.0 : in.a[k];
    }
    post_step_matrix(a, b, M);
}

// step 1 for the block of windows [w0, w1), w0 < w1: B[9] = B_b, *Bexp its exponent
IBDG_HD void post_block_matrix(const PostIn &in, uint32_t w0, uint32_t w1, double *B, int *Bexp)
{
    double R[9], bw[3], M[9];
    int e = 0;
    post_emission_weights(in, w0, bw);
    if (w0 == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            R[3 * q] = bw[0], R[3 * q + 1] = bw[1], R[3 * q + 2] = bw[2];
    } else {
        post_window_matrix(in, w0, bw, R);     // (a start gives the same three copies)
    }
    for (uint32_t w = w0 + 1; w < w1; ++w) {
        post_emission_weights(in, w, bw);
        post_window_matrix(in, w, bw, M);
#pragma unroll
        for (int q = 0; q < 3; ++q)
            post_vec_mat(R + 3 * q, M);
        post_rescale<9>(R, e);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i)
        B[i] = R[i];
    *Bexp = e;
}

// step 2 over mat [nbk][9], mexp [nbk] (step 1's): the forward walk leaves F_k in fin [nbk][3] and its exponent in fexp [nbk], k =
// 1 .. nbk - 1 (entry 0 of both is not touched: block 0 starts from b_0); the backward walk leaves G_k in gout [nbk][3]
IBDG_HD void post_forward_walk(const double *mat, const int *mexp, uint32_t nbk, double *fin, int *fexp)
{
    double v[3] = {mat[0], mat[1], mat[2]};
    int e = mexp[0], me = nbk > 2 ? mexp[1] : 0;
    for (uint32_t k = 1; k < nbk; ++k) {
        fin[3 * k] = v[0], fin[3 * k + 1] = v[1], fin[3 * k + 2] = v[2];
        fexp[k] = e;
        if (k + 1 < nbk) {
            // B_k first, and the exponent of B_{k+1} a step ahead: on the device one thread walks, and every read it has to
            // wait for in the middle of a step is LDS latency times 255
            double M[9];
#pragma unroll
            for (int i = 0; i < 9; ++i)
                M[i] = mat[9 * k + i];
            const int me_next = mexp[k + 1];
            post_vec_mat(v, M);
            e += me;
            post_rescale<3>(v, e);
            me = me_next;
        }
    }
}

IBDG_HD void post_backward_walk(const double *mat, uint32_t nbk, double *gout)
{
    double g[3] = {1.0, 1.0, 1.0};
    int ge = 0;
#pragma unroll 1                      // (one dependent chain: a second copy of the step gains nothing)
    for (uint32_t k = nbk; k-- > 0;) {
        gout[3 * k] = g[0], gout[3 * k + 1] = g[1], gout[3 * k + 2] = g[2];
        if (k > 0) {
            double M[9];
#pragma unroll
            for (int i = 0; i < 9; ++i)
                M[i] = mat[9 * k + i];
            post_mat_vec(M, g);
            post_rescale<3>(g, ge);
        }
    }
}

// steps 3 and 4 for the block of windows [w0, w1), w0 < w1, from G = G_b, F = F_b and its exponent Fexp (not used by block 0):
// post [n_win][3] holds beta_w of the block's windows from step 3 to step 4, which leaves gamma_w there; acc = the block's sum of
// gamma in window order; *D, *Dexp: D and v's exponent at window w1 - 1 (Z, for the last block)
IBDG_HD void post_block_gamma(const PostIn &in, uint32_t w0, uint32_t w1, const double *G, const double *F, int Fexp,
                              double *__restrict__ post, double acc[3], double *D, int *Dexp)
{
    double bw[3], M[9];
    // 3
    double be[3] = {G[0], G[1], G[2]};
    int ge = 0;
    for (uint32_t w = w1; w-- > w0;) {
        double *p = post + 3 * (size_t)w;
        p[0] = be[0], p[1] = be[1], p[2] = be[2];
        if (w > w0) {
            post_emission_weights(in, w, bw);
            post_window_matrix(in, w, bw, M);
            post_mat_vec(M, be);
            post_rescale<3>(be, ge);
        }
    }
    // 4
    double v[3] = {F[0], F[1], F[2]}, d = 0.0;
    int e = Fexp;
    double sum[3] = {0.0, 0.0, 0.0};
    for (uint32_t w = w0; w < w1; ++w) {
        double *p = post + 3 * (size_t)w;
        post_emission_weights(in, w, bw);
        if (w == 0) {
            v[0] = bw[0], v[1] = bw[1], v[2] = bw[2];
            e = 0;
        } else {
            post_window_matrix(in, w, bw, M);
            post_vec_mat(v, M);
            post_rescale<3>(v, e);
        }
        const double p0 = v[0] * p[0], p1 = v[1] * p[1], p2 = v[2] * p[2];
        d = (p0 + p1) + p2;
        const bool dead = d == 0.0;               // the dead-chain rule: no path has weight, gamma_w = (0, 0, 0), by selects
        const double g0 = dead ? 0.0 : p0 / d, g1 = dead ? 0.0 : p1 / d, g2 = dead ? 0.0 : p2 / d;
        p[0] = g0, p[1] = g1, p[2] = g2;
        sum[0] += g0, sum[1] += g1, sum[2] += g2;
    }
    acc[0] = sum[0], acc[1] = sum[1], acc[2] = sum[2];
    *D = d, *Dexp = e;
}

// the two tables, T1 = tab[0..256), T2 = tab[256..512) (made once, by libm's exp2)
const double *post_tables();
// a[0..2] = the weights of P_01, P_02, P_12 (states_penalties' integers)
void post_penalty_weights(const int64_t P[3], double a[3]);

// the host twin (ibdg_log2_posteriors[_chains]_host): post [n_win][3] or NULL, expect[3], z_mant and z_exp with Z = z_mant *
// 2^z_exp (1, 0 for n_win = 0); starts, shift, fn as above
int log2_posteriors_host(const char *fn, const double *tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                         size_t n_starts, const int32_t *shift, double *post, double expect[3], double *z_mant, int *z_exp, char *err, size_t err_len);

// ---- segments: the maximal runs of one state along the path, with what backs each of them -------------------
//
// Inputs: path[n_win] of 4.8; the emissions e_w[s] (the integers above); optionally gamma_w[s] of 4.9; optionally the positions
// pos_first[w] <= pos_last[w] of every window's first and last site.  Window w starts a segment iff w == 0, path[w] !=
// path[w - 1] or w starts a chain (seg_start; the chain of a segment follows from `first`); segment k (0-based, in window order) runs from its start f to the window before the next start, or to n_win - 1.
//   record   ibdg_segment (include/ibdgem_hip.h, 56 bytes): first = f, n_win = its windows, state = path[f], reserved = 0;
//            e[s] = sum of e_w[s] over its windows (|e_w[s]| <= 2^40, n_win <= 2^21: |sum| <= 2^61; a window whose emission is
//            (0, 0, 0) adds nothing); post_q = sum of q_w = states_rint(gamma_w[state] * 2^32) (the product with a power of two is
//            exact, ties to even; q_w <= 2^32, the sum <= 2^53); post_min = min of gamma_w[state] (gamma is never NaN -- a dead chain's is (0, 0, 0), the rule of 4.9 --: no NaN rule).  post_q = 0 and post_min = 0.0 when the
//            posteriors are not asked for
//   summary  uint64[12] per individual, for s = 0, 1, 2: [s] n_seg[s], [3 + s] longest_win[s] (the largest n_win of a segment
//            in state s, 0 if none), [6 + s] bp[s] = sum over the state's segments of span = pos_last[last window] -
//            pos_first[f] + 1 (modulo 2^64), [9 + s] longest_bp[s]; the two bp groups are 0 without positions
// Every one of these is an integer +, a max or an fp64 min of values that are themselves the same bits on either side:
// associative and exact, so the result does not depend on how the windows are cut into blocks.  That is why the twin walks
// the windows once in order, the kernels cut them into 256 blocks, and neither needs an order rule as the posteriors do.  Both
// add windows to a SegAcc and finished segments to the summary with the functions below.
constexpr double SEG_POST_Q = 4294967296.0;      // 2^32: q_w = rint(gamma * 2^32)

// what a run of windows in one state adds up to: a whole segment, or a piece of one that the kernel's blocks cut
struct SegAcc {
    int64_t e[3];
    uint64_t q;
    double mn;
};

// whether window w starts a segment: prev = the state of window w - 1 (3, "no state", before window 0), s = that of w
IBDG_HD bool seg_start(const uint32_t *__restrict__ mask, uint32_t w, unsigned prev, unsigned s)
{
    const bool c = chain_start(mask, w);       // (asked first, not behind the states: its read does not wait for theirs)
    return s != prev || c;
}

IBDG_HD void seg_reset(SegAcc &a)
{
    a.e[0] = a.e[1] = a.e[2] = 0;
    a.q = 0;
    a.mn = __builtin_inf();
}

// a window in state s: l its row of the table, g its row of gamma or NULL
IBDG_HD void seg_add_window(SegAcc &a, const double *__restrict__ l, const double *__restrict__ g, unsigned s)
{
    int64_t e[3];
    states_emission(l, e);
    a.e[0] += e[0], a.e[1] += e[1], a.e[2] += e[2];
    if (g) {
        a.q += (uint64_t)states_rint(g[s] * SEG_POST_Q);
        a.mn = g[s] < a.mn ? g[s] : a.mn;
    }
}

// another piece of the same segment
IBDG_HD void seg_add_piece(SegAcc &a, const SegAcc &h)
{
    a.e[0] += h.e[0], a.e[1] += h.e[1], a.e[2] += h.e[2];
    a.q += h.q;
    a.mn = h.mn < a.mn ? h.mn : a.mn;
}

IBDG_HD void seg_record(ibdg_segment *r, uint32_t first, uint32_t n, unsigned state, const SegAcc &a, bool with_post)
{
    r->first = first, r->n_win = n, r->state = state, r->reserved = 0;
    r->e[0] = a.e[0], r->e[1] = a.e[1], r->e[2] = a.e[2];
    r->post_q = a.q;
    r->post_min = with_post ? a.mn : 0.0;
}

// word i of the summary joins two partial results: groups 0 and 2 (n_seg, bp) add, groups 1 and 3 (the two longest) take the larger
IBDG_HD uint64_t seg_summary_join(int i, uint64_t x, uint64_t y)
{
    return (i / 3 & 1) ? (y > x ? y : x) : x + y;
}

// a finished segment of len windows and span bp (0 without positions) in state s enters the summary v[12]
IBDG_HD void seg_summary_add(uint64_t v[12], unsigned s, uint64_t len, uint64_t span)
{
    const uint64_t one[4] = {1, len, span, span};
#pragma unroll
    for (int i = 0; i < 12; ++i)
        v[i] = s == (unsigned)(i % 3) ? seg_summary_join(i, v[i], one[i / 3]) : v[i];
}

// the host twin (ibdg_log2_segments[_chains]_host): seg [seg_cap] or NULL, *n_seg the true count, summary[12]; starts, shift, fn as above
int log2_segments_host(const char *fn, const double *tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                       size_t n_starts, const int32_t *shift, int with_post, const uint64_t *pos_first, const uint64_t *pos_last, ibdg_segment *seg,
                       size_t seg_cap, uint64_t *n_seg, uint64_t summary[12], char *err, size_t err_len);

// ---- sampled paths: K paths drawn from P(path | all windows) under the weights of 4.9 -----------------------
//
// Forward filtering, backward sampling.  Inputs: the table, the penalties, the chains and shifts of the posteriors, the number of
// draws K (1 .. SAMPLE_MAX_DRAWS), a 64-bit seed and a 64-bit stream per individual (callers pass the individual's index in the
// panel: a draw depends on (seed, stream, k) and on nothing about batches, slots or devices).
//   alpha     alpha_w[0..2] = the vector v that step 4 above holds at window w after post_rescale (b_0 at window 0), mantissas
//             only: the common exponent cancels in the draw.  post_block_alpha is that half of step 4 and writes them
//             [n_win][3]; the steps before it (post_block_matrix, post_forward_walk) are the posteriors' own.
//   numbers   sm64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) *
//             0x94D049BB133111EB; z ^ z >> 31 (uint64, wrapping).  key(t, k) = sm64(sm64(sm64(seed) ^ stream_t) ^ k), r(t, k, w) =
//             sm64(key ^ w), U = (double)(r >> 11) * 2^-53 in [0, 1), exact.  One sm64 per window and draw, integers only.
//   a draw    for w = n_win - 1 .. 0: c_q = alpha_w[q] at the last window, else c_q = alpha_w[q] * a_{w+1}[q][s'] with s' the
//             state drawn at w + 1 and a_{w+1} the switch weights of the step into w + 1 (post_window_weights: (1, 1, 1) at a
//             chain start, the shifted weights with shifts, 1 on the diagonal; b_{w+1}[s'] is common to the three and left
//             out).  D = (c_0 + c_1) + c_2, x = U * D; the state is 0 if x < c_0, else 1 if x < c_0 + c_1, else 2
//             (sample_pick).  fp64, no contraction.
//   x < D     for every normal D: U <= 1 - 2^-53, so U D <= D - D 2^-53 <= D - ulp(D) / 2, and the product rounded to nearest
//             is at most the double below D.  With x < D = (c_0 + c_1) + c_2 a state of weight 0 is never drawn: c_2 = 0 gives
//             x < c_0 + c_1, and c_1 = 0 besides gives x < c_0; c_0 = 0 fails x < c_0 always.  (A subnormal D needs every
//             c_q below 2^-1022 under an alpha whose largest entry is in [1, 2): an s' whose own probability is below 2^-1000.)
//   total     D = 0 gives x = 0 and state 2, the same integer on either side.  Under a live alpha that needs an s' of weight 0
//             at w + 1, which by the line above is never drawn.  In a dead chain (4.9) it does happen: where alpha_w itself is
//             (0, 0, 0), from the window at which the chain dies to the end, and at the window in front of a step whose weights
//             are all 0.  Such an individual's draws are state 2 there and the usual rule in front of that -- defined bytes, of
//             a distribution that does not exist (the posteriors' gamma = 0 says so).
//   maps      the three answers for s' = 0, 1, 2 are window w's map in the form of `from` (sample_map); the last window's map
//             is constant (sample_last_map).  Maps over three states compose associatively (map_after), so a draw is the same
//             bytes for any blocking: the kernel composes per block and scans as k_log2_states does, the twin walks once from
//             the back, and neither needs an order rule beyond alpha's.
//   record    uint64[15] per draw: [0..2] the windows per state, [3..14] the 12 words of the segments' summary above for the
//             drawn path (seg_start, seg_summary_add, chains respected; the last six 0 without positions).
constexpr size_t SAMPLE_MAX_DRAWS = 65536;
constexpr int SAMPLE_RECORD = 15;

IBDG_HD uint64_t sm64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ z >> 27) * 0x94D049BB133111EBull;
    return z ^ z >> 31;
}

IBDG_HD uint64_t sample_key(uint64_t seed, uint64_t stream, uint64_t k)
{
    return sm64(sm64(sm64(seed) ^ stream) ^ k);
}

// U of window w under a draw's key
IBDG_HD double sample_u(uint64_t key, uint32_t w)
{
    return (double)(sm64(key ^ w) >> 11) * post_pow2(-53);
}

IBDG_HD unsigned sample_pick(double c0, double c1, double c2, double U)
{
    const double c01 = c0 + c1;
    const double x = U * (c01 + c2);
    return x < c0 ? 0u : x < c01 ? 1u : 2u;
}

// the state at window w given s' = sp at w + 1, from alpha_w and a = a01, a02, a12 of the step into w + 1 (the product with the
// diagonal's 1.0 is exact)
IBDG_HD unsigned sample_state(const double al[3], const double a[3], unsigned sp, double U)
{
    const double c0 = al[0] * (sp == 0 ? 1.0 : sp == 1 ? a[0] : a[1]);
    const double c1 = al[1] * (sp == 0 ? a[0] : sp == 1 ? 1.0 : a[2]);
    const double c2 = al[2] * (sp == 0 ? a[1] : sp == 1 ? a[2] : 1.0);
    return sample_pick(c0, c1, c2, U);
}

// window w's map: s' at w + 1 -> the state at w
IBDG_HD unsigned sample_map(const double al[3], const double a[3], double U)
{
    return sample_state(al, a, 0, U) | sample_state(al, a, 1, U) << 2 | sample_state(al, a, 2, U) << 4;
}

// the last window's: its state whatever comes in
IBDG_HD unsigned sample_last_map(const double al[3], double U)
{
    return sample_pick(al[0], al[1], al[2], U) * (1u | 1u << 2 | 1u << 4);
}

// the map of window w of a draw (n_win windows, alpha [n_win][3]), as the kernel's threads form it ...
IBDG_HD unsigned sample_window_map(const PostIn &in, const double *__restrict__ alpha, uint32_t n_win, uint32_t w, uint64_t key)
{
    const double *al = alpha + 3 * (size_t)w;
    const double U = sample_u(key, w);
    if (w + 1 == n_win)
        return sample_last_map(al, U);
    double a[3];
    post_window_weights(in, w + 1, a);
    return sample_map(al, a, U);
}

// ... and that map's answer for sp alone, which is all the twin's single walk needs: map_at(sample_window_map(..), sp)
IBDG_HD unsigned sample_window_state(const PostIn &in, const double *__restrict__ alpha, uint32_t n_win, uint32_t w, uint64_t key,
                                     unsigned sp)
{
    const double *al = alpha + 3 * (size_t)w;
    const double U = sample_u(key, w);
    if (w + 1 == n_win)
        return sample_pick(al[0], al[1], al[2], U);
    double a[3];
    post_window_weights(in, w + 1, a);
    return sample_state(al, a, sp, U);
}

// the forward half of step 4 for the block of windows [w0, w1), w0 < w1, from F = F_b and its exponent (not used by block 0):
// alpha_w into alpha [n_win][3]
IBDG_HD void post_block_alpha(const PostIn &in, uint32_t w0, uint32_t w1, const double *F, int Fexp, double *__restrict__ alpha)
{
    double bw[3], M[9];
    double v[3] = {F[0], F[1], F[2]};
    int e = Fexp;
    for (uint32_t w = w0; w < w1; ++w) {
        double *p = alpha + 3 * (size_t)w;
        post_emission_weights(in, w, bw);
        if (w == 0) {
            v[0] = bw[0], v[1] = bw[1], v[2] = bw[2];
            e = 0;
        } else {
            post_window_matrix(in, w, bw, M);
            post_vec_mat(v, M);
            post_rescale<3>(v, e);
        }
        p[0] = v[0], p[1] = v[1], p[2] = v[2];
    }
}

// the host twin (ibdg_log2_samples_host): K = n_samples draws of one individual under (seed, stream); paths [K][n_win] or NULL,
// out [K][15]; pos_first, pos_last [n_win] or both NULL; starts, shift, fn as above
int log2_samples_host(const char *fn, const double *tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                      size_t n_starts, const int32_t *shift, size_t n_samples, uint64_t seed, uint64_t stream, const uint64_t *pos_first,
                      const uint64_t *pos_last, uint8_t *paths, uint64_t *out, char *err, size_t err_len);

// ---- switches: the pairwise companion of the posteriors, and the expected number of switches ------------------
//
// For every step w - 1 -> w the joint probability of (state before, state after) given all windows, under the weights of 4.9:
// xi_w[q][s] = alpha_{w-1}[q] M_w[q][s] beta_w[s] / Z.  Inputs, blocking and steps 1, 2 and 3 are the posteriors' own
// (post_block_matrix, the two walks, the backward half of post_block_gamma); post_block_switches below does step 3 as it
// stands and then a forward pass like step 4.  At every window w >= 1 of the block, before v is advanced into w -- v is alpha
// at w - 1: F_b at a block's first window, b_0 at window 1 --, with M = M_w of post_window_matrix and beta_w what step 3 kept:
//   x[q][s] = (v[q] * M[3 q + s]) * beta_w[s]             nine values; the exponents of v and beta are common factors of the
//                                                         nine and are not carried
//   r_q     = (x[q][0] + x[q][1]) + x[q][2],  X = (r_0 + r_1) + r_2
//   y_01    = x[0][1] + x[1][0],  y_02 = x[0][2] + x[2][0],  y_12 = x[1][2] + x[2][1]
//   sw_w[k] = y_k / X, or 0 if X == 0 (the dead-chain rule of 4.9: v, M and beta are finite and non-negative, so X is never
//             NaN and no sw is)                           k = 0, 1, 2 for the pairs 01, 02, 12
//   sw_0    = (0, 0, 0)
// fp64, no contraction, in this order.  sw_w[k] = P(path_{w-1}, path_w are the two states of pair k | everything); their sum
// is P(path_{w-1} != path_w | everything).
// The counted rule.  A step is counted for pair k iff w >= 1, w does not start a chain, and there are no shifts or P_k +
// shift[w] <= 0 (switch_counted): the steps whose weight is p_k up to the shift.  A chain start's weight is 1 and a step
// capped at 1 does not depend on p_k either; neither is part of d log Z / d log p_k = E_post[n_k].  All shifts 0 count what
// no shifts count.
//   n[k]       the sum of sw_w[k] over the counted steps: the block's sum in window order from 0.0 (a step that is not counted
//              adds +0.0, which leaves a sum that is never negative as it is), the 256 partial sums joined by step 5's tree
//   counted[k] the number of counted steps: an integer, the same for every individual (switch_counted_steps, on the host)
// Roundings on the way to one sw_w[k] and to n[k]: tests/hp_switch_ref.py counts them the way hp_post_ref counts R.
// The prior.  The same pass over a table that says nothing (b = 1 everywhere: a NULL table in the host twin) gives the
// expectation of n_k under the weights alone.  switch_penalty_update moves p_k by the ratio of the two.

// whether the step into window w >= 1 is counted for pair k (0, 1, 2 = 01, 02, 12)
IBDG_HD bool switch_counted(const PostIn &in, uint32_t w, int k)
{
    const bool st = chain_start(in.starts, w);
    const bool capped = in.shift && in.P[k] + in.shift[w] > 0;
    return !st && !capped;
}

// sw[0..2] of the step from v = alpha at w - 1 through M = M_w to be = beta_w
IBDG_HD void switch_step(const double v[3], const double M[9], const double be[3], double sw[3])
{
    double x[9];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int s = 0; s < 3; ++s)
            x[3 * q + s] = (v[q] * M[3 * q + s]) * be[s];
    const double r0 = (x[0] + x[1]) + x[2], r1 = (x[3] + x[4]) + x[5], r2 = (x[6] + x[7]) + x[8];
    const double X = (r0 + r1) + r2;
    const double y0 = x[1] + x[3], y1 = x[2] + x[6], y2 = x[5] + x[7];
    const bool dead = X == 0.0;                   // the dead-chain rule, by selects
    sw[0] = dead ? 0.0 : y0 / X, sw[1] = dead ? 0.0 : y1 / X, sw[2] = dead ? 0.0 : y2 / X;
}

// step 3 and the switches' forward pass for the block of windows [w0, w1), w0 < w1, from G = G_b, F = F_b and its exponent (not
// used by block 0): scr [n_win][3] holds beta_w of the block's windows from step 3 on; ROWS: the forward pass leaves sw_w there
// (else beta stays).  acc = the block's sum of the counted sw in window order
template <bool ROWS>
IBDG_HD void post_block_switches(const PostIn &in, uint32_t w0, uint32_t w1, const double *G, const double *F, int Fexp,
                                 double *__restrict__ scr, double acc[3])
{
    double bw[3], M[9];
    // 3
    double be[3] = {G[0], G[1], G[2]};
    int ge = 0;
    for (uint32_t w = w1; w-- > w0;) {
        double *p = scr + 3 * (size_t)w;
        p[0] = be[0], p[1] = be[1], p[2] = be[2];
        if (w > w0) {
            post_emission_weights(in, w, bw);
            post_window_matrix(in, w, bw, M);
            post_mat_vec(M, be);
            post_rescale<3>(be, ge);
        }
    }
    // forward
    double v[3] = {F[0], F[1], F[2]};
    int e = Fexp;
    double sum[3] = {0.0, 0.0, 0.0};
    for (uint32_t w = w0; w < w1; ++w) {
        double *p = scr + 3 * (size_t)w;
        double sw[3] = {0.0, 0.0, 0.0};
        post_emission_weights(in, w, bw);
        if (w == 0) {
            v[0] = bw[0], v[1] = bw[1], v[2] = bw[2];
            e = 0;
        } else {
            post_window_matrix(in, w, bw, M);
            switch_step(v, M, p, sw);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                sum[k] += switch_counted(in, w, k) ? sw[k] : 0.0;
            post_vec_mat(v, M);
            post_rescale<3>(v, e);
        }
        if (ROWS)
            p[0] = sw[0], p[1] = sw[1], p[2] = sw[2];
    }
    acc[0] = sum[0], acc[1] = sum[1], acc[2] = sum[2];
}

// counted[k]: the counted steps of pair k among n_win windows (mask, shift: checked, or NULL)
void switch_counted_steps(size_t n_win, const int64_t P[3], const uint32_t *mask, const int32_t *shift, uint64_t counted[3]);

// the host twin (ibdg_log2_switches_host): tab [n_win][3] or NULL (every window says nothing), sw [n_win][3] or NULL, expect[3] =
// n, counted[3]; starts, shift, fn as above
int log2_switches_host(const char *fn, const double *tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                       size_t n_starts, const int32_t *shift, double *sw, double expect[3], uint64_t counted[3], char *err,
                       size_t err_len);

// The update: next[k] = min(1, max(1e-300, p[k] * total[k] / (T * prior[k]))) where total[k] and prior[k] are finite and > 0,
// else next[k] = p[k].  total: the posterior n summed over T individuals; prior: one individual's n on the NULL table.  Plain
// fp64, (p * total) / ((double)T * prior).  It is the multiplicative step towards the penalties at which the posterior
// expectation of the counted switches equals the expectation under the weights alone (DESIGN 4.14 says what is and is not known
// about where it goes).
void switch_penalty_update(const double p[3], const double total[3], size_t T, const double prior[3], double next[3]);

// ---- the fit: the update repeated over the tables of all T individuals of a site list --------------------------
//
// An iteration with penalties p: total[k] = the individuals' n[k] under p added in their order from 0.0; prior and counted from the
// NULL table under p; next = switch_penalty_update(p, total, T, prior).  The iteration stood iff for every pair
// |states_penalties(next)[k] - states_penalties(p)[k]| <= 1: no penalty moved by more than one quantum, the resolution at which
// the kernels and the twin read a penalty at all.  (Exact repetition is not the rule: once inside a quantum the integers jitter
// by a few quanta for as long as one iterates.)  The fit from p_0 runs iterations 1, 2, ... with p_{i} = next_{i-1}, and ends
// behind the first that stood or behind max_iter; the fitted penalties are that iteration's next.  One function makes the row,
// the update and the verdict for every route: the device's loop, the twin's and the host program's.

// row = (p, total, prior, counted), next, *stood.  0, or 1 + k where p[k] is not in (0, 1]
int switch_fit_step(const double p[3], const double total[3], size_t T, const double prior[3], const uint64_t counted[3],
                    ibdg_fit_row *row, double next[3], int *stood);

// the host twin of the fit (ibdg_log2_fit_host): tabs[T] tables [n_win][3]; rows [max_iter]; starts, shift, fn, err as above
int log2_fit_host(const char *fn, const double *const *tabs, size_t T, size_t n_win, const double p[3], const uint32_t *starts,
                  size_t n_starts, const int32_t *shift, size_t max_iter, ibdg_fit_row *rows, size_t *n_rows, int *stood,
                  double fitted[3], char *err, size_t err_len);

}  // namespace ibdg
