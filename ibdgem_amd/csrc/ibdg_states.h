// ibdg_states.h -- the integer log-domain IBD-state path: what its host twin (ibdg_states_host.cpp), its
// kernel (ibdg_states.hip) and the entry points share.  No HIP type in here: the host twin needs no device.
//
// Input l[w][0..2] = log2 LIBD0/1/2 of window w and the switch penalties p01, p02, p12.  In quanta of 2^-16 bit:
//   emission   a NaN column, or a maximum that is not finite: e = (0, 0, 0) (the window says nothing).  Otherwise
//              d_s = l_s - max(l) (one fp64 subtraction), clamped below at -2^24, e_s = (int64) rint(d_s * 65536), ties to
//              even: the product is exact, so e_s is the same integer wherever it is formed
//   penalties  P_xy = llrint(log2(p_xy) * 65536) by the host's libm, clamped below at -2^40; 0 on the diagonal
//   recurrence score[0][s] = e_0[s], from[0][s] = s; score[i][s] = max_q(score[i-1][q] + pen[q][s]) + e_i[s], q = 0, 1, 2
//              with strict >: the lowest state wins a tie (argmax3 of hgpath.c)
//   traceback  from argmax3(score[n-1]), as hg_solve
// (max, +) over integers is exact and associative: the scores, hence the `from` entries, hence the path are the same
// integers for any blocking of the windows.  n_win <= 2^21 keeps |score| < 2^62 (a step moves a score by at most 2^40
// down -- its own state's emission -- and never up).
#pragma once
#include "../../include/ibdgem_hip.h"      // ibdg_segment

#include <stddef.h>
#include <stdint.h>

namespace ibdg {

constexpr size_t STATES_MAX_WIN = (size_t)1 << 21;
constexpr double STATES_QUANTA = 65536.0;               // per bit
constexpr double STATES_D_MIN = -16777216.0;            // clamp of l_s - max(l), bits
constexpr int64_t STATES_PEN_MIN = -((int64_t)1 << 40); // clamp of a penalty, quanta

// P[0..2] = P_01, P_02, P_12; 1 if a p is NaN or outside (0, 1] (bad: its index 0..2)
int states_penalties(double p01, double p02, double p12, int64_t P[3], int *bad);

// the host twin (ibdg_log2_states_host): path [n_win] or NULL, score [n_win][3] or NULL, count[3]; err: room for a message
int log2_states_host(const double *tab, size_t n_win, double p01, double p02, double p12, uint8_t *path, int64_t *score,
                     uint64_t count[3], char *err, size_t err_len);

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
// Order (part of the definition: floating-point products are not associative).  C = ceil(n_win / 256), block b owns windows
// [b C, (b + 1) C) (w0 .. w1 - 1), nbk = ceil(n_win / C) blocks own windows.
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
//                     M_w), post_rescale.  p_s = v[s] * beta_w[s]; D = (p_0 + p_1) + p_2; gamma_w[s] = p_s / D; acc[s] +=
//                     gamma_w[s] (acc starts at 0: the block's sum in window order).  At w = n_win - 1: Z = D * 2^(v's exponent).
//   5  expect         part[b] = acc (0 for a b that owns no window), b = 0 .. 255; for d = 128, 64, .. 1: part[b] = part[b] +
//                     part[b + d] for b < d; expect = part[0].
// log2_z = log2(D) + exponent: one libm log2 and one addition on the host, in the device route too.
// Roundings on the way to one gamma, counted as hp_post_ref.R counts them: at most 14 per window.
#if defined(__HIP__) || defined(__HIPCC__)
#define IBDG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define IBDG_HD inline
#endif

constexpr int POST_BLOCKS = 256;         // blocks of windows (the kernel's STATES_THREADS)
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

// v[0..N) * 2^e stays what it is; the largest entry comes to [1, 2).  Nothing happens if that entry is 0 or subnormal.
template <int N>
IBDG_HD void post_rescale(double *v, int &e)
{
    double mx = v[0];
#pragma unroll
    for (int i = 1; i < N; ++i)
        mx = v[i] > mx ? v[i] : mx;
    const int E = (int)(__builtin_bit_cast(uint64_t, mx) >> 52 & 0x7ff) - 1023;
    if (E == 0 || E < -1022 || E > 1022)
        return;
    const double sc = post_pow2(-E);
#pragma unroll
    for (int i = 0; i < N; ++i)
        v[i] *= sc;
    e += E;
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

// the two tables, T1 = tab[0..256), T2 = tab[256..512) (made once, by libm's exp2)
const double *post_tables();
// a[0..2] = the weights of P_01, P_02, P_12 (states_penalties' integers)
void post_penalty_weights(const int64_t P[3], double a[3]);

// the host twin (ibdg_log2_posteriors_host): post [n_win][3] or NULL, expect[3], z_mant and z_exp with Z = z_mant * 2^z_exp (1, 0
// for n_win = 0)
int log2_posteriors_host(const double *tab, size_t n_win, double p01, double p02, double p12, double *post, double expect[3],
                         double *z_mant, int *z_exp, char *err, size_t err_len);

// ---- segments: the maximal runs of one state along the path, with what backs each of them -------------------
//
// Inputs: path[n_win] of 4.8; the emissions e_w[s] (the integers above); optionally gamma_w[s] of 4.9; optionally the positions
// pos_first[w] <= pos_last[w] of every window's first and last site.  Window w starts a segment iff w == 0 or path[w] !=
// path[w - 1]; segment k (0-based, in window order) runs from its start f to the window before the next start, or to n_win - 1.
//   record   ibdg_segment (include/ibdgem_hip.h, 56 bytes): first = f, n_win = its windows, state = path[f], reserved = 0;
//            e[s] = sum of e_w[s] over its windows (|e_w[s]| <= 2^40, n_win <= 2^21: |sum| <= 2^61; a window whose emission is
//            (0, 0, 0) adds nothing); post_q = sum of q_w = llrint(gamma_w[state] * 2^32) (the product with a power of two is
//            exact, ties to even: llrint in the default rounding mode here, __double2ll_rn on the device; q_w <= 2^32, the sum
//            <= 2^53); post_min = min of gamma_w[state] (gamma is never NaN: no NaN rule).  post_q = 0 and post_min = 0.0 when the
//            posteriors are not asked for
//   summary  uint64[12] per individual, for s = 0, 1, 2: [s] n_seg[s], [3 + s] longest_win[s] (the largest n_win of a segment
//            in state s, 0 if none), [6 + s] bp[s] = sum over the state's segments of span = pos_last[last window] -
//            pos_first[f] + 1 (modulo 2^64), [9 + s] longest_bp[s]; the two bp groups are 0 without positions
// Every one of these is an integer +, a max or an fp64 min of values that are themselves the same bits on either side:
// associative and exact, so the result does not depend on how the windows are cut into blocks.  That is why the twin walks
// the windows once in order, the kernels cut them into 256 blocks, and neither needs an order rule as the posteriors do.
constexpr double SEG_POST_Q = 4294967296.0;      // 2^32: q_w = rint(gamma * 2^32)

// the host twin (ibdg_log2_segments_host): seg [seg_cap] or NULL, *n_seg the true count, summary[12]
int log2_segments_host(const double *tab, size_t n_win, double p01, double p02, double p12, int with_post, const uint64_t *pos_first,
                       const uint64_t *pos_last, ibdg_segment *seg, size_t seg_cap, uint64_t *n_seg, uint64_t summary[12], char *err,
                       size_t err_len);

}  // namespace ibdg
