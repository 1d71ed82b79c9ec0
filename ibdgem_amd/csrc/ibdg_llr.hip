// ibdg_llr.hip -- segmented sums of the window log-likelihood ratios of the last run (ibdg_window_llr_sums).
//
// The reference's chromosome-arm statistic (bin/chrarm-stats.py) sums, over a range of summary windows,
// log2(L2'/L0') and log2(L1'/L0') with L' = L, or 2^-1074 where L == 0.  Here the window table of the last run
// (win_ll, [T][n_win][3] doubles) is reduced where it lies:
//   k_llr_partial  one block per (individual, segment, block of LLR_BLK windows): its share of both sums
//                  as a double-double, into a slab of partials (no atomics)
//   k_llr_combine  one thread per (individual, segment): the partials added in increasing block order
// Every log2 term enters the double-double on its own (a = +log2 L2' - log2 L0', never a rounded difference or
// the log of a ratio, which overflows at L0' = 2^-1074): the sum is exact to ~2^-100 of the terms' magnitudes,
// so its rounded value does not depend on how the windows were split into blocks, batches or devices.
// Built with -ffp-contract=off (Makefile): TwoSum is exact only without fused multiply-add rewrites.
// ibdg_window_log2_llr_sums: the same two kernels over win_log2 (option "log_windows"), whose entries are the terms.
// Bytes: 24 per window read once per segment covering it, 32 per partial; the launch is bound by memory.
#include "ibdg_kernels.h"

#include <hip/hip_runtime.h>

namespace ibdg {

namespace {

constexpr int LLR_THREADS = 256;

struct DD {
    double hi, lo;
};

// Knuth's TwoSum: s + e == a + b exactly (round to nearest, no contraction)
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e)
{
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

__device__ __forceinline__ void dd_add_d(DD &x, double v)
{
    double s, e;
    two_sum(x.hi, v, s, e);
    e += x.lo;
    x.hi = s + e;                       // FastTwoSum (|s| >= |e| up to the low part's size)
    x.lo = e - (x.hi - s);
}

__device__ __forceinline__ void dd_add(DD &x, DD y)
{
    double s, e;
    two_sum(x.hi, y.hi, s, e);
    e += x.lo + y.lo;
    x.hi = s + e;
    x.lo = e - (x.hi - s);
}

__device__ __forceinline__ double lg(double v)
{
    return log2(v == 0.0 ? 4.9406564584124654e-324 : v);      // 2^-1074: the script's resolve(); NaN stays NaN
}

__device__ __forceinline__ DD shfl_down(DD v, int d)
{
    DD r;
    r.hi = __shfl_down(v.hi, d, 64);
    r.lo = __shfl_down(v.lo, d, 64);
    return r;
}

// grid-stride over items (t, s, b); item i: b = i % nb, (t * n_seg + s) = i / nb
// LOG: the table holds log2 of the columns already (win_log2): its entries are the terms
template <bool LOG>
__global__ __launch_bounds__(LLR_THREADS) void k_llr_partial(const double *__restrict__ win_ll, uint32_t n_win,
                                                             const uint32_t *__restrict__ seg, uint32_t n_seg, uint32_t nb,
                                                             uint64_t n_items, double *__restrict__ part)
{
    __shared__ DD red[2][LLR_THREADS / 64];
    for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint64_t ts = item / nb;
        const uint32_t b = (uint32_t)(item - ts * nb);
        const uint32_t s = (uint32_t)(ts % n_seg), t = (uint32_t)(ts / n_seg);
        const uint32_t first = seg[2 * s], end = seg[2 * s + 1];
        // windows [w0, w1) of this block (empty when the segment has fewer blocks than the widest one)
        const uint64_t w0 = (uint64_t)first + (uint64_t)b * LLR_BLK;
        const uint64_t w1 = w0 + LLR_BLK < end ? w0 + LLR_BLK : end;
        const double *tab = win_ll + (size_t)t * n_win * 3;
        DD a = {0.0, 0.0}, c = {0.0, 0.0};
        for (uint64_t w = w0 + threadIdx.x; w < w1; w += LLR_THREADS) {
            const double l0 = LOG ? tab[3 * w] : lg(tab[3 * w]), l1 = LOG ? tab[3 * w + 1] : lg(tab[3 * w + 1]),
                         l2 = LOG ? tab[3 * w + 2] : lg(tab[3 * w + 2]);
            dd_add_d(a, l2);
            dd_add_d(a, -l0);
            dd_add_d(c, l1);
            dd_add_d(c, -l0);
        }
        // fixed tree: lanes, then the block's waves in order
        for (int d = 32; d > 0; d >>= 1) {
            dd_add(a, shfl_down(a, d));
            dd_add(c, shfl_down(c, d));
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) {
            red[0][wave] = a;
            red[1][wave] = c;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            DD x = red[0][0], y = red[1][0];
            for (int k = 1; k < LLR_THREADS / 64; ++k) {
                dd_add(x, red[0][k]);
                dd_add(y, red[1][k]);
            }
            double *p = part + item * 4;
            p[0] = x.hi;
            p[1] = x.lo;
            p[2] = y.hi;
            p[3] = y.lo;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(LLR_THREADS) void k_llr_combine(const double *__restrict__ part, uint32_t nb, uint64_t n_ts,
                                                             double *__restrict__ out)
{
    const uint64_t ts = (uint64_t)blockIdx.x * LLR_THREADS + threadIdx.x;
    if (ts >= n_ts)
        return;
    const double *p = part + ts * nb * 4;
    DD x = {p[0], p[1]}, y = {p[2], p[3]};
    for (uint32_t b = 1; b < nb; ++b) {
        dd_add(x, DD{p[4 * b], p[4 * b + 1]});
        dd_add(y, DD{p[4 * b + 2], p[4 * b + 3]});
    }
    double *o = out + ts * 4;
    o[0] = x.hi;
    o[1] = x.lo;
    o[2] = y.hi;
    o[3] = y.lo;
}

}  // namespace

void launch_llr_sums(const double *win_ll, uint32_t n_win, uint32_t n_targets, const uint32_t *seg, uint32_t n_seg,
                     uint32_t nb, double *part, double *out, hipStream_t st, bool from_log)
{
    const uint64_t n_ts = (uint64_t)n_targets * n_seg, n_items = n_ts * nb;
    if (n_items == 0)
        return;
    const uint64_t grid = n_items < LLR_MAX_BLOCKS ? n_items : LLR_MAX_BLOCKS;
    if (from_log)
        hipLaunchKernelGGL(k_llr_partial<true>, dim3((unsigned)grid), dim3(LLR_THREADS), 0, st, win_ll, n_win, seg, n_seg, nb,
                           n_items, part);
    else
        hipLaunchKernelGGL(k_llr_partial<false>, dim3((unsigned)grid), dim3(LLR_THREADS), 0, st, win_ll, n_win, seg, n_seg, nb,
                           n_items, part);
    hipLaunchKernelGGL(k_llr_combine, dim3((unsigned)((n_ts + LLR_THREADS - 1) / LLR_THREADS)), dim3(LLR_THREADS), 0, st,
                       part, nb, n_ts, out);
}

}  // namespace ibdg
