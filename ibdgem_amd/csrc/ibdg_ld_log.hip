// ibdg_ld_log.hip -- option "log_windows": log2 of the window likelihoods, for windows whose likelihoods leave the
// double range.
//
// The window columns are products of about window x coverage probabilities.  The counting kernels (ibdg_ld_popcount.hip)
// hold every background individual's window product as a mantissa and an EXACT integer exponent, and then call ldexp on
// it: at 30x coverage every LIBD0 of a summary is 0.  Here the same pairs are kept as pairs to the end:
//
//   k_ld_log        --LD: LIBD0 and LIBD1 of a window, log2 of the background mean of the binomial window products
//                   (src/ibdgem.c:714-753).  A workgroup per (window, comparison individual), a wave per chunk of 64
//                   background individuals (one a lane).  The wave walks the window's segments on the tiles the site list
//                   uses, takes the weighted popcounts of the header of ibdg_ld_popcount.hip with (mask, count) statements
//                   and forms E2 and E3 as there; the five products of the lane are (m, e) = (m1[E2] m2[E3], eK' + e1 + e2).
//                   The wave takes eRef = max e over its CONTRIBUTING lanes (weight > 0: not the comparison individual,
//                   not -N, not beyond n_ids) and adds w ldexp(m, e - eRef) in the order of wave_sum_to_lane63; the chunks'
//                   (sum, eRef) pairs meet in LDS, where one wave per column rescales them to their maximum, adds them one
//                   lane a chunk and then in the same tree, and lane 63 writes log2(mK' sum / n_bg) + eRef.
//                   No ldexp ever leaves the neighbourhood of 1: a term more than 1100 binades below its reference is 0,
//                   i.e. below 2^-1074 of the sum.  The integers do not depend on the layout or the grouping and the
//                   additions have one order: the same bits from either tile layout and for one individual or many.
//   k_win_log_rows  every other column (all three of a non-LD run, LIBD2 of an --LD run): the sum over the window's rows
//                   with reads of log2 of the per-site value ibdg_get_site_ll returns -- k_rows_windows' arithmetic,
//                   operation for operation, DBL_MIN clamp included -- as a double-double (TwoSum), rounded once.
//
// Built with -ffp-contract=off like the rest (TwoSum is exact only without fused multiply-add).
#include "ibdg_kernels.h"
#include "ibdg_ld_dev.h"

#include <hip/hip_runtime.h>

#include <climits>

namespace ibdg {

namespace {

constexpr int LOG_THREADS = 256, LOG_WAVES = LOG_THREADS / 64;
constexpr int NO_EXP = INT_MIN;         // the exponent of a chunk or lane that contributes nothing
constexpr int FAR_BELOW = -1100;        // a term this many binades below its reference is 0 (ldexp of a mantissa <= 1)

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// m 2^(e - ref), ref >= e
__device__ __forceinline__ double rescale(double m, int e, int ref)
{
    const int d = e - ref;
    return __builtin_ldexp(m, d < FAR_BELOW ? FAR_BELOW : d);
}

// (m, e) of rho^E2 sigma^E3 2^eK from the {mantissa, exponent} tables
__device__ __forceinline__ void table_product(const LdLogArgs &a, int eK, uint32_t E2, uint32_t E3, double &m, int &e)
{
    const uint32_t top = a.tab_len - 1;
    const PowEntry p1 = a.pow_rho[E2 < top ? E2 : top], p2 = a.pow_sigma[E3 < top ? E3 : top];
    m = p1.m * p2.m;
    e = eK + p1.e + p2.e;
}

}  // namespace

__global__ __launch_bounds__(LOG_THREADS) void k_ld_log(LdLogArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *cs = reinterpret_cast<double *>(smem);                  // [2][n_chunks] the chunks' sums, IBD0 | IBD1
    int *ce = reinterpret_cast<int *>(cs + 2 * (size_t)a.n_chunks); // [2][n_chunks] and their reference exponents
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x, t = blockIdx.y;
    uint32_t tgt = a.targets[t];
    IBDG_CHECK_TGT(tgt, a.lanes, __func__);
    const WinConst wc = a.wconst[w];
    const uint32_t s0 = wc.seg_begin;
    uint32_t s1 = a.wconst[w + 1].seg_begin;
    s1 = s1 < a.n_segs ? s1 : a.n_segs;
    const uint4 *tbase = a.t32 + (size_t)(tgt >> 6) * a.n_pairs * 64 + (tgt & 63);

    // <t,cov> and <t,alt> of the comparison individual's two haplotypes over the window
    uint32_t TC[2] = {0, 0}, TA[2] = {0, 0};
    for (uint32_t s = s0; s < s1; ++s) {
        const Seg &S = a.segs[s];
        const uint32_t q = S.tile >> 1;
        if (q >= a.n_pairs)
            continue;
        const uint2 tw = reinterpret_cast<const uint2 *>(tbase + (size_t)q * 64)[S.tile & 1];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            TC[0] += (uint32_t)__popc(tw.x & S.cov[k]) << k;
            TC[1] += (uint32_t)__popc(tw.y & S.cov[k]) << k;
            TA[0] += (uint32_t)__popc(tw.x & S.alt[k]) << k;
            TA[1] += (uint32_t)__popc(tw.y & S.alt[k]) << k;
        }
    }
    const uint32_t AT = wc.alt_total;

    for (uint32_t c = wave; c < a.n_chunks; c += LOG_WAVES) {
        uint32_t C[2] = {0, 0}, CH = 0, A[2] = {0, 0}, G[4] = {0, 0, 0, 0};
        const uint4 *cbase = a.t32 + (size_t)c * a.n_pairs * 64 + lane;
        for (uint32_t s = s0; s < s1; ++s) {
            const Seg &S = a.segs[s];               // wave-uniform: scalar loads
            const uint32_t q = S.tile >> 1;
            if (q >= a.n_pairs)
                continue;
            const uint2 x = reinterpret_cast<const uint2 *>(cbase + (size_t)q * 64)[S.tile & 1];
            const uint2 tw = reinterpret_cast<const uint2 *>(tbase + (size_t)q * 64)[S.tile & 1];
            const uint32_t nc = (S.flags >> 16) & 0xff, na = S.flags >> 24;
            for (uint32_t k = 0; k < nc && k < 8; ++k) {
                const uint32_t cov = S.cov[k];
                const uint32_t u0 = x.x & cov, u1 = x.y & cov;
                C[0] += (uint32_t)__popc(u0) << k;
                C[1] += (uint32_t)__popc(u1) << k;
                CH += (uint32_t)__popc(u0 & x.y) << k;
                G[0] += (uint32_t)__popc(u0 & tw.x) << k;
                G[1] += (uint32_t)__popc(u1 & tw.x) << k;
                G[2] += (uint32_t)__popc(u0 & tw.y) << k;
                G[3] += (uint32_t)__popc(u1 & tw.y) << k;
            }
            for (uint32_t k = 0; k < na && k < 8; ++k) {
                const uint32_t alt = S.alt[k];
                A[0] += (uint32_t)__popc(x.x & alt) << k;
                A[1] += (uint32_t)__popc(x.y & alt) << k;
            }
        }
        // the exponents of the header of ibdg_ld_popcount.hip
        //   pDg[x0+x1]:  E3 = C(x0)+C(x1)-2C(x0&x1)        E2 = ALT - A(x0) - A(x1) + C(x0&x1)
        //   pDg[t +x ]:  E3 = <t,cov> + C(x) - 2G(x,t)     E2 = ALT - <t,alt> - A(x) + G(x,t)
        double m0, mq[4];
        int e0, eq[4];
        table_product(a, wc.eK, AT - A[0] - A[1] + CH, C[0] + C[1] - 2 * CH, m0, e0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xh = i & 1, th = i >> 1;
            table_product(a, wc.eK, AT - TA[th] - A[xh] + G[i], TC[th] + C[xh] - 2 * G[i], mq[i], eq[i]);
        }
        const uint32_t id = c * 64 + lane;
        const double wgt = id < a.lanes && id != tgt ? a.base_w[id] : 0.0;      // :714: the comparison individual is excluded
        const bool in = wgt > 0.0;
        // the lane's four IBD1 products at their own maximum (:744-745), then both columns at the wave's
        int e1 = eq[0];
#pragma unroll
        for (int i = 1; i < 4; ++i)
            e1 = eq[i] > e1 ? eq[i] : e1;
        const double q1 = ((rescale(mq[0], eq[0], e1) + rescale(mq[1], eq[1], e1)) + rescale(mq[2], eq[2], e1)) + rescale(mq[3], eq[3], e1);
        const int r0 = wave_max(in ? e0 : NO_EXP), r1 = wave_max(in ? e1 : NO_EXP);
        const double v0 = in ? rescale(wgt * m0, e0, r0) : 0.0;
        const double v1 = in ? rescale(wgt * q1, e1, r1) : 0.0;
        const double t0 = wave_sum_to_lane63(v0), t1 = wave_sum_to_lane63(v1);
        if (lane == 63) {
            cs[c] = t0; ce[c] = r0;
            cs[a.n_chunks + c] = t1; ce[a.n_chunks + c] = r1;
        }
    }
    __syncthreads();
    if (wave < 2) {                     // wave 0: IBD0, wave 1: IBD1
        const double *s = cs + (size_t)wave * a.n_chunks;
        const int *e = ce + (size_t)wave * a.n_chunks;
        int ref = NO_EXP;
        for (uint32_t c = lane; c < a.n_chunks; c += 64)
            ref = e[c] > ref ? e[c] : ref;
        ref = wave_max(ref);
        double sum = 0.0;
        for (uint32_t c = lane; c < a.n_chunks; c += 64)
            if (e[c] != NO_EXP)         // (a chunk without a contributing lane has no exponent to rescale from)
                sum += rescale(s[c], e[c], ref);
        sum = wave_sum_to_lane63(sum);
        if (lane == 63) {
            const int n_bg = a.base_sum - (int)a.base_w[tgt];       // :742-750
            const double mean = (sum * wc.mK) / (double)(wave ? n_bg * 4 : n_bg);     // an empty background: 0 / 0
            a.win_log2[((size_t)t * a.n_win + w) * 3 + wave] = log2(mean) + (double)(ref == NO_EXP ? 0 : ref);
        }
    }
}

size_t ld_log_lds_bytes(uint32_t n_chunks) { return (size_t)n_chunks * 2 * (sizeof(double) + sizeof(int)); }

void launch_ld_log(const LdLogArgs &a, unsigned n_targets, hipStream_t st)
{
    if (a.n_win == 0 || n_targets == 0)
        return;
    hipLaunchKernelGGL(k_ld_log, dim3(a.n_win, n_targets), dim3(LOG_THREADS), ld_log_lds_bytes(a.n_chunks), st, a);
}

// ---------------------------------------------------------------------------
// The row-sum columns
// ---------------------------------------------------------------------------
namespace {

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
    x.hi = s + e;
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

// LIBD0, LIBD1, LIBD2 of covered row j of the site list for individual tgt: rows_turn<ROWS_FULL> of ibdg_kernels.hip,
// operation for operation (src/ibd-math.c:84-142, src/ibdgem.c:643-651)
template <bool ALL>
__device__ __forceinline__ void site_values(const RowsArgs &a, uint32_t tgt, size_t j, double (&v)[3])
{
    const uint2 rc = a.rec_cov[j];
    const double *L = reinterpret_cast<const double *>(reinterpret_cast<const char *>(a.lut) + rc.y);
    const double p00 = L[0], p01 = L[1], p11 = L[2];
    unsigned g;
    if (a.t32) {
        const uint2 *p = reinterpret_cast<const uint2 *>(a.t32 + ((size_t)(tgt >> 6) * a.n_pairs + (rc.x >> 6)) * 64 + (tgt & 63));
        const uint2 tw = p[(rc.x >> 5) & 1];
        g = ((tw.x >> (rc.x & 31)) & 1u) + ((tw.y >> (rc.x & 31)) & 1u);
    } else {
        const uint64_t *row = a.panel + (size_t)rc.x * a.stride;
        g = (unsigned)((row[2 * (tgt >> 6)] >> (tgt & 63)) & 1u) + (unsigned)((row[2 * (tgt >> 6) + 1] >> (tgt & 63)) & 1u);
    }
    v[2] = g == 0 ? p00 : (g == 1 ? p01 : p11);
    if (!ALL)
        return;
    const size_t s = a.cov_site[j];
    const uint32_t k = a.alt_count[rc.x];
    double f = (double)k / (double)(int)(2u * a.n_ids);       // src/ibd-parse.c:98
    double pw1 = a.pow_tab[2 * k], pw2 = a.pow_tab[2 * k + 1];
    if (a.fo) {
        const double fo = a.fo[3 * s];
        if (fo == fo) {                // not NaN: -A override (src/ibdgem.c:609-614)
            f = fo;
            pw1 = a.fo[3 * s + 1];
            pw2 = a.fo[3 * s + 2];
        }
    }
    const double omf = 1 - f;
    double ibd0 = 1.0;
    if (!(p00 == 1 || p01 == 1 || p11 == 1)) {
        const double t1 = pw1 * p00;
        const double t2 = ((2 * omf) * f) * p01;
        const double t3 = pw2 * p11;
        ibd0 = (t1 + t2) + t3;
        if (ibd0 == 0.0)
            ibd0 = 2.2250738585072014e-308;      // DBL_MIN
    }
    double ibd1;
    if (g == 0)
        ibd1 = (f * p01) + (omf * p00);
    else if (g == 1)
        ibd1 = ((0.5 * p01) + ((0.5 * omf) * p00)) + ((0.5 * f) * p11);
    else
        ibd1 = (omf * p01) + (f * p11);
    if (ibd1 == 0.0)
        ibd1 = 2.2250738585072014e-308;
    v[0] = ibd0;
    v[1] = ibd1;
}

}  // namespace

// A wave per (window, comparison individual): its lanes take the window's rows with reads 64 at a time, every log2 enters
// the lane's double-double on its own, the lanes meet in a fixed tree.  ALL: the three columns of a non-LD run; else LIBD2.
template <bool ALL>
__global__ __launch_bounds__(LOG_THREADS) void k_win_log_rows(RowsArgs a, double *__restrict__ win_log2)
{
    const unsigned lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * LOG_WAVES + (threadIdx.x >> 6), t = blockIdx.y;
    if (w >= a.n_win)
        return;
    uint32_t tgt = a.targets[t];
    IBDG_CHECK_TGT(tgt, a.n_ids, __func__);
    const size_t b = (size_t)w * a.window, e = b + a.window < a.n_cov ? b + a.window : a.n_cov;
    DD acc[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    for (size_t j = b + lane; j < e; j += 64) {
        double v[3];
        site_values<ALL>(a, tgt, j, v);
#pragma unroll
        for (int i = ALL ? 0 : 2; i < 3; ++i)
            dd_add_d(acc[i], log2(v[i]));
    }
#pragma unroll
    for (int i = ALL ? 0 : 2; i < 3; ++i) {
        for (int d = 32; d > 0; d >>= 1) {
            DD o;
            o.hi = __shfl_down(acc[i].hi, d, 64);
            o.lo = __shfl_down(acc[i].lo, d, 64);
            dd_add(acc[i], o);
        }
        if (lane == 0)
            win_log2[((size_t)t * a.n_win + w) * 3 + i] = acc[i].hi;
    }
}

void launch_win_log_rows(const RowsArgs &a, unsigned n_targets, double *win_log2, hipStream_t st)
{
    if (a.n_win == 0 || n_targets == 0)
        return;
    const dim3 grid((a.n_win + LOG_WAVES - 1) / LOG_WAVES, n_targets);
    if (a.ld_mode)
        hipLaunchKernelGGL(k_win_log_rows<false>, grid, dim3(LOG_THREADS), 0, st, a, win_log2);
    else
        hipLaunchKernelGGL(k_win_log_rows<true>, grid, dim3(LOG_THREADS), 0, st, a, win_log2);
}

}  // namespace ibdg
