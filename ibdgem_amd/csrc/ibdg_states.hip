// ibdg_states.hip -- IBD-state paths (ibdg_window_log2_states), posteriors (ibdg_window_log2_posteriors, k_log2_posteriors
// below) and segments (ibdg_window_log2_segments, ibdg_get_log2_segments: k_log2_segments_count, k_log2_segments_write at
// the end) over the log2 window table of the last run.  The paths: the integer
// (max, +) recurrence of ibdg_states.h, whose host twin is ibdg_states_host.cpp.  Same integers by construction: the
// emissions are exact products of an fp64 difference, everything behind them is int64 add / compare / select.
//
// k_log2_states: a workgroup of STATES_THREADS per comparison individual, grid-stride over the individuals.  Thread b owns
// windows [b C, (b + 1) C), C = ceil(n_win / STATES_THREADS).
//   pass 1  the block's step matrices A_w[q][s] = pen[q][s] + e_w[s] multiplied (max, +) into one 3 x 3 matrix in LDS (block
//           0 starts from three copies of the row e_0); thread 0 then walks the blocks' matrices in order and leaves every
//           block the exact score vector at the end of the block before it
//   pass 2  the block's windows again from that vector: the sequential recurrence's own scores (written where asked for),
//           `from` as 6 bits per window in the individual's path bytes, and the block's backward map (state at its last
//           window -> state at the last window of the block before)
//   pass 3  the backward maps composed from the last block down (a suffix scan over the 256 maps of 6 bits in LDS), every
//           thread traces its own windows backward, overwriting `from` with the state; the counts meet in LDS
// No atomics.  Reads: a thread walks its own 24-byte rows, lanes 24 C bytes apart (DESIGN 4.8 has the measurement).
#include "ibdg_kernels.h"
#include "ibdg_states.h"

#include <hip/hip_runtime.h>

namespace ibdg {

namespace {

struct Pen {
    int64_t p01, p02, p12;
};

__device__ __forceinline__ void emission(const double *__restrict__ l, int64_t e[3])
{
    const double l0 = l[0], l1 = l[1], l2 = l[2];
    e[0] = e[1] = e[2] = 0;
    if (l0 != l0 || l1 != l1 || l2 != l2)
        return;
    double m = l0 > l1 ? l0 : l1;
    m = m > l2 ? m : l2;
    if (!(m - m == 0.0))                       // +-inf
        return;
    const double v[3] = {l0, l1, l2};
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        double d = v[s] - m;
        d = d < STATES_D_MIN ? STATES_D_MIN : d;
        e[s] = __double2ll_rn(d * STATES_QUANTA);
    }
}

// v'[s] = max_q(v[q] + pen[q][s]) + e[s], lowest q on a tie; returns from[s] in bits 2 s, 2 s + 1
__device__ __forceinline__ unsigned step(int64_t v[3], const int64_t pen[3][3], const int64_t e[3])
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

__device__ __forceinline__ int argmax3(const int64_t v[3])
{
    int m = v[1] > v[0] ? 1 : 0;
    return v[2] > v[m] ? 2 : m;
}

// a map of the three states as 6 bits (state s -> bits 2 s, 2 s + 1); (a after b)(s) = a(b(s))
__device__ __forceinline__ unsigned map_at(unsigned a, unsigned s) { return a >> (2 * s) & 3; }
__device__ __forceinline__ unsigned map_after(unsigned a, unsigned b)
{
    return map_at(a, map_at(b, 0)) | map_at(a, map_at(b, 1)) << 2 | map_at(a, map_at(b, 2)) << 4;
}
constexpr unsigned MAP_ID = 0 | 1 << 2 | 2 << 4;

__global__ __launch_bounds__(STATES_THREADS) void k_log2_states(const double *__restrict__ win_log2, uint32_t n_win,
                                                                uint32_t n_targets, Pen P, uint8_t *__restrict__ path,
                                                                int64_t *__restrict__ score, uint64_t *__restrict__ count)
{
    __shared__ int64_t mat[STATES_THREADS][9];      // 18 KB
    __shared__ int64_t vin[STATES_THREADS][3];      // score vector at the end of the block before
    __shared__ uint8_t maps[2][STATES_THREADS];
    __shared__ uint32_t cnt[STATES_THREADS / 64][3];
    __shared__ int last_state;

    const int64_t pen[3][3] = {{0, P.p01, P.p02}, {P.p01, 0, P.p12}, {P.p02, P.p12, 0}};
    const uint32_t b = threadIdx.x;
    const uint32_t C = (n_win + STATES_THREADS - 1) / STATES_THREADS;
    const uint32_t nbk = (n_win + C - 1) / C;        // blocks that own windows (n_win >= 1)
    const uint64_t w0 = (uint64_t)b * C;
    const uint64_t w1 = w0 + C < n_win ? w0 + C : n_win;
    const bool own = b < nbk;

    for (uint32_t t = blockIdx.x; t < n_targets; t += gridDim.x) {
        const double *tab = win_log2 + (size_t)t * n_win * 3;
        uint8_t *pt = path + (size_t)t * n_win;
        int64_t *sc = score ? score + (size_t)t * n_win * 3 : nullptr;

        // pass 1
        if (own) {
            int64_t r[3][3], e[3];
            emission(tab + 3 * w0, e);
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    r[q][s] = b == 0 ? e[s] : pen[q][s] + e[s];
            for (uint64_t w = w0 + 1; w < w1; ++w) {
                emission(tab + 3 * w, e);
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    (void)step(r[q], pen, e);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    mat[b][3 * q + s] = r[q][s];
        }
        __syncthreads();
        if (b == 0) {
            // block 0's three rows are the score vector at its end
            int64_t v[3] = {mat[0][0], mat[0][1], mat[0][2]};
            for (uint32_t k = 1; k < nbk; ++k) {
                vin[k][0] = v[0], vin[k][1] = v[1], vin[k][2] = v[2];
                int64_t nv[3];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    int64_t best = v[0] + mat[k][s];
#pragma unroll
                    for (int q = 1; q < 3; ++q) {
                        const int64_t c = v[q] + mat[k][3 * q + s];
                        best = c > best ? c : best;
                    }
                    nv[s] = best;
                }
                v[0] = nv[0], v[1] = nv[1], v[2] = nv[2];
            }
            last_state = argmax3(v);
        }
        __syncthreads();

        // pass 2
        unsigned back = MAP_ID;
        if (own) {
            int64_t v[3], e[3];
            uint64_t w = w0;
            if (b == 0) {
                emission(tab, v);
                pt[0] = (uint8_t)MAP_ID;
                if (sc)
                    sc[0] = v[0], sc[1] = v[1], sc[2] = v[2];
                w = 1;
            } else {
                v[0] = vin[b][0], v[1] = vin[b][1], v[2] = vin[b][2];
            }
            for (; w < w1; ++w) {
                emission(tab + 3 * w, e);
                const unsigned f = step(v, pen, e);
                pt[w] = (uint8_t)f;
                if (sc)
                    sc[3 * w] = v[0], sc[3 * w + 1] = v[1], sc[3 * w + 2] = v[2];
                back = map_after(back, f);         // state at w -> state at w0 - 1 (block 0: at window 0)
            }
        }
        maps[0][b] = (uint8_t)back;
        __syncthreads();

        // pass 3: maps[..][k] becomes block k's map after block k + 1's after ... after the last block's
        int cur = 0;
        for (uint32_t d = 1; d < STATES_THREADS; d <<= 1) {
            unsigned m = maps[cur][b];
            if (b + d < STATES_THREADS)
                m = map_after(m, maps[cur][b + d]);
            maps[cur ^ 1][b] = (uint8_t)m;
            cur ^= 1;
            __syncthreads();
        }
        uint32_t n[3] = {0, 0, 0};
        if (own) {
            // the state at this block's last window: the last block's is the best final score's, any other's is what the
            // blocks behind it map that one to
            unsigned st = b + 1 == nbk ? (unsigned)last_state : map_at(maps[cur][b + 1], (unsigned)last_state);
            for (uint64_t w = w1; w-- > w0;) {
                const unsigned f = pt[w];
                pt[w] = (uint8_t)st;
                n[0] += st == 0, n[1] += st == 1, n[2] += st == 2;
                st = map_at(f, st);
            }
        }
#pragma unroll
        for (int s = 0; s < 3; ++s)
            for (int d = 32; d > 0; d >>= 1)
                n[s] += __shfl_down(n[s], d, 64);
        if ((b & 63) == 0)
            cnt[b >> 6][0] = n[0], cnt[b >> 6][1] = n[1], cnt[b >> 6][2] = n[2];
        __syncthreads();
        if (b < 3) {
            uint64_t sum = 0;
            for (int k = 0; k < STATES_THREADS / 64; ++k)
                sum += cnt[k][b];
            count[(size_t)t * 3 + b] = sum;
        }
        __syncthreads();       // (LDS is reused by the next individual)
    }
}

struct PenW {
    double a[3];      // the weights of P_01, P_02, P_12 (post_penalty_weights)
};

__device__ __forceinline__ void emission_weights(const double *__restrict__ l, const double *T, double b[3])
{
    int64_t e[3];
    emission(l, e);
#pragma unroll
    for (int s = 0; s < 3; ++s)
        b[s] = post_weight(e[s], T, T + 256);
}

// k_log2_posteriors: the sum-product pass of ibdg_states.h (its steps 1 .. 5 are the numbers below), same launch and blocking
// as k_log2_states.  scr [T][n_win][3] holds beta_w from step 3 to step 4, which overwrites it with gamma_w: the thread
// that wrote a row is the one that reads it.  out [T][5] = expect[3], Z's mantissa, Z's exponent (as a double).  The walks of
// step 2 run in two waves side by side (thread 0 forward, thread 64 backward).  No atomics; the same reads as k_log2_states,
// three times.
__global__ __launch_bounds__(STATES_THREADS) void k_log2_posteriors(const double *__restrict__ win_log2, uint32_t n_win,
                                                                    uint32_t n_targets, PenW W, const double *__restrict__ tables,
                                                                    double *__restrict__ scr, double *__restrict__ out)
{
    __shared__ double mat[STATES_THREADS][9];       // 18 KB: B_b
    __shared__ double fin[STATES_THREADS][3];       // F_b
    __shared__ double gout[STATES_THREADS][3];      // G_b
    __shared__ double part[STATES_THREADS][3];
    __shared__ double T[512];                       // T1, T2
    __shared__ int mexp[STATES_THREADS], fexp[STATES_THREADS];

    const uint32_t b = threadIdx.x;
    const uint32_t C = (n_win + STATES_THREADS - 1) / STATES_THREADS;
    const uint32_t nbk = (n_win + C - 1) / C;
    const uint64_t w0 = (uint64_t)b * C;
    const uint64_t w1 = w0 + C < n_win ? w0 + C : n_win;
    const bool own = b < nbk;
    const double a[3] = {W.a[0], W.a[1], W.a[2]};

    T[b] = tables[b], T[b + STATES_THREADS] = tables[b + STATES_THREADS];
    __syncthreads();

    for (uint32_t t = blockIdx.x; t < n_targets; t += gridDim.x) {
        const double *tab = win_log2 + (size_t)t * n_win * 3;
        double *sc = scr + (size_t)t * n_win * 3;

        // 1
        if (own) {
            double R[9], bw[3], M[9];
            int e = 0;
            emission_weights(tab + 3 * w0, T, bw);
            if (b == 0) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    R[3 * q] = bw[0], R[3 * q + 1] = bw[1], R[3 * q + 2] = bw[2];
            } else {
                post_step_matrix(a, bw, R);
            }
            for (uint64_t w = w0 + 1; w < w1; ++w) {
                emission_weights(tab + 3 * w, T, bw);
                post_step_matrix(a, bw, M);
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    post_vec_mat(R + 3 * q, M);
                post_rescale<9>(R, e);
            }
#pragma unroll
            for (int i = 0; i < 9; ++i)
                mat[b][i] = R[i];
            mexp[b] = e;
        }
        __syncthreads();
        // 2
        if (b == 0) {
            double v[3] = {mat[0][0], mat[0][1], mat[0][2]};
            int e = mexp[0];
            for (uint32_t k = 1; k < nbk; ++k) {
                fin[k][0] = v[0], fin[k][1] = v[1], fin[k][2] = v[2];
                fexp[k] = e;
                if (k + 1 < nbk) {
                    double M[9];
#pragma unroll
                    for (int i = 0; i < 9; ++i)
                        M[i] = mat[k][i];
                    post_vec_mat(v, M);
                    e += mexp[k];
                    post_rescale<3>(v, e);
                }
            }
        } else if (b == 64) {
            double g[3] = {1.0, 1.0, 1.0};
            int ge = 0;
            for (uint32_t k = nbk; k-- > 0;) {
                gout[k][0] = g[0], gout[k][1] = g[1], gout[k][2] = g[2];
                if (k > 0) {
                    double M[9];
#pragma unroll
                    for (int i = 0; i < 9; ++i)
                        M[i] = mat[k][i];
                    post_mat_vec(M, g);
                    post_rescale<3>(g, ge);
                }
            }
        }
        __syncthreads();
        double acc[3] = {0.0, 0.0, 0.0};
        if (own) {
            double bw[3], M[9];
            // 3
            double be[3] = {gout[b][0], gout[b][1], gout[b][2]};
            int ge = 0;
            for (uint64_t w = w1; w-- > w0;) {
                sc[3 * w] = be[0], sc[3 * w + 1] = be[1], sc[3 * w + 2] = be[2];
                if (w > w0) {
                    emission_weights(tab + 3 * w, T, bw);
                    post_step_matrix(a, bw, M);
                    post_mat_vec(M, be);
                    post_rescale<3>(be, ge);
                }
            }
            // 4
            double v[3] = {fin[b][0], fin[b][1], fin[b][2]};
            int e = fexp[b];
            for (uint64_t w = w0; w < w1; ++w) {
                emission_weights(tab + 3 * w, T, bw);
                if (w == 0) {
                    v[0] = bw[0], v[1] = bw[1], v[2] = bw[2];
                    e = 0;
                } else {
                    post_step_matrix(a, bw, M);
                    post_vec_mat(v, M);
                    post_rescale<3>(v, e);
                }
                const double p0 = v[0] * sc[3 * w], p1 = v[1] * sc[3 * w + 1], p2 = v[2] * sc[3 * w + 2];
                const double D = (p0 + p1) + p2;
                const double g0 = p0 / D, g1 = p1 / D, g2 = p2 / D;
                sc[3 * w] = g0, sc[3 * w + 1] = g1, sc[3 * w + 2] = g2;
                acc[0] += g0, acc[1] += g1, acc[2] += g2;
                if (w + 1 == n_win)
                    out[(size_t)t * 5 + 3] = D, out[(size_t)t * 5 + 4] = (double)e;
            }
        }
        // 5
        part[b][0] = acc[0], part[b][1] = acc[1], part[b][2] = acc[2];
        __syncthreads();
        for (uint32_t d = STATES_THREADS / 2; d > 0; d >>= 1) {
            if (b < d) {
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    part[b][s] = part[b][s] + part[b + d][s];
            }
            __syncthreads();
        }
        if (b < 3)
            out[(size_t)t * 5 + b] = part[0][b];
        __syncthreads();       // (LDS is reused by the next individual)
    }
}

// ---- segments (ibdg_states.h): same launch and blocking as the two kernels above -------------------------------
// A window starts a segment iff its state differs from the window's before it (window 0 always: 3 stands for "no state").

// k_log2_segments_count: out [T][13] = the summary's 12 words, then the individual's number of segments.  path as
// k_log2_states left it.  Every thread finds the first start among its windows; a suffix minimum over the 256 blocks in LDS gives
// each the next start behind its block (n_win if none), so a backward walk over its own windows knows where every segment
// that starts there ends.  Sums and maxima by shuffles, then over the four waves in LDS.  No atomics.
__global__ __launch_bounds__(STATES_THREADS) void k_log2_segments_count(const uint8_t *__restrict__ path, uint32_t n_win,
                                                                        uint32_t n_targets, const uint64_t *__restrict__ pos_first,
                                                                        const uint64_t *__restrict__ pos_last,
                                                                        uint64_t *__restrict__ out)
{
    __shared__ uint32_t nxt[2][STATES_THREADS];
    __shared__ uint64_t red[STATES_THREADS / 64][12];

    const uint32_t b = threadIdx.x;
    const uint32_t C = (n_win + STATES_THREADS - 1) / STATES_THREADS;
    const uint32_t nbk = (n_win + C - 1) / C;
    const uint32_t w0 = b * C < n_win ? b * C : n_win;
    const uint32_t w1 = w0 + C < n_win ? w0 + C : n_win;
    const bool own = b < nbk;

    for (uint32_t t = blockIdx.x; t < n_targets; t += gridDim.x) {
        const uint8_t *pt = path + (size_t)t * n_win;
        uint32_t fs = n_win;
        if (own) {
            unsigned prev = b == 0 ? 3u : pt[w0 - 1];
            for (uint32_t w = w0; w < w1; ++w) {
                const unsigned s = pt[w];
                if (s != prev) {
                    fs = w;
                    break;
                }
                prev = s;
            }
        }
        nxt[0][b] = fs;
        __syncthreads();
        // nxt[..][k] becomes the first start in block k or behind it
        int cur = 0;
        for (uint32_t d = 1; d < STATES_THREADS; d <<= 1) {
            uint32_t m = nxt[cur][b];
            if (b + d < STATES_THREADS) {
                const uint32_t o = nxt[cur][b + d];
                m = o < m ? o : m;
            }
            nxt[cur ^ 1][b] = m;
            cur ^= 1;
            __syncthreads();
        }
        uint64_t v[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (own) {
            uint32_t end = b + 1 < STATES_THREADS ? nxt[cur][b + 1] : n_win;     // where the segment at hand ends (exclusive)
            unsigned s = pt[w1 - 1];
            for (uint32_t w = w1; w-- > w0;) {
                const unsigned p = w == 0 ? 3u : pt[w - 1];
                if (p != s) {
                    const uint64_t len = end - w;
                    const uint64_t span = pos_first ? pos_last[end - 1] - pos_first[w] + 1 : 0;
#pragma unroll
                    for (unsigned k = 0; k < 3; ++k) {
                        const bool is = s == k;
                        v[k] += is;
                        v[3 + k] = is && len > v[3 + k] ? len : v[3 + k];
                        v[6 + k] += is ? span : 0;
                        v[9 + k] = is && span > v[9 + k] ? span : v[9 + k];
                    }
                    end = w;
                }
                s = p;
            }
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            for (int d = 32; d > 0; d >>= 1) {
                const uint64_t o = __shfl_down((unsigned long long)v[i], d, 64);
                v[i] = (i / 3 & 1) ? (o > v[i] ? o : v[i]) : v[i] + o;
            }
            if ((b & 63) == 0)
                red[b >> 6][i] = v[i];
        }
        __syncthreads();
        if (b < 13) {
            uint64_t r = 0;
            if (b < 12) {
                for (int k = 0; k < STATES_THREADS / 64; ++k)
                    r = (b / 3 & 1) ? (red[k][b] > r ? red[k][b] : r) : r + red[k][b];
            } else {
                for (int k = 0; k < STATES_THREADS / 64; ++k)
                    r += red[k][0] + red[k][1] + red[k][2];
            }
            out[(size_t)t * 13 + b] = r;
        }
        __syncthreads();       // (LDS is reused by the next individual)
    }
}

struct SegAcc {
    int64_t e[3];
    uint64_t q;
    double mn;
};

__device__ __forceinline__ void seg_reset(SegAcc &a)
{
    a.e[0] = a.e[1] = a.e[2] = 0;
    a.q = 0;
    a.mn = __builtin_inf();
}

__device__ __forceinline__ void seg_record(ibdg_segment *__restrict__ r, uint32_t first, uint32_t n, unsigned state, const SegAcc &a,
                                           bool with_post)
{
    r->first = first, r->n_win = n, r->state = state, r->reserved = 0;
    r->e[0] = a.e[0], r->e[1] = a.e[1], r->e[2] = a.e[2];
    r->post_q = a.q;
    r->post_min = with_post ? a.mn : 0.0;
}

// k_log2_segments_write: the records, individual t's from seg[off[t]] on in window order (off: the exclusive sums of the counts
// of k_log2_segments_count over the same paths).  post: gamma as k_log2_posteriors left it, or NULL.  A thread walks its windows
// once with one accumulator: at a start it is the block's head (the windows before its first start: they belong to a segment
// that started in an earlier block) or the total of a segment that lies inside the block, which is written there and then;
// at the block's end it is the tail of the block's last segment (or the head, if the block has no start).  An inclusive scan
// of the blocks' start counts gives every thread the index of its first record.  The owner of a tail then adds the heads of
// the blocks behind it, up to and with the first one that has a start -- a segment may cover any number of whole blocks --
// and writes that record.  No atomics: every record has one writer, every head one reader.
__global__ __launch_bounds__(STATES_THREADS) void k_log2_segments_write(const double *__restrict__ win_log2,
                                                                        const uint8_t *__restrict__ path,
                                                                        const double *__restrict__ post, uint32_t n_win,
                                                                        uint32_t n_targets, const uint64_t *__restrict__ off,
                                                                        ibdg_segment *__restrict__ seg)
{
    __shared__ int64_t hd_e[STATES_THREADS][3];
    __shared__ uint64_t hd_q[STATES_THREADS];
    __shared__ double hd_mn[STATES_THREADS];
    __shared__ uint32_t fst[STATES_THREADS];            // the block's first start, n_win if it has none
    __shared__ uint32_t cnt[2][STATES_THREADS];

    const uint32_t b = threadIdx.x;
    const uint32_t C = (n_win + STATES_THREADS - 1) / STATES_THREADS;
    const uint32_t nbk = (n_win + C - 1) / C;
    const uint32_t w0 = b * C < n_win ? b * C : n_win;
    const uint32_t w1 = w0 + C < n_win ? w0 + C : n_win;
    const bool own = b < nbk;
    const bool with_post = post != nullptr;
    constexpr uint32_t NONE = 0xffffffffu;

    for (uint32_t t = blockIdx.x; t < n_targets; t += gridDim.x) {
        const double *tab = win_log2 + (size_t)t * n_win * 3;
        const uint8_t *pt = path + (size_t)t * n_win;
        const double *po = with_post ? post + (size_t)t * n_win * 3 : nullptr;
        ibdg_segment *out = seg + off[t];

        uint32_t ns = 0, fs = n_win;
        const unsigned before = !own || b == 0 ? 3u : pt[w0 - 1];
        if (own) {
            unsigned prev = before;
            for (uint32_t w = w0; w < w1; ++w) {
                const unsigned s = pt[w];
                if (s != prev) {
                    fs = ns ? fs : w;
                    ++ns;
                }
                prev = s;
            }
        }
        cnt[0][b] = ns;
        fst[b] = fs;
        __syncthreads();
        int cur = 0;
        for (uint32_t d = 1; d < STATES_THREADS; d <<= 1) {
            uint32_t m = cnt[cur][b];
            if (b >= d)
                m += cnt[cur][b - d];
            cnt[cur ^ 1][b] = m;
            cur ^= 1;
            __syncthreads();
        }
        uint32_t k = cnt[cur][b] - ns;                  // the block's first record
        SegAcc a;
        seg_reset(a);
        uint32_t start = NONE;
        unsigned state = 0;
        bool head_out = false;
        if (own) {
            unsigned prev = before;
            for (uint32_t w = w0; w < w1; ++w) {
                const unsigned s = pt[w];
                if (s != prev) {
                    if (start == NONE) {
                        hd_e[b][0] = a.e[0], hd_e[b][1] = a.e[1], hd_e[b][2] = a.e[2];
                        hd_q[b] = a.q, hd_mn[b] = a.mn;
                        head_out = true;
                    } else {
                        seg_record(out + k, start, w - start, state, a, with_post);
                        ++k;
                    }
                    seg_reset(a);
                    start = w, state = s;
                }
                prev = s;
                int64_t e[3];
                emission(tab + 3 * (size_t)w, e);
                a.e[0] += e[0], a.e[1] += e[1], a.e[2] += e[2];
                if (with_post) {
                    const double g = po[3 * (size_t)w + s];
                    a.q += (uint64_t)__double2ll_rn(g * SEG_POST_Q);
                    a.mn = g < a.mn ? g : a.mn;
                }
            }
        }
        if (!head_out) {                                // no start: all of the block (nothing, for a block without windows)
            hd_e[b][0] = a.e[0], hd_e[b][1] = a.e[1], hd_e[b][2] = a.e[2];
            hd_q[b] = a.q, hd_mn[b] = a.mn;
        }
        __syncthreads();
        if (start != NONE) {
            uint32_t end = n_win;
            for (uint32_t j = b + 1; j < nbk; ++j) {
                a.e[0] += hd_e[j][0], a.e[1] += hd_e[j][1], a.e[2] += hd_e[j][2];
                a.q += hd_q[j];
                a.mn = hd_mn[j] < a.mn ? hd_mn[j] : a.mn;
                if (fst[j] != n_win) {
                    end = fst[j];
                    break;
                }
            }
            seg_record(out + k, start, end - start, state, a, with_post);
        }
        __syncthreads();       // (LDS is reused by the next individual)
    }
}

}  // namespace

void launch_log2_states(const double *win_log2, uint32_t n_win, uint32_t n_targets, const int64_t P[3], uint8_t *path,
                        int64_t *score, uint64_t *count, hipStream_t st)
{
    if (n_win == 0 || n_targets == 0)
        return;
    const uint32_t grid = n_targets < STATES_MAX_BLOCKS ? n_targets : STATES_MAX_BLOCKS;
    hipLaunchKernelGGL(k_log2_states, dim3(grid), dim3(STATES_THREADS), 0, st, win_log2, n_win, n_targets, Pen{P[0], P[1], P[2]},
                       path, score, count);
}

void launch_log2_posteriors(const double *win_log2, uint32_t n_win, uint32_t n_targets, const double a[3], const double *tables,
                            double *scr, double *out, hipStream_t st)
{
    if (n_win == 0 || n_targets == 0)
        return;
    const uint32_t grid = n_targets < STATES_MAX_BLOCKS ? n_targets : STATES_MAX_BLOCKS;
    hipLaunchKernelGGL(k_log2_posteriors, dim3(grid), dim3(STATES_THREADS), 0, st, win_log2, n_win, n_targets, PenW{{a[0], a[1], a[2]}},
                       tables, scr, out);
}

void launch_log2_segments_count(const uint8_t *path, uint32_t n_win, uint32_t n_targets, const uint64_t *pos_first,
                                const uint64_t *pos_last, uint64_t *out, hipStream_t st)
{
    if (n_win == 0 || n_targets == 0)
        return;
    const uint32_t grid = n_targets < STATES_MAX_BLOCKS ? n_targets : STATES_MAX_BLOCKS;
    hipLaunchKernelGGL(k_log2_segments_count, dim3(grid), dim3(STATES_THREADS), 0, st, path, n_win, n_targets, pos_first, pos_last, out);
}

void launch_log2_segments_write(const double *win_log2, const uint8_t *path, const double *post, uint32_t n_win, uint32_t n_targets,
                                const uint64_t *off, ibdg_segment *seg, hipStream_t st)
{
    if (n_win == 0 || n_targets == 0)
        return;
    const uint32_t grid = n_targets < STATES_MAX_BLOCKS ? n_targets : STATES_MAX_BLOCKS;
    hipLaunchKernelGGL(k_log2_segments_write, dim3(grid), dim3(STATES_THREADS), 0, st, win_log2, path, post, n_win, n_targets, off,
                       seg);
}

}  // namespace ibdg
