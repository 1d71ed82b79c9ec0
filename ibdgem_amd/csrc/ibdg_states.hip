// ibdg_states.hip -- IBD-state paths (ibdg_window_log2_states), posteriors (ibdg_window_log2_posteriors, k_log2_posteriors
// below) and segments (ibdg_window_log2_segments, ibdg_get_log2_segments: k_log2_segments_count, k_log2_segments_write at
// the end) over the log2 window table of the last run.  ibdg_states.h has the definition and every step of it as a function:
// the kernels here are its parallel callers, the host twin (ibdg_states_host.cpp) the serial one, so both give the same bits.
// Only here: how a workgroup cuts the windows among its threads and joins their results (scan_lds, join_threads).
// Paths drawn from the posterior (ibdg_window_log2_samples: k_log2_alpha, k_log2_sample_paths, k_log2_sample_records, behind the
// segment kernels) use the same blocking, a workgroup per (individual, draw) pair.
// The switches (ibdg_window_log2_switches: k_log2_switches, behind those) are the posteriors' kernel with another forward pass.
// The fit's pass (ibdg_log2_store_switches: k_log2_switch_expect, behind it) is that kernel over a table store, with the beta
// scratch of the launched workgroups in place of every individual's.
//
// k_log2_states: a workgroup of STATES_THREADS per comparison individual, grid-stride over the individuals.  Thread b owns
// windows [b C, (b + 1) C), C = ceil(n_win / STATES_THREADS) (Blocks).
//   pass 1  the block's step matrices A_w[q][s] = pen[q][s] + e_w[s] multiplied (max, +) into one 3 x 3 matrix in LDS (block
//           0 starts from three copies of the row e_0); thread 0 then walks the blocks' matrices in order and leaves every
//           block the exact score vector at the end of the block before it
//   pass 2  the block's windows again from that vector: the sequential recurrence's own scores (written where asked for),
//           `from` as 6 bits per window in the individual's path bytes, and the block's backward map (state at its last
//           window -> state at the last window of the block before)
//   pass 3  the backward maps composed from the last block down (a suffix scan over the 256 maps of 6 bits in LDS), every
//           thread traces its own windows backward, overwriting `from` with the state; the counts meet in LDS
// No atomics.  Reads: a thread walks its own 24-byte rows, lanes 24 C bytes apart (DESIGN 4.8 has the measurement).
// Chains: all four kernels take the starts' mask, or NULL; a thread reads the bits of its own windows
// (chain_start) and takes a start's penalties, weights or segment border by a select.  Each kernel has two instantiations,
// picked by the launch: CH = false for a NULL mask, in which every question about a start folds to "no" at compile time -- the
// code of the kernels before there were chains --, and CH = true, which knows its mask is there and asks without a branch
// (chains_of below).
// Step shifts: k_log2_states and k_log2_posteriors take the windows' shifts [n_win], or NULL, as a second switch
// SH of their instantiation (steps_of below): SH = false is the code above to the instruction, SH = true reads a window's shift
// one window ahead of the step that uses it -- the address waits for nothing the recurrence makes -- and forms the window's
// penalties (states_window_penalties) or weights (post_window_matrix) from the integers.  Steps without chains are the
// instantiation <false, true>, not a zero mask: no mask to allocate, and no read of one.  The segment kernels read no shift.
#include "ibdg_kernels.h"
#include "ibdg_states.h"

#include <hip/hip_runtime.h>

namespace ibdg {

namespace {

static_assert(STATES_THREADS == STATES_BLOCKS, "a thread per block of windows");

struct Pen {
    int64_t p01, p02, p12;
};

// Scans one value per thread with op (associative) through the double-buffered LDS array buf, 8 steps of all threads: entry b
// becomes op(b, b + 1, .., 255) (BACK) or op(0, .., b - 1, b).  Returns the buffer that holds the result, behind a barrier.
template <bool BACK, typename T, typename Op>
__device__ __forceinline__ int scan_lds(T (*buf)[STATES_THREADS], uint32_t b, T mine, Op op)
{
    buf[0][b] = mine;
    __syncthreads();
    int cur = 0;
    for (uint32_t d = 1; d < STATES_THREADS; d <<= 1) {
        T m = buf[cur][b];
        if (BACK ? b + d < STATES_THREADS : b >= d)
            m = BACK ? (T)op(m, buf[cur][b + d]) : (T)op(buf[cur][b - d], m);
        buf[cur ^ 1][b] = m;
        cur ^= 1;
        __syncthreads();
    }
    return cur;
}

// v[0..N) joined over the workgroup's threads with op(i, x, y) (associative, commutative, 0 neutral): by shuffles within a wave,
// then over the waves' results in red (LDS), behind a barrier.  Thread i < N returns word i's result.
template <int N, typename T, typename Op>
__device__ __forceinline__ T join_threads(T (&v)[N], T (*red)[N], uint32_t b, Op op)
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        for (int d = 32; d > 0; d >>= 1)
            v[i] = op(i, v[i], __shfl_down(v[i], d, 64));
        if ((b & 63) == 0)
            red[b >> 6][i] = v[i];
    }
    __syncthreads();
    T r = 0;
    if (b < N)
        for (int k = 0; k < STATES_THREADS / 64; ++k)
            r = op((int)b, r, red[k][b]);
    return r;
}

// the mask as instantiation CH sees it: a NULL the compiler knows about, or a pointer it may load from without asking
template <bool CH>
__device__ __forceinline__ const uint32_t *chains_of(const uint32_t *starts)
{
    if (!CH)
        return nullptr;
    __builtin_assume(starts != nullptr);
    return starts;
}

// the shifts as instantiation SH sees them, in the same way
template <bool SH>
__device__ __forceinline__ const int32_t *steps_of(const int32_t *shift)
{
    if (!SH)
        return nullptr;
    __builtin_assume(shift != nullptr);
    return shift;
}

template <bool CH, bool SH>
__global__ __launch_bounds__(STATES_THREADS) void k_log2_states(const double *__restrict__ win_log2, uint32_t n_win,
                                                                uint32_t n_targets, Pen P, const uint32_t *__restrict__ starts_arg,
                                                                const int32_t *__restrict__ shift_arg, uint8_t *__restrict__ path,
                                                                int64_t *__restrict__ score, uint64_t *__restrict__ count)
{
    const uint32_t *__restrict__ starts = chains_of<CH>(starts_arg);
    const int32_t *__restrict__ shift = steps_of<SH>(shift_arg);
    __shared__ int64_t mat[STATES_THREADS][3][3];   // 18 KB
    __shared__ int64_t vin[STATES_THREADS][3];      // score vector at the end of the block before
    __shared__ uint8_t maps[2][STATES_THREADS];
    __shared__ uint32_t cnt[STATES_THREADS / 64][3];
    __shared__ int last_state;

    const int64_t Pq[3] = {P.p01, P.p02, P.p12};
    const int64_t none[3] = {0, 0, 0};
    const uint32_t b = threadIdx.x;
    const Blocks B(n_win);                           // (n_win >= 1)
    const uint32_t w0 = B.begin(b), w1 = B.end(b);
    const bool own = b < B.nbk;
    // the shift of window w of this block, read a window ahead: the last window's stands in behind the block's end (own: w0 < w1)
    const auto shift_at = [&](uint32_t w) { return step_shift(shift, w < w1 ? w : w1 - 1); };

    for (uint32_t t = blockIdx.x; t < n_targets; t += gridDim.x) {
        const double *tab = win_log2 + (size_t)t * n_win * 3;
        uint8_t *pt = path + (size_t)t * n_win;
        int64_t *sc = score ? score + (size_t)t * n_win * 3 : nullptr;

        // pass 1
        if (own) {
            int64_t r[3][3], e[3];
            states_emission(tab + 3 * (size_t)w0, e);
            const bool first = b == 0 || chain_start(starts, w0);      // no penalty into the block's first window
            int64_t Pw[3];                                              // (else window w0's own penalties)
            states_window_penalties(Pq, false, SH, shift_at(w0), Pw);
            int32_t sh = shift_at(w0 + 1);
            const int64_t pen[3][3] = {{0, Pw[0], Pw[1]}, {Pw[0], 0, Pw[2]}, {Pw[1], Pw[2], 0}};
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    r[q][s] = first ? e[s] : pen[q][s] + e[s];
            for (uint32_t w = w0 + 1; w < w1; ++w) {
                const int32_t sh_next = shift_at(w + 1);
                states_emission(tab + 3 * (size_t)w, e);
                const bool st = chain_start(starts, w);
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    (void)states_shift_step(r[q], Pq, e, st, SH, sh);
                sh = sh_next;
            }
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    mat[b][q][s] = r[q][s];
        }
        __syncthreads();
        if (b == 0) {
            // block 0's three rows are the score vector at its end; a block's matrix steps a vector like penalties without an emission
            int64_t v[3] = {mat[0][0][0], mat[0][0][1], mat[0][0][2]};
            for (uint32_t k = 1; k < B.nbk; ++k) {
                vin[k][0] = v[0], vin[k][1] = v[1], vin[k][2] = v[2];
                (void)states_step(v, mat[k], none);
            }
            last_state = argmax3(v);
        }
        __syncthreads();

        // pass 2
        unsigned back = MAP_ID;
        if (own) {
            int64_t v[3], e[3];
            uint32_t w = w0;
            if (b == 0) {
                states_emission(tab, v);
                pt[0] = (uint8_t)MAP_ID;
                if (sc)
                    sc[0] = v[0], sc[1] = v[1], sc[2] = v[2];
                w = 1;
            } else {
                v[0] = vin[b][0], v[1] = vin[b][1], v[2] = vin[b][2];
            }
            int32_t sh = shift_at(w);
            for (; w < w1; ++w) {
                const int32_t sh_next = shift_at(w + 1);
                states_emission(tab + 3 * (size_t)w, e);
                const unsigned f = states_shift_step(v, Pq, e, chain_start(starts, w), SH, sh);
                sh = sh_next;
                pt[w] = (uint8_t)f;
                if (sc)
                    sc[3 * (size_t)w] = v[0], sc[3 * (size_t)w + 1] = v[1], sc[3 * (size_t)w + 2] = v[2];
                back = map_after(back, f);         // state at w -> state at w0 - 1 (block 0: at window 0)
            }
        }
        // pass 3: maps[..][k] becomes block k's map after block k + 1's after ... after the last block's
        const int cur = scan_lds<true>(maps, b, (uint8_t)back, [](unsigned x, unsigned y) { return map_after(x, y); });
        uint32_t n[3] = {0, 0, 0};
        if (own) {
            // the state at this block's last window: the last block's is the best final score's, any other's is what the
            // blocks behind it map that one to
            unsigned st = b + 1 == B.nbk ? (unsigned)last_state : map_at(maps[cur][b + 1], (unsigned)last_state);
            for (uint32_t w = w1; w-- > w0;) {
                const unsigned f = pt[w];
                pt[w] = (uint8_t)st;
                n[0] += st == 0, n[1] += st == 1, n[2] += st == 2;
                st = map_at(f, st);
            }
        }
        const uint32_t sum = join_threads(n, cnt, b, [](int, uint32_t x, uint32_t y) { return x + y; });
        if (b < 3)
            count[(size_t)t * 3 + b] = sum;
        __syncthreads();       // (LDS is reused by the next individual)
    }
}

struct PenW {
    double a[3];      // the weights of P_01, P_02, P_12 (post_penalty_weights)
    int64_t P[3];     // ... and the integers themselves, which a window with a shift forms its own weights from
};

// k_log2_posteriors: the sum-product pass of ibdg_states.h (steps 1 .. 4 are its functions, called per thread with pointers into
// LDS; step 5 is the tree below), same launch and blocking as k_log2_states.  scr [T][n_win][3] holds beta_w from step 3 to step
// 4, which overwrites it with gamma_w: the thread that wrote a row is the one that reads it.  starts: the chains' mask or NULL
// (PostIn carries it to the steps), shift: the step shifts or NULL (likewise).  out [T][5] = expect[3], Z's
// mantissa, Z's exponent (as a double).  The walks of step 2 run in two waves side by side (thread 0 forward, thread 64
// backward).  No atomics; the same reads as k_log2_states, three times.
template <bool CH, bool SH>
__global__ __launch_bounds__(STATES_THREADS) void k_log2_posteriors(const double *__restrict__ win_log2, uint32_t n_win,
                                                                    uint32_t n_targets, PenW W, const double *__restrict__ tables,
                                                                    const uint32_t *__restrict__ starts_arg,
                                                                    const int32_t *__restrict__ shift_arg,
                                                                    double *__restrict__ scr, double *__restrict__ out)
{
    const uint32_t *__restrict__ starts = chains_of<CH>(starts_arg);
    const int32_t *__restrict__ shift = steps_of<SH>(shift_arg);
    __shared__ double mat[STATES_THREADS][9];       // 18 KB: B_b
    __shared__ double fin[STATES_THREADS][3];       // F_b
    __shared__ double gout[STATES_THREADS][3];      // G_b
    __shared__ double part[STATES_THREADS][3];
    __shared__ double T[512];                       // T1, T2
    __shared__ int mexp[STATES_THREADS], fexp[STATES_THREADS];

    const uint32_t b = threadIdx.x;
    const Blocks B(n_win);
    const uint32_t w0 = B.begin(b), w1 = B.end(b);
    const bool own = b < B.nbk;

    T[b] = tables[b], T[b + STATES_THREADS] = tables[b + STATES_THREADS];
    __syncthreads();

    for (uint32_t t = blockIdx.x; t < n_targets; t += gridDim.x) {
        const PostIn in = {win_log2 + (size_t)t * n_win * 3, T, {W.a[0], W.a[1], W.a[2]}, starts, shift,
                           {W.P[0], W.P[1], W.P[2]}};
        // 1
        if (own)
            post_block_matrix(in, w0, w1, mat[b], &mexp[b]);
        __syncthreads();
        // 2
        if (b == 0)
            post_forward_walk(mat[0], mexp, B.nbk, fin[0], fexp);
        else if (b == 64)
            post_backward_walk(mat[0], B.nbk, gout[0]);
        __syncthreads();
        // 3, 4
        double acc[3] = {0.0, 0.0, 0.0}, D;
        int e;
        if (own) {
            post_block_gamma(in, w0, w1, gout[b], fin[b], fexp[b], scr + (size_t)t * n_win * 3, acc, &D, &e);
            if (w1 == n_win)
                out[(size_t)t * 5 + 3] = D, out[(size_t)t * 5 + 4] = (double)e;
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
// A window starts a segment iff its state differs from the window's before it (window 0 always: 3 stands for "no state") or it
// starts a chain (seg_start; starts: the chains' mask or NULL).

// k_log2_segments_count: out [T][13] = the summary's 12 words, then the individual's number of segments.  path as
// k_log2_states left it.  Every thread finds the first start among its windows; a suffix minimum over the 256 blocks in LDS gives
// each the next start behind its block (n_win if none), so a backward walk over its own windows knows where every segment
// that starts there ends.  Sums and maxima over the threads by join_threads.  No atomics.
template <bool CH>
__global__ __launch_bounds__(STATES_THREADS) void k_log2_segments_count(const uint8_t *__restrict__ path, uint32_t n_win,
                                                                        uint32_t n_targets, const uint64_t *__restrict__ pos_first,
                                                                        const uint64_t *__restrict__ pos_last,
                                                                        const uint32_t *__restrict__ starts_arg,
                                                                        uint64_t *__restrict__ out)
{
    const uint32_t *__restrict__ starts = chains_of<CH>(starts_arg);
    __shared__ uint32_t nxt[2][STATES_THREADS];
    __shared__ uint64_t red[STATES_THREADS / 64][12];

    const uint32_t b = threadIdx.x;
    const Blocks B(n_win);
    const uint32_t w0 = B.begin(b), w1 = B.end(b);
    const bool own = b < B.nbk;

    for (uint32_t t = blockIdx.x; t < n_targets; t += gridDim.x) {
        const uint8_t *pt = path + (size_t)t * n_win;
        uint32_t fs = n_win;
        if (own) {
            unsigned prev = b == 0 ? 3u : pt[w0 - 1];
            for (uint32_t w = w0; w < w1; ++w) {
                const unsigned s = pt[w];
                if (seg_start(starts, w, prev, s)) {
                    fs = w;
                    break;
                }
                prev = s;
            }
        }
        // nxt[..][k] becomes the first start in block k or behind it
        const int cur = scan_lds<true>(nxt, b, fs, [](uint32_t x, uint32_t y) { return y < x ? y : x; });
        uint64_t v[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (own) {
            uint32_t end = b + 1 < STATES_THREADS ? nxt[cur][b + 1] : n_win;     // where the segment at hand ends (exclusive)
            unsigned s = pt[w1 - 1];
            for (uint32_t w = w1; w-- > w0;) {
                const unsigned p = w == 0 ? 3u : pt[w - 1];
                if (seg_start(starts, w, p, s)) {
                    seg_summary_add(v, s, end - w, pos_first ? pos_last[end - 1] - pos_first[w] + 1 : 0);
                    end = w;
                }
                s = p;
            }
        }
        uint64_t r = join_threads(v, red, b, [](int i, uint64_t x, uint64_t y) { return seg_summary_join(i, x, y); });
        if (b == 12)
            for (int k = 0; k < STATES_THREADS / 64; ++k)
                r += red[k][0] + red[k][1] + red[k][2];
        if (b < 13)
            out[(size_t)t * 13 + b] = r;
        __syncthreads();       // (LDS is reused by the next individual)
    }
}

// k_log2_segments_write: the records, individual t's from seg[off[t]] on in window order (off: the exclusive sums of the counts
// of k_log2_segments_count over the same paths).  post: gamma as k_log2_posteriors left it, or NULL.  A thread walks its windows
// once with one accumulator: at a start it is the block's head (the windows before its first start: they belong to a segment
// that started in an earlier block) or the total of a segment that lies inside the block, which is written there and then;
// at the block's end it is the tail of the block's last segment (or the head, if the block has no start).  An inclusive scan
// of the blocks' start counts gives every thread the index of its first record.  The owner of a tail then adds the heads of
// the blocks behind it, up to and with the first one that has a start -- a segment may cover any number of whole blocks --
// and writes that record.  No atomics: every record has one writer, every head one reader.
template <bool CH>
__global__ __launch_bounds__(STATES_THREADS) void k_log2_segments_write(const double *__restrict__ win_log2,
                                                                        const uint8_t *__restrict__ path,
                                                                        const double *__restrict__ post, uint32_t n_win,
                                                                        uint32_t n_targets, const uint64_t *__restrict__ off,
                                                                        const uint32_t *__restrict__ starts_arg,
                                                                        ibdg_segment *__restrict__ seg)
{
    const uint32_t *__restrict__ starts = chains_of<CH>(starts_arg);
    __shared__ SegAcc hd[STATES_THREADS];               // the blocks' heads
    __shared__ uint32_t fst[STATES_THREADS];            // the block's first start, n_win if it has none
    __shared__ uint32_t cnt[2][STATES_THREADS];

    const uint32_t b = threadIdx.x;
    const Blocks B(n_win);
    const uint32_t w0 = B.begin(b), w1 = B.end(b);
    const bool own = b < B.nbk;
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
                if (seg_start(starts, w, prev, s)) {
                    fs = ns ? fs : w;
                    ++ns;
                }
                prev = s;
            }
        }
        fst[b] = fs;
        const int cur = scan_lds<false>(cnt, b, ns, [](uint32_t x, uint32_t y) { return x + y; });
        uint32_t k = cnt[cur][b] - ns;                  // the block's first record
        SegAcc a;
        seg_reset(a);
        uint32_t start = NONE;
        unsigned state = 0;
        if (own) {
            unsigned prev = before;
            for (uint32_t w = w0; w < w1; ++w) {
                const unsigned s = pt[w];
                if (seg_start(starts, w, prev, s)) {
                    if (start == NONE)
                        hd[b] = a;
                    else
                        seg_record(out + k++, start, w - start, state, a, with_post);
                    seg_reset(a);
                    start = w, state = s;
                }
                prev = s;
                seg_add_window(a, tab + 3 * (size_t)w, with_post ? po + 3 * (size_t)w : nullptr, s);
            }
        }
        if (start == NONE)                              // no start: all of the block (nothing, for a block without windows)
            hd[b] = a;
        __syncthreads();
        if (start != NONE) {
            uint32_t end = n_win;
            for (uint32_t j = b + 1; j < B.nbk; ++j) {
                seg_add_piece(a, hd[j]);
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

// ---- sampled paths (ibdg_states.h) -----------------------------------------------------------------------------

// k_log2_alpha: steps 1 and 2 (the forward walk alone) and the forward half of step 4 of the posteriors, with their launch, blocking
// and step functions; alpha [T][n_win][3] out.  A kernel of its own, so that k_log2_posteriors keeps its code, its LDS and its one
// launch.
template <bool CH, bool SH>
__global__ __launch_bounds__(STATES_THREADS) void k_log2_alpha(const double *__restrict__ win_log2, uint32_t n_win, uint32_t n_targets,
                                                               PenW W, const double *__restrict__ tables,
                                                               const uint32_t *__restrict__ starts_arg,
                                                               const int32_t *__restrict__ shift_arg, double *__restrict__ alpha)
{
    const uint32_t *__restrict__ starts = chains_of<CH>(starts_arg);
    const int32_t *__restrict__ shift = steps_of<SH>(shift_arg);
    __shared__ double mat[STATES_THREADS][9];       // 18 KB: B_b
    __shared__ double fin[STATES_THREADS][3];       // F_b
    __shared__ double T[512];                       // T1, T2
    __shared__ int mexp[STATES_THREADS], fexp[STATES_THREADS];

    const uint32_t b = threadIdx.x;
    const Blocks B(n_win);
    const uint32_t w0 = B.begin(b), w1 = B.end(b);
    const bool own = b < B.nbk;

    T[b] = tables[b], T[b + STATES_THREADS] = tables[b + STATES_THREADS];
    __syncthreads();

    for (uint32_t t = blockIdx.x; t < n_targets; t += gridDim.x) {
        const PostIn in = {win_log2 + (size_t)t * n_win * 3, T, {W.a[0], W.a[1], W.a[2]}, starts, shift,
                           {W.P[0], W.P[1], W.P[2]}};
        if (own)
            post_block_matrix(in, w0, w1, mat[b], &mexp[b]);
        __syncthreads();
        if (b == 0)
            post_forward_walk(mat[0], mexp, B.nbk, fin[0], fexp);
        __syncthreads();
        if (own)
            post_block_alpha(in, w0, w1, fin[b], fexp[b], alpha + (size_t)t * n_win * 3);
        __syncthreads();       // (LDS is reused by the next individual)
    }
}

// k_log2_sample_paths: a workgroup per (individual, draw) pair, grid-stride over the launch's pairs; the blocking of k_log2_states,
// whose passes 2 and 3 these are with sampled maps in place of argmax maps.
//   pass A  a thread walks its windows backward: window w's map (state at w + 1 -> state at w) from alpha_w, the switch weights
//           into w + 1 and r(t, k, w) (sample_window_map), kept as 6 bits in the pair's path bytes and composed into the block's
//           map (state at the next block's first window -> state at this block's first)
//   scan    the blocks' maps composed from the last block down (scan_lds); the last window's map is constant, so what enters
//           behind it does not matter and there is no last_state to share
//   pass B  every thread resolves its windows from the state the blocks behind it give, overwriting the maps; the counts meet in
//           LDS (join_threads) and go to words 0..2 of the pair's record
// No atomics, no transcendental; T1, T2 are read with shifts only (SH), as in k_log2_posteriors.
template <bool CH, bool SH>
__global__ __launch_bounds__(STATES_THREADS) void k_log2_sample_paths(const double *__restrict__ alpha, uint32_t n_win, uint64_t p0,
                                                                      uint32_t n_pairs, uint32_t K, PenW W,
                                                                      const double *__restrict__ tables,
                                                                      const uint32_t *__restrict__ starts_arg,
                                                                      const int32_t *__restrict__ shift_arg, uint64_t seed,
                                                                      const uint64_t *__restrict__ stream, uint8_t *__restrict__ path,
                                                                      uint64_t *__restrict__ rec)
{
    const uint32_t *__restrict__ starts = chains_of<CH>(starts_arg);
    const int32_t *__restrict__ shift = steps_of<SH>(shift_arg);
    __shared__ uint8_t maps[2][STATES_THREADS];
    __shared__ uint32_t cnt[STATES_THREADS / 64][3];
    __shared__ double T[SH ? 512 : 1];              // T1, T2

    const uint32_t b = threadIdx.x;
    const Blocks B(n_win);                           // (n_win >= 1)
    const uint32_t w0 = B.begin(b), w1 = B.end(b);
    const bool own = b < B.nbk;

    if (SH) {
        T[b] = tables[b], T[b + STATES_THREADS] = tables[b + STATES_THREADS];
        __syncthreads();
    }
    const PostIn in = {nullptr, T, {W.a[0], W.a[1], W.a[2]}, starts, shift, {W.P[0], W.P[1], W.P[2]}};

    for (uint32_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const uint64_t g = p0 + p;
        const uint64_t t = g / K, k = g % K;
        const double *al = alpha + (size_t)t * n_win * 3;
        uint8_t *pt = path + (size_t)p * n_win;
        const uint64_t key = sample_key(seed, stream[t], k);

        // pass A
        unsigned blk = MAP_ID;
        if (own) {
            // (four windows a trip: their rows of alpha wait for nothing the loop makes, and asked for together they cost one
            // latency, not four -- 58 ms against 87 for the call at 34 599 windows)
#pragma unroll 4
            for (uint32_t w = w1; w-- > w0;) {
                const unsigned m = sample_window_map(in, al, n_win, w, key);
                pt[w] = (uint8_t)m;
                blk = map_after(m, blk);
            }
        }
        // maps[..][j] becomes block j's map after block j + 1's after ... after the last block's
        const int cur = scan_lds<true>(maps, b, (uint8_t)blk, [](unsigned x, unsigned y) { return map_after(x, y); });
        // pass B
        uint32_t n[3] = {0, 0, 0};
        if (own) {
            unsigned st = b + 1 < B.nbk ? map_at(maps[cur][b + 1], 0) : 0;     // the state at window w1 (none behind the last)
#pragma unroll 8                  // (likewise the maps' bytes)
            for (uint32_t w = w1; w-- > w0;) {
                st = map_at(pt[w], st);
                pt[w] = (uint8_t)st;
                n[0] += st == 0, n[1] += st == 1, n[2] += st == 2;
            }
        }
        const uint32_t sum = join_threads(n, cnt, b, [](int, uint32_t x, uint32_t y) { return x + y; });
        if (b < 3)
            rec[(size_t)p * SAMPLE_RECORD + b] = sum;
        __syncthreads();       // (LDS is reused by the next pair)
    }
}

// k_log2_sample_records: words 3..14 of every pair's record = the 12 summary words k_log2_segments_count left for its path
__global__ __launch_bounds__(STATES_THREADS) void k_log2_sample_records(const uint64_t *__restrict__ sout, uint32_t n_pairs,
                                                                        uint64_t *__restrict__ rec)
{
    const size_t i = (size_t)blockIdx.x * STATES_THREADS + threadIdx.x;
    if (i < (size_t)n_pairs * 12)
        rec[i / 12 * SAMPLE_RECORD + 3 + i % 12] = sout[i / 12 * 13 + i % 12];
}

// ---- switches (ibdg_states.h) -----------------------------------------------------------------------------------

// k_log2_switches: k_log2_posteriors with post_block_switches in the place of post_block_gamma -- its launch, blocking, walks
// (threads 0 and 64), tree and LDS (42 KB; no D or Z to keep).  scr [T][n_win][3] holds beta_w from step 3 on, and with ROWS
// sw_w after the forward pass: the thread that wrote a row is the one that reads it.  out [T][3] = n.  A kernel of its own, so
// that the others keep their code.  No atomics; the same reads as k_log2_posteriors.  k_log2_switch_expect below is this body
// with ROWS = false and another scratch base: a change here is a change there.
template <bool CH, bool SH, bool ROWS>
__global__ __launch_bounds__(STATES_THREADS) void k_log2_switches(const double *__restrict__ win_log2, uint32_t n_win,
                                                                  uint32_t n_targets, PenW W, const double *__restrict__ tables,
                                                                  const uint32_t *__restrict__ starts_arg,
                                                                  const int32_t *__restrict__ shift_arg,
                                                                  double *__restrict__ scr, double *__restrict__ out)
{
    const uint32_t *__restrict__ starts = chains_of<CH>(starts_arg);
    const int32_t *__restrict__ shift = steps_of<SH>(shift_arg);
    __shared__ double mat[STATES_THREADS][9];       // 18 KB: B_b
    __shared__ double fin[STATES_THREADS][3];       // F_b
    __shared__ double gout[STATES_THREADS][3];      // G_b
    __shared__ double part[STATES_THREADS][3];
    __shared__ double T[512];                       // T1, T2
    __shared__ int mexp[STATES_THREADS], fexp[STATES_THREADS];

    const uint32_t b = threadIdx.x;
    const Blocks B(n_win);
    const uint32_t w0 = B.begin(b), w1 = B.end(b);
    const bool own = b < B.nbk;

    T[b] = tables[b], T[b + STATES_THREADS] = tables[b + STATES_THREADS];
    __syncthreads();

    for (uint32_t t = blockIdx.x; t < n_targets; t += gridDim.x) {
        const PostIn in = {win_log2 + (size_t)t * n_win * 3, T, {W.a[0], W.a[1], W.a[2]}, starts, shift,
                           {W.P[0], W.P[1], W.P[2]}};
        // 1
        if (own)
            post_block_matrix(in, w0, w1, mat[b], &mexp[b]);
        __syncthreads();
        // 2
        if (b == 0)
            post_forward_walk(mat[0], mexp, B.nbk, fin[0], fexp);
        else if (b == 64)
            post_backward_walk(mat[0], B.nbk, gout[0]);
        __syncthreads();
        // 3, forward
        double acc[3] = {0.0, 0.0, 0.0};
        if (own)
            post_block_switches<ROWS>(in, w0, w1, gout[b], fin[b], fexp[b], scr + (size_t)t * n_win * 3, acc);
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
            out[(size_t)t * 3 + b] = part[0][b];
        __syncthreads();       // (LDS is reused by the next individual)
    }
}

// ---- the fit's pass over a table store (ibdg_states.h) ----------------------------------------------------------
//
// k_log2_switch_expect: k_log2_switches<CH, SH, false> over tabs [n_tables][n_win][3] -- the same step functions in the same
// order, so out [n_tables][3] holds the twin's bytes -- with one difference: the beta scratch belongs to the WORKGROUP, scr +
// blockIdx.x * n_win * 3, not to the individual, so a launch over a whole store needs gridDim.x tables' worth of scratch and not a
// second store.  Reusing it for the workgroup's next individual needs no barrier beyond the loop's own: post_block_switches
// writes beta_w for w in [w0, w1) of the calling thread's block and its forward pass reads these rows only, in the same thread,
// behind the writes in program order; no other thread reads or writes a row of that range, for this individual or the next
// (w0, w1 depend on n_win and threadIdx.x alone).  What the loop's barriers order is LDS, as in its siblings.  A kernel of its
// own, so that the others keep their code.  No atomics.
template <bool CH, bool SH>
__global__ __launch_bounds__(STATES_THREADS) void k_log2_switch_expect(const double *__restrict__ tabs, uint32_t n_win,
                                                                       uint32_t n_tables, PenW W, const double *__restrict__ tables,
                                                                       const uint32_t *__restrict__ starts_arg,
                                                                       const int32_t *__restrict__ shift_arg,
                                                                       double *__restrict__ scr, double *__restrict__ out)
{
    const uint32_t *__restrict__ starts = chains_of<CH>(starts_arg);
    const int32_t *__restrict__ shift = steps_of<SH>(shift_arg);
    __shared__ double mat[STATES_THREADS][9];       // 18 KB: B_b
    __shared__ double fin[STATES_THREADS][3];       // F_b
    __shared__ double gout[STATES_THREADS][3];      // G_b
    __shared__ double part[STATES_THREADS][3];
    __shared__ double T[512];                       // T1, T2
    __shared__ int mexp[STATES_THREADS], fexp[STATES_THREADS];

    const uint32_t b = threadIdx.x;
    const Blocks B(n_win);
    const uint32_t w0 = B.begin(b), w1 = B.end(b);
    const bool own = b < B.nbk;
    double *__restrict__ const beta = scr + (size_t)blockIdx.x * n_win * 3;

    T[b] = tables[b], T[b + STATES_THREADS] = tables[b + STATES_THREADS];
    __syncthreads();

    for (uint32_t t = blockIdx.x; t < n_tables; t += gridDim.x) {
        const PostIn in = {tabs + (size_t)t * n_win * 3, T, {W.a[0], W.a[1], W.a[2]}, starts, shift, {W.P[0], W.P[1], W.P[2]}};
        // 1
        if (own)
            post_block_matrix(in, w0, w1, mat[b], &mexp[b]);
        __syncthreads();
        // 2
        if (b == 0)
            post_forward_walk(mat[0], mexp, B.nbk, fin[0], fexp);
        else if (b == 64)
            post_backward_walk(mat[0], B.nbk, gout[0]);
        __syncthreads();
        // 3, forward
        double acc[3] = {0.0, 0.0, 0.0};
        if (own)
            post_block_switches<false>(in, w0, w1, gout[b], fin[b], fexp[b], beta, acc);
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
            out[(size_t)t * 3 + b] = part[0][b];
        __syncthreads();       // (LDS is reused by the next individual)
    }
}

// the one launch of all four: nothing for no windows or no individuals, else a workgroup per individual under STATES_MAX_BLOCKS
template <typename K, typename... A>
void launch_kernel(K kernel, uint32_t n_win, uint32_t n_targets, hipStream_t st, A... args)
{
    if (n_win == 0 || n_targets == 0)
        return;
    const uint32_t grid = n_targets < STATES_MAX_BLOCKS ? n_targets : STATES_MAX_BLOCKS;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(STATES_THREADS), 0, st, args...);
}

// ... of the instantiation for this mask (with: CH = true, without: CH = false)
#define launch_per_individual(kernel, starts, ...) \
    ((starts) ? launch_kernel(kernel<true>, __VA_ARGS__) : launch_kernel(kernel<false>, __VA_ARGS__))

// ... and for these shifts (with: SH = true, without: SH = false)
#define launch_per_individual_steps(kernel, starts, shift, ...)                                                               \
    ((shift) ? ((starts) ? launch_kernel(kernel<true, true>, __VA_ARGS__) : launch_kernel(kernel<false, true>, __VA_ARGS__)) \
             : ((starts) ? launch_kernel(kernel<true, false>, __VA_ARGS__) : launch_kernel(kernel<false, false>, __VA_ARGS__)))

}  // namespace

void launch_log2_states(const double *win_log2, uint32_t n_win, uint32_t n_targets, const int64_t P[3], const uint32_t *starts,
                        const int32_t *shift, uint8_t *path, int64_t *score, uint64_t *count, hipStream_t st)
{
    launch_per_individual_steps(k_log2_states, starts, shift, n_win, n_targets, st, win_log2, n_win, n_targets, Pen{P[0], P[1], P[2]},
                                starts, shift, path, score, count);
}

void launch_log2_posteriors(const double *win_log2, uint32_t n_win, uint32_t n_targets, const int64_t P[3], const double a[3],
                            const double *tables, const uint32_t *starts, const int32_t *shift, double *scr, double *out,
                            hipStream_t st)
{
    launch_per_individual_steps(k_log2_posteriors, starts, shift, n_win, n_targets, st, win_log2, n_win, n_targets,
                                PenW{{a[0], a[1], a[2]}, {P[0], P[1], P[2]}}, tables, starts, shift, scr, out);
}

void launch_log2_segments_count(const uint8_t *path, uint32_t n_win, uint32_t n_targets, const uint64_t *pos_first,
                                const uint64_t *pos_last, const uint32_t *starts, uint64_t *out, hipStream_t st)
{
    launch_per_individual(k_log2_segments_count, starts, n_win, n_targets, st, path, n_win, n_targets, pos_first, pos_last, starts, out);
}

void launch_log2_segments_write(const double *win_log2, const uint8_t *path, const double *post, uint32_t n_win, uint32_t n_targets,
                                const uint64_t *off, const uint32_t *starts, ibdg_segment *seg, hipStream_t st)
{
    launch_per_individual(k_log2_segments_write, starts, n_win, n_targets, st, win_log2, path, post, n_win, n_targets, off, starts, seg);
}

void launch_log2_alpha(const double *win_log2, uint32_t n_win, uint32_t n_targets, const int64_t P[3], const double a[3],
                       const double *tables, const uint32_t *starts, const int32_t *shift, double *alpha, hipStream_t st)
{
    launch_per_individual_steps(k_log2_alpha, starts, shift, n_win, n_targets, st, win_log2, n_win, n_targets,
                                PenW{{a[0], a[1], a[2]}, {P[0], P[1], P[2]}}, tables, starts, shift, alpha);
}

void launch_log2_sample_paths(const double *alpha, uint32_t n_win, uint64_t p0, uint32_t n_pairs, uint32_t K, const int64_t P[3],
                              const double a[3], const double *tables, const uint32_t *starts, const int32_t *shift, uint64_t seed,
                              const uint64_t *stream, uint8_t *path, uint64_t *rec, hipStream_t st)
{
    launch_per_individual_steps(k_log2_sample_paths, starts, shift, n_win, n_pairs, st, alpha, n_win, p0, n_pairs, K,
                                PenW{{a[0], a[1], a[2]}, {P[0], P[1], P[2]}}, tables, starts, shift, seed, stream, path, rec);
}

template <bool ROWS>
static void launch_switches(const double *win_log2, uint32_t n_win, uint32_t n_targets, const PenW &W, const double *tables,
                            const uint32_t *starts, const int32_t *shift, double *scr, double *out, hipStream_t st)
{
    if (shift)
        starts ? launch_kernel(k_log2_switches<true, true, ROWS>, n_win, n_targets, st, win_log2, n_win, n_targets, W, tables, starts, shift, scr, out)
               : launch_kernel(k_log2_switches<false, true, ROWS>, n_win, n_targets, st, win_log2, n_win, n_targets, W, tables, starts, shift, scr, out);
    else
        starts ? launch_kernel(k_log2_switches<true, false, ROWS>, n_win, n_targets, st, win_log2, n_win, n_targets, W, tables, starts, shift, scr, out)
               : launch_kernel(k_log2_switches<false, false, ROWS>, n_win, n_targets, st, win_log2, n_win, n_targets, W, tables, starts, shift, scr, out);
}

void launch_log2_switches(const double *win_log2, uint32_t n_win, uint32_t n_targets, const int64_t P[3], const double a[3],
                          const double *tables, const uint32_t *starts, const int32_t *shift, bool rows, double *scr, double *out,
                          hipStream_t st)
{
    const PenW W{{a[0], a[1], a[2]}, {P[0], P[1], P[2]}};
    rows ? launch_switches<true>(win_log2, n_win, n_targets, W, tables, starts, shift, scr, out, st)
         : launch_switches<false>(win_log2, n_win, n_targets, W, tables, starts, shift, scr, out, st);
}

// (the grid is the caller's, who sized scr by it: switch_expect_grid)
void launch_log2_switch_expect(const double *tabs, uint32_t n_win, uint32_t n_tables, uint32_t grid, const int64_t P[3],
                               const double a[3], const double *tables, const uint32_t *starts, const int32_t *shift, double *scr,
                               double *out, hipStream_t st)
{
    if (n_win == 0 || n_tables == 0 || grid == 0)
        return;
    const PenW W{{a[0], a[1], a[2]}, {P[0], P[1], P[2]}};
    const dim3 g(grid < n_tables ? grid : n_tables), blk(STATES_THREADS);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, g, blk, 0, st, tabs, n_win, n_tables, W, tables, starts, shift, scr, out); };
    if (shift)
        starts ? go(k_log2_switch_expect<true, true>) : go(k_log2_switch_expect<false, true>);
    else
        starts ? go(k_log2_switch_expect<true, false>) : go(k_log2_switch_expect<false, false>);
}

void launch_log2_sample_records(const uint64_t *sout, uint32_t n_pairs, uint64_t *rec, hipStream_t st)
{
    if (n_pairs == 0)
        return;
    const uint32_t grid = (uint32_t)(((size_t)n_pairs * 12 + STATES_THREADS - 1) / STATES_THREADS);
    hipLaunchKernelGGL(k_log2_sample_records, dim3(grid), dim3(STATES_THREADS), 0, st, sout, n_pairs, rec);
}

}  // namespace ibdg
