// ibdg_ld_images.hip -- what the --LD counting kernels (ibdg_ld_popcount.hip) read, built ahead of them: the panel
// transposed into 32-row tiles (once per upload, or compacted once per site list) and, per comparison individual, the
// LDS-ready images of every segment and window (widths and layouts: ibdg_ld_layout.h) that a workgroup stages with
// plain contiguous copies.
#include "ibdg_kernels.h"
#include "ibdg_ld_dev.h"
#include "ibdg_ld_layout.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

namespace ibdg {

// ---------------------------------------------------------------------------
// Panel transposition (once per upload): site-major rows ->
//     t32[chunk][tile_pair][lane] = uint4 { x0(tile 2q), x1(2q), x0(2q+1), x1(2q+1) }
// x0/x1 = first/second haplotype of individual 64*chunk+lane, bit j = row 32*tile + j.
// A wave reads one tile pair as one fully coalesced 1 KiB global_load_dwordx4, and the four
// pairs of an 8-tile "oct" are 4 KiB contiguous.  Tiles are padded to whole octs (zero bits).
//
// One wave per (tile pair, chunk): lane j loads the chunk's two haplotype words of row 64 q + j (16 bytes;
// the eight waves of a workgroup take eight neighbouring chunks, i.e. whole 128-byte pieces of the rows), and
// the two 64 x 64 bit matrices (rows on lanes, individuals on bits) are transposed in registers by the
// recursive block exchange: at block size s lane l and lane l ^ s swap the off-diagonal s x s blocks --
//     l & s == 0:  w = (w & K) | (t << s & ~K),      l & s != 0:  w = (w & ~K) | (t >> s & K),
// t = the partner's word, K = the bits whose index has bit s clear -- as ONE v_alignbit (a rotation by s or
// 32 - s, whichever the lane needs) and ONE v_bfi per 32-bit word and step; the exchanges are a
// v_permlane32_swap (s = 32), ds_swizzle (16, 4) and DPP moves (8, 2, 1).  ~65 vector instructions per KiB,
// where the first version (every lane picking its bit out of 128 wave-uniform row words) spent ~400 and
// read every row word through the scalar cache: 9.4 ms for the 2.56 GB panel then.
// ---------------------------------------------------------------------------
template <int S>
__device__ __forceinline__ uint32_t partner_word(uint32_t w)
{
    if (S == 16 || S == 4)
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)w, (S << 10) | 0x1f);
    constexpr int ctrl = S == 8 ? 0x128 /* row_ror:8 */ : (S == 2 ? 0x4E /* quad_perm [2,3,0,1] */ : 0xB1 /* [1,0,3,2] */);
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, ctrl, 0xf, 0xf, true);
}

template <int S>
__device__ __forceinline__ uint32_t block_exchange(uint32_t w, uint32_t lane)
{
    constexpr uint32_t K = S == 16 ? 0x0000ffffu : S == 8 ? 0x00ff00ffu : S == 4 ? 0x0f0f0f0fu : S == 2 ? 0x33333333u : 0x55555555u;
    const bool up = lane & S;
    const uint32_t t = partner_word<S>(w);
    const uint32_t rot = __builtin_amdgcn_alignbit(t, t, up ? S : 32 - S);      // t >> s (up) or t << s, as a rotation
    const uint32_t keep = up ? ~K : K;
    return (w & keep) | (rot & ~keep);                                           // v_bfi_b32
}

// one step of the block exchange on the four words of a lane
template <int S>
__device__ __forceinline__ void exchange_step(uint4 &w, uint32_t lane)
{
    w.x = block_exchange<S>(w.x, lane);
    w.y = block_exchange<S>(w.y, lane);
    w.z = block_exchange<S>(w.z, lane);
    w.w = block_exchange<S>(w.w, lane);
}

// the two 64 x 64 bit matrices of a wave (lane = row; {plane 0 lo, hi, plane 1 lo, hi}) transposed in registers:
// afterwards lane = individual, the return value the uint4 of the layout above
__device__ __forceinline__ uint4 transpose_pair(uint4 w, uint32_t lane)
{
    // s = 32: the high halves of lanes 0..31 and the low halves of lanes 32..63 change places
    {
        auto p0 = __builtin_amdgcn_permlane32_swap(w.x, w.y, false, false);
        w.x = p0[0];
        w.y = p0[1];
        auto p1 = __builtin_amdgcn_permlane32_swap(w.z, w.w, false, false);
        w.z = p1[0];
        w.w = p1[1];
    }
    exchange_step<16>(w, lane);
    exchange_step<8>(w, lane);
    exchange_step<4>(w, lane);
    exchange_step<2>(w, lane);
    exchange_step<1>(w, lane);
    // w.x / w.y = rows 0..31 / 32..63 of the first haplotype, w.z / w.w of the second
    return make_uint4(w.x, w.z, w.y, w.w);
}

__global__ __launch_bounds__(512) void k_transpose32(const uint64_t *__restrict__ panel,
                                                     uint32_t stride, size_t n_rows,
                                                     uint32_t n_chunks, uint32_t n_pairs,
                                                     uint4 *__restrict__ t32)
{
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    const unsigned c = blockIdx.y * 8 + wave;
    if (c >= n_chunks)
        return;
    const uint32_t pair = blockIdx.x;
    const size_t r = (size_t)pair * 64 + lane;
    uint4 w = make_uint4(0, 0, 0, 0);                 // {plane 0 lo, hi, plane 1 lo, hi} of row r
    if (r < n_rows)
        w = *reinterpret_cast<const uint4 *>(panel + r * stride + 2 * c);
    t32[((size_t)c * n_pairs + pair) * 64 + lane] = transpose_pair(w, lane);
}

// ---------------------------------------------------------------------------
// The compacted layout of ONE site list (once per ibdg_upload_sites, or once the runs on it have added up): only the
// rows that carry reads, in the order of the site list --
//     virtual row v = (j / W) * R + j % W      for covered row j (W = window, R = virtual rows per window)
// R = W (the default since round 5): the rows back to back, v = j, no padding -- a window of 100 rows spans 3.1 tiles and
// is cut into 4.1 segments where the panel's own tiles (13.5 % rows without reads) make it 3.6 tiles / 4.6 segments;
// R = 32 * TPW, TPW = ceil(W / 32) (round 4, option "compact_align" 32): every window starts on a tile boundary, 4 segments
// per window of 100 but 28 % of the tile words are padding
// -- gathered from the site-major panel through the covered-row list and transposed like above, same uint4
// layout, so the --LD kernels run on it unchanged (their segments are cut from the virtual rows,
// ibdg_prep.hip).  In the reference the rows a window multiplies are the rows that passed the filter chain
// and carry reads (src/ibdgem.c:596-601, :657-663), however far apart they lie in the panel: here a window
// costs TPW tile words whatever the pileup's density, where the in-place tiles cost one word per 32 PANEL
// rows between its first and last row; and no tile is shared by two windows (4 segments per window of 100
// rows instead of 4.6).  The rows of the virtual tiles beyond a window's W (and beyond the last covered row)
// are zero bits.  Access pattern as in k_transpose32: a lane fetches 16 bytes of its row, the eight waves of a
// workgroup eight neighbouring chunks = one 128-byte piece of each of the 64 rows.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_gather_transpose32(const uint64_t *__restrict__ panel, uint32_t stride,
                                                            const uint2 *__restrict__ rec_cov, uint32_t n_cov,
                                                            uint32_t window, uint32_t win_rows /* R */,
                                                            uint32_t n_chunks, uint32_t n_pairs,
                                                            uint4 *__restrict__ t32)
{
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    const unsigned c = blockIdx.y * 8 + wave;
    if (c >= n_chunks)
        return;
    const uint32_t pair = blockIdx.x;
    const uint64_t v = (uint64_t)pair * 64 + lane;
    uint64_t j = v;                      // rows back to back (win_rows == window, the default): virtual row = covered row
    bool in_window = true;
    if (win_rows != window) {            // (wave-uniform: an alignment was asked for)
        const uint64_t win = v / win_rows;
        const uint32_t k = (uint32_t)(v - win * win_rows);
        j = win * window + k;
        in_window = k < window;
    }
    uint4 w = make_uint4(0, 0, 0, 0);
    if (in_window && j < n_cov)
        w = *reinterpret_cast<const uint4 *>(panel + (size_t)rec_cov[j].x * stride + 2 * c);
    t32[((size_t)c * n_pairs + pair) * 64 + lane] = transpose_pair(w, lane);
}

// ---------------------------------------------------------------------------
// Per target, one thread per segment and eight per window: the LDS-ready images the --LD kernel stages
// with plain contiguous copies -- every segment's 8-word record (IBDG_REC_WORDS, layout above) with the
// target's haplotype words of its tile filled in, and the window's 8 constants (IBDG_WC_WORDS) built
// from <t0,cov>, <t1,cov>, <t0,alt>, <t1,alt> summed over the window's rows.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_win_target(PopArgs a, uint32_t *__restrict__ rec_ready,
                                                    uint32_t *__restrict__ wc_ready)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned t = blockIdx.y;
    uint32_t tgt = a.targets[a.t_base + t];
    IBDG_CHECK_TGT(tgt, a.lanes, __func__);
    const uint4 *tt = reinterpret_cast<const uint4 *>(a.t32) + (size_t)(tgt >> 6) * a.n_pairs * 64 + (tgt & 63);
    if (i < a.n_segs) {                      // thread i: the record of segment i
        const Seg S = a.segs[i];
        const uint2 at = tile_words(tt, S.tile);
        uint4 *o = reinterpret_cast<uint4 *>(rec_ready + ((size_t)t * a.n_segs + i) * IBDG_REC_WORDS);
        o[0] = make_uint4(S.flags, S.cov[0], S.cov[1], S.cov[2]);
        o[1] = make_uint4(S.alt[0], S.alt[1], at.x, at.y);
    }
    if ((i >> 3) < a.n_win) {                // threads 8w..8w+7: the constants of window w
        const uint32_t w = i >> 3;
        uint32_t a0cov = 0, a1cov = 0, a0alt = 0, a1alt = 0;
        const uint32_t s1 = a.wconst[w + 1].seg_begin;
        for (uint32_t s = a.wconst[w].seg_begin + (i & 7); s < s1; s += 8) {    // a window has ~4-5 segments
            const Seg &S = a.segs[s];
            const uint2 at = tile_words(tt, S.tile);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                a0cov += (uint32_t)__popc(at.x & S.cov[k]) << k;
                a1cov += (uint32_t)__popc(at.y & S.cov[k]) << k;
                a0alt += (uint32_t)__popc(at.x & S.alt[k]) << k;
                a1alt += (uint32_t)__popc(at.y & S.alt[k]) << k;
            }
        }
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) {    // the 8 lanes of a window sit in one wave (8 | 64, i is 8-aligned)
            a0cov += __shfl_xor(a0cov, m);
            a1cov += __shfl_xor(a1cov, m);
            a0alt += __shfl_xor(a0alt, m);
            a1alt += __shfl_xor(a1alt, m);
        }
        if ((i & 7) == 0) {
            const uint32_t *wcs = reinterpret_cast<const uint32_t *>(a.wconst + w);    // mK(2) eK ct at seg_begin
            uint4 *o = reinterpret_cast<uint4 *>(wc_ready + ((size_t)t * a.n_win + w) * IBDG_WC_WORDS);
            const uint32_t AT = wcs[4];
            o[0] = make_uint4(wcs[2], 16 * AT, 16 * a0cov, 16 * a1cov);
            o[1] = make_uint4(16 * (AT - a0alt), 16 * (AT - a1alt), 0, 0);
        }
    }
}

// ---------------------------------------------------------------------------
// The same for the counts on the matrix cores (round 4; DESIGN.md s4.1, docs/DESIGN_rounds_1-4.md s4.1c).
//
// v_mfma_scale_f32_16x16x128_f8f6f4 multiplies a 16 x 128 matrix A by a 128 x 16 matrix B; lane l holds 32 K-elements
// of row (A) / column (B) l % 16: k = 32 (l / 16) .. + 31.  A is made block diagonal,
//     A[4 kb' + sum][32 kb + r] = weight_sum[r]  if kb == kb'  else 0
// and every lane supplies ITS OWN tile word as "column l % 16, K block l / 16" (its bits as FP4 numbers).  Then
//     D[4 kb + sum][n] = sum_r weight_sum[r] * bit_r(word of lane n + 16 kb)
// and the C/D layout (column = lane % 16, rows 4 (lane / 16) .. + 3 in the lane's four registers) returns to every lane
// the four weighted sums of its own word: <x,cov> <x,alt> <x & t0,cov> <x & t1,cov> -- one instruction for the twelve
// (mask, count) pairs of a haplotype word, no lane movement.  Bits become FP4 (e2m1) without shifts where possible:
//     dword 0 = x & 0x11111111  rows 4j     value 0.5      dword 2 = x & 0x44444444         rows 4j + 2  value 2
//     dword 1 = x & 0x22222222  rows 4j + 1 value 1        dword 3 = (x >> 3) & 0x11111111  rows 4j + 3  value 0.5
// (nibble 1000 is -0: useless) and A carries w, w/2, w/4, w in FP6 e2m3, exact for w = 0..7, with the block scale 2:
// every product is w, the sums are exact integers in f32 (tools/ubench/fp4_count.hip checks the layout with random
// words and weights).  Only the 16 lanes with l % 16 / 4 == l / 16 hold a non-zero A fragment: lanes 20 kb + sum read
// the 24 bytes of `sum` from the segment's record, the others keep zeros.
// Element k = 8 d + j of a lane's 32  <->  row r = 4 j + d of the tile.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fp6_weight_code(uint32_t w, int d)
{
    // e2m3 (bias 1, exponent 0 = subnormal m/8) of w (d = 0, 3), w/2 (d = 1), w/4 (d = 2), w = 0..7, as bytes of two words
    const uint32_t lo = d == 1 ? 0x0c080400u : d == 2 ? 0x06040200u : 0x14100800u;
    const uint32_t hi = d == 1 ? 0x16141210u : d == 2 ? 0x0e0c0a08u : 0x1e1c1a18u;
    return ((w & 4 ? hi : lo) >> (8 * (w & 3))) & 0xffu;
}

// the first eight words of a matrix-core record.  Control word of this form: bits 0-13 ring byte offset of the NEXT
// segment's tile words, 14 planes beyond cov 0-2 / alt 0-2 present, 15 last segment of its window, 16-23 tile pairs to
// advance before the next segment
__device__ __forceinline__ void mx_record_header(uint32_t *o, const Seg &S, uint2 at)
{
    const uint32_t ncov = (S.flags >> 16) & 0xff, nalt = S.flags >> 24;
    const uint32_t fl = ((S.flags & 7) * 1024 + ((S.flags >> 3) & 1) * 8) | ((ncov > 3 || nalt > 3) ? 1u << 14 : 0u) |
                        (((S.flags >> 13) & 1) << 15) | (((S.flags >> 4) & 0xff) << 16);
    uint4 *oh = reinterpret_cast<uint4 *>(o);
    oh[0] = make_uint4(fl, S.cov[0], S.cov[1], S.cov[2]);
    oh[1] = make_uint4(at.x, at.y, ncov | (nalt << 8), 0);
}

__global__ __launch_bounds__(256) void k_win_target_mx(PopArgs a, uint32_t *__restrict__ rec_ready,
                                                       uint32_t *__restrict__ wc_ready)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned t = blockIdx.y;
    uint32_t tgt = a.targets[a.t_base + t];
    IBDG_CHECK_TGT(tgt, a.lanes, __func__);
    const uint4 *tt = reinterpret_cast<const uint4 *>(a.t32) + (size_t)(tgt >> 6) * a.n_pairs * 64 + (tgt & 63);
    if ((i >> 2) < a.n_segs) {               // threads 4s .. 4s+3: the four A fragments of segment s
        const uint32_t sg = i >> 2, sum = i & 3;
        const Seg &S = a.segs[sg];
        IBDG_CHECK_IDX(S.tile, 2 * a.n_pairs, "k_win_target_mx tile");
        const uint2 at = tile_words(tt, S.tile);
        // the rows' weights of this thread's sum as three bit planes of the magnitude and one of the sign (bit 5 of the e2m3 code):
        //   <x,cov> <x,alt> <x & t0,cov> <x & t1,cov>                            -- the form that counts everything
        //   <x, cov (1 - 2 t0)>  <x, cov (1 - 2 t1)>  <x, t0 cov - alt>  <x, t1 cov - alt>   -- ibd1: C(x) - 2 G(x,t) and G(x,t) - A(x),
        //   the table exponents of the IBD1 products up to the window's constants; |weight| <= 7
        uint32_t p0, p1, p2, neg = 0;
        if (!a.ibd1) {
            if (sum == 1) {
                p0 = S.alt[0]; p1 = S.alt[1]; p2 = S.alt[2];
            } else {
                const uint32_t m = sum == 0 ? 0xffffffffu : sum == 2 ? at.x : at.y;
                p0 = S.cov[0] & m; p1 = S.cov[1] & m; p2 = S.cov[2] & m;
            }
        } else {
            const uint32_t tb = (sum & 1) ? at.y : at.x;
            if (sum < 2) {
                p0 = S.cov[0]; p1 = S.cov[1]; p2 = S.cov[2];
                neg = tb;                                       // (-0 where the row has no reads: adds nothing)
            } else {
                // t cov - alt for the 32 rows at once, bit-sliced: a three-bit subtraction, then the magnitude of the negative ones
                const uint32_t x0 = S.cov[0] & tb, x1 = S.cov[1] & tb, x2 = S.cov[2] & tb;
                const uint32_t y0 = S.alt[0], y1 = S.alt[1], y2 = S.alt[2];
                const uint32_t d0 = x0 ^ y0, b0 = ~x0 & y0;
                const uint32_t e1 = x1 ^ y1, d1 = e1 ^ b0, b1 = (~x1 & y1) | (~e1 & b0);
                const uint32_t e2 = x2 ^ y2, d2 = e2 ^ b1;
                neg = (~x2 & y2) | (~e2 & b1);                  // the borrow out of bit 2: the difference is negative
                const uint32_t r1 = ~d1 ^ ~d0, r2 = ~d2 ^ (~d1 & ~d0);      // -d = ~d + 1 (bit 0 stays)
                p0 = d0;
                p1 = (d1 & ~neg) | (r1 & neg);
                p2 = (d2 & ~neg) | (r2 & neg);
            }
        }
        uint32_t f[6] = {0, 0, 0, 0, 0, 0};   // 32 x 6 bits
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const int d = k >> 3, r = 4 * (k & 7) + d;
            const uint32_t w = ((p0 >> r) & 1u) | (((p1 >> r) & 1u) << 1) | (((p2 >> r) & 1u) << 2);
            const uint32_t code = fp6_weight_code(w, d) | (((neg >> r) & 1u) << 5);
            const int pos = 6 * k, wd = pos >> 5, sh = pos & 31;
            f[wd] |= code << sh;
            if (sh > 26)
                f[wd + 1] |= code >> (32 - sh);
        }
        uint32_t *o = rec_ready + ((size_t)t * a.n_segs + sg) * IBDG_RECX_WORDS;
        uint2 *fo = reinterpret_cast<uint2 *>(o + 8 + 6 * sum);
        fo[0] = make_uint2(f[0], f[1]);
        fo[1] = make_uint2(f[2], f[3]);
        fo[2] = make_uint2(f[4], f[5]);
        if (sum == 0)
            mx_record_header(o, S, at);
    }
    if ((i >> 3) < a.n_win) {                // threads 8w..8w+7: the constants of window w (as k_win_target)
        const uint32_t w = i >> 3;
        uint32_t a0cov = 0, a1cov = 0, a0alt = 0, a1alt = 0;
        const uint32_t s1 = a.wconst[w + 1].seg_begin;
        for (uint32_t s = a.wconst[w].seg_begin + (i & 7); s < s1; s += 8) {
            const Seg &S = a.segs[s];
            const uint2 at = tile_words(tt, S.tile);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                a0cov += (uint32_t)__popc(at.x & S.cov[k]) << k;
                a1cov += (uint32_t)__popc(at.y & S.cov[k]) << k;
                a0alt += (uint32_t)__popc(at.x & S.alt[k]) << k;
                a1alt += (uint32_t)__popc(at.y & S.alt[k]) << k;
            }
        }
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) {
            a0cov += __shfl_xor(a0cov, m);
            a1cov += __shfl_xor(a1cov, m);
            a0alt += __shfl_xor(a0alt, m);
            a1alt += __shfl_xor(a1alt, m);
        }
        if ((i & 7) == 0) {
            const uint32_t *wcs = reinterpret_cast<const uint32_t *>(a.wconst + w);
            uint4 *o = reinterpret_cast<uint4 *>(wc_ready + ((size_t)t * a.n_win + w) * IBDG_WC_WORDS);
            const uint32_t AT = wcs[4];
            // byte offsets into tables of 8-byte entries (the matrix-core form's power tables, see its window end)
            const uint32_t sc = a.tab_in_lds ? 8 : 16;       // (16-byte entries where the tables stay in global memory)
            // (ibd1: the sums reach the window end as the bits of 1.5 * 2^23 + sum, whose low 24 bits are 2^22 + sum: the constants
            //  take 8 * 2^22 back, modulo 2^32 like the address arithmetic they enter)
            const uint32_t bias = a.ibd1 ? 1u << 25 : 0u;
            o[0] = make_uint4(wcs[2], sc * AT, sc * a0cov - bias, sc * a1cov - bias);
            o[1] = make_uint4(sc * (AT - a0alt) - bias, sc * (AT - a1alt) - bias, 0, 0);
        }
    }
}

// ---------------------------------------------------------------------------
// The IBD1 form's images in two steps (round 5).  What k_win_target_mx builds per comparison individual and segment -- four
// fragments of 32 signed FP6 weights -- depends on the individual only through WHICH of two values a row's weight takes:
//     sums 0 / 1  cov (1 - 2 t):   +cov or -cov   = the code of cov with the sign bit of the rows where t is set
//     sums 2 / 3  t cov - alt:     -alt or cov - alt
// so the three fragments COV, F0 = code(-alt), F1 = code(cov - alt) are made ONCE per site list (k_frag_base, 72 bytes per
// segment), and an individual's images are bit selections between them: its tile word's 32 bits spread into 32 six-bit
// fields (M: 0x3f where the row's t is set), by a 256-entry table a byte at a time --
//     sum 0 / 1 = COV | (M & SIGN)        sum 2 / 3 = (F1 & M) | (F0 & ~M)
// -- ~100 instructions for a segment's two fragments of one target haplotype word instead of ~500 per fragment: the kernel
// that runs beside the previous step's --LD kernel for every NEW individual costs that kernel a third of what it did.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void fp6_fragment(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t neg, uint32_t (&f)[6])
{
#pragma unroll
    for (int i = 0; i < 6; ++i)
        f[i] = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const int d = k >> 3, r = 4 * (k & 7) + d;
        const uint32_t w = ((p0 >> r) & 1u) | (((p1 >> r) & 1u) << 1) | (((p2 >> r) & 1u) << 2);
        const uint32_t code = fp6_weight_code(w, d) | (((neg >> r) & 1u) << 5);
        const int pos = 6 * k, wd = pos >> 5, sh = pos & 31;
        f[wd] |= code << sh;
        if (sh > 26)
            f[wd + 1] |= code >> (32 - sh);
    }
}

// t cov - alt for 32 rows at once, bit-sliced (cov planes x, alt planes y): a three-bit subtraction, then the magnitude of
// the negative ones
__device__ __forceinline__ void sliced_diff(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t y0, uint32_t y1, uint32_t y2,
                                            uint32_t &p0, uint32_t &p1, uint32_t &p2, uint32_t &neg)
{
    const uint32_t d0 = x0 ^ y0, b0 = ~x0 & y0;
    const uint32_t e1 = x1 ^ y1, d1 = e1 ^ b0, b1 = (~x1 & y1) | (~e1 & b0);
    const uint32_t e2 = x2 ^ y2, d2 = e2 ^ b1;
    neg = (~x2 & y2) | (~e2 & b1);                  // the borrow out of bit 2: the difference is negative
    const uint32_t r1 = ~d1 ^ ~d0, r2 = ~d2 ^ (~d1 & ~d0);      // -d = ~d + 1 (bit 0 stays)
    p0 = d0;
    p1 = (d1 & ~neg) | (r1 & neg);
    p2 = (d2 & ~neg) | (r2 & neg);
}

// once per site list: [segment][COV, F0, F1][6 words]
__global__ __launch_bounds__(256) void k_frag_base(PopArgs a, uint32_t *__restrict__ frag_base)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t sg = i / 3, which = i - 3 * sg;
    if (sg >= a.n_segs)
        return;
    const Seg &S = a.segs[sg];
    uint32_t p0, p1, p2, neg;
    if (which == 0) {
        p0 = S.cov[0]; p1 = S.cov[1]; p2 = S.cov[2]; neg = 0;
    } else if (which == 1) {
        p0 = S.alt[0]; p1 = S.alt[1]; p2 = S.alt[2]; neg = 0xffffffffu;          // (-0 where the row has no alt read)
    } else {
        sliced_diff(S.cov[0], S.cov[1], S.cov[2], S.alt[0], S.alt[1], S.alt[2], p0, p1, p2, neg);
    }
    uint32_t f[6];
    fp6_fragment(p0, p1, p2, neg, f);
    uint2 *o = reinterpret_cast<uint2 *>(frag_base + ((size_t)sg * 3 + which) * 6);
    o[0] = make_uint2(f[0], f[1]);
    o[1] = make_uint2(f[2], f[3]);
    o[2] = make_uint2(f[4], f[5]);
}

// per comparison individual: two threads per segment (one per haplotype word of the individual), eight per window
__global__ __launch_bounds__(256) void k_win_target_x1(PopArgs a, const uint32_t *__restrict__ frag_base,
                                                       uint32_t *__restrict__ rec_ready, uint32_t *__restrict__ wc_ready)
{
    // eight rows' bits -> eight six-bit fields of ones (48 bits), one entry per thread of the workgroup
    __shared__ uint2 spread8[256];
    {
        const uint32_t b = threadIdx.x;
        uint64_t m = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            m |= (b >> j) & 1u ? (uint64_t)0x3f << (6 * j) : 0;
        spread8[b] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned t = blockIdx.y;
    uint32_t tgt = a.targets[a.t_base + t];
    IBDG_CHECK_TGT(tgt, a.lanes, __func__);
    const uint4 *tt = reinterpret_cast<const uint4 *>(a.t32) + (size_t)(tgt >> 6) * a.n_pairs * 64 + (tgt & 63);
    if ((i >> 1) < a.n_segs) {
        const uint32_t sg = i >> 1, ts = i & 1;
        const Seg &S = a.segs[sg];
        IBDG_CHECK_IDX(S.tile, 2 * a.n_pairs, "k_win_target_x1 tile");
        const uint2 at = tile_words(tt, S.tile);
        const uint32_t tw = ts ? at.y : at.x;
        // M: element k = 8 d + j of the fragment is row 4 j + d of the tile
        uint32_t m[6];
        {
            uint2 e[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t x = (tw >> d) & 0x11111111u;           // rows d, 4 + d, ..., 28 + d at bits 0, 4, ..., 28
                x = (x | (x >> 3)) & 0x03030303u;
                x = (x | (x >> 6)) & 0x000f000fu;
                x = (x | (x >> 12)) & 0xffu;
                e[d] = spread8[x];
            }
            m[0] = e[0].x;
            m[1] = e[0].y | (e[1].x << 16);
            m[2] = (e[1].x >> 16) | (e[1].y << 16);
            m[3] = e[2].x;
            m[4] = e[2].y | (e[3].x << 16);
            m[5] = (e[3].x >> 16) | (e[3].y << 16);
        }
        const uint2 *fb = reinterpret_cast<const uint2 *>(frag_base + (size_t)sg * 18);
        const uint2 c0 = fb[0], c1 = fb[1], c2 = fb[2];         // COV
        const uint2 u0 = fb[3], u1 = fb[4], u2 = fb[5];         // F0
        const uint2 v0 = fb[6], v1 = fb[7], v2 = fb[8];         // F1
        // bit 5 of every six-bit field: the pattern repeats after 96 bits
        constexpr uint32_t SG0 = 0x20820820u, SG1 = 0x08208208u, SG2 = 0x82082082u;
        uint32_t *o = rec_ready + ((size_t)t * a.n_segs + sg) * IBDG_RECX_WORDS;
        uint2 *fa = reinterpret_cast<uint2 *>(o + 8 + 6 * ts), *fd = reinterpret_cast<uint2 *>(o + 8 + 6 * (2 + ts));
        fa[0] = make_uint2(c0.x | (m[0] & SG0), c0.y | (m[1] & SG1));
        fa[1] = make_uint2(c1.x | (m[2] & SG2), c1.y | (m[3] & SG0));
        fa[2] = make_uint2(c2.x | (m[4] & SG1), c2.y | (m[5] & SG2));
        fd[0] = make_uint2((v0.x & m[0]) | (u0.x & ~m[0]), (v0.y & m[1]) | (u0.y & ~m[1]));
        fd[1] = make_uint2((v1.x & m[2]) | (u1.x & ~m[2]), (v1.y & m[3]) | (u1.y & ~m[3]));
        fd[2] = make_uint2((v2.x & m[4]) | (u2.x & ~m[4]), (v2.y & m[5]) | (u2.y & ~m[5]));
        if (ts == 0)
            mx_record_header(o, S, at);
    }
    if ((i >> 3) < a.n_win) {                // threads 8w..8w+7: the constants of window w (as k_win_target_mx, ibd1)
        const uint32_t w = i >> 3;
        uint32_t a0cov = 0, a1cov = 0, a0alt = 0, a1alt = 0;
        const uint32_t s1 = a.wconst[w + 1].seg_begin;
        for (uint32_t s = a.wconst[w].seg_begin + (i & 7); s < s1; s += 8) {
            const Seg &S = a.segs[s];
            const uint2 at = tile_words(tt, S.tile);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                a0cov += (uint32_t)__popc(at.x & S.cov[k]) << k;
                a1cov += (uint32_t)__popc(at.y & S.cov[k]) << k;
                a0alt += (uint32_t)__popc(at.x & S.alt[k]) << k;
                a1alt += (uint32_t)__popc(at.y & S.alt[k]) << k;
            }
        }
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) {
            a0cov += __shfl_xor(a0cov, m);
            a1cov += __shfl_xor(a1cov, m);
            a0alt += __shfl_xor(a0alt, m);
            a1alt += __shfl_xor(a1alt, m);
        }
        if ((i & 7) == 0) {
            const uint32_t *wcs = reinterpret_cast<const uint32_t *>(a.wconst + w);
            uint4 *o = reinterpret_cast<uint4 *>(wc_ready + ((size_t)t * a.n_win + w) * IBDG_WC_WORDS);
            const uint32_t AT = wcs[4];
            const uint32_t bias = 1u << 25;              // (see k_win_target_mx)
            o[0] = make_uint4(wcs[2], 8 * AT, 8 * a0cov - bias, 8 * a1cov - bias);
            o[1] = make_uint4(8 * (AT - a0alt) - bias, 8 * (AT - a1alt) - bias, 0, 0);
        }
    }
}

__global__ __launch_bounds__(256) void k_win_target_mt(PopArgs a, uint32_t *__restrict__ rec_ready,
                                                       uint32_t *__restrict__ wc_ready)
{
    constexpr int TB = IBDG_MT;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned g = blockIdx.y;                     // group of TB comparison individuals
    const uint4 *tt[TB];
#pragma unroll
    for (int j = 0; j < TB; ++j) {
        const uint32_t tgt = a.targets[a.t_base + g * TB + j];
        tt[j] = reinterpret_cast<const uint4 *>(a.t32) + (size_t)(tgt >> 6) * a.n_pairs * 64 + (tgt & 63);
    }
    if (i < a.n_segs) {
        const Seg S = a.segs[i];
        uint4 *o = reinterpret_cast<uint4 *>(rec_ready + ((size_t)g * a.n_segs + i) * IBDG_RECM_WORDS);
        o[0] = make_uint4(S.flags, S.cov[0], S.cov[1], S.cov[2]);
        o[1] = make_uint4(S.alt[0], S.alt[1], 0, 0);
#pragma unroll
        for (int j = 0; j < TB; j += 2) {
            const uint2 ta = tile_words(tt[j], S.tile);
            const uint2 tb = j + 1 < TB ? tile_words(tt[j + 1 < TB ? j + 1 : j], S.tile) : make_uint2(0, 0);
            o[2 + j / 2] = make_uint4(ta.x, ta.y, tb.x, tb.y);
        }
    }
    if ((i >> 3) < a.n_win) {
        const uint32_t w = i >> 3;
        uint32_t acc[TB][4];
#pragma unroll
        for (int j = 0; j < TB; ++j)
            acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0;
        const uint32_t s1 = a.wconst[w + 1].seg_begin;
        for (uint32_t s = a.wconst[w].seg_begin + (i & 7); s < s1; s += 8) {
            const Seg &S = a.segs[s];
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                const uint2 at = tile_words(tt[j], S.tile);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    acc[j][0] += (uint32_t)__popc(at.x & S.cov[k]) << k;
                    acc[j][1] += (uint32_t)__popc(at.y & S.cov[k]) << k;
                    acc[j][2] += (uint32_t)__popc(at.x & S.alt[k]) << k;
                    acc[j][3] += (uint32_t)__popc(at.y & S.alt[k]) << k;
                }
            }
        }
#pragma unroll
        for (int m = 1; m < 8; m <<= 1)
#pragma unroll
            for (int j = 0; j < TB; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    acc[j][q] += __shfl_xor(acc[j][q], m);
        if ((i & 7) == 0) {
            const uint32_t *wcs = reinterpret_cast<const uint32_t *>(a.wconst + w);
            uint4 *o = reinterpret_cast<uint4 *>(wc_ready + ((size_t)g * a.n_win + w) * IBDG_WCM_WORDS);
            const uint32_t AT = wcs[4];
            o[0] = make_uint4(wcs[0], wcs[1], wcs[2], wcs[3]);
            o[1] = make_uint4(16 * AT, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TB; ++j)
                o[2 + j] = make_uint4(16 * acc[j][0], 16 * acc[j][1], 16 * (AT - acc[j][2]), 16 * (AT - acc[j][3]));
        }
    }
}

// ---------------------------------------------------------------------------
void launch_transpose32(const uint64_t *panel, uint32_t stride, size_t n_rows, uint32_t n_chunks,
                        uint32_t n_pairs, uint32_t *t32, hipStream_t st)
{
    if (n_pairs == 0)
        return;
    hipLaunchKernelGGL(k_transpose32, dim3(n_pairs, (n_chunks + 7) / 8), dim3(512), 0, st, panel, stride,
                       n_rows, n_chunks, n_pairs, reinterpret_cast<uint4 *>(t32));
}

void launch_gather_transpose32(const uint64_t *panel, uint32_t stride, const uint2 *rec_cov, uint32_t n_cov,
                               uint32_t window, uint32_t win_rows, uint32_t n_chunks, uint32_t n_pairs, uint32_t *t32,
                               hipStream_t st)
{
    if (n_pairs == 0)
        return;
    hipLaunchKernelGGL(k_gather_transpose32, dim3(n_pairs, (n_chunks + 7) / 8), dim3(512), 0, st, panel, stride, rec_cov,
                       n_cov, window, win_rows, n_chunks, n_pairs, reinterpret_cast<uint4 *>(t32));
}

// ev.start / ev.stop (may be null): events the dispatch itself updates with the kernel's start and
// stop time (hipExtLaunchKernel) -- no event-record packet on the stream.
void launch_win_target(const PopArgs &a, unsigned n_targets, hipStream_t st, KernelEvents ev)
{
    if (a.n_win == 0)
        return;
    if (a.mx_counts && a.ibd1 && a.frag_base && a.tab_in_lds) {
        const uint32_t n = a.n_segs * 2 > a.n_win * 8 ? a.n_segs * 2 : a.n_win * 8;
        hipExtLaunchKernelGGL(k_win_target_x1, dim3((n + 255) / 256, n_targets), dim3(256), 0, st, ev.start, ev.stop, 0, a, a.frag_base,
                              const_cast<uint32_t *>(a.rec_ready), const_cast<uint32_t *>(a.wc_ready));
        return;
    }
    if (a.mx_counts) {
        const uint32_t n = a.n_segs * 4 > a.n_win * 8 ? a.n_segs * 4 : a.n_win * 8;
        hipExtLaunchKernelGGL(k_win_target_mx, dim3((n + 255) / 256, n_targets), dim3(256), 0, st, ev.start, ev.stop, 0, a,
                              const_cast<uint32_t *>(a.rec_ready), const_cast<uint32_t *>(a.wc_ready));
        return;
    }
    const uint32_t n = a.n_segs > a.n_win * 8 ? a.n_segs : a.n_win * 8;
    hipExtLaunchKernelGGL(k_win_target, dim3((n + 255) / 256, n_targets), dim3(256), 0, st, ev.start, ev.stop, 0, a,
                          const_cast<uint32_t *>(a.rec_ready), const_cast<uint32_t *>(a.wc_ready));
}

// the IBD1 form's three fragments per segment that do not depend on the comparison individual (72 bytes per segment)
void launch_frag_base(const PopArgs &a, uint32_t *frag_base, hipStream_t st)
{
    if (a.n_segs == 0)
        return;
    hipLaunchKernelGGL(k_frag_base, dim3((a.n_segs * 3 + 255) / 256), dim3(256), 0, st, a, frag_base);
}

size_t ld_popcount_rec_bytes(int mx_counts) { return (mx_counts ? IBDG_RECX_WORDS : IBDG_REC_WORDS) * 4; }

// The same for groups of IBDG_MT comparison individuals (a.t_base = first of them, n_groups groups)
int ld_popcount_mt_width(void) { return IBDG_MT; }
size_t ld_popcount_mt_rec_bytes(void) { return IBDG_RECM_WORDS * 4; }
size_t ld_popcount_mt_wc_bytes(void) { return IBDG_WCM_WORDS * 4; }

void launch_win_target_mt(const PopArgs &a, unsigned n_groups, hipStream_t st, KernelEvents ev)
{
    if (a.n_win == 0 || n_groups == 0)
        return;
    const uint32_t n = a.n_segs > a.n_win * 8 ? a.n_segs : a.n_win * 8;
    hipExtLaunchKernelGGL(k_win_target_mt, dim3((n + 255) / 256, n_groups), dim3(256), 0, st, ev.start, ev.stop, 0, a,
                          const_cast<uint32_t *>(a.rec_ready), const_cast<uint32_t *>(a.wc_ready));
}

}  // namespace ibdg
