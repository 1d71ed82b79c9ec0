// ibdg_ld_popcount.hip -- the fast --LD kernel: exponent counting on a tile-transposed panel.
//
// What it computes is what src/ibdgem.c:669-722 and :736-753 of the reference compute:
// for every background individual the five window products of P(D|G) factors, then the
// background averages.  How: every factor is one of (src/ibd-math.c:57-70)
//     pDg[0] = C (1-e)^r e^a      pDg[1] = C (1/2)^(r+a)      pDg[2] = C (1-e)^a e^r
// (C = binomial coefficient, r/a = n_ref/n_alt of the row, e = epsilon), so a product over the
// rows of a window is exactly
//     prod = K * (1-e)^E1 * e^E2 * 2^-E3,    K = prod C,
//          = K' * rho^E2 * sigma^E3,  K' = K (1-e)^reads, rho = e/(1-e), sigma = 1/(2(1-e)),
//     E3 = reads on rows where the genotype is 1, E2 = reads that contradict a homozygous
//     genotype (alt reads under 0, ref reads under 2), E1 = all reads - E2 - E3.
// E2 and E3 are integers: sums of small per-row weights over the rows selected by haplotype
// bits -- weighted popcounts.  With the panel transposed into 32-row tiles (one u32 per
// individual, haplotype and tile) a weighted popcount over 32 rows is, per bit-plane k of the
// weights, one v_and_b32 with a wave-uniform mask and one accumulating v_bcnt_u32_b32.
// Per individual and window nine such sums are needed (x0,x1 = its two haplotypes, t0,t1 the
// target's, cov = r+a):
//     A(x0) A(x1)             <x, alt>
//     C(x0) C(x1) C(x0&x1)    <x, cov>
//     G(x,t) for 4 pairs      <x & t, cov>
// and the exponents follow without further per-row work:
//     pDg[x0+x1]:  E3 = C(x0)+C(x1)-2C(x0&x1)        E2 = ALT - A(x0) - A(x1) + C(x0&x1)
//     pDg[t +x ]:  E3 = <t,cov> + C(x) - 2G(x,t)     E2 = ALT - <t,alt> - A(x) + G(x,t)
// The integers are exact, so rows may be visited in any grouping; the floating-point value
//     mK' * ldexp(m1[E2] * m2[E3], eK' + e1[E2] + e2[E3])
// (tables of rho^n and sigma^n as mantissa/exponent pairs, built on the host in extended
// precision; mK' is applied after the sum over the background) carries ~4 roundings, i.e. it is CLOSER to the exact product than the reference's
// 100 sequential multiplications: against an extended-precision reference of the same operation it is within 4 units
// of roundoff (2^-53) on MI355X at every window length, where its bound is 25.6 units (tests/hp_ref.py; bar against the
// oracle: 1e-10).
// Values below the double range come out as 0/subnormal from the final ldexp, like the
// reference's running product.  The host enables this kernel only when the P(D|G) table is
// the unclamped binomial form (no DBL_MIN clamp, exact coefficients); otherwise the strict
// multiplying kernel in ibdg_kernels.hip is used.
//
// Round 4: for ONE comparison individual per workgroup the four sums of a haplotype word that a lane needs --
// <x,cov> <x,alt> <x & t0,cov> <x & t1,cov> -- come from one v_mfma_scale_f32_16x16x128_f8f6f4 with a block-diagonal FP6
// weight matrix and the word's bits as FP4 numbers (k_win_target_mx in ibdg_ld_images.hip, lds_fetch_mx, segment_mx; template parameter MX
// of k_ld_popcount; DESIGN.md s4.1, docs/DESIGN_rounds_1-4.md s4.1c); only <x0 & x1,cov> is still three (mask, count) pairs.  The sums are the same
// integers, the results the same bits.  The pairs described above remain the form of option mx_counts 0 and of the kernel
// for groups of four comparison individuals (k_ld_popcount_mt).
//
// Round 5, the IBD1 form (k_ld_popcount<.., IBD1 = true>; PopArgs::ibd1): the product of an individual's OWN
// genotype factors (pDg[x0+x1] above) does not depend on the comparison individual, so ONE launch per site list and background
// keeps it for every individual and window (PopArgs::p2_out) and later launches count the four pDg[t+x] products only: the
// rows' weights become cov (1 - 2 t) and t cov - alt (signed FP6), the instruction's four sums per word are
//     C(x) - 2 G(x,t0)   C(x) - 2 G(x,t1)   G(x,t0) - A(x)   G(x,t1) - A(x)
// -- E3 and E2 above up to the window's constants --, the accumulators start from 1.5 * 2^23 so that their bits ARE the sums,
// and the finalising step takes IBD0 from the kept products in the additions of a launch that counts everything
// (ibd0_from_pass, ibdg_ld_dev.h): the same bits from either form.  A new individual's images are bit selections between
// three fragments made once per site list (k_frag_base, k_win_target_x1).
//
// The file top to bottom: LDS reads and wave sums in assembly, the counting statements, the tile ring (TileRing), the start of
// a workgroup (run_span, run_prologue), one segment step per form (segment_vec / _mt / _mx / _x1), the window ends, the
// forms of k_ld_popcount (run_vector_form, run_matrix_form, run_ibd1_form), k_ld_popcount_mt, k_ld_finalize, the launchers.
// The images these kernels stage are built in ibdg_ld_images.hip; their widths and the LDS layout are in ibdg_ld_layout.h.
#include "ibdg_kernels.h"
#include "ibdg_ld_dev.h"
#include "ibdg_ld_layout.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

// cache policy of the tile stream's direct-to-LDS loads (aux of global_load_lds: 0 default, 2 = nt, non-temporal): every tile
// pair is read once by one wave, 2.56 GB per launch = ten times the last-level cache.  nt measured 1.5-2 % faster per step
// on one box, builds alternating (profiles/r05_ab_nt.txt: 0.606 / 0.607 against 0.617 / 0.615 ms with a new individual per
// step, 0.581 / 0.586 against 0.596 / 0.596 with the same one); -DIBDG_TILE_AUX=0 brings the default policy back.
#ifndef IBDG_TILE_AUX
#define IBDG_TILE_AUX 2
#endif

namespace ibdg {

typedef int mx_v8i __attribute__((ext_vector_type(8)));
typedef float mx_v4f __attribute__((ext_vector_type(4)));
typedef uint32_t mx_u4 __attribute__((ext_vector_type(4)));      // (plain vector types: the struct ones cannot be tied asm operands)
typedef uint32_t mx_u2 __attribute__((ext_vector_type(2)));


// the bits of a tile word as 32 FP4 numbers (0 or 0.5 / 1 / 2 / 0.5 by dword, see above)
__device__ __forceinline__ mx_v8i bits_to_fp4(uint32_t x)
{
    mx_v8i b = {0, 0, 0, 0, 0, 0, 0, 0};
    b[0] = (int)(x & 0x11111111u);
    b[1] = (int)(x & 0x22222222u);
    b[2] = (int)(x & 0x44444444u);
    b[3] = (int)((x >> 3) & 0x11111111u);
    return b;
}

// the lanes that hold a non-zero A fragment: 20 kb + sum
#define IBDG_MX_A_LANES 0xF0000F0000F0000Full

// One segment's LDS reads of the matrix-core form: the broadcast header (flags and the cov planes for the x0&x1 counts),
// the lane's two tile words and -- in the 16 lanes that carry one -- the A fragment; the other lanes keep their zeros.
__device__ __forceinline__ void lds_fetch_mx(uint4 &h0, uint2 &x, mx_u4 &a_lo, mx_u2 &a_hi, uint32_t rec_addr, uint32_t x_addr,
                                             uint32_t frag_addr)
{
    // (EXEC is narrowed to the fragment lanes for two reads and put back to what it WAS: a caller inside a divergent
    // branch keeps its dead lanes dead)
    uint64_t exec_was;
    asm volatile("ds_read_b128 %0, %5\n\t"
                 "ds_read_b64 %1, %6\n\t"
                 "s_mov_b64 %4, exec\n\t"
                 "s_and_b64 exec, %4, %8\n\t"
                 "ds_read2_b64 %2, %7 offset1:1\n\t"
                 "ds_read_b64 %3, %7 offset:16\n\t"
                 "s_mov_b64 exec, %4\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(h0), "=&v"(x), "+v"(a_lo), "+v"(a_hi), "=&s"(exec_was)
                 : "v"(rec_addr), "v"(x_addr), "v"(frag_addr), "s"((uint64_t)IBDG_MX_A_LANES)
                 : "memory", "scc");
}

// The same for the IBD1 form, from ONE address register: frag_base = record + 24 * (lane & 3) per lane.  The record's first
// word (its control word) is read by every lane at its own base -- lane 0's is the record itself, and only lane 0's copy is
// used (v_readfirstlane) --, the fragment of lane 20 kb + sum sits 32 bytes further on.
__device__ __forceinline__ void lds_fetch_x1(uint32_t &ctl, uint2 &x, mx_u4 &a_lo, mx_u2 &a_hi, uint32_t x_addr, uint32_t frag_base)
{
    uint64_t exec_was;
    asm volatile("ds_read_b32 %0, %6\n\t"
                 "ds_read_b64 %1, %5\n\t"
                 "s_mov_b64 %4, exec\n\t"
                 "s_and_b64 exec, %4, %7\n\t"
                 "ds_read2_b64 %2, %6 offset0:4 offset1:5\n\t"
                 "ds_read_b64 %3, %6 offset:48\n\t"
                 "s_mov_b64 exec, %4\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(ctl), "=&v"(x), "+v"(a_lo), "+v"(a_hi), "=&s"(exec_was)
                 : "v"(x_addr), "v"(frag_base), "s"((uint64_t)IBDG_MX_A_LANES)
                 : "memory", "scc");
}

// Two wave-wide sums at once through a 1 KiB LDS scratch of the wave: every lane writes its two
// addends into two arrays of 64 doubles; lane 32j+p then reads elements 2p, 2p+1 of sum j (one
// 16-byte read at scratch + 16*lane), adds them, and the 32 lanes of half j finish with five
// exchange-and-add steps.  Every lane of the first half ends up with the total of the first sum,
// every lane of the second half with the second.  Fixed order, no barrier (the scratch is the wave's
// own and a wave's LDS operations execute in order); 6 VALU instructions for the two sums of a window.
__device__ __forceinline__ double wave_sum2(double a, double b, uint32_t scr_w, uint32_t scr_r)
{
    uint4 r;
    asm volatile("ds_write_b64 %1, %2\n\t"
                 "ds_write_b64 %1, %3 offset:512\n\t"
                 "ds_read_b128 %0, %4\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(r)
                 : "v"(scr_w), "v"(a), "v"(b), "v"(scr_r)
                 : "memory");
    double v = __hiloint2double((int)r.y, (int)r.x) + __hiloint2double((int)r.w, (int)r.z);
    // a butterfly over the 32 lanes of each half: after every step the lanes of a group hold the same
    // subtotal, so the tree is the one of the DPP sequence this replaced (quad_perm, quad_perm,
    // row_half_mirror, row_mirror, row_bcast:15) and the totals are the same bits
    v = swz_add<1>(v);
    v = swz_add<2>(v);
    v = swz_add<4>(v);
    v = swz_add<8>(v);
    v = swz_add<16>(v);
    return v;
}

// The same with the five exchange steps as DPP moves (two v_mov_dpp and the add per step: 15 vector instructions instead
// of 5, but no trip through the LDS crossbar and nothing to wait for): the additions and their order are those of the
// swizzle form -- after every step the lanes of a group hold the same subtotal, so a mirror within the group's double is the
// exchange with lane ^ X -- and the totals are the same bits.  For the matrix-core form, whose wave time is LDS round trips.
// Lanes 31 and 63 hold the totals of the first and second sum (row_bcast:15 fills rows 1 and 3 only).
__device__ __forceinline__ double wave_sum2_dpp(double a, double b, uint32_t scr_w, uint32_t scr_r)
{
    uint4 r;
    asm volatile("ds_write_b64 %1, %2\n\t"
                 "ds_write_b64 %1, %3 offset:512\n\t"
                 "ds_read_b128 %0, %4\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(r)
                 : "v"(scr_w), "v"(a), "v"(b), "v"(scr_r)
                 : "memory");
    double v = __hiloint2double((int)r.y, (int)r.x) + __hiloint2double((int)r.w, (int)r.z);
    v = dpp_add<0xB1, 0xf>(v);      // quad_perm [1,0,3,2]      lane ^ 1
    v = dpp_add<0x4E, 0xf>(v);      // quad_perm [2,3,0,1]      lane ^ 2
    v = dpp_add<0x141, 0xf>(v);     // row_half_mirror          the other quad of the eight
    v = dpp_add<0x140, 0xf>(v);     // row_mirror               the other eight of the row
    v = dpp_add<0x142, 0xa>(v);     // row_bcast:15 into rows 1 and 3: the other row of the half
    return v;
}

// Two CONSECUTIVE windows' sums in that tree (the IBD1 form's paired window end): the first window of a pair parks every
// lane's value in the first array of the wave's scratch and goes on -- no wait, no reduction --, the second one writes the
// second array and does the rest of wave_sum2_dpp.  Lane 31 ends up with the first window's total, lane 63 with the
// second's; the last step goes without its row mask (wave_sum_lane63_only: the other rows take sums nobody reads, and the
// step needs no zeroed destination).  The pair add is the lane ^ 1 level of wave_sum_lane63_only, the five steps are the
// lane number's bits 1-5: the same additions, the same bits.  16 vector instructions for two windows instead of 36.
__device__ __forceinline__ void wave_sum_park(double a, uint32_t scr_w)
{
    asm volatile("ds_write_b64 %0, %1" : : "v"(scr_w), "v"(a) : "memory");
}

__device__ __forceinline__ double wave_sum_pair_dpp(double b, uint32_t scr_w, uint32_t scr_r)
{
    uint4 r;
    asm volatile("ds_write_b64 %1, %2 offset:512\n\t"
                 "ds_read_b128 %0, %3\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(r)
                 : "v"(scr_w), "v"(b), "v"(scr_r)
                 : "memory");
    double v = __hiloint2double((int)r.y, (int)r.x) + __hiloint2double((int)r.w, (int)r.z);
    v = dpp_add<0xB1, 0xf>(v);      // quad_perm [1,0,3,2]
    v = dpp_add<0x4E, 0xf>(v);      // quad_perm [2,3,0,1]
    v = dpp_add<0x141, 0xf>(v);     // row_half_mirror
    v = dpp_add<0x140, 0xf>(v);     // row_mirror
    v = dpp_add<0x142, 0xf>(v);     // row_bcast:15: rows 1 and 3 take the other row of their half
    return v;
}

// ---------------------------------------------------------------------------
// The --LD loop.
//
// Work split: a workgroup = 8 waves = 8 chunks of 64 background individuals (one individual
// per lane) x one run of consecutive windows (run_begin[]: up to `win_per_group` windows, fewer
// towards the end of the grid -- the host's guided run lengths; workgroups of a run are adjacent
// in blockIdx order).  Each wave streams its chunk's tile pairs exactly once.
//
// Two kernels share this design: k_ld_popcount (one comparison individual per workgroup) and
// k_ld_popcount_mt (four).  Both perform the same operations in the same order per result.
// Their loops are written so that a window's first segment STARTS the counters (segment_*<FIRST = true>)
// and the others add to them (segment_*<false>): nothing is reset between windows.
//
// Data movement (all of it asynchronous to the arithmetic):
//   * once per workgroup the run's segment records (+ the target's haplotype words per
//     segment), the per-window constants and the two power tables are copied to LDS;
//   * the wave's tile pairs go HBM -> LDS by direct-to-LDS loads (global_load_lds_dwordx4,
//     1 KiB per instruction, no VGPRs) into a private ring of NS slots, NS-1 loads in flight
//     while a pair is consumed.  Landing is tracked with counted s_waitcnt vmcnt
//     (vector-memory ops of a wave complete in issue order).
//   * per segment one asm statement reads the hot half of the record with two broadcast
//     ds_read_b128 (masks and the target's words land in VGPRs: VALU instructions with VGPR
//     operands only issue at twice the rate of those with an SGPR operand) and the lane's own
//     two tile words with one ds_read_b64.
//   All LDS reads in the loop are asm: hipcc drains vmcnt(0) before any LDS read that follows
//   a direct-to-LDS load, which would serialise the ring (and so would table look-ups from
//   global memory at the end of every window -- hence the tables in LDS).
// Arithmetic per segment: per weight bit-plane 14 VALU ops for the seven cov-weighted counts
// and 4 for the two alt-weighted ones; three cov planes and two alt planes unconditionally,
// higher planes (rare) under one uniform test.
// At the end of each window the lane turns its counts into the five products, the wave sums
// count[n]*product over its 64 individuals (DPP moves, fixed order) and lane 63 stores the
// per-chunk partial; k_ld_finalize adds the chunks (one wave per window, same fixed order),
// applies the mantissa of K' and divides.
// ---------------------------------------------------------------------------


// Issue and wait in ONE statement: an asm output must be final when the statement ends,
// because hipcc is free to copy it to another register right afterwards (it did, with the
// wait in a later statement: the copy read the register before the LDS data had landed).
// The LDS latency is covered by the other resident waves of the SIMD instead.
__device__ __forceinline__ void lds_fetch(uint4 &h0, uint4 &h1, uint2 &x, uint32_t rec_addr, uint32_t x_addr)
{
    asm volatile("ds_read_b128 %0, %3\n\t"
                 "ds_read_b128 %1, %3 offset:16\n\t"
                 "ds_read_b64 %2, %4\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(h0), "=&v"(h1), "=&v"(x)
                 : "v"(rec_addr), "v"(x_addr)
                 : "memory");
}

// The counting itself is written in assembly, one statement per group of (mask, count) pairs, for the sake of ONE
// scalar instruction inside every pair:
//     v_and_b32 t, x, m ; s_nop 0 ; v_bcnt_u32_b32 c, t, c
// Back to back, a 1:1 stream of v_and_b32 (2.2 cycles per wave alone) and v_bcnt_u32_b32 (4.2) issues at 3.8-4.0
// cycles per instruction; with one scalar instruction per pair -- s_nop 0, any SALU instruction, before or after
// the count -- it issues at 3.2, the average of its parts; two per pair, one per four vector instructions or
// s_nop 1 lose it again (tools/ubench/nop_mix.hip, profiles/r02_nop_mix.txt).  hipcc knows nothing of this and
// moves scalar work of the loop into the stream wherever it fits, so the pairs are fenced by scheduling barriers
// (segment_vec, segment_mt) and everything scalar is computed before them.
// A0..: what the count starts from -- "0" for the first segment of a window (the counters start there, nothing is
// zeroed between windows), the counter itself afterwards.
// One statement per segment (per weight plane in the kernel for several individuals): between two asm statements
// hipcc's hazard recogniser puts an s_nop of its own, a second scalar instruction for that pair.
#define IBDG_PAIR_SET(tmp, a, b, cnt) \
    "v_and_b32 %[" #tmp "], %[" #a "], %[" #b "]\n\ts_nop 0\n\tv_bcnt_u32_b32 %[" #cnt "], %[" #tmp "], 0\n\t"
#define IBDG_PAIR_ADD(tmp, a, b, cnt) \
    "v_and_b32 %[" #tmp "], %[" #a "], %[" #b "]\n\ts_nop 0\n\tv_bcnt_u32_b32 %[" #cnt "], %[" #tmp "], %[" #cnt "]\n\t"
// C(x0) C(x1) C(x0&x1) and the four G(x,t) of weight plane k (u0 = x0 & cov, u1 = x1 & cov are shared)
#define IBDG_COV_PLANE_TEXT(P, k) \
    P(u0, x0, cov##k, c0##k) P(u1, x1, cov##k, c1##k) P(t, hom, cov##k, ch##k) \
    P(t, u0, at0, g00##k) P(t, u1, at0, g01##k) P(t, u0, at1, g10##k) P(t, u1, at1, g11##k)
#define IBDG_ALT_TEXT(P) P(t, x0, alt0, a00) P(t, x1, alt0, a10) P(t, x0, alt1, a01) P(t, x1, alt1, a11)
#define IBDG_SEG_TEXT(P) IBDG_COV_PLANE_TEXT(P, 0) IBDG_COV_PLANE_TEXT(P, 1) IBDG_COV_PLANE_TEXT(P, 2) IBDG_ALT_TEXT(P)
#define IBDG_CNT3(C, name, arr) [name##0] C(arr[0]), [name##1] C(arr[1]), [name##2] C(arr[2])

// the 25 counts of one segment for one comparison individual
template <bool FIRST>
__device__ __forceinline__ void count_segment(uint32_t (&c0)[3], uint32_t (&c1)[3], uint32_t (&ch)[3], uint32_t (&g00)[3],
                                              uint32_t (&g01)[3], uint32_t (&g10)[3], uint32_t (&g11)[3], uint32_t (&A0)[2],
                                              uint32_t (&A1)[2], uint32_t x0, uint32_t x1, uint32_t hom, uint32_t cov0,
                                              uint32_t cov1, uint32_t cov2, uint32_t alt0, uint32_t alt1, uint32_t at0, uint32_t at1)
{
    uint32_t u0, u1, t;
#define IBDG_OUT_SET(v) "=&v"(v)
#define IBDG_OUT_ADD(v) "+v"(v)
#define IBDG_SEG_OPERANDS(C)                                                                                              \
    : IBDG_CNT3(C, c0, c0), IBDG_CNT3(C, c1, c1), IBDG_CNT3(C, ch, ch), IBDG_CNT3(C, g00, g00), IBDG_CNT3(C, g01, g01),   \
      IBDG_CNT3(C, g10, g10), IBDG_CNT3(C, g11, g11), [a00] C(A0[0]), [a01] C(A0[1]), [a10] C(A1[0]), [a11] C(A1[1]),     \
      [u0] "=&v"(u0), [u1] "=&v"(u1), [t] "=&v"(t)                                                                        \
    : [x0] "v"(x0), [x1] "v"(x1), [hom] "v"(hom), [cov0] "v"(cov0), [cov1] "v"(cov1), [cov2] "v"(cov2), [alt0] "v"(alt0), \
      [alt1] "v"(alt1), [at0] "v"(at0), [at1] "v"(at1)
    if (FIRST)
        asm volatile(IBDG_SEG_TEXT(IBDG_PAIR_SET) IBDG_SEG_OPERANDS(IBDG_OUT_SET));
    else
        asm volatile(IBDG_SEG_TEXT(IBDG_PAIR_ADD) IBDG_SEG_OPERANDS(IBDG_OUT_ADD));
#undef IBDG_SEG_OPERANDS
}

// the same for four comparison individuals, one weight plane per statement: the common three counts and 4 x 4 G(x,t)
#define IBDG_G4_TEXT(P, j) P(t, u0, ta##j, g##j##0) P(t, u1, ta##j, g##j##1) P(t, u0, tb##j, g##j##2) P(t, u1, tb##j, g##j##3)
#define IBDG_PLANE4_TEXT(P) P(u0, x0, cov, c0) P(u1, x1, cov, c1) P(t, hom, cov, ch) IBDG_G4_TEXT(P, 0) IBDG_G4_TEXT(P, 1) IBDG_G4_TEXT(P, 2) IBDG_G4_TEXT(P, 3)
#define IBDG_G4_OPS(C, j) [g##j##0] C(gq[j][0][k]), [g##j##1] C(gq[j][1][k]), [g##j##2] C(gq[j][2][k]), [g##j##3] C(gq[j][3][k])
template <bool FIRST>
__device__ __forceinline__ void count_plane_mt(uint32_t &c0, uint32_t &c1, uint32_t &ch, uint32_t (&gq)[4][4][3], int k,
                                               uint32_t x0, uint32_t x1, uint32_t hom, uint32_t cov, const uint32_t (&tw)[4][2])
{
    uint32_t u0, u1, t;
#define IBDG_P4_OPERANDS(C)                                                                                               \
    : [c0] C(c0), [c1] C(c1), [ch] C(ch), IBDG_G4_OPS(C, 0), IBDG_G4_OPS(C, 1), IBDG_G4_OPS(C, 2), IBDG_G4_OPS(C, 3),     \
      [u0] "=&v"(u0), [u1] "=&v"(u1), [t] "=&v"(t)                                                                        \
    : [x0] "v"(x0), [x1] "v"(x1), [hom] "v"(hom), [cov] "v"(cov), [ta0] "v"(tw[0][0]), [tb0] "v"(tw[0][1]),               \
      [ta1] "v"(tw[1][0]), [tb1] "v"(tw[1][1]), [ta2] "v"(tw[2][0]), [tb2] "v"(tw[2][1]), [ta3] "v"(tw[3][0]), [tb3] "v"(tw[3][1])
    if (FIRST)
        asm volatile(IBDG_PLANE4_TEXT(IBDG_PAIR_SET) IBDG_P4_OPERANDS(IBDG_OUT_SET));
    else
        asm volatile(IBDG_PLANE4_TEXT(IBDG_PAIR_ADD) IBDG_P4_OPERANDS(IBDG_OUT_ADD));
#undef IBDG_P4_OPERANDS
}

template <bool FIRST>
__device__ __forceinline__ void count_alt(uint32_t (&A0)[2], uint32_t (&A1)[2], uint32_t x0, uint32_t x1, uint32_t alt0, uint32_t alt1)
{
    uint32_t t;
    if (FIRST)
        asm volatile(IBDG_ALT_TEXT(IBDG_PAIR_SET)
                     : [a00] "=&v"(A0[0]), [a01] "=&v"(A0[1]), [a10] "=&v"(A1[0]), [a11] "=&v"(A1[1]), [t] "=&v"(t)
                     : [x0] "v"(x0), [x1] "v"(x1), [alt0] "v"(alt0), [alt1] "v"(alt1));
    else
        asm volatile(IBDG_ALT_TEXT(IBDG_PAIR_ADD)
                     : [a00] "+v"(A0[0]), [a01] "+v"(A0[1]), [a10] "+v"(A1[0]), [a11] "+v"(A1[1]), [t] "=&v"(t)
                     : [x0] "v"(x0), [x1] "v"(x1), [alt0] "v"(alt0), [alt1] "v"(alt1));
}

// the record of a segment for four comparison individuals (IBDG_RECM_WORDS) and the lane's tile words
__device__ __forceinline__ void lds_fetch_mt(uint4 &h0, uint4 &h1, uint4 &h2, uint4 &h3, uint2 &x, uint32_t rec_addr,
                                             uint32_t x_addr)
{
    asm volatile("ds_read_b128 %0, %5\n\t"
                 "ds_read_b128 %1, %5 offset:16\n\t"
                 "ds_read_b128 %2, %5 offset:32\n\t"
                 "ds_read_b128 %3, %5 offset:48\n\t"
                 "ds_read_b64 %4, %6\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(h0), "=&v"(h1), "=&v"(h2), "=&v"(h3), "=&v"(x)
                 : "v"(rec_addr), "v"(x_addr)
                 : "memory");
}

// ---------------------------------------------------------------------------
// The tile ring of one wave: NS slots of 1 KiB, filled by direct-to-LDS loads in issue order and read one pair at a time.
// Slot of pair q: (q - q0) % NS, q0 = the run's first pair.  q_issue is the next pair to request, a NOMINAL number that
// runs past the run's last pair q_last; what happens there is the guard policy:
//   REREQUEST = false (vector forms): nothing is requested past q_last, so fewer than NS - 1 loads may be in flight and
//     the wait falls back to vmcnt(0);
//   REREQUEST = true (matrix-core forms): every advance requests a pair -- past the run's last one that pair again, into
//     a slot nobody reads any more -- so the count of loads in flight stays the nominal one and one counted wait serves.
// ---------------------------------------------------------------------------
template <int NS, bool REREQUEST>
struct TileRing {
    static constexpr int SLOTS = NS;
    const uint4 *xt;            // the lane's 16 bytes of the wave's chunk (+ pair * 64)
    char *ring;                 // the wave's NS slots
    uint32_t q0, q_last;
    uint32_t q_issue;

    __device__ __forceinline__ void request()
    {
        if (REREQUEST || q_issue <= q_last)
            __builtin_amdgcn_global_load_lds((const void *)(xt + (size_t)(q_issue < q_last ? q_issue : q_last) * 64),
                                             (lds_void *)(ring + ((q_issue - q0) % NS) * 1024), 16, 0, IBDG_TILE_AUX);
        ++q_issue;
    }
    // pairs q0 .. q0+NS-1
    __device__ __forceinline__ void prime()
    {
#pragma unroll
        for (int i = 0; i < NS; ++i)
            request();
    }
    // the oldest pair in flight has landed: all but the NS - 1 requests after it are complete
    __device__ __forceinline__ void wait_first()
    {
        if (REREQUEST || q_issue - 1 <= q_last)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NS - 1) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // move on by adv pairs: as many requests, then the pair the next segment reads has landed
    __device__ __forceinline__ void advance(uint32_t adv)
    {
        for (uint32_t i = 0; i < adv; ++i)
            request();
        wait_first();
    }
    // leave no direct-to-LDS load in flight when the wave ends
    __device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

// Staging of the window constants: the table base each word indexes is added on the way into LDS.  i = index of the uint4
// within the run's constants: two per window of one comparison individual, WCW / 4 per window of a group.
template <int WCW>
__device__ __forceinline__ uint4 stage_wc(uint4 v, uint32_t i, uint32_t tab1, uint32_t tab2)
{
    if constexpr (WCW == IBDG_WC_WORDS) {
        if (i & 1) {
            v.x += tab1;
            v.y += tab1;
            v.z = tab2;
        } else {
            v.y += tab1;
            v.z += tab2;
            v.w += tab2;
        }
    } else {
        const uint32_t j = i % (WCW / 4);
        if (j == 1) {
            v.x += tab1;
            v.y = tab2;
        } else if (j >= 2) {
            v.x += tab2;
            v.y += tab2;
            v.z += tab1;
            v.w += tab1;
        }
    }
    return v;
}

// Which run and which chunks a workgroup serves: workgroup bx of the run workgroups.  Workgroups of one run are
// neighbours in blockIdx order (and so in dispatch order): the runs at the end of the grid are the short ones (host:
// guided run lengths)
struct RunSpan {
    uint32_t cgroup;                // group of waves_per_group chunks
    uint32_t w0, w1;                // windows
    uint32_t seg0, seg1, nseg;      // segments; nseg == 0: nothing to do
};

__device__ __forceinline__ RunSpan run_span(uint32_t bx, const uint32_t *__restrict__ run_begin, const WinConst *__restrict__ wconst,
                                            const PopArgs &a)
{
    RunSpan sp;
    const uint32_t run = bx / a.n_cgroups;
    sp.cgroup = bx - run * a.n_cgroups;
    sp.w0 = run_begin[run];
    sp.w1 = run_begin[run + 1];
    sp.seg0 = wconst[sp.w0].seg_begin;
    sp.seg1 = wconst[sp.w1].seg_begin;
    sp.nseg = sp.seg1 - sp.seg0;
    return sp;
}

// What a wave knows of its run once the workgroup has staged it
struct Run {
    const Seg *segs;                // the rare weight planes of segment s of the run: segs[seg0 + s]
    const uint4 *pow_1me, *pow_eps; // the power tables in global memory
    uint32_t seg0, nseg, w0;        // first segment, segments, first window
    bool has_chunk;                 // false: the wave's chunk lies beyond the panel, nothing to do
    uint32_t c, lane;               // the wave's chunk of 64 background individuals
    uint32_t rec_addr, wc_base, tab1;   // LDS addresses of the records, the window constants and the rho^n table
    uint32_t ring_lane;             // ... of the lane's 16 bytes of ring slot 0
    uint32_t x_off0;                // ring byte offset of the first segment's words
    uint32_t scr_w, scr_r;          // the lane's write / read address in the wave's 1 KiB scratch for wave_sum2
};

// The start of every workgroup of k_ld_popcount and k_ld_popcount_mt with a run to serve (sp.nseg != 0): the LDS carve-up
// (ld_lds_layout, as the host sized it), the ring primed, the run's images staged, the barrier.  RECW / WCW: words per
// segment record / window's constants of the form; ENTRY: bytes per power-table entry in LDS; img: which comparison
// individual's (or group's) images.  A wave whose has_chunk comes back false ends there.
template <int RECW, int WCW, bool TAB_LDS, int ENTRY, bool SCRATCH, class Ring>
__device__ __forceinline__ Run run_prologue(const RunSpan &sp, Ring &ring, char *smem, unsigned img, const uint4 *__restrict__ t32,
                                            const Seg *__restrict__ segs, const uint32_t *__restrict__ rec_ready,
                                            const uint32_t *__restrict__ wc_ready, const uint4 *__restrict__ pow_1me,
                                            const uint4 *__restrict__ pow_eps, const PopArgs &a)
{
    constexpr int NS = Ring::SLOTS;
    constexpr bool PLAIN = ENTRY == 8;      // (matrix-core form with the tables in LDS: plain doubles -- see its window end)
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    const uint32_t w0 = sp.w0, w1 = sp.w1, seg0 = sp.seg0, seg1 = sp.seg1, nseg = sp.nseg;

    const LdsLayout lay = ld_lds_layout(a.max_seg, a.win_per_group, a.tab_len, RECW, WCW, TAB_LDS ? ENTRY : 0, NS,
                                        a.waves_per_group, SCRATCH);
    uint32_t *rec_lds = reinterpret_cast<uint32_t *>(smem + lay.rec);     // [max_seg][RECW]
    uint32_t *wc_lds = reinterpret_cast<uint32_t *>(smem + lay.wc);       // [win_per_group][WCW]
    uint4 *tab_lds = reinterpret_cast<uint4 *>(smem + lay.tab);

    // ---- prime the ring FIRST: pairs q0 .. q0+NS-1 (not past the run's last pair).  The
    // direct-to-LDS loads fly while the workgroup stages its records and tables below, so the
    // two start-up latencies of a workgroup overlap instead of adding up.
    const unsigned c = sp.cgroup * a.waves_per_group + wave;
    const bool has_chunk = c < a.n_chunks;
    const uint32_t tile0 = segs[seg0].tile;
    ring.ring = smem + lay.ring + (size_t)wave * NS * 1024;
    ring.xt = t32 + (size_t)c * a.n_pairs * 64 + lane;
    ring.q0 = tile0 >> 1;
    ring.q_last = segs[seg1 - 1].tile >> 1;
    ring.q_issue = ring.q0;
    IBDG_CHECK_IDX(ring.q_last, a.n_pairs, "run_prologue last pair");
    IBDG_CHECK_IDX(ring.q0, ring.q_last + 1, "run_prologue first pair");
    if (has_chunk)
        ring.prime();

    // ---- stage the run's records, window constants and tables (whole workgroup)
    {
        // plain contiguous copies (k_win_target* prepared the LDS images): every load of a thread is
        // independent of the others, so the whole staging costs about one memory latency
        const uint4 *rsrc = reinterpret_cast<const uint4 *>(rec_ready) + ((size_t)img * a.n_segs + seg0) * (RECW / 4);
        uint4 *rdst = reinterpret_cast<uint4 *>(rec_lds);
        for (uint32_t i = threadIdx.x; i < nseg * (RECW / 4); i += blockDim.x)
            rdst[i] = rsrc[i];
        // with the tables in LDS the constants become LDS addresses (table base + 16 * exponent), otherwise
        // they stay byte offsets into the global tables
        const uint32_t stab1 = TAB_LDS ? (uint32_t)(uintptr_t)(lds_void *)tab_lds : 0u;
        const uint32_t stab2 = TAB_LDS ? stab1 + a.tab_len * ENTRY : 0u;
        const uint4 *wsrc = reinterpret_cast<const uint4 *>(wc_ready) + ((size_t)img * a.n_win + w0) * (WCW / 4);
        uint4 *wdst = reinterpret_cast<uint4 *>(wc_lds);
        for (uint32_t i = threadIdx.x; i < (w1 - w0) * (WCW / 4); i += blockDim.x)
            wdst[i] = stage_wc<WCW>(wsrc[i], i, stab1, stab2);
        if (TAB_LDS && PLAIN) {
            // rho^n * 2^(s n) and sigma^n as plain doubles: the mantissas of the {mantissa, exponent} tables, exactly (a power
            // of two moves no bit); s = a.rho_shift keeps rho^n inside the double range for every n of the table
            // (the host checks), sigma = 1 / (2 (1 - eps)) > 1/2 needs none
            double *td = reinterpret_cast<double *>(tab_lds);
            const PowEntry *p1 = reinterpret_cast<const PowEntry *>(pow_1me), *p2 = reinterpret_cast<const PowEntry *>(pow_eps);
            for (uint32_t i = threadIdx.x; i < 2 * a.tab_len; i += blockDim.x) {
                const PowEntry e = i < a.tab_len ? p1[i] : p2[i - a.tab_len];
                td[i] = __builtin_ldexp(e.m, e.e + (i < a.tab_len ? (int)(a.rho_shift * i) : 0));
            }
        } else if (TAB_LDS) {
            for (uint32_t i = threadIdx.x; i < 2 * a.tab_len; i += blockDim.x)
                tab_lds[i] = i < a.tab_len ? pow_1me[i] : pow_eps[i - a.tab_len];
        }
    }
    __syncthreads();

    Run r;
    r.has_chunk = has_chunk;
    r.segs = segs;
    r.pow_1me = pow_1me;
    r.pow_eps = pow_eps;
    r.seg0 = seg0;
    r.nseg = nseg;
    r.w0 = w0;
    r.c = c;
    r.lane = lane;
    r.rec_addr = (uint32_t)(uintptr_t)(lds_void *)rec_lds;      // same value in every lane (VGPR)
    r.wc_base = (uint32_t)(uintptr_t)(lds_void *)wc_lds;
    r.tab1 = (uint32_t)(uintptr_t)(lds_void *)tab_lds;
    r.ring_lane = (uint32_t)(uintptr_t)(lds_void *)ring.ring + lane * 16;
    r.x_off0 = (tile0 & 1) * 8;
    // the wave's 1 KiB scratch for wave_sum2, behind the rings
    const uint32_t scr = (uint32_t)(uintptr_t)(lds_void *)(smem + lay.scratch + wave * 1024);
    r.scr_w = scr + lane * 8;
    r.scr_r = scr + lane * 16;
    return r;
}

// Where a segment's tile words sit in the ring and how far the ring must advance before the
// NEXT segment are precomputed by the host into each record's flag word (ring slot relative to
// the run's first pair), so the loop carries no tile/pair arithmetic:
//   flags = next slot (3) | next half (1) | pairs to advance (8) | rare planes (1) | last (1) | .. | ncov (8) | nalt (8)
// (the matrix-core records carry the control word of mx_record_header instead).  What moves from segment to segment:
struct SegCursor {
    uint32_t rec_addr;      // LDS address of the segment's record, same value in every lane (VGPR)
    uint32_t frag_addr;     // matrix-core forms: of the lane's A fragment
    uint32_t x_off;         // ring byte offset of the segment's tile words
    uint32_t s;             // segment of the run
};

constexpr int FC = 3, FA = 2;      // weight bit-planes with counters of their own (cov, alt)

// Counters per weight bit-plane: three planes for the cov-weighted sums, two for the
// alt-weighted ones are kept apart (one v_bcnt_u32_b32 accumulates into them directly);
// the rare higher planes are shifted into plane 0 as they are counted.  They are plain arrays of the kernel, handed on by
// reference -- c0 c1 ch: C(x0) C(x1) C(x0&x1), A0 A1: A(x0) A(x1), gq[TB][4]: G(x0,t0) G(x1,t0) G(x0,t1) G(x1,t1) per
// comparison individual -- and not members of one struct: as such k_ld_popcount_mt took two more registers.

// the weight planes beyond those (flags bit 12), for TB comparison individuals with the tile words tw
template <int TB>
__device__ __forceinline__ void rare_planes(uint32_t (&c0)[FC], uint32_t (&c1)[FC], uint32_t (&ch)[FC], uint32_t (&A0)[FA],
                                            uint32_t (&A1)[FA], uint32_t (&gq)[TB][4][FC], const Seg &S, uint32_t flags,
                                            uint2 x, uint32_t hom, const uint32_t (&tw)[TB][2])
{
    const uint32_t ncov = (flags >> 16) & 0xff, nalt = flags >> 24;
    // (a handful of turns at the most: a vector body with its prologue and remainder only costs registers)
#pragma clang loop vectorize(disable)
    for (uint32_t k = FC; k < ncov; ++k) {
        const uint32_t cov = S.cov[k];              /* uniform: scalar load */
        const uint32_t u0 = x.x & cov, u1 = x.y & cov;
        c0[0] += (uint32_t)__popc(u0) << k;
        c1[0] += (uint32_t)__popc(u1) << k;
        ch[0] += (uint32_t)__popc(hom & cov) << k;
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            gq[j][0][0] += (uint32_t)__popc(u0 & tw[j][0]) << k;
            gq[j][1][0] += (uint32_t)__popc(u1 & tw[j][0]) << k;
            gq[j][2][0] += (uint32_t)__popc(u0 & tw[j][1]) << k;
            gq[j][3][0] += (uint32_t)__popc(u1 & tw[j][1]) << k;
        }
    }
#pragma clang loop vectorize(disable)
    for (uint32_t k = FA; k < nalt; ++k) {
        const uint32_t alt = S.alt[k];
        A0[0] += (uint32_t)__popc(x.x & alt) << k;
        A1[0] += (uint32_t)__popc(x.y & alt) << k;
    }
}

// One segment of the vector form: fetch its record and tile words, advance the ring, count.  FIRST: the first segment of
// a window (the counters start there, so nothing has to be zeroed).  Returns the record's flag word.
template <bool FIRST, class Ring>
__device__ __forceinline__ uint32_t segment_vec(Ring &ring, SegCursor &cur, const Run &r, uint32_t (&c0)[FC], uint32_t (&c1)[FC],
                                                uint32_t (&ch)[FC], uint32_t (&A0)[FA], uint32_t (&A1)[FA], uint32_t (&gq)[1][4][FC])
{
    uint4 h0, h1;
    uint2 x;
    lds_fetch(h0, h1, x, cur.rec_addr, r.ring_lane + cur.x_off);
    const uint32_t flags = __builtin_amdgcn_readfirstlane(h0.x);
    const uint32_t adv = (flags >> 4) & 0xff;
    if (adv)
        ring.advance(adv);
    cur.x_off = (flags & 7) * 1024 + ((flags >> 3) & 1) * 8;
    const uint32_t cov0 = h0.y, cov1 = h0.z, cov2 = h0.w, alt0 = h1.x, alt1 = h1.y;
    const uint32_t tw[1][2] = {{h1.z, h1.w}};
    const uint32_t hom = x.x & x.y;
    __builtin_amdgcn_sched_barrier(0);
    count_segment<FIRST>(c0, c1, ch, gq[0][0], gq[0][1], gq[0][2], gq[0][3], A0, A1, x.x, x.y, hom, cov0, cov1,
                         cov2, alt0, alt1, tw[0][0], tw[0][1]);
    __builtin_amdgcn_sched_barrier(0);
    if (flags & (1u << 12))
        rare_planes<1>(c0, c1, ch, A0, A1, gq, r.segs[r.seg0 + cur.s], flags, x, hom, tw);
    cur.rec_addr += IBDG_REC_WORDS * 4;
    ++cur.s;
    return flags;
}

// The same for groups of IBDG_MT comparison individuals
template <bool FIRST, class Ring>
__device__ __forceinline__ uint32_t segment_mt(Ring &ring, SegCursor &cur, const Run &r, uint32_t (&c0)[FC], uint32_t (&c1)[FC],
                                               uint32_t (&ch)[FC], uint32_t (&A0)[FA], uint32_t (&A1)[FA], uint32_t (&gq)[IBDG_MT][4][FC])
{
    static_assert(IBDG_MT == 4, "lds_fetch_mt and count_plane_mt are written for four comparison individuals");
    uint4 h0, h1, h2, h3;
    uint2 x;
    lds_fetch_mt(h0, h1, h2, h3, x, cur.rec_addr, r.ring_lane + cur.x_off);
    const uint32_t flags = __builtin_amdgcn_readfirstlane(h0.x);
    const uint32_t adv = (flags >> 4) & 0xff;
    if (adv)
        ring.advance(adv);
    cur.x_off = (flags & 7) * 1024 + ((flags >> 3) & 1) * 8;
    const uint32_t cov0 = h0.y, cov1 = h0.z, cov2 = h0.w, alt0 = h1.x, alt1 = h1.y;
    const uint32_t tw[4][2] = {{h2.x, h2.y}, {h2.z, h2.w}, {h3.x, h3.y}, {h3.z, h3.w}};
    const uint32_t hom = x.x & x.y;
    __builtin_amdgcn_sched_barrier(0);
    count_plane_mt<FIRST>(c0[0], c1[0], ch[0], gq, 0, x.x, x.y, hom, cov0, tw);
    count_plane_mt<FIRST>(c0[1], c1[1], ch[1], gq, 1, x.x, x.y, hom, cov1, tw);
    count_plane_mt<FIRST>(c0[2], c1[2], ch[2], gq, 2, x.x, x.y, hom, cov2, tw);
    count_alt<FIRST>(A0, A1, x.x, x.y, alt0, alt1);
    __builtin_amdgcn_sched_barrier(0);
    if (flags & (1u << 12))
        rare_planes<IBDG_MT>(c0, c1, ch, A0, A1, gq, r.segs[r.seg0 + cur.s], flags, x, hom, tw);
    cur.rec_addr += IBDG_RECM_WORDS * 4;
    ++cur.s;
    return flags;
}

// The matrix-core forms: the two accumulators (the four sums of x0 / x1 as exact integers in f32) and the lane's A
// fragment -- zero except in the lanes 20 kb + sum, which read the 24 bytes of `sum` behind the record's header
struct MxCounts {
    mx_v4f acc0, acc1;
    mx_u4 af_lo;
    mx_u2 af_hi;
};

// the two matrix instructions of a segment; a window's first segment starts the accumulators from `start`
template <bool FIRST>
__device__ __forceinline__ void mx_accumulate(MxCounts &m, uint2 x, const mx_v4f &start)
{
    const mx_v8i av = {(int)m.af_lo.x, (int)m.af_lo.y, (int)m.af_lo.z, (int)m.af_lo.w, (int)m.af_hi.x, (int)m.af_hi.y, 0, 0};
    m.acc0 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bits_to_fp4(x.x), FIRST ? start : m.acc0, 2, 4, 0, 0x7f80, 1,
                                                              0x7f80);
    m.acc1 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bits_to_fp4(x.y), FIRST ? start : m.acc1, 2, 4, 0, 0x7f80, 1,
                                                              0x7f80);
}

// One segment with the counts of the two haplotype words on the matrix cores (acc0 / acc1: <x,cov> <x,alt> <x&t0,cov>
// <x&t1,cov> of x0 / x1; a window's first segment starts them from zero) and the three planes of <x0&x1,cov> as
// (mask, count) pairs.  Returns the record's control word.
template <bool FIRST, class Ring>
__device__ __forceinline__ uint32_t segment_mx(Ring &ring, SegCursor &cur, const Run &r, MxCounts &m, uint32_t (&ch)[FC])
{
    uint4 h0;
    uint2 x;
    lds_fetch_mx(h0, x, m.af_lo, m.af_hi, cur.rec_addr, r.ring_lane + cur.x_off, cur.frag_addr);
    const uint32_t flags = __builtin_amdgcn_readfirstlane(h0.x);
    const uint32_t adv = flags >> 16;
    if (adv)
        ring.advance(adv);
    cur.x_off = flags & 0x3fff;
    const uint32_t hom = x.x & x.y;
    const mx_v4f zero = {0.f, 0.f, 0.f, 0.f};
    mx_accumulate<FIRST>(m, x, zero);
    if (FIRST) {
        ch[0] = __popc(hom & h0.y); ch[1] = __popc(hom & h0.z); ch[2] = __popc(hom & h0.w);
    } else {
        ch[0] += __popc(hom & h0.y); ch[1] += __popc(hom & h0.z); ch[2] += __popc(hom & h0.w);
    }
    if (flags & (1u << 14)) {
        const Seg &S = r.segs[r.seg0 + cur.s];
        const uint4 h1 = lds_read_b128(cur.rec_addr + 16);
        const uint2 at = make_uint2(h1.x, h1.y);
        const uint32_t nn = __builtin_amdgcn_readfirstlane(h1.z), ncov = nn & 0xff, nalt = nn >> 8;
        for (uint32_t k = 3; k < ncov; ++k) {
            const uint32_t cov = S.cov[k];              /* uniform: scalar load */
            const uint32_t u0 = x.x & cov, u1 = x.y & cov;
            m.acc0[0] += (float)((uint32_t)__popc(u0) << k);
            m.acc1[0] += (float)((uint32_t)__popc(u1) << k);
            ch[0] += (uint32_t)__popc(hom & cov) << k;
            m.acc0[2] += (float)((uint32_t)__popc(u0 & at.x) << k);
            m.acc1[2] += (float)((uint32_t)__popc(u1 & at.x) << k);
            m.acc0[3] += (float)((uint32_t)__popc(u0 & at.y) << k);
            m.acc1[3] += (float)((uint32_t)__popc(u1 & at.y) << k);
        }
        for (uint32_t k = 3; k < nalt; ++k) {
            const uint32_t alt = S.alt[k];
            m.acc0[1] += (float)((uint32_t)__popc(x.x & alt) << k);
            m.acc1[1] += (float)((uint32_t)__popc(x.y & alt) << k);
        }
    }
    cur.rec_addr += IBDG_RECX_WORDS * 4;
    cur.frag_addr += IBDG_RECX_WORDS * 4;
    ++cur.s;
    return flags;
}

// The IBD1 form (PopArgs::ibd1): no counts for the individual's own genotype factors -- their products come from the one pass
// over the site list --, and the four sums of a word are the table exponents themselves (k_win_target_mx); a window's first
// segment starts the accumulators from bias4 = 1.5 * 2^23, so that their BITS hold the (signed) sums.  cur.frag_addr is the
// one address register of lds_fetch_x1.
template <bool FIRST, class Ring>
__device__ __forceinline__ uint32_t segment_x1(Ring &ring, SegCursor &cur, const Run &r, MxCounts &m, const mx_v4f &bias4)
{
    uint32_t ctl;
    uint2 x;
    lds_fetch_x1(ctl, x, m.af_lo, m.af_hi, r.ring_lane + cur.x_off, cur.frag_addr);
    const uint32_t flags = __builtin_amdgcn_readfirstlane(ctl);
    const uint32_t adv = flags >> 16;
    if (adv)
        ring.advance(adv);
    cur.x_off = flags & 0x3fff;
    mx_accumulate<FIRST>(m, x, bias4);
    if (flags & (1u << 14)) {
        const Seg &S = r.segs[r.seg0 + cur.s];
        const uint4 h1 = lds_read_b128((uint32_t)__builtin_amdgcn_readfirstlane((int)cur.frag_addr) + 16);
        const uint2 at = make_uint2(h1.x, h1.y);
        const uint32_t nn = __builtin_amdgcn_readfirstlane(h1.z), ncov = nn & 0xff, nalt = nn >> 8;
        for (uint32_t k = 3; k < ncov; ++k) {
            const uint32_t cov = S.cov[k];              /* uniform: scalar load */
            const uint32_t u0 = x.x & cov, u1 = x.y & cov;
            const int c0 = __popc(u0), c1 = __popc(u1), mk = 1 << k;
            const int g00 = __popc(u0 & at.x), g01 = __popc(u1 & at.x);
            const int g10 = __popc(u0 & at.y), g11 = __popc(u1 & at.y);
            m.acc0[0] += (float)((c0 - 2 * g00) * mk);
            m.acc0[1] += (float)((c0 - 2 * g10) * mk);
            m.acc0[2] += (float)(g00 * mk);
            m.acc0[3] += (float)(g10 * mk);
            m.acc1[0] += (float)((c1 - 2 * g01) * mk);
            m.acc1[1] += (float)((c1 - 2 * g11) * mk);
            m.acc1[2] += (float)(g01 * mk);
            m.acc1[3] += (float)(g11 * mk);
        }
        for (uint32_t k = 3; k < nalt; ++k) {
            const uint32_t alt = S.alt[k];
            const float a0 = (float)((uint32_t)__popc(x.x & alt) << k), a1 = (float)((uint32_t)__popc(x.y & alt) << k);
            m.acc0[2] -= a0;
            m.acc0[3] -= a0;
            m.acc1[2] -= a1;
            m.acc1[3] -= a1;
        }
    }
    cur.frag_addr += IBDG_RECX_WORDS * 4;
    ++cur.s;
    return flags;
}

// ---------------------------------------------------------------------------
// Window ends.  The sums of one background individual over a window's rows, x = its haplotype, t = the comparison
// individual's:
struct WindowSums {
    uint32_t C[2], CH;      // C(x0) C(x1) C(x0&x1)
    uint32_t al[2];         // A(x0) A(x1)
    uint32_t G[4];          // G(x0,t0) G(x1,t0) G(x0,t1) G(x1,t1): the order of the four IBD1 products
};

// -32, the multiplier of the 2 G(x,t) term in an address of 16-byte entries, kept in a VGPR (no inline constant)
__device__ __forceinline__ uint32_t vgpr_m32()
{
    uint32_t m32 = (uint32_t)-32;
    asm volatile("" : "+v"(m32));
    return m32;
}

// Where rho^E2 (ad[O + 2i]) and sigma^E3 (ad[O + 2i + 1]) of the IBD1 product i sit, table base + exponent << SH:
//   pDg[At+hx] (ibdgem.c:716-719):     E3 = <t,cov> + Cx - 2 G(x,t)  E2 = AT - <t,alt> - ax + G(x,t)
// kb[t] / kc[t]: the window's constants, table base + (AT - <t,alt>) << SH / + <t,cov> << SH
template <int SH, int O, int N>
__device__ __forceinline__ void ibd1_addresses(uint32_t (&ad)[N], const uint32_t (&G)[4], const uint32_t (&al)[2],
                                               const uint32_t (&C)[2], const uint32_t (&kb)[2], const uint32_t (&kc)[2],
                                               uint32_t m32)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = i & 1, t = i >> 1;
        ad[O + 2 * i] = lshl_add<SH>(G[i], mad24<-(1 << SH)>(al[x], kb[t]));
        if constexpr (SH == 4)
            ad[O + 2 * i + 1] = mad24r(G[i], m32, lshl_add<SH>(C[x], kc[t]));
        else
            ad[O + 2 * i + 1] = mad24<-(2 << SH)>(G[i], lshl_add<SH>(C[x], kc[t]));
    }
}

// ... and of the product of the individual's own genotype factors
//   pDg[x0+x1] (ibdgem.c:715): E3 = C0 + C1 - 2 CH          E2 = AT - a0 - a1 + CH
template <int SH, int N>
__device__ __forceinline__ void own_addresses(uint32_t (&ad)[N], const WindowSums &u, uint32_t kAT, uint32_t ktab2)
{
    ad[0] = lshl_add<SH>(u.CH - (u.al[0] + u.al[1]), kAT);
    ad[1] = lshl_add<SH>(mad24<-2>(u.CH, u.C[0] + u.C[1]), ktab2);
}

// N / 2 table entries of 16 bytes each way, from LDS in one round trip or from global memory
template <bool TAB_LDS, int N>
__device__ __forceinline__ void read_entries(uint4 (&pw)[N], const uint32_t (&ad)[N], const Run &r)
{
    if constexpr (!TAB_LDS) {
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            pw[2 * i] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(r.pow_1me) + ad[2 * i]);
            pw[2 * i + 1] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(r.pow_eps) + ad[2 * i + 1]);
        }
    } else if constexpr (N == 2) {
        lds_read2(pw[0], pw[1], ad[0], ad[1]);
    } else if constexpr (N == 8) {
        lds_read_pow8(pw, ad);
    } else {
        lds_read_pow10(pw, ad);
    }
}

// N products from tables of plain doubles (8-byte entries in LDS, pq[2i] / pq[2i + 1] from ad[2i] / ad[2i + 1]).  rho^E2
// sits in its table as rho^E2 * 2^(s E2), s = rho_shift: the product's exponent is made up for it from the table address
// itself, eK - s E2 = (8 eK + s tab1 - s ad) >> 3
template <int N>
__device__ __forceinline__ void ld_products_plain(const uint2 (&pq)[2 * N], const uint32_t (&ad)[2 * N], int eK, uint32_t tab1,
                                                  uint32_t rho_shift, double (&val)[N])
{
    if (rho_shift == 8) {                  // (the host's choice where the table allows it): eK - 8 E2 = eK + tab1 - ad
        const uint32_t e1 = (uint32_t)eK + tab1;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double m1 = __hiloint2double((int)pq[2 * i].y, (int)pq[2 * i].x);
            const double m2 = __hiloint2double((int)pq[2 * i + 1].y, (int)pq[2 * i + 1].x);
            val[i] = __builtin_ldexp(m1 * m2, (int)(e1 - ad[2 * i]));
        }
    } else {
        const uint32_t e8 = mad24r(tab1, rho_shift, (uint32_t)eK << 3);        // 8 eK + s tab1 (wave-uniform)
        const uint32_t ms = 0u - rho_shift;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double m1 = __hiloint2double((int)pq[2 * i].y, (int)pq[2 * i].x);
            const double m2 = __hiloint2double((int)pq[2 * i + 1].y, (int)pq[2 * i + 1].x);
            val[i] = __builtin_ldexp(m1 * m2, (int)mad24r(ad[2 * i], ms, e8) >> 3);
        }
    }
}

// where the wave's sums of window w go: [0] the IBD0 terms, [1] the IBD1 terms of comparison individual t
__device__ __forceinline__ double *partial_of(const PopArgs &a, const Run &r, unsigned t, uint32_t w)
{
    return a.partial + (((size_t)(a.t_base + t) * a.n_win + w) * a.n_chunks + r.c) * 2;
}

// The window end of one comparison individual with tables of {mantissa, exponent} entries (16 bytes): the five products
// of the lane's individual times its multiplicity, the two wave sums, the chunk's partials.  k0, k1: the window's constants.
template <bool TAB_LDS>
__device__ __forceinline__ void window_end_entries(const Run &r, const PopArgs &a, unsigned t, uint32_t w, double wgt,
                                                   const uint4 &k0, const uint4 &k1, const WindowSums &u, uint32_t m32)
{
    const int eK = (int)k0.x;
    // table addresses of 16*AT, 16*<t0,cov>, 16*<t1,cov>, 16*(AT-<t0,alt>), 16*(AT-<t1,alt>), 0
    const uint32_t kAT = k0.y, ktab2 = k1.z, kc[2] = {k0.z, k0.w}, kb[2] = {k1.x, k1.y};
    uint32_t ad[10];
    own_addresses<4>(ad, u, kAT, ktab2);
    ibd1_addresses<4, 2>(ad, u.G, u.al, u.C, kb, kc, m32);
    uint4 pw[10];
    read_entries<TAB_LDS>(pw, ad, r);
    const double P2 = ld_value(eK, pw[0], pw[1]);
    const double Q00 = ld_value(eK, pw[2], pw[3]);
    const double Q01 = ld_value(eK, pw[4], pw[5]);
    const double Q10 = ld_value(eK, pw[6], pw[7]);
    const double Q11 = ld_value(eK, pw[8], pw[9]);
    double s0 = wgt * P2;                                   // :743
    double s1 = wgt * (((Q00 + Q01) + Q10) + Q11);          // :744-745
    if (a.p2_out)
        a.p2_out[(size_t)w * a.lanes + r.c * 64 + r.lane] = s0;
    const double tot = wave_sum2(s0, s1, r.scr_w, r.scr_r);      // first half: sum of s0, second half: of s1
    if ((r.lane & 31) == 31)
        partial_of(a, r, t, w)[r.lane >> 5] = tot;
}

// The same with the tables as plain doubles in LDS (the matrix-core form that counts everything)
__device__ __forceinline__ void window_end_plain(const Run &r, const PopArgs &a, unsigned t, uint32_t w, double wgt,
                                                 const uint4 &k0, const uint4 &k1, const WindowSums &u)
{
    const int eK = (int)k0.x;
    const uint32_t kAT = k0.y, ktab2 = k1.z, kc[2] = {k0.z, k0.w}, kb[2] = {k1.x, k1.y};
    uint32_t ad[10];
    own_addresses<3>(ad, u, kAT, ktab2);
    ibd1_addresses<3, 2>(ad, u.G, u.al, u.C, kb, kc, 0u);
    uint2 pq[10];
    lds_read_pow10_b64(pq, ad);
    double val[5];
    ld_products_plain<5>(pq, ad, eK, r.tab1, a.rho_shift, val);
    double s0 = wgt * val[0];                                   // :743
    if (a.p2_out)
        a.p2_out[(size_t)w * a.lanes + r.c * 64 + r.lane] = s0;
    double s1 = wgt * (((val[1] + val[2]) + val[3]) + val[4]);  // :744-745
    const double tot = a.sum_dpp ? wave_sum2_dpp(s0, s1, r.scr_w, r.scr_r) : wave_sum2(s0, s1, r.scr_w, r.scr_r);
    if ((r.lane & 31) == 31)
        partial_of(a, r, t, w)[r.lane >> 5] = tot;
}

// the constants of window w of the run, broadcast into VGPRs
__device__ __forceinline__ void read_window_constants(uint4 &k0, uint4 &k1, const Run &r, uint32_t w)
{
    lds_read2(k0, k1, r.wc_base + (w - r.w0) * (IBDG_WC_WORDS * 4), r.wc_base + (w - r.w0) * (IBDG_WC_WORDS * 4) + 16);
}

// ---------------------------------------------------------------------------
// The forms of k_ld_popcount: what a wave does with its run, one window per turn (a run's windows are consecutive, and a
// run ends with the last segment of a window).
// ---------------------------------------------------------------------------

// the vector form (option mx_counts 0): every count a (mask, count) pair
template <bool TAB_LDS, class Ring>
__device__ __forceinline__ void run_vector_form(Ring &ring, const Run &r, const PopArgs &a, unsigned t)
{
    const double wgt = a.weight[(size_t)(a.t_base + t) * a.lanes + r.c * 64 + r.lane];
    uint32_t c0[FC], c1[FC], ch[FC], A0[FA], A1[FA];
    uint32_t gq[1][4][FC];
    ring.wait_first();          // the first pair must have landed (it was requested before the staging loads, so it has)
    const uint32_t m32 = vgpr_m32();
    SegCursor cur = {r.rec_addr, 0, r.x_off0, 0};
    for (uint32_t w = r.w0; cur.s < r.nseg; ++w) {
        uint32_t flags = segment_vec<true>(ring, cur, r, c0, c1, ch, A0, A1, gq);              // its first segment starts the counters
        while (!(flags & (1u << 13)) && cur.s < r.nseg)                   // the others add to them
            flags = segment_vec<false>(ring, cur, r, c0, c1, ch, A0, A1, gq);
        uint4 k0, k1;
        read_window_constants(k0, k1, r, w);
        WindowSums u;
        u.CH = planes_sum<FC>(ch);
        u.C[0] = planes_sum<FC>(c0); u.C[1] = planes_sum<FC>(c1);
        u.G[0] = planes_sum<FC>(gq[0][0]); u.G[1] = planes_sum<FC>(gq[0][1]);
        u.G[2] = planes_sum<FC>(gq[0][2]); u.G[3] = planes_sum<FC>(gq[0][3]);
        u.al[0] = planes_sum<FA>(A0); u.al[1] = planes_sum<FA>(A1);
        window_end_entries<TAB_LDS>(r, a, t, w, wgt, k0, k1, u, m32);
    }
    ring.drain();
}

// the matrix-core form that counts everything (mx_counts 1, ibd0_after 0)
template <bool TAB_LDS, class Ring>
__device__ __forceinline__ void run_matrix_form(Ring &ring, const Run &r, const PopArgs &a, unsigned t)
{
    const double wgt = a.weight[(size_t)(a.t_base + t) * a.lanes + r.c * 64 + r.lane];
    uint32_t ch[FC];
    ring.wait_first();
    const uint32_t m32 = TAB_LDS ? 0u : vgpr_m32();
    MxCounts m = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0, 0, 0, 0}, {0, 0}};
    SegCursor cur = {r.rec_addr, r.rec_addr + 32 + 24 * (r.lane & 3), r.x_off0, 0};
    for (uint32_t w = r.w0; cur.s < r.nseg; ++w) {
        uint32_t flags = segment_mx<true>(ring, cur, r, m, ch);
        while (!(flags & (1u << 15)))
            flags = segment_mx<false>(ring, cur, r, m, ch);
        uint4 k0, k1;
        read_window_constants(k0, k1, r, w);
        WindowSums u;
        u.CH = planes_sum<FC>(ch);
        u.C[0] = (uint32_t)m.acc0[0]; u.al[0] = (uint32_t)m.acc0[1]; u.G[0] = (uint32_t)m.acc0[2]; u.G[2] = (uint32_t)m.acc0[3];
        u.C[1] = (uint32_t)m.acc1[0]; u.al[1] = (uint32_t)m.acc1[1]; u.G[1] = (uint32_t)m.acc1[2]; u.G[3] = (uint32_t)m.acc1[3];
        if constexpr (TAB_LDS)
            window_end_plain(r, a, t, w, wgt, k0, k1, u);
        else
            window_end_entries<false>(r, a, t, w, wgt, k0, k1, u, m32);
    }
    ring.drain();
}

// One window of the IBD1 form after its segments: the four IBD1 products of the lane's individual (:716-719, :744-745)
// times its multiplicity
__device__ __forceinline__ double ibd1_window_value(const Run &r, const PopArgs &a, const MxCounts &m, uint32_t w, double wgt)
{
    uint4 k0, k1;
    read_window_constants(k0, k1, r, w);
    const int eK = (int)k0.x;
    const uint32_t kc0 = k0.z, kc1 = k0.w, kb0 = k1.x, kb1 = k1.y;     // (less 8 * 2^22 each, k_win_target_mx)
    // acc[0] / [1] = C(x) - 2 G(x,t0 / t1), acc[2] / [3] = G(x,t0 / t1) - A(x); v_mad_i32_i24 reads the low 24 bits of the
    // accumulator's own bits.  Products in the order of the other forms: (t0,x0) (t0,x1) (t1,x0) (t1,x1).
    uint32_t ad[8];
    ad[0] = mad24<8>(__float_as_uint(m.acc0[2]), kb0);   ad[1] = mad24<8>(__float_as_uint(m.acc0[0]), kc0);
    ad[2] = mad24<8>(__float_as_uint(m.acc1[2]), kb0);   ad[3] = mad24<8>(__float_as_uint(m.acc1[0]), kc0);
    ad[4] = mad24<8>(__float_as_uint(m.acc0[3]), kb1);   ad[5] = mad24<8>(__float_as_uint(m.acc0[1]), kc1);
    ad[6] = mad24<8>(__float_as_uint(m.acc1[3]), kb1);   ad[7] = mad24<8>(__float_as_uint(m.acc1[1]), kc1);
    uint2 pq[8];
    lds_read_pow8_b64(pq, ad);
    double val[4];
    ld_products_plain<4>(pq, ad, eK, r.tab1, a.rho_shift, val);
    return wgt * (((val[0] + val[1]) + val[2]) + val[3]);
}

// the IBD1 form (ibd0_after 1): the timed kernel.  PAIR (PopArgs::pair_sums): two consecutive windows of the run share one
// sum tree through the wave's scratch (wave_sum_pair_dpp); a run's odd last window, and every window without PAIR, ends
// with the DPP moves alone
template <bool PAIR, class Ring>
__device__ __forceinline__ void run_ibd1_form(Ring &ring, const Run &r, const PopArgs &a, unsigned t)
{
    const double wgt = a.weight[(size_t)(a.t_base + t) * a.lanes + r.c * 64 + r.lane];
    ring.wait_first();
    MxCounts m = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0, 0, 0, 0}, {0, 0}};
    // 1.5 * 2^23 in four registers that stay: the start value of a window's accumulators (an inline constant it is not)
    mx_v4f bias4 = {12582912.f, 12582912.f, 12582912.f, 12582912.f};
    asm volatile("" : "+v"(bias4));
    SegCursor cur = {0, r.rec_addr + 24 * (r.lane & 3), r.x_off0, 0};
    // the sum over the wave's 64 individuals in the tree of wave_sum2 (the lane number's bits in turn)
    uint32_t w = r.w0;
    // a window's segments and the lane's value of it
    auto window_value = [&]() {
        uint32_t flags = segment_x1<true>(ring, cur, r, m, bias4);
        while (!(flags & (1u << 15)))
            flags = segment_x1<false>(ring, cur, r, m, bias4);
        return ibd1_window_value(r, a, m, w, wgt);
    };
    // PAIR: lane 31 stores the first window's sum, lane 63 the second's, one window's partials further on
    const uint32_t second = PAIR ? (r.lane >> 5) * a.n_chunks * 2 : 0;
    while (cur.s < r.nseg) {
        const double v = window_value();
        if (PAIR && cur.s < r.nseg) {           // another window of the run follows: the two share a tree
            wave_sum_park(v, r.scr_w);
            ++w;
            const double tot = wave_sum_pair_dpp(window_value(), r.scr_w, r.scr_r);
            if ((r.lane & 31) == 31)
                partial_of(a, r, t, w - 1)[1 + second] = tot;
        } else {
            const double tot = wave_sum_lane63_only(v);
            if (r.lane == 63)
                partial_of(a, r, t, w)[1] = tot;
        }
        ++w;
    }
    ring.drain();
}

// The first workgroups of the grid (a.fin_prev != null: ceil(windows / waves of a workgroup) of them) do the finalising step of the PREVIOUS
// run of the same shape -- k_ld_finalize's arithmetic, a wave per window -- whose partial sums that launch left in the
// other half of their buffer: complete and visible, a kernel boundary lies between.  The workgroups of the runs follow.
// True: this workgroup was one of them; otherwise bx becomes its number among the run workgroups.
__device__ __forceinline__ bool fused_finalize(uint32_t &bx, unsigned t, const WinConst *__restrict__ wconst, const PopArgs &a)
{
    if (!a.fin_prev)
        return false;
    const uint32_t n_fin = (a.n_win + a.waves_per_group - 1) / a.waves_per_group;
    if (bx >= n_fin) {
        bx -= n_fin;
        return false;
    }
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t w = bx * a.waves_per_group + wave;
    if (w < a.n_win) {
        const unsigned tt = a.t_base + t;
        double t0 = 0.0, t1 = 0.0;
        chunk_partial_sums(reinterpret_cast<const double2 *>(a.fin_prev) + ((size_t)tt * a.n_win + w) * a.n_chunks, a.n_chunks, lane,
                           t0, t1);
        finalize_window(t0, t1, a.fin_p2c, a.fin_p2w, a.fin_targets, a.lanes, a.n_chunks, a.n_win, w, tt, lane, wconst,
                        a.n_refpanel, a.win_ll, "fused finalize");
    }
    return true;
}

template <int NS, bool TAB_LDS, bool MX, bool IBD1 = false, bool PAIR = false>
__global__ __launch_bounds__(512) void k_ld_popcount(const uint4 *__restrict__ t32,
                                                     const Seg *__restrict__ segs,
                                                     const uint32_t *__restrict__ rec_ready,
                                                     const WinConst *__restrict__ wconst,
                                                     const uint32_t *__restrict__ wc_ready,
                                                     const uint4 *__restrict__ pow_1me,
                                                     const uint4 *__restrict__ pow_eps,
                                                     const uint32_t *__restrict__ run_begin,
                                                     PopArgs a)
{
    static_assert(!IBD1 || (MX && TAB_LDS), "the IBD1 form exists with the counts on the matrix cores and the tables in LDS");
    static_assert(!PAIR || IBD1, "the paired window end is the IBD1 form's");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned t = blockIdx.z;
    uint32_t bx = blockIdx.x;
    if (fused_finalize(bx, t, wconst, a))
        return;
    const RunSpan sp = run_span(bx, run_begin, wconst, a);
    if (sp.nseg == 0)
        return;
    TileRing<NS, MX> ring;
    const Run r = run_prologue<MX ? IBDG_RECX_WORDS : IBDG_REC_WORDS, IBDG_WC_WORDS, TAB_LDS, MX && TAB_LDS ? 8 : 16, !IBD1 || PAIR>(
        sp, ring, smem, t, t32, segs, rec_ready, wc_ready, pow_1me, pow_eps, a);
    if (!r.has_chunk)
        return;
    if constexpr (IBD1)
        run_ibd1_form<PAIR>(ring, r, a, t);
    else if constexpr (MX)
        run_matrix_form<TAB_LDS>(ring, r, a, t);
    else
        run_vector_form<TAB_LDS>(ring, r, a, t);
}

// ---------------------------------------------------------------------------
// Several comparison individuals per workgroup (BASELINE.json configs[4]: hundreds of them against
// one panel).  Of the nine sums per background individual and window only the four G(x,t) depend
// on the comparison individual; A(x0) A(x1) C(x0) C(x1) C(x0&x1), the tile words, the masks and
// the product of the individual's own genotype factors (ibdgem.c:715) do not.  A workgroup of
// k_ld_popcount_mt therefore serves TB comparison individuals at once: per segment the common
// 13 counts are taken once and 12 more per individual; per window the common exponents and P2
// once, then per individual the four IBD1 products, its weight (the individual itself is
// excluded from its own background, ibdgem.c:714) and its two wave sums -- in exactly the
// operations and order of k_ld_popcount, so the results are the same bits.  The window end is written in the
// kernel's body: as a function of its own, with the same text, the kernel took two more registers.
// (LDS images, written by k_win_target_mt: ibdg_ld_layout.h)
// ---------------------------------------------------------------------------

template <int NS, bool TAB_LDS>
__global__ __launch_bounds__(512) void k_ld_popcount_mt(const uint4 *__restrict__ t32,
                                                        const Seg *__restrict__ segs,
                                                        const uint32_t *__restrict__ rec_ready,
                                                        const WinConst *__restrict__ wconst,
                                                        const uint32_t *__restrict__ wc_ready,
                                                        const uint4 *__restrict__ pow_1me,
                                                        const uint4 *__restrict__ pow_eps,
                                                        const uint32_t *__restrict__ run_begin,
                                                        PopArgs a)
{
    constexpr int TB = IBDG_MT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned g = blockIdx.z;                     // group of TB comparison individuals
    const RunSpan sp = run_span(blockIdx.x, run_begin, wconst, a);
    if (sp.nseg == 0)
        return;
    TileRing<NS, false> ring;
    const Run r = run_prologue<IBDG_RECM_WORDS, IBDG_WCM_WORDS, TAB_LDS, 16, true>(sp, ring, smem, g, t32, segs, rec_ready, wc_ready,
                                                                                  pow_1me, pow_eps, a);
    if (!r.has_chunk)
        return;
    double wgt[TB];
#pragma unroll
    for (int j = 0; j < TB; ++j)
        wgt[j] = a.weight[(size_t)(a.t_base + g * TB + j) * a.lanes + r.c * 64 + r.lane];
    uint32_t c0[FC], c1[FC], ch[FC], A0[FA], A1[FA];
    uint32_t gq[TB][4][FC];
    ring.wait_first();
    const uint32_t m32 = vgpr_m32();
    SegCursor cur = {r.rec_addr, 0, r.x_off0, 0};
    for (uint32_t w = r.w0; cur.s < r.nseg; ++w) {               // one window per turn (a run's windows are consecutive)
        uint32_t flags = segment_mt<true>(ring, cur, r, c0, c1, ch, A0, A1, gq);      // its first segment starts the counters
        while (!(flags & (1u << 13)) && cur.s < r.nseg)          // the others add to them
            flags = segment_mt<false>(ring, cur, r, c0, c1, ch, A0, A1, gq);
        const uint32_t wc_addr = r.wc_base + (w - r.w0) * (IBDG_WCM_WORDS * 4);
        static_assert(TB == 4, "the six-read statement below fetches 8 + 4*4 words");
        uint4 k0, k1, kt4[4];                     // the window's constants of all TB individuals in one round trip
        asm volatile("ds_read_b128 %0, %6\n\t"
                     "ds_read_b128 %1, %6 offset:16\n\t"
                     "ds_read_b128 %2, %6 offset:32\n\t"
                     "ds_read_b128 %3, %6 offset:48\n\t"
                     "ds_read_b128 %4, %6 offset:64\n\t"
                     "ds_read_b128 %5, %6 offset:80\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(k0), "=&v"(k1), "=&v"(kt4[0]), "=&v"(kt4[1]), "=&v"(kt4[2]), "=&v"(kt4[3])
                     : "v"(wc_addr)
                     : "memory");
        const int eK = (int)k0.z;
        const uint32_t kAT = k1.x, ktab2 = k1.y;
        WindowSums u;
        u.C[0] = planes_sum<FC>(c0); u.C[1] = planes_sum<FC>(c1); u.CH = planes_sum<FC>(ch);
        u.al[0] = planes_sum<FA>(A0); u.al[1] = planes_sum<FA>(A1);
        double P2;
        {
            uint32_t ad[2];
            own_addresses<4>(ad, u, kAT, ktab2);
            uint4 pw[2];
            read_entries<TAB_LDS>(pw, ad, r);
            P2 = ld_value(eK, pw[0], pw[1]);
        }
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            const uint4 kt = kt4[j];
            const uint32_t kc[2] = {kt.x, kt.y}, kb[2] = {kt.z, kt.w};
            const uint32_t G[4] = {planes_sum<FC>(gq[j][0]), planes_sum<FC>(gq[j][1]), planes_sum<FC>(gq[j][2]), planes_sum<FC>(gq[j][3])};
            uint32_t ad[8];
            ibd1_addresses<4, 0>(ad, G, u.al, u.C, kb, kc, m32);
            uint4 pw[8];
            read_entries<TAB_LDS>(pw, ad, r);
            const double Q00 = ld_value(eK, pw[0], pw[1]);
            const double Q01 = ld_value(eK, pw[2], pw[3]);
            const double Q10 = ld_value(eK, pw[4], pw[5]);
            const double Q11 = ld_value(eK, pw[6], pw[7]);
            double s0 = wgt[j] * P2;                                   // :743
            double s1 = wgt[j] * (((Q00 + Q01) + Q10) + Q11);          // :744-745
            const double tot = wave_sum2(s0, s1, r.scr_w, r.scr_r);      // lane 31: sum of s0, lane 63: of s1
            if ((r.lane & 31) == 31)
                partial_of(a, r, g * TB + j, w)[r.lane >> 5] = tot;
        }
    }
    ring.drain();
}

// Sum the per-chunk partials of a window and take the background average (src/ibdgem.c:751-752).
// One wave per window (chunk_partial_sums, finalize_window).
__global__ __launch_bounds__(256) void k_ld_finalize(PopFinalArgs a)
{
    const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= a.n_win)
        return;
    const unsigned lane = threadIdx.x & 63;
    const unsigned t = blockIdx.y + a.t_base;
    double t0 = 0.0, t1 = 0.0;
    if (a.halves) {
        // k_ld_mfma sums 32 individuals per wave: a chunk's sum is (individuals 0..31) + (32..63), the last
        // addition of the 64-lane tree of wave_sum2
        const double2 *p = reinterpret_cast<const double2 *>(a.partial) + ((size_t)(t - a.p_t0) * a.n_win + w) * a.n_chunks * 2;
        for (uint32_t c = lane; c < a.n_chunks; c += 64) {
            const double2 v = p[2 * c], u = p[2 * c + 1];
            t0 += v.x + u.x;
            t1 += v.y + u.y;
        }
    } else {
        chunk_partial_sums(reinterpret_cast<const double2 *>(a.partial) + ((size_t)(t - a.p_t0) * a.n_win + w) * a.n_chunks,
                           a.n_chunks, lane, t0, t1);
    }
    finalize_window(t0, t1, a.p2c, a.p2w, a.targets, a.lanes, a.n_chunks, a.n_win, w, t, lane, a.wconst, a.n_refpanel, a.win_ll,
                    "k_ld_finalize");
}

// ---------------------------------------------------------------------------
// LDS of one workgroup: records + window constants (+ power tables) rounded to 1 KiB, then 8 rings (+ wave_sum2 scratch).
// multi_target: 0 = one comparison individual (vector-ALU counts), 1 = groups of IBDG_MT, 2 = one, counts on the matrix
// cores, 3 = the IBD1 form of 2: no scratch, 4 = the IBD1 form with the paired window end: the scratch again
size_t ld_popcount_lds_bytes(uint32_t max_seg, uint32_t win_per_group, uint32_t tab_len, int tab_in_lds,
                             int ring_slots, int multi_target)
{
    const bool mt = multi_target == 1, mx = multi_target >= 2 && multi_target <= 4;
    return ld_lds_layout(max_seg, win_per_group, tab_len, mt ? IBDG_RECM_WORDS : mx ? IBDG_RECX_WORDS : IBDG_REC_WORDS,
                         mt ? IBDG_WCM_WORDS : IBDG_WC_WORDS, tab_in_lds ? (mx ? 8 : 16) : 0,      // (matrix-core form: plain doubles)
                         ring_slots, 8, multi_target != 3)
        .bytes;
}

// the run-time ring depth as the compile-time NS of the kernels: launch(std::integral_constant<int, NS>)
template <class F>
static int with_ring_slots(uint32_t ring_slots, F &&launch)
{
    switch (ring_slots) {
    case 2:
        return launch(std::integral_constant<int, 2>());
    case 3:
        return launch(std::integral_constant<int, 3>());
    case 4:
        return launch(std::integral_constant<int, 4>());
    default:
        return launch(std::integral_constant<int, 8>());
    }
}

// ev.start / ev.stop (may be null): events the dispatch itself updates with the kernel's start and
// stop time (hipExtLaunchKernel) -- no event-record packet on the stream.
using CountKernel = void (*)(const uint4 *, const Seg *, const uint32_t *, const WinConst *, const uint32_t *, const uint4 *,
                             const uint4 *, const uint32_t *, PopArgs);
static int launch_counting(CountKernel kern, size_t lds, const PopArgs &a, dim3 grid, hipStream_t st, KernelEvents ev)
{
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return 1;
    hipExtLaunchKernelGGL(kern, grid, dim3(64 * a.waves_per_group), (uint32_t)lds, st, ev.start, ev.stop, 0,
                          (const uint4 *)a.t32, a.segs, a.rec_ready, a.wconst, a.wc_ready, (const uint4 *)a.pow_1me,
                          (const uint4 *)a.pow_eps, a.run_begin, a);
    return 0;
}

template <int NS, bool TAB, bool MX, bool IBD1 = false, bool PAIR = false>
static int launch_pop(const PopArgs &a, dim3 grid, hipStream_t st, KernelEvents ev)
{
    return launch_counting(k_ld_popcount<NS, TAB, MX, IBD1, PAIR>,
                           ld_popcount_lds_bytes(a.max_seg, a.win_per_group, a.tab_len, TAB, NS, IBD1 ? (PAIR ? 4 : 3) : MX ? 2 : 0), a,
                           grid, st, ev);
}

int launch_ld_popcount(const PopArgs &a, unsigned n_targets, int planes, hipStream_t st, KernelEvents ev)
{
    if (a.n_win == 0)
        return 0;
    if (planes < 1 || planes > 8)
        return 1;
    dim3 grid(a.n_runs * a.n_cgroups + (a.fin_prev ? (a.n_win + a.waves_per_group - 1) / a.waves_per_group : 0), 1, n_targets);
    if (a.ibd1 && (!a.mx_counts || !a.tab_in_lds || a.p2_out))
        return 1;
    if (a.pair_sums && !a.ibd1)
        return 1;
    return with_ring_slots(a.ring_slots, [&](auto ns) {
        constexpr int NS = decltype(ns)::value;
        if (a.ibd1)
            return a.pair_sums ? launch_pop<NS, true, true, true, true>(a, grid, st, ev) : launch_pop<NS, true, true, true>(a, grid, st, ev);
        if (a.mx_counts)
            return a.tab_in_lds ? launch_pop<NS, true, true>(a, grid, st, ev) : launch_pop<NS, false, true>(a, grid, st, ev);
        return a.tab_in_lds ? launch_pop<NS, true, false>(a, grid, st, ev) : launch_pop<NS, false, false>(a, grid, st, ev);
    });
}

// The same for groups of IBDG_MT comparison individuals (a.t_base = first of them, n_groups groups)
int launch_ld_popcount_mt(const PopArgs &a, unsigned n_groups, hipStream_t st, KernelEvents ev)
{
    if (a.n_win == 0 || n_groups == 0)
        return 0;
    dim3 grid(a.n_runs * a.n_cgroups, 1, n_groups);
    return with_ring_slots(a.ring_slots, [&](auto ns) {
        constexpr int NS = decltype(ns)::value;
        const size_t lds = ld_popcount_lds_bytes(a.max_seg, a.win_per_group, a.tab_len, a.tab_in_lds != 0, NS, 1);
        return launch_counting(a.tab_in_lds ? k_ld_popcount_mt<NS, true> : k_ld_popcount_mt<NS, false>, lds, a, grid, st, ev);
    });
}

void launch_ld_finalize(const PopFinalArgs &a, unsigned n_targets, hipStream_t st, KernelEvents ev)
{
    if (a.n_win == 0)
        return;
    hipExtLaunchKernelGGL(k_ld_finalize, dim3((a.n_win + 3) / 4, n_targets), dim3(256), 0, st, ev.start, ev.stop, 0, a);
}

}  // namespace ibdg
