// ibdg_ld_layout.h -- what the image builders (ibdg_ld_images.hip), the counting kernels (ibdg_ld_popcount.hip) and the
// host's LDS sizing share: the widths of the LDS-ready segment records and window constants, and where a workgroup of the
// counting kernels keeps them.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

// LDS image of a segment (8 words, 16-byte aligned):
//   flags | cov0 cov1 cov2 | alt0 alt1 | target words t0 t1
// The masks of the rare higher weight bit-planes (cov3.., alt2..) stay in the global Seg array and
// are fetched with scalar loads by the few segments that have them (flags bit 12) -- keeping them
// out of LDS is what lets a fourth workgroup fit on a CU.
// flags = ring slot of the NEXT segment's pair (3) | its tile half (1) | pairs to advance before it (8)
//       | rare planes present (1) | last segment of its window (1) | - | ncov (8) | nalt (8)   (host-built)
// The hot half is read with two BROADCAST ds_read_b128 (every lane the same address), so the
// masks land in VGPRs: on gfx950 a VALU instruction with an SGPR operand issues at half the rate
// of one with VGPR operands only (tools/ubench/issue_rates.hip: v_and_b32 4.1 vs 2.4 cycles),
// and a wave-uniform mask is just as good in a VGPR.
#define IBDG_REC_WORDS 8
// LDS image of a window's constants (8 words), all but eK already table BYTE OFFSETS (16 bytes per
// entry), so that the window end forms its ten table addresses without a shift of their own:
//   eK  16*AT  16*<t0,cov>  16*<t1,cov> | 16*(AT-<t0,alt>)  16*(AT-<t1,alt>)  0  -
// (k_win_target); while a workgroup stages them it adds the LDS address of the table each one indexes
// (rho^n: words 1, 4, 5; sigma^n: words 2, 3, 6), see stage_wc.
#define IBDG_WC_WORDS 8
// LDS image of a segment for the counts on the matrix cores (k_ld_popcount<.., MX = true>; 32 words):
//   flags cov0 cov1 cov2 | t0 t1 - - | four A fragments of 24 bytes: the rows' weights in FP6 for the sums
//   <x,cov> <x,alt> <x & t0,cov> <x & t1,cov>  (k_win_target_mx; flags bit 12 there: planes beyond cov 0-2 / alt 0-2)
#define IBDG_RECX_WORDS 32
// LDS images for groups of IBDG_MT comparison individuals (k_ld_popcount_mt, written by k_win_target_mt):
//   segment, 8 + 2 TB words:        flags cov0 cov1 cov2 | alt0 alt1 - - | TB x {t0 t1}   (IBDG_RECM_WORDS)
//   window, 8 + 4 TB words:         mK(2) eK CT | 16*AT 0 - - | TB x {16*<t0,cov> 16*<t1,cov> 16*(AT-<t0,alt>) 16*(AT-<t1,alt>)}
//   (table byte offsets like IBDG_WC_WORDS; the staging adds the table bases, stage_wc)
#ifndef IBDG_MT
#define IBDG_MT 4
#endif
#define IBDG_RECM_WORDS (8 + 4 * ((IBDG_MT + 1) / 2))      /* target words padded to whole uint4 */
#define IBDG_WCM_WORDS (8 + 4 * IBDG_MT)

namespace ibdg {

// LDS of one workgroup of the counting kernels, as byte offsets: [max_seg] records, [win_per_group] window constants, the
// two power tables (tab_entry_bytes per entry: 16 as {mantissa, exponent} pairs, 8 as plain doubles, 0 where they stay in
// global memory), then from the next KiB on a ring of ring_slots tile pairs per wave and -- for the forms that sum through
// LDS -- 1 KiB of wave_sum2 scratch per wave.
struct LdsLayout {
    size_t rec, wc, tab, ring, scratch, bytes;
};

__host__ __device__ constexpr LdsLayout ld_lds_layout(uint32_t max_seg, uint32_t win_per_group, uint32_t tab_len, uint32_t rec_words,
                                                      uint32_t wc_words, uint32_t tab_entry_bytes, uint32_t ring_slots,
                                                      uint32_t waves, bool has_scratch)
{
    const size_t head = ((size_t)max_seg * rec_words + (size_t)win_per_group * wc_words) * 4 + 15;
    const size_t ring = (head + (size_t)tab_len * 2 * tab_entry_bytes + 1023) & ~(size_t)1023;
    const size_t scratch = ring + (size_t)waves * ring_slots * 1024;
    return {0, (size_t)max_seg * rec_words * 4, head & ~(size_t)15, ring, scratch, scratch + (has_scratch ? (size_t)waves * 1024 : 0)};
}

}  // namespace ibdg
