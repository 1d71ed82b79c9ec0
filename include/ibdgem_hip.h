/*
 * include/ibdgem_hip.h -- C ABI of the MI355X IBD-likelihood engine.
 *
 * Drop-in boundary for ONE path of Paleogenomics/IBDGem: the per-SNP
 * P(D|IBD0,1,2) arithmetic of src/ibd-math.c and the window / --LD
 * background-panel loop that the reference writes inline in
 * compare_impute()/compare_vcf() (src/ibdgem.c:558-760 and :247-462).
 *
 * The reference has no FFI for this path: the host program
 * calls find_pDgG/find_pDgf/find_pDgIBD1 (src/ibd-math.h:14-63) once per row
 * and runs the LD loop in place.  This header is the seam a maintainer binds
 * instead (INTEGRATION.md shows the patch to compare_impute): the host keeps
 * parsing and row filtering (integer work, src/ibdgem.c:573-630), hands the
 * engine the rows that survive, and prints what comes back.
 *
 * Conventions (mirroring the reference's, src/ibdgem.c:947-1041):
 *   - every call returns 0 on success, non-zero on error; the message is
 *     available from ibdg_last_error(); the library never exits the process
 *     and never falls back to a CPU implementation;
 *   - the caller owns all host buffers; the context owns all device memory;
 *   - one context per device, used from one host thread at a time.
 *
 * Plain C: pointers and sizes only.
 */
#ifndef IBDGEM_HIP_H
#define IBDGEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBDG_ABI_VERSION 5   /* (still 5, additions only: ibdg_log2_switches_host, ibdg_window_log2_switches, ibdg_window_log2_switches_prior, ibdg_switch_penalty_update -- the probability of a switch at every step, the expected switches and the penalties they suggest; ibdg_log2_segments_host, ibdg_window_log2_segments, ibdg_get_log2_segments -- the path's segments with exact scores and support; ibdg_log2_posteriors_host, ibdg_window_log2_posteriors -- forward-backward IBD-state probabilities over the log2 table; option log_windows with ibdg_get_window_log2, ibdg_get_window_log2_all -- window likelihoods as logs that do not underflow; ibdg_upload_candidates, ibdg_num_candidates, ibdg_select_variable_sites, ibdg_get_site_candidates -- the -v site lists made on the device.)  5: ibdg_num_targets, ibdg_upload_panel_fd, ibdg_window_llr_sums; a run over new comparison individuals queues without a host wait; options ibd0_after, mfma_batch_groups, mfma_wg_sum; ibdg_last_count_unit 3.  4: ibdg_ld_layout, ibdg_last_count_unit, ibdg_get_window_ll_all; options compact_tiles, compact_density, compact_targets; the strict kernel is no
                              * longer what a sparse pileup gets.  3: options site_results, stage_workers; ibdg_get_site_af
                              * computes on demand; ibdg_last_run_ms out[4] is 0 */

typedef struct ibdg_ctx ibdg_ctx;

int ibdg_abi_version(void);

/* Number of visible HIP devices (0 if none / no driver). */
int ibdg_device_count(void);

/* Create an engine on `device`.  Replaces init_nCk() + the per-row
 * find_pDgG() calls (src/ibdgem.c:1168, :632-634; src/ibd-math.c:13-81):
 * the (max_cov+1)^2 x 3 table of P(D|G) is built here on the host with libm
 * pow(), exactly as the reference evaluates it, and kept on the device.
 * epsilon = -e, max_cov = -M.  Returns NULL on failure (see
 * ibdg_last_error(NULL)). */
ibdg_ctx *ibdg_create(int device, double epsilon, unsigned max_cov);

/* Replaces destroy_nCk() (src/ibd-math.c:34-43) and frees all device memory. */
void ibdg_destroy(ibdg_ctx *ctx);

/* Last error message of `ctx` (or of the last failed ibdg_create when ctx is
 * NULL).  Never NULL; empty string when there was no error. */
const char *ibdg_last_error(const ibdg_ctx *ctx);

/* Host-side helper: the P(D|G) table the context uses, as
 * out[(n_ref*(max_cov+1)+n_alt)*3 + g], g = 0:(0,0) 1:het 2:(1,1)
 * (src/ibd-math.c:46-81).  out holds (max_cov+1)^2*3 doubles. */
int ibdg_pdg_table(double epsilon, unsigned max_cov, double *out);

/* Host-side twins of find_pDgf and find_pDgIBD1 (src/ibd-math.h:40-63, src/ibd-math.c:84-142) for one
 * row: P(D|IBD0) and P(D|IBD1) from the allele frequency f, the three P(D|G) of the row (a row of
 * ibdg_pdg_table) and, for IBD1, the comparison individual's two alleles (0/1; anything else leaves the
 * value at 1.0 like the reference).  Same operations in the same order as the device kernel (libm pow,
 * no fused multiply-add, zero -> DBL_MIN), so they return the bits ibdg_get_site_ll returns.  For spot
 * checks and bindings that want single values; the engine itself never computes on the host. */
double ibdg_pdg_ibd0(double f, double p00, double p01, double p11);
double ibdg_pdg_ibd1(unsigned a0, unsigned a1, double f, double p00, double p01, double p11);

/* ---- phased panel (the .hap rows / VCF GT columns) ---------------------- */

/* A packed row is ibdg_row_words(n_ids) 64-bit words: for individual n,
 * chunk = n/64, bit = n%64; word[2*chunk] holds the first haplotype
 * (reference hap_buf[4n], src/ibdgem.c:638), word[2*chunk+1] the second
 * (hap_buf[4n+2], :639).  Unused high bits are zero. */
size_t ibdg_row_words(unsigned n_ids);

/* Pack one row of 2*n_ids alleles (0/1 bytes, [2n]=first, [2n+1]=second). */
void ibdg_pack_alleles(const uint8_t *alleles, unsigned n_ids, uint64_t *row);

/* Pack one IMPUTE .hap text row ("0 1 1 0 ...", the reference's hap_buf):
 * characters at even offsets are alleles.  Returns 0, or 1 if the row is
 * shorter than 4*n_ids-1 characters or holds a character other than '0'/'1'
 * at an allele offset. */
int ibdg_pack_hap_text(const char *hap_line, unsigned n_ids, uint64_t *row);

/* Upload n_rows packed rows (host memory, row-major, ibdg_row_words each).
 * Also computes the per-row alternate-allele counts on the device
 * (find_f_impute/find_f_vcf, src/ibd-parse.c:91-110) unless deferred to
 * ibdg_run (see ibdg_set_option "count_in_run"). */
int ibdg_upload_panel(ibdg_ctx *ctx, const uint64_t *rows, size_t n_rows, unsigned n_ids);

/* Same, with the packed rows in a FILE: n_rows x ibdg_row_words(n_ids) x 8 bytes from byte `offset` of the open file `fd`
 * (the host program's packed-panel cache).  The engine's staging threads read the file (pread) straight into their
 * page-locked buffers: the caller maps nothing, so there are no page faults on 2.56 GB of mapping during the upload and
 * no page-table entries to take down when the process ends (80 ms of a 0.45 s run of the host program).  The file
 * offset of `fd` is neither used nor changed; an error if the file ends before the rows do. */
int ibdg_upload_panel_fd(ibdg_ctx *ctx, int fd, uint64_t offset, size_t n_rows, unsigned n_ids);

/* Same, from memory that is already on this context's device
 * (e.g. a torch tensor's data_ptr()); copied device-to-device. */
int ibdg_upload_panel_dev(ibdg_ctx *ctx, const void *dev_rows, size_t n_rows, unsigned n_ids);

/* ---- the rows of one comparison ------------------------------------------ */

/* The rows that passed the reference's filter chain (src/ibdgem.c:584-626)
 * in file order: row_index into the uploaded panel (NULL: site s is panel row
 * s, n_sites <= panel rows), read counts after -D culling
 * (src/ibdgem.c:620-628; n_ref+n_alt <= max_cov), optional -A
 * frequency (NaN = use the panel's own; pointer may be NULL), window = -w.
 * Rows with n_ref+n_alt == 0 get per-site values but join no window
 * (src/ibdgem.c:657-663).  Windows are consecutive runs of `window` covered
 * rows; the last may be shorter (src/ibdgem.c:572-578, :736).
 * The three arrays are copied to the device (6 bytes per row) and everything
 * else -- the covered-row list, the windows, the per-window constants of the
 * --LD kernel -- is derived there (ibdgem_amd/csrc/ibdg_prep.hip); arrays from
 * ibdg_host_alloc are copied at link speed.  Returns when the device is done. */
int ibdg_upload_sites(ibdg_ctx *ctx, const uint32_t *row_index, const uint8_t *n_ref,
                      const uint8_t *n_alt, const double *f_override, size_t n_sites,
                      unsigned window);

/* Same, with row_index / n_ref / n_alt already in this context's device memory
 * (uint32 / uint8 / uint8; dev_row_index may be NULL as above).  f_override
 * stays a HOST array (or NULL): its powers are taken with the host's libm.
 * The call first waits for the whole device (the arrays may come from any stream); with option
 * "dev_inputs_ready" 1 the caller vouches that they are complete and the wait is left out -- the
 * preparation of one context can then run under the --LD kernel of another on the same GPU. */
int ibdg_upload_sites_dev(ibdg_ctx *ctx, const void *dev_row_index, const void *dev_n_ref,
                          const void *dev_n_alt, const double *f_override, size_t n_sites,
                          unsigned window);

/* -v / --variable-sites-only: the rows of a comparison depend on the comparison individual (src/ibdgem.c:584 skips a row
 * at which it is 0/0), but the rows that passed every OTHER filter are the pileup's.  They go to the device once ...
 *
 * The rows of one pileup that passed every filter that does not depend on the comparison individual (what
 * ibdg_upload_sites takes when there is no -v), kept on the device until replaced or until a panel is uploaded.  Same
 * argument rules and errors as ibdg_upload_sites (rows outside the panel and read counts beyond max_cov are reported here,
 * with the candidate's index); f_override may be NULL, its powers are taken with the host's libm once, here.  Does not
 * change the current site list.  6 bytes per candidate of device memory (2 with row_index NULL), 24 more with overrides. */
int ibdg_upload_candidates(ibdg_ctx *ctx, const uint32_t *row_index, const uint8_t *n_ref, const uint8_t *n_alt,
                           const double *f_override, size_t n_cand);
size_t ibdg_num_candidates(const ibdg_ctx *ctx);

/* ... and this makes the current site list, as ibdg_upload_sites would, from the candidates at which individual `target`
 * carries at least one alternate allele, in candidate order.  Everything is derived on the device (the flags from the
 * tile-transposed panel, count / scan / scatter, then the preparation of any upload); the candidates stay.  Afterwards
 * ibdg_num_sites / ibdg_num_windows / ibdg_get_windows / ibdg_run / ibdg_get_* behave exactly as after ibdg_upload_sites of
 * that filtered list (an empty selection included).  Errors: no panel, no candidates, target >= n_ids, window = 0. */
int ibdg_select_variable_sites(ibdg_ctx *ctx, uint32_t target, unsigned window);

/* For each site of the current list its index into the candidates: out[ibdg_num_sites].  An error if the current list
 * did not come from ibdg_select_variable_sites. */
int ibdg_get_site_candidates(ibdg_ctx *ctx, uint32_t *out);

/* Clocks of the last ibdg_upload_sites[_dev] (ms): out[0] host-to-device copies
 * of the arrays, out[1] preparation on the device including its two small
 * read-backs, out[2] the whole call on the host's clock.  After ibdg_select_variable_sites out[0] is the selection
 * (its three kernels and the hand-over of the number selected) instead of copies. */
int ibdg_upload_ms(ibdg_ctx *ctx, float out[3]);

/* Page-locked host memory for arrays handed to ibdg_upload_* / ibdg_get_*:
 * copies to and from it run at the link's speed instead of going through a
 * staging buffer.  NULL on failure.  Any host memory works; this is optional. */
void *ibdg_host_alloc(size_t bytes);
void ibdg_host_free(void *p);

size_t ibdg_num_sites(const ibdg_ctx *ctx);
size_t ibdg_num_windows(const ibdg_ctx *ctx);
/* Comparison individuals of the last ibdg_run: what ibdg_get_window_ll_all copies is
 * ibdg_num_targets x ibdg_num_windows x 3 doubles. */
size_t ibdg_num_targets(const ibdg_ctx *ctx);

/* Per window: index (into the uploaded site list) of its first and last
 * covered row, and NUM_SITES (src/ibdgem.c:723-730, :751-756).  Any pointer
 * may be NULL. */
int ibdg_get_windows(ibdg_ctx *ctx, uint32_t *first, uint32_t *last, uint32_t *n_covered);

/* ---- run ------------------------------------------------------------------- */

/* Evaluate n_targets comparisons (the reference's loop over data->uids,
 * src/ibdgem.c:522) in one call.
 *   targets[t]  individual index of the compared sample (cmp_idx/2)
 *   bg_count    NULL = every individual is background once
 *               (src/ibdgem.c:517-520), else n_ids bytes: how many times the
 *               individual appears in the -B list (read_rf keeps duplicates,
 *               src/ibd-parse.c:262-308); one byte each, so at most 255
 *               listings of one individual (the host program refuses more)
 *   pu_id       individual whose name equals -N, or -1 (src/ibdgem.c:501-506)
 *   ld_mode     --LD: LIBD0/LIBD1 of each window are the background averages
 *               of src/ibdgem.c:736-753; otherwise the plain products (:755).
 * Results stay on the device until fetched. */
int ibdg_run(ibdg_ctx *ctx, const uint32_t *targets, size_t n_targets, const uint8_t *bg_count,
             int pu_id, int ld_mode);

/* AF column: alt-allele fraction per uploaded site (or the -A override): alt count / (2 n_ids), src/ibd-parse.c:98.
 * Computed by this call (it depends on the panel row only), after an ibdg_run. */
int ibdg_get_site_af(ibdg_ctx *ctx, double *af);
/* LIBD0, LIBD1, LIBD2 per site of target t: out[n_sites][3] (tab columns 12-14).  After an --LD run this is the table of the
 * last run's individual t, put together when fetched from the site list's row table (made once per upload of sites or panel
 * by the first --LD run that keeps per-site results); after a non-LD run, the run's own per-site values. */
int ibdg_get_site_ll(ibdg_ctx *ctx, size_t t, double *out);
/* LIBD0, LIBD1, LIBD2 per window of target t: out[n_windows][3] (summary columns 4-6). */
int ibdg_get_window_ll(ibdg_ctx *ctx, size_t t, double *out);
/* The same for every target of the last ibdg_run in one copy: out[ibdg_num_targets][n_windows][3] (a caller that runs batches of
 * comparison individuals takes a batch's tables off the device at once and can queue the next batch before it goes
 * through them: the host program's --summary-only loop, reference src/ibdgem.c:522 with :751-756). */
int ibdg_get_window_ll_all(ibdg_ctx *ctx, double *out);
/* Option "log_windows": log2 of LIBD0, LIBD1, LIBD2 per window of target t, out[n_windows][3] -- the summary columns for
 * windows whose likelihoods leave the double range (at 30x coverage every LIBD0 of a window of 100 rows is below 2^-1074
 * and ibdg_get_window_ll returns 0).  --LD, LIBD0 and LIBD1: log2 of the mean over the background (bg_count's multiplicities,
 * the target and pu_id excluded, src/ibdgem.c:714) of the exact binomial window products, each kept as a mantissa and an
 * integer exponent to the end -- no product is ever brought into the double range; NaN for an empty background, like the
 * linear columns.  Every other column (all three of a non-LD run, LIBD2 of an --LD run): the sum over the window's rows
 * with reads of log2 of the fp64 per-site value ibdg_get_site_ll returns (DBL_MIN clamp included), as a double-double
 * rounded once.  Same waits as ibdg_get_window_ll ("async").  An error if the last ibdg_run was made with the option off. */
int ibdg_get_window_log2(ibdg_ctx *ctx, size_t t, double *out);
/* The same for every target of the last ibdg_run in one copy: out[ibdg_num_targets][n_windows][3]. */
int ibdg_get_window_log2_all(ibdg_ctx *ctx, double *out);
/* The other direction: tab[n_targets][n_windows][3] replaces the log2 table of the last ibdg_run, for tests and for callers
 * that gathered a table elsewhere.  Any double is allowed, NaN and +-inf included.  Everything the ibdg_window_log2_* calls keep
 * (the path, the posteriors, alpha, the segment records, the draws) goes stale; nothing else of the run changes -- the linear
 * window and per-site tables stay -- and the next ibdg_run writes its own table again.  Returns after the copy: tab may go.
 * Errors: no results, the last ibdg_run made with the option off, n_targets != ibdg_num_targets, NULL tab. */
int ibdg_set_window_log2(ibdg_ctx *ctx, const double *tab, size_t n_targets);
/* For each comparison individual t of the last ibdg_run and each window range s = [first[s], end[s]) of its
 * site list: the sums over the range of log2(L2') - log2(L0') and log2(L1') - log2(L0') (L' = L, or 2^-1074 where
 * L == 0), each as a double-double: out[((t * n_seg) + s) * 4 + {0,1,2,3}] = {IBD2/IBD0 hi, lo, IBD1/IBD0 hi, lo}.
 * The terms of the reference's bin/chrarm-stats.py, taken as differences of fp64 logs and summed on the device without
 * copying the window tables back; a NaN window makes its sums NaN, an empty range gives 0, 0.  hi + lo rounded is the
 * same for any split of a range into parts whose double-doubles are added in order.  Errors: no results, end[s] <
 * first[s], end[s] > ibdg_num_windows, NULL arrays with n_seg > 0.  Returns after the sums are in host memory. */
int ibdg_window_llr_sums(ibdg_ctx *ctx, const uint32_t *first, const uint32_t *end, size_t n_seg, double *out);
/* The same sums from the log2 table of option "log_windows": the terms are the table's own entries, +l2, -l0 and +l1, -l0 --
 * no log2 and no 2^-1074 in place of a likelihood that left the double range.  Same out layout, double-double, order of
 * additions, NaN handling, empty ranges and errors; also an error if the last ibdg_run was made with the option off.  An infinite
 * entry (a run writes none; a table of ibdg_set_window_log2 may hold one) makes the sums of a range that holds it NaN, like a NaN. */
int ibdg_window_log2_llr_sums(ibdg_ctx *ctx, const uint32_t *first, const uint32_t *end, size_t n_seg, double *out);

/* The IBD-state path of one window table in the log domain, in integers.  log2_tab[n_win][3] = log2 LIBD0/1/2; p01, p02,
 * p12 the switch penalties of the reference's hiddengem (in (0, 1]).  In quanta of 2^-16 bit: a window's emission is e_s =
 * llrint((l_s - max(l)) * 65536), the difference clamped below at -2^24 -- (0, 0, 0) if a column is NaN or the maximum is not
 * finite --; a penalty is llrint(log2(p) * 65536), clamped below at -2^40, 0 for staying; score[0][s] = e_0[s], score[i][s] =
 * max_q(score[i-1][q] + pen[q][s]) + e_i[s] in int64, the lowest q winning a tie; the path is traced back from the best final
 * score (lowest state on a tie), as the reference's program does with products of probabilities.  No product, so nothing
 * underflows, and a window whose linear columns are all 0 is a window like any other.  path[n_win] (states 0, 1, 2) and
 * score[n_win][3] may be NULL; count[3] = windows per state (all 0 for n_win = 0).  Needs no device.  Errors
 * (ibdg_last_error(NULL)): a penalty outside (0, 1] or NaN, n_win > 2^21 (the bound that keeps |score| < 2^62), NULL count. */
int ibdg_log2_states_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, uint8_t *path,
                          int64_t *score, uint64_t count[3]);
/* The same for every comparison individual of the last ibdg_run, on the device, over its log2 table (option "log_windows"):
 * path[T][n_win], score[T][n_win][3] (either may be NULL: only what is asked for leaves the device), count[T][3].  The same
 * integers as ibdg_log2_states_host on ibdg_get_window_log2's table, bit for bit: integer (max, +) is exact and
 * associative, so the blocks the kernel cuts the windows into do not show.  Same waits as ibdg_get_window_log2; returns with
 * the outputs in host memory.  Errors: no results, the last ibdg_run made with the option off, a penalty out of range,
 * more than 2^21 windows, NULL count. */
int ibdg_window_log2_states(ibdg_ctx *ctx, double p01, double p02, double p12, uint8_t *path, int64_t *score,
                            uint64_t *count);
/* The sum-product companion of ibdg_log2_states_host: IBD-state posteriors of one window table.  The weights are the path's own
 * integers: an emission e_s or a penalty P (quanta of 2^-16 bit, <= 0) weighs 2^(x / 65536), formed as ldexp(T1[j] * T2[i], k) for
 * x = 65536 k + 256 j + i from two 256-entry tables of exp2 made once on the host; an emission weight below 2^-1000 is 0, a
 * window's best state weighs exactly 1.  weight(path) = prod_w b_w[path_w] * prod_{w >= 1} a[path_{w-1}][path_w], Z its sum over
 * all paths; post[n_win][3] (may be NULL) = P(state at window w | all windows), expect[3] = its sums over the windows (expected
 * windows per state), *log2_z = log2 Z.  fp64 sums and products with an integer exponent carried beside every vector, so
 * nothing leaves the double range at any depth or length; the order of the operations is fixed (ibdgem_amd/csrc/ibdg_states.h)
 * and is the device's.  No output is ever NaN: where the weights leave no path (Z = 0: a shifted switch weight that is exactly 0
 * between windows with different single live states, or products of penalties near 1e-300 that underflow) a window's three
 * probabilities are 0, expect omits it and *log2_z = -inf (the dead-chain rule).  Needs no device.  n_win = 0:
 * expect = 0, log2_z = 0.  Errors (ibdg_last_error(NULL)): a penalty outside
 * (0, 1] or NaN, n_win > 2^21, NULL expect or log2_z. */
int ibdg_log2_posteriors_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, double *post,
                              double expect[3], double *log2_z);
/* The same for every comparison individual of the last ibdg_run, on the device, over its log2 table (option "log_windows"):
 * post[T][n_win][3] (may be NULL: then 40 bytes per individual leave the device), expect[T][3], log2_z[T].  The same bytes as
 * ibdg_log2_posteriors_host on ibdg_get_window_log2's table: the same operations in the same order, no atomics.  Same waits as
 * ibdg_get_window_log2; returns with the outputs in host memory.  Errors: no results, the last ibdg_run made with the option
 * off, a penalty out of range, more than 2^21 windows, NULL expect or log2_z. */
int ibdg_window_log2_posteriors(ibdg_ctx *ctx, double p01, double p02, double p12, double *post, double *expect,
                                double *log2_z);
/* A segment of an IBD-state path: a maximal run of windows in one state (ibdgem_amd/csrc/ibdg_states.h).  56 bytes,
 * no padding.  e[s]: the sum over its windows of the emission e_w[s] of ibdg_log2_states_host (quanta of 2^-16 bit; e[state] -
 * max of the other two is the segment's log2 likelihood ratio); post_q: the sum over its windows of llrint(gamma_w[state] *
 * 2^32), gamma the posteriors of ibdg_log2_posteriors_host (post_q / (n_win * 2^32) is their mean); post_min: their minimum.
 * The last two are 0 where the posteriors were not asked for. */
typedef struct ibdg_segment {
    uint32_t first, n_win;      /* its first window (0-based) and how many it has */
    uint32_t state, reserved;   /* 0, 1, 2; 0 */
    int64_t e[3];
    uint64_t post_q;
    double post_min;
} ibdg_segment;
/* The segments of one window table's path.  Runs ibdg_log2_states_host, with with_post != 0 also ibdg_log2_posteriors_host,
 * then walks the path once.  pos_first[n_win], pos_last[n_win]: the position of every window's first and last site, or both NULL.
 * seg (may be NULL) takes at most seg_cap records in window order; *n_seg is always the true count.  summary[12], for state s
 * = 0, 1, 2: [s] its segments, [3 + s] the windows of its longest, [6 + s] the sum over its segments of (pos_last of the last
 * window - pos_first of the first + 1), [9 + s] the largest of these; the last six are 0 without positions.  Integer sums,
 * maxima and an fp64 minimum only: exact whatever the order, hence the same bytes as the device's.  n_win = 0: no segment,
 * summary 0.  Needs no device.  Errors (ibdg_last_error(NULL)): those of the two functions it runs, NULL n_seg or summary, one
 * position array without the other, a window with pos_last < pos_first. */
int ibdg_log2_segments_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, int with_post,
                            const uint64_t *pos_first, const uint64_t *pos_last, ibdg_segment *seg, size_t seg_cap,
                            uint64_t *n_seg, uint64_t summary[12]);
/* The same for every comparison individual of the last ibdg_run, on the device: the kernel of ibdg_window_log2_states, with
 * with_post that of ibdg_window_log2_posteriors -- neither is launched again where that call was made with these penalties since
 * the last ibdg_run --, then one that counts.  pos_first / pos_last [n_win] (both or neither) are the
 * site list's, shared by the individuals.  n_seg[T], summary[T][12]: 104 bytes per individual leave the device.  Same waits
 * as ibdg_get_window_log2; returns with the outputs in host memory.  n_win = 0: zeros.  Errors: no results, the last ibdg_run
 * made with option "log_windows" off, a penalty out of range, more than 2^21 windows, NULL n_seg or summary, one position
 * array without the other, a window with pos_last < pos_first. */
int ibdg_window_log2_segments(ibdg_ctx *ctx, double p01, double p02, double p12, int with_post, const uint64_t *pos_first,
                              const uint64_t *pos_last, uint64_t *n_seg, uint64_t *summary);
/* The records of the last ibdg_window_log2_segments call: the individuals' segments back to back, individual t's n_seg[t]
 * records behind those of the individuals before it (the device holds them as compactly).  cap: the records seg has room
 * for.  Errors: no ibdg_window_log2_segments since the last ibdg_run (or since a later ibdg_window_log2_states /
 * ibdg_window_log2_posteriors call, which reuse its paths), cap smaller than the sum of n_seg, NULL seg with a sum > 0. */
int ibdg_get_log2_segments(ibdg_ctx *ctx, ibdg_segment *seg, size_t cap);
/* Window chains: the three log-domain calls above treat the windows as one chain; a chain start is a window that is
 * treated the way window 0 is -- uniform entry, no switch penalty into it.  starts[n_starts]: the windows >= 1 that start a chain,
 * strictly increasing, every entry in [1, n_win); window 0 always starts one.  At a start the path's step takes every penalty as 0
 * (score[w][s] = max_q score[w-1][q] + e_w[s]; the scores are not reset), the posteriors' step matrix is M_w[q][s] = b_w[s], and a
 * segment begins whatever the state before.  The chains are then independent: inside chain [c0, c1) the path, the posteriors and
 * the segments are those of the table's rows [c0, c1) alone (the scores are the slice's plus max_q score[c0-1][q]; the
 * posteriors within the rounding of the joint pass), counts and expect are the sums, log2 Z the sum, and no segment crosses a
 * border; the chain of a segment follows from its `first`.  The three functions below are ibdg_log2_states_host,
 * ibdg_log2_posteriors_host and ibdg_log2_segments_host with the starts as two more arguments; n_starts = 0 (starts may be NULL)
 * gives their bytes.  Errors, beside theirs: an entry that is 0, >= n_win, or not above the one before it (the message names
 * it), NULL starts with n_starts > 0. */
int ibdg_log2_states_chains_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, uint8_t *path,
                                 int64_t *score, uint64_t count[3], const uint32_t *starts, size_t n_starts);
int ibdg_log2_posteriors_chains_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, double *post,
                                     double expect[3], double *log2_z, const uint32_t *starts, size_t n_starts);
int ibdg_log2_segments_chains_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, int with_post,
                                   const uint64_t *pos_first, const uint64_t *pos_last, ibdg_segment *seg, size_t seg_cap,
                                   uint64_t *n_seg, uint64_t summary[12], const uint32_t *starts, size_t n_starts);
/* The chains of the current site list, for ibdg_window_log2_states / _posteriors / _segments and ibdg_get_log2_segments on the
 * device: the same bytes as the three functions above with these starts.  n_starts = 0 (starts may be NULL) clears them.  They
 * belong to the site list: a later upload of sites or of a panel clears them, an ibdg_run does not (batches of individuals share
 * a list).  The call makes the paths, posteriors and records kept from earlier calls stale; it adds no launch to any call and
 * nothing to ibdg_run.  Errors: the entries' as above (against ibdg_num_windows), no valid site list; a refused call leaves the
 * chains as they were. */
int ibdg_set_window_chains(ibdg_ctx *ctx, const uint32_t *starts, size_t n_starts);
/* The number of chains of the current site list: the starts set plus window 0's; 0 without windows. */
size_t ibdg_num_window_chains(const ibdg_ctx *ctx);
/* Step shifts: every step of the chain pays the same p01 / p02 / p12 in the calls above; a step shift gives each
 * window its own.  shift[n_win]: one int32 per window in quanta of 2^-16 bit, |shift[w]| <= 2^30; shift[0] is ignored.  For a
 * window w >= 1 that does not start a chain the step into w uses P_xy(w) = min(0, max(-2^40, P_xy + shift[w])) for xy = 01, 02,
 * 12 (P_xy = llrint(log2(p_xy) * 65536), the path's integers) and 0 on the diagonal: a shift of +65536 doubles the switch
 * weights of that step, capped at 1, a shift of -65536 halves them.  A chain start wins over the shift (penalty 0, a segment
 * begins); a shift alone never begins a segment.  The path takes its step with these integers; the posteriors take the
 * weights of these integers by the emissions' rule (a weight below 2^-1000 is 0), so that all shifts 0 gives the bytes of
 * no shifts for p >= 2^-1000; the segments change through the path and the posteriors only.  The three functions below are
 * the _chains_host functions with the shifts as one more argument; NULL gives their bytes.  Errors, beside theirs: an entry
 * w >= 1 outside +-2^30 (the message names it). */
int ibdg_log2_states_steps_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, uint8_t *path,
                                int64_t *score, uint64_t count[3], const uint32_t *starts, size_t n_starts, const int32_t *shift);
int ibdg_log2_posteriors_steps_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, double *post,
                                    double expect[3], double *log2_z, const uint32_t *starts, size_t n_starts,
                                    const int32_t *shift);
int ibdg_log2_segments_steps_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, int with_post,
                                  const uint64_t *pos_first, const uint64_t *pos_last, ibdg_segment *seg, size_t seg_cap,
                                  uint64_t *n_seg, uint64_t summary[12], const uint32_t *starts, size_t n_starts,
                                  const int32_t *shift);
/* The step shifts of the current site list, for ibdg_window_log2_states / _posteriors / _segments and ibdg_get_log2_segments on
 * the device: the same bytes as the three functions above with these shifts (and the chains set).  n: ibdg_num_windows, or 0
 * (shift may be NULL) to clear them.  Their lifetime is the chains': a later upload of sites or of a panel clears them, an
 * ibdg_run does not; the call makes the paths, posteriors and records kept from earlier calls stale; it adds no launch to any
 * call and nothing to ibdg_run.  Errors: no valid site list, an n that is neither, NULL shift with n > 0, an entry outside
 * +-2^30; a refused call leaves the steps as they were. */
int ibdg_set_window_steps(ibdg_ctx *ctx, const int32_t *shift, size_t n);
/* 1 if the current site list has step shifts, else 0. */
int ibdg_has_window_steps(const ibdg_ctx *ctx);
/* Sampled paths: n_samples paths of one window table drawn from P(path | all windows) under the weights of
 * ibdg_log2_posteriors_steps_host, by forward filtering and backward sampling (ibdgem_amd/csrc/ibdg_states.h has the rule to the
 * bit: the forward vectors are that pass's own doubles, one splitmix64 value per (draw, window) keyed by seed, stream and the
 * draw's number, three fp64 products, two sums and two comparisons per state drawn).  starts / n_starts and shift as in the
 * _steps_host functions (n_starts = 0 and NULL for none); stream: the individual's, by convention its index in the panel -- a draw
 * depends on (seed, stream, k) alone, and draw k is the same whatever n_samples is.  pos_first / pos_last [n_win] as for the
 * segments, or both NULL.  paths [n_samples][n_win] (may be NULL): the drawn states.  out [n_samples][15], per draw: [0..2] its
 * windows per state, [3..14] the summary[12] of ibdg_log2_segments_host for the drawn path.  Needs no device.  n_win = 0: every
 * record 0.  Errors (ibdg_last_error(NULL)): those of ibdg_log2_posteriors_steps_host, n_samples outside 1 .. 65536, NULL out,
 * one position array without the other, a window with pos_last < pos_first. */
int ibdg_log2_samples_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                           size_t n_starts, const int32_t *shift, size_t n_samples, uint64_t seed, uint64_t stream,
                           const uint64_t *pos_first, const uint64_t *pos_last, uint8_t *paths, uint64_t *out);
/* The same for every comparison individual of the last ibdg_run, on the device, over the context's chains and steps: stream[T],
 * out [T][n_samples][15] -- 120 n_samples bytes per individual leave the device.  The same bytes as ibdg_log2_samples_host on
 * ibdg_get_window_log2's table with stream[t].  The forward vectors are made by the first call with these penalties on a run
 * and kept as the paths and posteriors are; the draws run a workgroup per (individual, draw) pair in chunks of pairs whose
 * paths and records stay under 256 MiB of device memory.  Same waits as ibdg_get_window_log2.  Errors: those of
 * ibdg_window_log2_posteriors, n_samples outside 1 .. 65536, NULL out or stream, one position array without the other, a window
 * with pos_last < pos_first. */
int ibdg_window_log2_samples(ibdg_ctx *ctx, double p01, double p02, double p12, size_t n_samples, uint64_t seed,
                             const uint64_t *stream, const uint64_t *pos_first, const uint64_t *pos_last, uint64_t *out);
/* Draw k of individual t of the last ibdg_window_log2_samples call again: path[n_win], the bytes of ibdg_log2_samples_host's
 * paths[k].  Errors: no such call since the last ibdg_run, ibdg_set_window_chains or ibdg_set_window_steps; t or k out of range;
 * NULL path. */
int ibdg_get_log2_sample_path(ibdg_ctx *ctx, size_t t, size_t k, uint8_t *path);
/* Switches: the pairwise companion of ibdg_log2_posteriors_steps_host under the same weights, chains and shifts.  For
 * every step w - 1 -> w, sw[w][k] = P(the states at w - 1 and w are the two of pair k | all windows), k = 0, 1, 2 for the pairs
 * 01, 02, 12 (either direction); sw[0] = (0, 0, 0); their sum over k is P(a switch at that step).  sw[n_win][3] may be NULL.
 * expect[3] = the sum of sw[w][k] over the counted steps of pair k: w >= 1, w does not start a chain, and without shifts or with
 * P_k + shift[w] <= 0 (a step whose switch weight is capped at 1 does not depend on p_k) -- the expected number of switches that
 * pay p_k, which is d log Z / d log p_k.  counted[3] = the number of counted steps, the same for every individual.  log2_tab ==
 * NULL stands for a table that says nothing (every emission weight 1): expect is then the expectation under the switch weights
 * alone, the prior of ibdg_switch_penalty_update.  The order of the fp64 operations is fixed (ibdgem_amd/csrc/ibdg_states.h) and is
 * the device's; where the weights leave no path the three probabilities of a step are 0, never NaN (the dead-chain rule).  Needs
 * no device.  n_win = 0 or 1: expect = 0, counted = 0.  Errors (ibdg_last_error(NULL)): a penalty outside (0, 1] or NaN, n_win >
 * 2^21, NULL expect or counted, the chains' and the shifts' as in the _steps_host functions. */
int ibdg_log2_switches_host(const double *log2_tab, size_t n_win, double p01, double p02, double p12, const uint32_t *starts,
                            size_t n_starts, const int32_t *shift, double *sw, double expect[3], uint64_t counted[3]);
/* The same for every comparison individual of the last ibdg_run, on the device, over its log2 table (or the one set by
 * ibdg_set_window_log2) and the context's chains and steps: sw[T][n_win][3] (may be NULL: then 24 bytes per individual leave the
 * device), expect[T][3].  The same bytes as ibdg_log2_switches_host on ibdg_get_window_log2's table.  One launch over the scratch
 * of ibdg_window_log2_posteriors: the posteriors and segment records kept from earlier calls go stale (a later call makes them
 * again).  Same waits as ibdg_get_window_log2; returns with the outputs in host memory.  Errors: those of
 * ibdg_window_log2_posteriors, NULL expect. */
int ibdg_window_log2_switches(ibdg_ctx *ctx, double p01, double p02, double p12, double *sw, double *expect);
/* The prior that goes with it: expect[3] and counted[3] of ibdg_log2_switches_host on the NULL table with ibdg_num_windows
 * windows and the context's chains and steps -- one individual's, the same for all.  Runs on the host, launches nothing and
 * leaves everything kept as it is.  Errors: no valid site list, a penalty out of range, more than 2^21 windows, NULL expect or
 * counted. */
int ibdg_window_log2_switches_prior(ibdg_ctx *ctx, double p01, double p02, double p12, double expect[3], uint64_t counted[3]);
/* One step of the penalties towards those at which the posterior expectation of the counted switches equals the expectation
 * under the switch weights alone: next[k] = min(1, max(1e-300, p[k] * total[k] / (n_individuals * prior[k]))) where total[k] and
 * prior[k] are finite and > 0, else next[k] = p[k].  total[3]: expect of the calls above summed over n_individuals individuals;
 * prior[3]: expect of ibdg_log2_switches_host on the NULL table with the same penalties, chains and shifts.  Plain fp64.  Whether
 * repeating the step converges is an observation on simulated input, not a theorem.  Errors: a NULL argument. */
int ibdg_switch_penalty_update(const double p[3], const double total[3], size_t n_individuals, const double prior[3], double next[3]);

/* ---- the fit of the switch penalties: the step above repeated over the kept tables of many individuals ---- */
/* One iteration of the fit as it is reported: the penalties it used, the individuals' expectations added in their order from
 * 0.0, one individual's prior and the counted steps.  96 bytes, no padding. */
typedef struct {
    double p[3], total[3], prior[3];
    uint64_t counted[3];
} ibdg_fit_row;
/* One step of the fit, the same for every route: row = its arguments, next = ibdg_switch_penalty_update's, and *stood = 1 iff
 * for every pair the penalty's integer, llrint(log2(.) * 65536) clamped below at -2^40 (the quanta the kernels read a penalty
 * in), differs between next and p by at most one -- a step below what the model resolves --, else 0.  Errors: a NULL argument,
 * a p[k] outside (0, 1] or NaN. */
int ibdg_switch_fit_step(const double p[3], const double total[3], size_t n_individuals, const double prior[3],
                         const uint64_t counted[3], ibdg_fit_row *row, double next[3], int *stood);
/* The fit on the host, one thread: from p, at most max_iter times { ibdg_log2_switches_host's expect of every table tabs[t]
 * [n_win][3], t < n_individuals, under starts and shift (as there), added in that order from 0.0; the prior and the counted steps
 * from the NULL table; ibdg_switch_fit_step; the next iteration takes `next` }, ending after the first iteration whose step
 * stood.  rows[max_iter]: an ibdg_fit_row per iteration made, *n_rows of them; *stood: whether the last one stood; fitted[3]: its
 * `next`.  max_iter == 0 or n_individuals == 0: no rows, *stood = 0, fitted = p.  Needs no device.  Errors
 * (ibdg_last_error(NULL)): a NULL argument (rows may be NULL with max_iter == 0, tabs with n_individuals == 0), a NULL table
 * with n_win > 0, and those of ibdg_log2_switches_host. */
int ibdg_log2_fit_host(const double *const *tabs, size_t n_individuals, size_t n_win, const double p[3], const uint32_t *starts,
                       size_t n_starts, const int32_t *shift, size_t max_iter, ibdg_fit_row *rows, size_t *n_rows, int *stood,
                       double fitted[3]);
/* The table store: the log2 window tables of many runs over ONE site list kept on the device, [capacity][n_win][3] doubles, so
 * that the fit can run over every individual of a pileup.  It belongs to the site list at hand: an upload of sites or of a panel
 * empties it and takes the reserve away; chains, steps and runs leave it alone.
 * ibdg_log2_store_reserve: an empty store for up to n_individuals tables (no memory yet: the buffer is allocated by the first
 * append, when the number of windows is known; a failed allocation is an error that names the bytes asked for).  Errors: no
 * valid site list (the store belongs to one), more than 2^31 - 1 individuals.
 * ibdg_log2_store_append: the log2 table of every comparison individual of the last ibdg_run (or the one set by
 * ibdg_set_window_log2) goes onto the store's end, device to device, behind the table's writers; complete when the call returns,
 * so the next run may replace the table.  Errors: no results, a run without option log_windows, no reserve, more individuals
 * than reserved.
 * ibdg_log2_store_count: the individuals stored (0 for an emptied store). */
int ibdg_log2_store_reserve(ibdg_ctx *ctx, size_t n_individuals);
int ibdg_log2_store_append(ibdg_ctx *ctx);
size_t ibdg_log2_store_count(ibdg_ctx *ctx);
/* expect[count][3] of ibdg_window_log2_switches for every stored individual under the context's chains and steps, in one launch
 * over the whole store (k_log2_switch_expect): the same bytes as ibdg_log2_switches_host per table.  Scratch of its own (a table's
 * worth per launched workgroup): the posteriors, segment records and draws kept from earlier calls stay as they are.  24 bytes
 * per individual leave the device.  Errors: those of ibdg_window_log2_switches, no reserve. */
int ibdg_log2_store_switches(ibdg_ctx *ctx, double p01, double p02, double p12, double *expect);
/* ibdg_log2_fit_host over the store: per iteration ibdg_log2_store_switches, the sum on the host in store order, the prior of
 * ibdg_window_log2_switches_prior, ibdg_switch_fit_step.  The same bytes as ibdg_log2_fit_host over the stored tables with the
 * context's chains and steps.  Errors: those of ibdg_log2_store_switches, a NULL argument. */
int ibdg_log2_store_fit(ibdg_ctx *ctx, const double p[3], size_t max_iter, ibdg_fit_row *rows, size_t *n_rows, int *stood,
                        double fitted[3]);
/* Alt-allele count of panel rows [first_row, first_row+n): out[n] (for tests). */
int ibdg_get_alt_counts(ibdg_ctx *ctx, size_t first_row, size_t n, uint32_t *out);

/* ---- measurement / tuning --------------------------------------------------- */

/* Device time of the last ibdg_run, from HIP events on the engine's streams:
 * out[0] total (first launch to last completion), out[1] alt-count kernel
 * (0 if not run), out[2] the kernel of the per-row values and window products,
 * out[3] the --LD launches, out[4] 0 (ms; up to ABI 2 the window products were
 * a kernel of their own).  The per-row kernel runs on a second stream beside
 * the --LD kernels, so the parts overlap and need not add up to the total. */
int ibdg_last_run_ms(ibdg_ctx *ctx, float out[5]);

/* The same for the run `back` calls ago (0 = the last one); the engine keeps the
 * events of its last 32 runs.  Waits for the engine's stream first, so it is the
 * way to time runs issued with the "async" option after ibdg_sync. */
int ibdg_run_ms(ibdg_ctx *ctx, unsigned back, float out[5]);

/* Duration (ms) of the dominant --LD kernel alone in that run (k_ld_popcount, or its
 * multi-individual form), from the start / stop times of its own dispatch packet.  An error if the
 * run used the strict kernel or was not an --LD run. */
int ibdg_run_kernel_ms(ibdg_ctx *ctx, unsigned back, float *ms);

/* Which --LD kernel the last ibdg_run used: 0 none (non-LD), 1 the strict
 * kernel (sequential fp64 products in the reference's order), 2 the
 * exponent-counting kernel (same values to ~1e-14), 3 the
 * reference-order mode (strict products, then the background sums taken
 * serially in the reference's order: LIBD0/LIBD1 of every window bit-identical
 * to the reference; ~12x the time of 2). */
int ibdg_last_ld_variant(const ibdg_ctx *ctx);

/* Which tiles the exponent-counting / matrix-core --LD kernels read for the site list at hand: 0 none prepared
 * (no sites, or only the strict kernel applies), 1 the panel's own 32-row tiles (every tile between a window's
 * first and last panel row is streamed), 2 the compacted tiles of this site list: only the rows that carry reads (the
 * rows the reference's window loop multiplies, src/ibdgem.c:596-601, :657-663), back to back (option "compact_align" 1, the
 * default since ABI 5; 32 = every window on a tile boundary), gathered and transposed once per ibdg_upload_sites -- or by
 * the ibdg_run with which the runs on this upload have added up to "compact_targets" comparison individuals -- so that a
 * window costs window / 32 tile words whatever the pileup's density.  Chosen per upload and per run (option
 * "compact_tiles"); the results are the same bits from either. */
int ibdg_ld_layout(const ibdg_ctx *ctx);

/* How the last ibdg_run's exponent-counting launches for single comparison individuals (k_ld_popcount: one individual,
 * or the one to four left over beside the groups of the other kernels) took the weighted sums of a haplotype word:
 * 2 = one matrix instruction per word (v_mfma_scale_f32_16x16x128_f8f6f4: the rows' weights as FP6, the word's bits as
 * FP4; option "mx_counts", the default), 1 = twelve (mask, count) pairs on the vector ALU, 0 = no such launch in that
 * run; 3 = form 2 counting the IBD1 sums only (the instruction returns the table exponents of the four IBD1 products
 * themselves), IBD0 taken from ONE pass over the site list that keeps every background individual's own product per
 * window -- src/ibdgem.c:715, :743: it does not depend on the comparison individual, whose only trace in that sum is its
 * own exclusion, :714 -- (option "ibd0_after").  The sums are exact integers and the floating-point additions the same
 * in the same order in every form: same results, bit for bit. */
int ibdg_last_count_unit(const ibdg_ctx *ctx);

/* How those launches of the last ibdg_run ended a window, i.e. summed its products over a wave's 64 background
 * individuals: 2 = two consecutive windows of a run in one sum tree through 1 KiB of LDS scratch per wave (form 3 above
 * with option "pair_sums" 1, the default, where the scratch leaves as many workgroups on a compute unit as the form has
 * without it), 1 = every window on its own, 0 = no such launch in that run.  The same additions in the same order either
 * way: same results, bit for bit. */
int ibdg_last_window_end(const ibdg_ctx *ctx);

/* Options: "dispatch_events" (0/1: time the --LD launches through their own
 * dispatch packets, which makes ibdg_run_kernel_ms available; costs ~10 us per
 * run more than the default single event record); "async" (0/1: ibdg_run returns as soon as its kernels are queued;
 * ibdg_sync, ibdg_run_ms and every ibdg_get_* wait for them -- lets a caller
 * queue one run per comparison individual without a host round trip between
 * them); "dev_inputs_ready" (0/1: ibdg_upload_sites_dev does not wait for the whole device first, see there);
 * "count_in_run" (0/1: recompute alt counts inside every ibdg_run,
 * so the timed region covers it; beside the --LD kernel the recount runs with "recount_blocks_per_cu"
 * single-wave workgroups per CU, default 4, 0 = its full grid); "site_blocks_per_cu" (default 2: workgroups per CU of the
 * per-row kernel beside the exponent-counting --LD kernel, 0 = its full grid) and "rows_blocks_per_cu" (default 0 = full
 * grid: the same for a non-LD run, where it has the chip to itself); "site_results" (what ibdg_run keeps per row: 1, the default,
 * LIBD0/1/2 of every row and comparison individual for ibdg_get_site_ll -- in --LD mode from the site list's row table, 32 bytes
 * per row, made by the first such run on an upload; 0 nothing -- no n_targets x n_sites x 24 bytes
 * of device memory, no per-row stores, and in --LD mode only the IBD2 pick of a row is computed at all: for callers that
 * want the window table only, e.g. hundreds of comparison individuals in one call; ibdg_get_site_ll then fails.  The AF
 * column never costs a run anything: ibdg_get_site_af computes it when called); "log_windows" (0/1, default 0: every later
 * ibdg_run also leaves log2 of its window columns on the device for ibdg_get_window_log2[_all], T x n_windows x 24 bytes and
 * two small launches per run; works with "site_results" 0 and 1; an --LD run then fails, naming the reason, where the
 * exponent-counting form cannot serve the site list -- a clamped P(D|G) table, max_cov > 50, no prepared segments: the
 * conditions under which "ld_variant" 2 is refused -- while the strict and reference-order variants of the linear columns do
 * not stop it; 0: no allocation, no launch, nothing else changes); "stage_workers" (1..8, default 8: host threads of that staging team -- a caller
 * whose contexts upload at the same time gives each its share); "staged_upload" (0/1, default 1: a panel of 256 MB or more in
 * ordinary host memory goes to the device through page-locked staging buffers filled by a team of host
 * threads instead of the runtime's pageable-memory path); "ld_variant" (0 = pick automatically,
 * 1 = strict, 2 = exponent counting, an error if not applicable, 3 = reference
 * order);
 * "compact_tiles" (set before ibdg_upload_sites: 0, the default = the compacted tiles of ibdg_ld_layout when fewer than
 * one panel row in "compact_density" (default 4) between the first and the last site carries reads, when the rows
 * are not in file order, or once the runs on one upload have added up to "compact_targets" (default 256) comparison
 * individuals -- the site list belongs to the pileup, src/ibdgem.c:522 runs every individual over the same rows; a
 * group of the matrix-core kernel counts as 20, an individual of the counting kernels as 12 (16 with "mx_counts" 0): what
 * each saves on the compacted tiles -- a single run 0.058 of 0.606 ms at chr1 x 2504 -- against the 1.3 ms of the gather
 * and the new segments, i.e. the 22nd single run on an upload re-lays it out -- the panel's own tiles otherwise; 1 =
 * always; -1 = never: sparse or unordered site lists then take the strict kernel);
 * "reserve_compact" (0/1, default 1, set before ibdg_upload_panel: the buffer of the compacted tiles, 1.3 x the
 * panel's, is allocated with the panel so that a re-layout never allocates);
 * "ibd0_after" (default 8; 0 = never: the single comparison individuals run on one upload and background add up, and
 * the run that reaches this number makes the pass of ibdg_last_count_unit's form 3 -- about the cost of one run, a fifth
 * of every later one saved; at once where a run of groups of 15 has made the pass already.  708 MB of device memory at
 * chr1 x 2504);
 * "mx_counts" (0/1, default 1: see ibdg_last_count_unit; applies where a run's records of 128 bytes per (window, tile)
 * segment fit the workgroup's LDS and the powers rho^n 2^(s n) of a window's table stay normal doubles, always so at the
 * table sizes kept in LDS); "sum_dpp" (0/1, default 1: the wave sums of that form exchange by DPP moves instead of
 * ds_swizzle -- same additions, same bits); "pair_sums" (0/1, default 1: see ibdg_last_window_end);
 * "finalize_in_next" (0/1, default 1; with "async" only: a run of single comparison individuals leaves its finalising
 * step -- the sum over the chunks and the background average, src/ibdgem.c:751-752 -- to the next run's --LD launch when
 * that run has the same shape, background and prepared sites (ABI 5: the individuals may differ); whoever reads results or
 * replaces inputs first gets a launch of its own for it: one launch, its gap and an event packet less per queued run, same
 * results);
 * "compact_align" (1, 2, 4, 8, 16 or 32, default 1, set before ibdg_upload_sites: the rows a window of the compacted tiles
 * is rounded up to -- 1 = the site list's rows with reads back to back, no padding; 32 = every window on a tile boundary,
 * round 4's layout);
 * "prep_ahead" (0/1, default 1; with "async" only: what a NEW comparison individual needs before its --LD kernel -- its
 * background weights and window / segment images -- is made on a third stream into a ring of four buffers while the runs
 * before still read theirs; 0: on the main stream, in front of the kernel);
 * "end_in_dispatch" (0/1, default 1: the end event of a run of single individuals is its --LD kernel's own completion
 * signal instead of an event packet behind the kernel -- 7 us less between two queued runs);
 * "chunks_per_wave" (strict kernel tiling, set before ibdg_upload_panel),
 * "waves_per_block" (strict kernel), "windows_per_wave", "guided_runs",
  * "ring_slots" (2, 3, 4 or 8), "record_lds_bytes" (exponent-counting kernel;
 * set before ibdg_upload_sites); "multi_target" (0/1, default 1: with four or more
 * comparison individuals in one ibdg_run, groups of four share a workgroup of
 * the exponent-counting kernel -- same results, ~1.4x the throughput); "mfma_targets" (0/1,
 * default 1: with "mfma_min" (1..15, default 4) or more comparison individuals in one ibdg_run,
 * groups of 15 go through the matrix-core kernel -- the sums that depend on the comparison
 * individual as integer matrix products; same results, ~2.5x the throughput of single runs; "mfma_plain_tau"
 * (0/1, default 1: that kernel looks the powers tau^G of a window up as plain doubles where none of them leaves the
 * double range -- the same bits as the {mantissa, exponent} table it uses otherwise, half the LDS traffic);
 * "mfma_batch_groups" (1..64, default 36: groups of 15 per launch of that kernel -- the groups' workgroups of one run sit
 * next to each other on one XCD, whose L2 then serves the panel's tile words to all but the first of them; bounded by a
 * sixteenth of the device's memory for the groups' operands and partial sums); "mfma_wg_sum" (0/1, default 1: a workgroup of
 * that kernel adds its eight waves' window sums up itself where its LDS allows: an eighth of the partial sums written)).
 * Returns non-zero for an unknown name or a value out of range. */
int ibdg_set_option(ibdg_ctx *ctx, const char *name, long value);

/* Reference-order mode only ("ld_variant" 3): the background individuals in the
 * order the reference walks them -- the lines of the -B file, duplicates kept
 * (data->refids, src/ibd-parse.c:262-308; src/ibdgem.c:741).  Must agree with
 * the bg_count given to ibdg_run.  n = 0 clears it: ascending individuals, each
 * bg_count[n] times, which is the reference's order when there is no -B. */
int ibdg_set_background_order(ibdg_ctx *ctx, const uint32_t *ids, size_t n);

/* Host-side self checks that need no device (for the CPU test tier): "wait_info" = the bounded poll the uploads
 * wait for the site preparation with (the word arrives / the stream ends without it / the stream fails / neither:
 * wall-clock bound).  0 = passed, 1 = unknown check, 2 = failed. */
int ibdg_selftest(const char *what);

/* Block until all work queued on the engine's stream is done. */
int ibdg_sync(ibdg_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* IBDGEM_HIP_H */
