// ibdg_ctx.h -- the state behind the C ABI (ibdg_api.cpp), grouped by what replaces it: a panel, the candidates of a
// pileup, an upload of sites, a layout cut from it, a background; the tables of the context; the options; and the cached
// device products, each with the key it was made for and its own rule of validity (fresh / made / drop).
// What stops being valid when an input changes is said once, in ibdg_api.cpp's panel_replaced, sites_replaced,
// layout_changed, background_changed and targets_changed.
#pragma once
#include "ibdg_kernels.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    uint64_t allocs = 0;        // bumped by ensure() whenever it hands out new memory: what was in the buffer is gone (a grown
                                // buffer may come back at the old address, so neither the address nor the capacity is the test)
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

inline void release_all(std::initializer_list<DevBuf *> bufs)
{
    for (DevBuf *b : bufs)
        b->release();
}

struct ibdg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;    // per-site + window-product kernels run beside the --LD kernels
    hipStream_t stream3 = nullptr;    // what a NEW comparison individual needs before its --LD kernel (indices, weights, the
                                      // individual's window / segment images), made under the --LD kernel of the run before
    std::string err;
    int n_cu = 256;
    size_t dev_mem_bytes = 0;               // the device's memory (hipMemGetInfo at ibdg_create)

    // page-locked staging for large panels from pageable memory (staged_upload)
    struct Staging {
        static constexpr int WORKERS = 8;
        static constexpr size_t BYTES = (size_t)8 << 20;
        void *stage[2 * WORKERS] = {};
        hipEvent_t stage_ev[2 * WORKERS] = {};
    } stg;

    // Set by ibdg_set_option (OPTION_TABLE below: names, ranges) and ibdg_set_background_order; nothing is derived here.
    struct Options {
        long count_in_run = 0;
        long dispatch_events = 0;   // 1: time the --LD launches through their own dispatch packets (hipExtLaunchKernel);
                                    // gives the dominant kernel's own duration, but costs ~10 us per run more than
                                    // one event record (measured), so it is off unless asked for
        long async = 0;    // 1: ibdg_run returns once its kernels are queued
        long rows_blocks = 0;   // non-LD run: workgroups of k_rows_windows per CU (resident grid, each wave takes several windows); 0 = one wave per pair of windows
        long dev_inputs_ready = 0;   // 1: ibdg_upload_sites_dev trusts the caller that its arrays are complete (no device-wide wait)
        long cpw = 0;      // 0 = auto
        long waves = 8;
        long variant = 0;  // 0 auto, 1 strict products, 2 exponent counting, 3 strict products + serial sums in
                           // the reference's order (bit-identical --LD columns)
        std::vector<uint32_t> bg_order;   // optional: the background list in the reference's order (ibdg_set_background_order)
        long wpg = 16;     // windows per wave in the fast kernel (upper bound unless set explicitly)
        bool wpg_fixed = false;
        long multi_target = 1;   // groups of comparison individuals share a workgroup (k_ld_popcount_mt)
        long mfma_targets = 1;   // 5 or more comparison individuals: groups of IBDG_TG through the matrix cores (k_ld_mfma)
        long mfma_plain_tau = 1; // k_ld_mfma looks tau^G up as a plain double where a window's powers allow it (same bits, half the LDS bytes)
        long mfma_min = 4;       // smallest (last) group worth a launch of its own (round 4: a group of 4 takes 2.09-2.17 ms, four single runs 2.5; a group of 3 2.14 against 1.87 for three single runs since their counts moved to the matrix cores -- 3 until then; of 2: 2.13 against 1.28)
        long mfma_wg_sum = 1;    // the matrix-core kernel's workgroups add their eight waves' sums up themselves (where LDS allows)
        long mfma_batch = 36;    // groups of 15 per launch of the matrix-core kernel (540 individuals)
        long guided = 4;   // shrink the runs towards the end of the grid (0 = uniform runs; n scales the
                           // estimate of workgroups in flight by n/4 -- 4 measured best at 500k and 4M rows)
        long ring = 2;     // LDS ring slots per wave (2, 3, 4 or 8); 2 measured fastest (fewest LDS bytes)
        long recbytes = 12 * 1024;   // LDS budget for one run's segment records
        long site_blocks = 2;        // 256-thread workgroups per CU of the per-row kernel inside an --LD run (k_win_ibd2; 0 = its full
                                     // grid): 2 the fastest step of 1, 2, 4 (8) in each round of profiles/r06_side_geometry.txt
        long recount_blocks = 4;     // single-wave workgroups per CU of k_alt_count when it runs inside an --LD run
                                     // (0 = the full grid; 4 measured best: tools/recount_sweep.py)
        long compact = 0;            // tiles the --LD kernels read: 0 = chosen per upload (the panel's own where the pileup is
                                     // dense, compacted where it is sparse or the rows are out of file order) and
                                     // per run (many comparison individuals), 1 = always compacted, -1 = never
        // single comparison individuals take their IBD0 terms from the IBD0 pass (Ibd0Pass) too once their runs on one upload
        // and background have added up to "ibd0_after" individuals (the pass costs about one run and saves a fifth of every later one)
        long ibd0_after = 8;         // 0: never
        long prep_ahead = 1;
        long end_in_dispatch = 1;    // the end event of a run of single individuals rides in its --LD kernel's dispatch packet (0: an event packet behind it): -7 us of a 91 us step on an eighth of a chromosome, profiles/r05_shard_steps.txt
        long fin_next = 1;           // queued runs of single individuals: a run's finalising step rides in the next run's --LD launch
        long sum_dpp = 1;            // ... its wave sums by DPP moves (0: ds_swizzle, as the vector-ALU form)
        long pair_sums = 1;          // the IBD1 form sums two consecutive windows of a run in one tree through LDS scratch, where the scratch costs no workgroup per CU (0: every window by DPP moves alone)
        long mx_counts = 1;          // k_ld_popcount: the counts of a haplotype word by one matrix instruction (0: 12 (mask, count) pairs)
        long reserve_compact = 1;    // their buffer is allocated with the panel's (a panel's worth x 1.3 of HBM more per context)
        long compact_align = 1;      // rows a window of the compacted tiles is rounded up to: 1 = the rows back to back (no padding; a
                                     // window straddles tiles like on the panel's own rows), 32 = every window on a tile boundary
                                     // (round 4's layout: 28 % padding at windows of 100 rows)
        long compact_density = 4;    // compacted when fewer than 1 panel row in this many between the first and last site carries reads
                                     // (tools/density_sweep.py: one comparison at 1 row in 3: 0.82 ms in place, 0.94 compacted; in 4: 0.76 / 0.76; in 5: 0.79 / 0.65)
        long compact_targets = 256;  // ... or when the runs on one upload add up to this many comparison individuals of the
                                     // matrix-core kernel k_ld_mfma (the re-layout is paid once: one of them saves 0.007 ms of
                                     // 0.185, the gather costs 1.5; an individual of the counting kernels counts as 16 with
                                     // (mask, count) pairs -- it saves 0.04-0.09 ms of 0.77 -- and as 12 with mx_counts: 0.058 of 0.606)
        long site_results = 1;       // 1: per-site LIBD0/1/2 kept for ibdg_get_site_ll; 0: not -- no T x n_sites x 24 B of HBM,
                                     // no per-site stores (window results only).  (The AF column is made on demand.)
        long staged_upload = 1;      // panels of 256 MB and more from pageable memory go through the staging team
        long log_windows = 0;        // 1: every run also leaves log2 of its window columns on the device (WinLog below); 0: no
                                     // allocation, no launch and no event edge of it
        long stage_workers = Staging::WORKERS;    // host threads of the staging team (two 8 MB page-locked buffers each): a caller with
                                                  // several contexts uploading at once gives each a share of the cores
    } opt;

    // Functions of epsilon and max_cov: made per context, the power tables grown on demand (grow_pow_tables)
    struct Tables {
        double eps = 0.02;
        unsigned max_cov = 20;
        std::vector<double> lut_h;
        DevBuf lut;
        bool pop_lut_ok = false;     // P(D|G) table is the unclamped binomial form
        std::vector<unsigned long> nck_h;
        DevBuf nck_dev;
        // power tables (functions of epsilon only; grown on demand, see grow_pow_tables)
        std::vector<ibdg::PowEntry> p1_h, p2_h, p3_h;      // rho^n, sigma^n, tau^n = (rho / sigma^2)^n (k_ld_mfma)
        std::vector<ibdg::WinRaw> pb_h;
        // pow1/pow2: rho^n, sigma^n as {f64 mantissa, i32 exponent}; powb: (1-eps)^n in the x87 format
        DevBuf pow1, pow2, pow3, powb;
        size_t tab_dev = 0;                 // entries the device copies hold
        size_t tab_fail_from = (size_t)-1;  // first exponent whose power leaves the 32-bit exponent field
        void free_bufs() { release_all({&lut, &nck_dev, &pow1, &pow2, &pow3, &powb}); }
    } tab;

    // The panel: replaced by ibdg_upload_panel* (prepare_panel lays the geometry out, panel_replaced says what goes with it)
    struct Panel {
        DevBuf panel, alt_count, t32, pow_tab;
        size_t n_rows = 0;
        unsigned n_ids = 0;
        uint32_t n_chunks = 0, stride = 0, n_groups = 0, n_pairs = 0;
        int cpw = 0;
        bool counts_valid = false;
        void free_bufs() { release_all({&panel, &alt_count, &t32, &pow_tab}); }
    } pan;

    // The candidates of one pileup (-v: ibdg_upload_candidates): the rows that passed every filter that does not look at the
    // comparison individual, kept until replaced or until a panel is uploaded.  ibdg_select_variable_sites compacts those at
    // which an individual is not 0/0 into in_row / in_ref / in_alt (and `fo`) -- the buffers an upload from the host fills --
    // and sel_cand, and hands them to upload_sites_core.  Stream edges: none of its own.  Writers and readers are all on the
    // main stream (the copies of ibdg_upload_candidates, the selection kernels, stage A behind them, the copy of
    // ibdg_get_site_candidates), every one of these calls waits on the host for all streams before it queues anything
    // (quiesce), and what reads in_* / sel_cand later on another stream (stage B on stream2: rec_cov only) is ordered behind
    // stage A by ev_prepA as after any upload.
    struct Candidates {
        DevBuf row, ref, alt, fo, sel_cand;
        size_t n_cand = 0;
        bool valid = false, have_rows = false, have_fo = false;
        bool sel_valid = false;             // the current site list came from ibdg_select_variable_sites (sel_cand is its map)
        void free_bufs() { release_all({&row, &ref, &alt, &fo, &sel_cand}); }
    } cand;

    // One upload of sites (the sites of the current comparison) and its hand-over from the preparation kernels.
    // The hand-over: every stage of the preparation (the selection of -v, stage A, each pass of stage B) accumulates what the
    // host must learn in info_dev, and its last workgroup copies the block to info_h, writes the stage's number to
    // info_h->seq last, and leaves info_dev as empty_prep_info() for the next.  The host takes the next number from prep_seq,
    // queues the stage and polls info_h->seq for it (wait_info).  Writers: the device alone writes info_dev and info_h, but
    // for clean_prep_info, which resets a fresh or dirty info_dev, and the upload of an empty list, which fills info_h itself;
    // hand_over alone writes prep_seq and sets prep_dirty, and it or clean_prep_info clears it.
    struct Sites {
        DevBuf rec_all, rec_cov, cov_site, fo;
        DevBuf in_row, in_ref, in_alt;      // device copies of the caller's arrays (ibdg_upload_sites)
        DevBuf scan_tmp, info_dev, win_first, win_last;
        ibdg::PrepInfo *info_h = nullptr;   // host-mapped mirror of the device's PrepInfo, filled in by the preparation kernels
        uint32_t prep_seq = 0;              // hand-overs so far (info_h->seq == prep_seq: the latest one has arrived)
        bool prep_dirty = false;            // the device's PrepInfo may hold the leavings of an upload that did not finish
        size_t seg_room = 0;                // segments the array was cleared for by stage A
        bool have_fo = false;
        size_t n_sites = 0;
        uint32_t n_cov = 0, window = 0, n_win = 0;
        uint32_t first_row = 0, last_row = 0;   // panel rows of the first / last site of the upload
        std::vector<uint32_t> win_first_h, win_last_h;   // fetched on the first ibdg_get_windows after an upload
        bool win_bounds_valid = false;
        bool sites_valid = false;           // an upload of sites has succeeded since the last upload of a panel
        hipEvent_t ev_up[3] = {};           // before the host-to-device copies, after them, after the last prep kernel
        hipEvent_t ev_prep2 = nullptr;      // stream2: the per-window constants of an upload are there
        hipEvent_t ev_prepA = nullptr;      // main stream: the site records of an upload are there (behind k_prep_site_scatter)
        float up_ms[3] = {0.f, 0.f, 0.f};   // copies, preparation on the device (with its host round trips), whole call
        bool up_ms_pending = false;         // the first two are still to be read from the events
        void free_bufs()
        { release_all({&rec_all, &rec_cov, &cov_site, &fo, &in_row, &in_ref, &in_alt, &scan_tmp, &info_dev, &win_first, &win_last}); }
    } sites;

    // What build_segments produces from the site list: the fast --LD variant's layout (exponent counting, ibdg_ld_popcount.hip).
    // The scalar fields belong to the accepted layout: commit_layout alone writes them.  That there is none say
    // build_segments at its start (pop_sites_ok), build_layout's reset (which also decides pop_dense_enough), sites_replaced
    // and panel_replaced; the runs add to relayout_credit.  The buffers and runs_h are filled by the attempt itself, before
    // its verdict: with pop_sites_ok false they may hold a refused attempt's.
    struct Layout {
        // the compacted tiles of the current site list (k_gather_transpose32) and whether the segments,
        // window constants and control words at hand were cut from them (true) or from the panel's own tiles (false)
        DevBuf t32c;
        uint32_t n_pairs_c = 0;
        bool compact = false;
        DevBuf segs, seg_first, wconst, wraw;
        uint32_t wpg = 0, max_seg = 0;     // most windows per workgroup run and its largest segment count
        uint32_t n_runs = 0;               // runs of consecutive windows (DevBuf runs: n_runs+1 first windows)
        DevBuf runs;
        std::vector<uint32_t> runs_h;
        int tab_in_lds = 0;
        int seg_ring = 4;                  // ring depth the segment control words were built for
        uint32_t n_segs = 0, ct_max = 0;
        int planes = 0;
        bool pop_sites_ok = false;   // site rows strictly increasing, segments built
        bool pop_dense_enough = true; // the site list went to the layout asked for (false: "compact_tiles" -1 on a sparse pileup)
        uint64_t relayout_credit = 0;      // what the runs on this upload would have saved on the compacted tiles so far, in
                                           // comparison individuals of the matrix-core kernel (see ibdg_run)
        void free_bufs() { release_all({&t32c, &segs, &seg_first, &wconst, &wraw, &runs}); }
    } lay;

    // The background of the last run whose device copy (base_w) is still valid
    struct Background {
        DevBuf base_w;                      // background multiplicities without the comparison individual's exclusion
        int base_sum = 0;                   // sum of base_w
        std::vector<uint8_t> prev_bg;
        int prev_pu = -2, prev_has_bg = -1;
        size_t prev_lanes = 0;
        uint64_t bg_gen = 1;                // bumped whenever the background multiplicities change
        void free_bufs() { release_all({&base_w}); }
    } bg;

    // Generations the cached products below are keyed by; only panel_replaced, sites_replaced and layout_changed bump them.
    uint64_t sites_gen = 0;            // bumped by every upload of sites and every change of layout
    uint64_t up_gen = 1;               // bumped by every upload of a panel or of sites (a change of layout leaves it)

    // Timing events of the last runs (asynchronous runs are timed after the fact).  Every event
    // record is a barrier packet the command processor retires in ~5 us, so the main stream carries
    // one per run (end of the --LD launches) plus a start only when the stream may have been idle.
    struct Timeline {
        static constexpr int EV_RING = 33;      // the last 32 runs can be queried
        struct EvSet {
            hipEvent_t start_own = nullptr;     // recorded when the previous run's end cannot serve as start
            hipEvent_t ld_end = nullptr;        // main stream, after the last --LD launch
            hipEvent_t k_start = nullptr, k_stop = nullptr;   // start / stop of the dominant --LD kernel's dispatch
            bool has_kernel_times = false;
            hipEvent_t s2_start = nullptr;      // stream2: before its first kernel of the run
            hipEvent_t s2_count = nullptr;      // stream2: after the alt-count kernel
            hipEvent_t s2_end = nullptr;        // stream2: after the per-site values and window products (one kernel)
            hipEvent_t prep = nullptr;          // main stream: the target operands of the matrix-core kernel are built
            hipEvent_t start = nullptr;         // start_own or the previous run's ld_end
            bool recount = false, ld = false;
            bool rows_on_main = false;          // non-LD run: the one kernel went to the main stream, stream2 was not used
        } evs[EV_RING];
        int ev_head = 0;
        long runs_done = 0;
        bool chain_ok = false;      // main stream has been busy since the head run's ld_end was queued
        bool s2_pending = false;    // stream2 holds work the main stream has not waited for yet
        hipEvent_t last_s2 = nullptr;
    } tl;

    // ---- the cached device products: buffers, the key they were made for, fresh() / made() / drop() ----

    // The site list's row table, [n_sites][4] {LIBD0, LIBD1 under genotype 0, 1, 2}: what the rows' per-site values are for any
    // comparison individual (they differ by the genotype picked).  Made by the first --LD run that keeps per-site results and
    // finds it stale, used by every later one: ibdg_get_site_ll expands it for the last run's individual t (k_site_expand).
    // It depends on the site records and -A overrides (an upload of sites), the alt counts and n_ids (an upload of the panel)
    // and the P(D|G) table (fixed per context) -- hence on up_gen.  Stream edges:
    //   writer  stream2 of the run that makes it (k_rows_windows<ROWS_TAB> for one individual, k_row_table for several),
    //           behind that run's recount of the alt counts when it recounts
    //   reader  k_site_expand on the main stream, behind join_streams (the main stream waits for stream2's last event, which
    //           comes after the writer), and the fetch behind it waits on the host for both streams: no reader outlives its call
    //   a rebuild happens only after an upload (which waits on the host for every stream before it changes anything) or when
    //   ensure() has replaced the buffer (which also waits for every stream first, and whose new buffer holds no table)
    struct RowTable {
        DevBuf row_tab;
        uint64_t up_gen = 0, allocs = 0;    // up_gen the table was made for (0: none), in which allocation of row_tab
        bool fresh(const ibdg_ctx &c) const { return up_gen == c.up_gen && allocs == row_tab.allocs; }
        void made(const ibdg_ctx &c) { up_gen = c.up_gen; allocs = row_tab.allocs; }
        void drop() { up_gen = 0; }
    } rt;

    // What does NOT depend on the comparison individuals (round 5): every background individual's weighted product of
    // its own genotype factors per window (src/ibdgem.c:715, :743 -- the IBD0 terms) and their sums per chunk, from one pass of
    // k_ld_popcount per site list and background (with some individual's images: the product does not look at them)
    struct Ibd0Pass {
        DevBuf p2w, p2c, p2_tw, p2_wt;
        uint64_t sites_gen = 0, bg_gen = 0;     // sites_gen / bg_gen the pass was made for
        int mx = -1;                            // ... and the form of its records (RunPlan::mx_counts)
        bool fresh(const ibdg_ctx &c, int mx_counts) const
        { return sites_gen == c.sites_gen && bg_gen == c.bg.bg_gen && mx == mx_counts; }
        void made(const ibdg_ctx &c, int mx_counts) { sites_gen = c.sites_gen; bg_gen = c.bg.bg_gen; mx = mx_counts; }
        void drop() { sites_gen = 0; }
    } p2;

    // The runs of single individuals on one upload and background so far, for option "ibd0_after" (plan_run)
    struct Ibd0Counter {
        uint64_t ibd0_runs = 0, bg_gen = 0;
        bool fresh(const ibdg_ctx &c) const { return bg_gen == c.bg.bg_gen; }
        void made(const ibdg_ctx &c) { bg_gen = c.bg.bg_gen; ibd0_runs = 0; }
        void drop() { bg_gen = 0; ibd0_runs = 0; }
    } ibd0;

    // [n_segs][3][6 words]: the IBD1 form's fragments that do not depend on the individual (k_frag_base)
    struct FragBase {
        DevBuf fragb;
        hipEvent_t ev_fb = nullptr;
        uint64_t sites_gen = 0;                 // sites_gen they were made for
        bool fresh(const ibdg_ctx &c) const { return sites_gen == c.sites_gen; }
        void made(const ibdg_ctx &c) { sites_gen = c.sites_gen; }
        void drop() { sites_gen = 0; }
    } fb;

    // the per-target LDS images of k_win_target (segment records with the target's tile words, window constants) depend
    // on the prepared sites and the targets only: a further run over the same sites and targets reuses them
    struct Images {
        DevBuf wtarget, twords;
        struct Key {                       // what the images were made for: sites_gen (0: nothing), comparison
            uint64_t gen;                  // individuals [first, first + count) of prev_targets, the form of the records (option
            uint32_t first, count;         // mx_counts, IBD1), the ring slot and the allocations of the two buffers
            int mx, ibd1, slot;
            uint64_t wt_allocs, tw_allocs;
            bool operator==(const Key &o) const
            {
                return gen == o.gen && first == o.first && count == o.count && mx == o.mx && ibd1 == o.ibd1 && slot == o.slot &&
                       wt_allocs == o.wt_allocs && tw_allocs == o.tw_allocs;
            }
        } key = {0, 0, 0, -1, -1, -1, 0, 0};
        Key key_for(const ibdg_ctx &c, uint32_t first, uint32_t count, int mx, int ibd1, int slot) const
        { return {c.sites_gen, first, count, mx, ibd1, slot, wtarget.allocs, twords.allocs}; }
        bool fresh(const Key &want) const { return key == want; }
        void made(const Key &k) { key = k; }
        void drop() { key.gen = 0; }
    } img;

    // Option "log_windows": log2 of LIBD0, LIBD1, LIBD2 of every window and comparison individual of the last run,
    // [T][n_win][3] (ibdg_ld_log.hip; ibdg_get_window_log2[_all]).  A result of a run like win_ll, not a cached product: every
    // run with the option on writes all of it, `valid` says whether the last run did.  Replaced by: the next run (whole), an
    // ensure() that swaps the buffer (which waits on the host for every stream first).  Stream edges:
    //   writers  k_ld_log (columns 0, 1 of an --LD run) on the main stream, in front of the run's --LD launches -- behind
    //            ring_settle, i.e. behind stream3's preparation of the individuals it reads, and inside the run's start / end
    //            events, so that ring_prepare's wait for a slot's last reader covers it ("end_in_dispatch" is off with the
    //            option on: the run's end is an event behind everything);
    //            k_win_log_rows (column 2 of an --LD run, all three otherwise) behind the run's k_rows_windows on ITS stream:
    //            stream2 in front of the run's s2_end, or the main stream of a non-LD run that needs no recount;
    //            ibdg_set_window_log2's copy of the caller's table over the whole of it, on the main stream behind join_streams
    //            and waited for on the host (it calls ls.drop(): what the state calls keep is a function of the table)
    //   readers  the copies of ibdg_get_window_log2[_all] only, on the main stream behind join_streams (the main stream waits
    //            for stream2's last event), followed by a host wait: no reader outlives its call
    //   the two writers of an --LD run are on different streams and write different columns; a queued next run's k_ld_log may
    //   overtake this run's k_win_log_rows as its --LD kernels overtake k_win_ibd2 on win_ll -- entries of results nobody can
    //   fetch any more.
    struct WinLog {
        DevBuf win_log2;
        bool valid = false;              // the last run was made with the option on
    } wlog;

    // The table store (ibdg_log2_store_*): win_log2 of many runs over ONE site list kept side by side,
    // `tabs` [cap][n_win][3] with `count` of them filled, for the fit of the switch penalties over every individual of a pileup.
    // Replaced by: a site list or a panel (sites_replaced, panel_replaced call empty(): the tables speak of the windows of the list
    // that goes; the reserve goes with them, so nothing is appended to a store that was sized for another list).  Runs, chains and
    // steps do not touch it: batches of individuals share a site list, and the chains and steps are read when a call is made.
    // `tabs` is allocated by the first append behind a reserve (n_win is known then) and keeps its memory when emptied; `scr`
    // [grid][n_win][3] and `out` [count][3] are k_log2_switch_expect's own scratch and output, so that nothing LogStates keeps
    // goes stale.  Stream edges:
    //   writer  ibdg_log2_store_append's device-to-device copy on the main stream behind join_streams (win_log2's writers are in
    //           front of it: WinLog above), waited for on the host before the call returns -- the next run may replace win_log2
    //   reader  k_log2_switch_expect on the main stream, followed by the copy of `out` and a host wait: no reader outlives its call
    struct LogStore {
        DevBuf tabs, scr, out;
        size_t cap = 0, count = 0;       // individuals reserved / stored
        bool reserved = false;
        void empty() { cap = count = 0; reserved = false; }
    } lstore;

    // The log-domain state calls over win_log2 of the last run (ibdg_window_log2_states / _posteriors / _segments,
    // ibdg_get_log2_segments; ibdg_states.hip).  Each product is a stage that is queued on the main stream behind join_streams
    // and followed, in the public call, by the copies out and a host wait: no reader of the table and no kernel of this group
    // outlives its call.  Two products are kept from call to call, with the penalties (in quanta) they were made for:
    //   the path   `path` (`from` on the way, then the states [T][n_win]) + `count` [T][3]          k_log2_states
    //   the post.  `post` (beta, then gamma [T][n_win][3]) + `pout` (expect, Z: [T][5])             k_log2_posteriors
    // A stage whose product is fresh for the call's penalties does not launch; `score` [T][n_win][3] is not kept, so a call
    // that wants scores launches anyway.  States, posteriors and segments with the same penalties on one run thus launch each
    // kernel once.  The key is the penalties and nothing else: both products are functions of win_log2 and the penalties, and
    // drop() is called where a run starts (ibdg_run), wherever have_results is cleared (panel_replaced, sites_replaced) and by
    // ibdg_set_window_log2 -- the only places where the table, T or n_win can change.  The buffers' allocation counts are NOT part of the key (as
    // they are for RowTable or Images): between two drops T and n_win are fixed, every ensure() of this group asks for the
    // same size again, and so it cannot move a buffer that holds a fresh product.
    // The records: records_made says that `path` (and with_post: `post`) are what the last ibdg_window_log2_segments used and
    // `n_seg` its counts, for ibdg_get_log2_segments to cut the records from.  Reuse goes forward only: a states or
    // posteriors call drops the records again (records_drop), whatever its penalties, and so does drop().
    // The chains: the windows that start a chain besides window 0, as ibdg_set_window_chains took them (`chains`,
    // strictly increasing in [1, n_win)), and their bits on the device (`cmask`, ceil(n_win / 32) words, uploaded by the setter
    // behind a host wait, read by all four kernels; mask() is NULL without chains).  They belong to the site list, not to a
    // run: the setter drops the kept products (drop()) and bumps `chain_gen`, which is part of both products' key beside the
    // penalties; panel_replaced and sites_replaced clear them (chains_clear); the start of a run does not -- batches of
    // individuals share a site list.
    // The steps: the windows' step shifts as ibdg_set_window_steps took them (`steps`, n_win entries or none) and
    // on the device (`cshift`, uploaded by the setter behind a host wait, read by k_log2_states and k_log2_posteriors; shift()
    // is NULL without steps).  Their lifetime is the chains' in every respect: the same generation counter, the same two
    // places that clear them (steps_clear), and a run that does not.
    // The draws: a third kept product under the same rule and key,
    //   alpha      `alpha` (the forward vectors [T][n_win][3])                                        k_log2_alpha
    // made by the first ibdg_window_log2_samples that finds it stale and by no other call; `smp` is what that call was made with
    // (penalties, K, seed, the streams, host and device), for ibdg_get_log2_sample_path to draw one path again -- dropped with
    // the products.  `spath` (the drawn paths of the pairs in flight), `srec` (their records) and `ssum` (their summaries
    // [pairs][13]) are scratch of one chunk of pairs.
    // The switches keep nothing: ibdg_window_log2_switches runs k_log2_switches over `post` and `pout` as its own
    // scratch and output, and marks the posteriors there stale (have[POST] = false, records_drop) before it launches.
    // The rest is scratch of one call: `ptab` (the two tables, uploaded with every posteriors launch), `spos` (the windows'
    // positions [2][n_win]), `sout` (summaries and counts [T][13]), `soff` (record offsets [T]), `recs` (the records).
    struct LogStates {
        DevBuf path, score, count, post, pout, ptab, spos, sout, soff, recs, cmask, cshift, alpha, sstream, spath, srec, ssum;
        enum Product { PATH, POST, ALPHA };
        bool have[3] = {false, false, false};
        int64_t P[3][3] = {};
        struct Draws {
            bool ok = false;
            int64_t P[3] = {};
            double a[3] = {};
            size_t K = 0;
            uint64_t seed = 0;
            std::vector<uint64_t> stream;
        } smp;
        std::vector<uint32_t> chains;    // the chain starts of the site list at hand
        uint64_t chain_gen = 1, gen[3] = {0, 0, 0};     // bumped with every change of `chains` or `steps`; what each product was made for
        const uint32_t *mask() const { return chains.empty() ? nullptr : (const uint32_t *)cmask.p; }
        void chains_clear() { if (!chains.empty()) ++chain_gen; chains.clear(); drop(); }
        std::vector<int32_t> steps;      // the step shifts of the site list at hand
        const int32_t *shift() const { return steps.empty() ? nullptr : (const int32_t *)cshift.p; }
        void steps_clear() { if (!steps.empty()) ++chain_gen; steps.clear(); drop(); }
        bool recs_ok = false, with_post = false;
        std::vector<uint64_t> n_seg;     // per individual of the last ibdg_window_log2_segments
        bool fresh(Product k, const int64_t want[3]) const
        { return have[k] && gen[k] == chain_gen && P[k][0] == want[0] && P[k][1] == want[1] && P[k][2] == want[2]; }
        void made(Product k, const int64_t made_for[3])
        { have[k] = true; gen[k] = chain_gen; P[k][0] = made_for[0]; P[k][1] = made_for[1]; P[k][2] = made_for[2]; }
        bool records_fresh() const { return recs_ok; }
        void records_made() { recs_ok = true; }
        void records_drop() { recs_ok = false; }
        void drop() { have[PATH] = have[POST] = have[ALPHA] = recs_ok = smp.ok = false; }
        void free_bufs()
        {
            release_all({&path, &score, &count, &post, &pout, &ptab, &spos, &sout, &soff, &recs, &cmask, &cshift, &alpha, &sstream, &spath,
                         &srec, &ssum});
        }
    } ls;

    // The finalising step of the last run of single individuals (k_ld_finalize's work) when it has been left to the NEXT
    // run's k_ld_popcount launch (option "finalize_in_next"): whoever reads results or replaces inputs first makes up for
    // it with a launch of its own (flush_finalize).  The partial sums alternate between the two halves of their buffer.
    struct PendingFin {
        bool pending = false;
        ibdg::PopFinalArgs args;
        unsigned count = 0;             // comparison individuals of the launch
        uint64_t sites_gen = 0;         // sites_gen of the run that left it
        int half = 0;                   // the half of `partial` the next such run writes
    } fin;

    // per-run scratch of the --LD launchers: the grouped individuals' images, the partial sums of the counting kernels;
    // many comparison individuals (k_ld_mfma): target operands of a batch of groups, window constants per slot,
    // partial sums per half chunk; ld_variant 3: per-individual products and the background order
    DevBuf wtarget_mt, twords_mt, partial, aimg, wc_slot, partial_h, vals, order;

    int last_variant = 0;
    int last_count_unit = 0;           // 2: the last --LD run's single-individual launches counted on the matrix cores, 1: by (mask, count) pairs, 0: no such launch
    int last_window_end = 0;           // ... and their window ends: 2: two consecutive windows per sum tree (the IBD1 form's paired end), 1: every window summed on its own, 0: no such launch
    // the comparison individuals of the previous ibdg_run whose device copies are still valid
    std::vector<uint32_t> prev_targets;
    // New comparison individuals reach the device without a host wait (the reference's loop hands every individual of the panel
    // to the same rows in turn, src/ibdgem.c:522: a NEW individual per run is the normal case): their indices go through a
    // weights kernel's arguments (a small ring of page-locked slots beyond IBDG_TG_INLINE of them) into one slot of a ring of
    // `targets` buffers (the kernels of earlier runs may still read the others), and the weights / background sizes that follow
    // from them are made on the device (k_target_weights) from the run's background multiplicities `base_w`; `nrefpanel` is a
    // ring as well -- a finalising step left to the next run reads its own run's entry.
    // `ring` and its functions (ring_prepare, ring_settle, ring_slot, ring_mark_readers) own all of it and its stream edges:
    // runs of up to AHEAD_MAX_T individuals keep SLOTS copies of it, so that the NEXT run's can be made (on stream3) while the
    // runs before still read theirs; larger runs use the buffers whole (slot 0), on the main stream.
    // (round 5, later: a RING of four instead of two halves -- the preparation of run i + 1 then waits for the end of run i - 3,
    // not of run i - 1, so it is long done when the --LD kernel of run i ends even on an eighth of a chromosome, where a step is
    // 70 us and the chain "wait, copy, weights, images, record" on stream3 takes 40: profiles/r05_shard_steps.txt)
    struct Ring {
        static constexpr int SLOTS = 4;             // of `targets`, `weight`, wtarget / twords
        static constexpr int NREF_SLOTS = 2 * SLOTS;   // `nrefpanel`, twice as long: a finalising step left to the next run
                                                        // reads its own run's entry one run later than anything else of that run
        static constexpr size_t AHEAD_MAX_T = 64;   // runs of up to that many individuals prepare ahead
        static constexpr int STAGE_SLOTS = 4;       // page-locked staging of the indices
        uint32_t *stage[STAGE_SLOTS] = {};
        size_t stage_cap = 0;                       // comparison individuals a staging slot holds
        hipEvent_t stage_ev[STAGE_SLOTS] = {};
        int stage_next = 0;
        int cur = 0;                                // the slot the current comparison individuals sit in
        int nref = 0;                               // ... and their slot of `nrefpanel`
        hipEvent_t main_read[SLOTS] = {}, s2_read[SLOTS] = {};   // the last reader of a slot: main stream, stream2
        bool main_pending[SLOTS] = {}, s2_pending[SLOTS] = {};
        hipEvent_t ready = nullptr;                 // the current comparison individuals' data are complete (where made)
        bool unsettled = false;                     // stream3 holds a preparation the other streams do not wait for yet
        hipEvent_t ev_s3sync = nullptr;             // main stream: the prepared sites stream3's kernels read are complete
        uint64_t s3_gen = 0;                        // sites_gen stream3 has been ordered behind
    } ring;

    // run state / results
    DevBuf targets, weight, nrefpanel, af, site_ll, win_ll;
    DevBuf llr_seg, llr_part, llr_out;  // ibdg_window_llr_sums: segments, partial sums per block of windows, the sums
    size_t n_targets = 0;
    bool have_results = false;
    int res_site_mode = 0;           // the mode the last run's results were produced under

    // every DevBuf of the context, through its groups
    void free_bufs()
    {
        tab.free_bufs(); pan.free_bufs(); cand.free_bufs(); sites.free_bufs(); lay.free_bufs(); bg.free_bufs();
        release_all({&rt.row_tab, &p2.p2w, &p2.p2c, &p2.p2_tw, &p2.p2_wt, &fb.fragb, &img.wtarget, &img.twords});
        release_all({&wtarget_mt, &twords_mt, &partial, &aimg, &wc_slot, &partial_h, &vals, &order});
        release_all({&targets, &weight, &nrefpanel, &af, &site_ll, &win_ll, &llr_seg, &llr_part, &llr_out, &wlog.win_log2});
        release_all({&lstore.tabs, &lstore.scr, &lstore.out});
        ls.free_bufs();
    }
};

// ibdg_set_option, one row per option: what it accepts and what else setting it does.  A value outside a RANGE or a SET is
// refused with "NAME must be <text>" (<text> null: "<lo>..<hi>"); a CLAMP pulls it into [lo, hi]; BOOL stores value != 0;
// ANY stores it unchecked.  SET: bit v of `lo` says value v is allowed.
struct OptionRow {
    const char *name;
    long ibdg_ctx::Options::*member;
    enum Kind { BOOL, RANGE, CLAMP, SET, ANY } kind;
    long lo = 0, hi = 0;
    const char *text = nullptr;
    enum Effect { NONE, JOIN_STREAMS, FIX_WPG } effect = NONE;  // join the streams first (a pending finalising step is made up
                                                                // for); the run length is the caller's from now on (wpg_fixed)
};

constexpr long opt_set(std::initializer_list<int> values)
{
    long m = 0;
    for (int v : values)
        m |= 1L << v;
    return m;
}

using Opt = ibdg_ctx::Options;
const OptionRow OPTION_TABLE[] = {
    {"count_in_run", &Opt::count_in_run, OptionRow::BOOL},
    {"multi_target", &Opt::multi_target, OptionRow::BOOL},
    {"mfma_targets", &Opt::mfma_targets, OptionRow::BOOL},
    {"mfma_plain_tau", &Opt::mfma_plain_tau, OptionRow::BOOL},
    {"mfma_min", &Opt::mfma_min, OptionRow::RANGE, 1, IBDG_TG},
    {"guided_runs", &Opt::guided, OptionRow::ANY},
    {"compact_align", &Opt::compact_align, OptionRow::SET, opt_set({1, 2, 4, 8, 16, 32}), 0, "1, 2, 4, 8, 16 or 32"},
    {"mfma_wg_sum", &Opt::mfma_wg_sum, OptionRow::BOOL},
    {"mfma_batch_groups", &Opt::mfma_batch, OptionRow::CLAMP, 1, 64},
    {"ibd0_after", &Opt::ibd0_after, OptionRow::CLAMP, 0, LONG_MAX},
    {"end_in_dispatch", &Opt::end_in_dispatch, OptionRow::BOOL},
    {"prep_ahead", &Opt::prep_ahead, OptionRow::BOOL},
    {"dispatch_events", &Opt::dispatch_events, OptionRow::BOOL},
    {"async", &Opt::async, OptionRow::BOOL},
    {"dev_inputs_ready", &Opt::dev_inputs_ready, OptionRow::BOOL},
    {"staged_upload", &Opt::staged_upload, OptionRow::BOOL},
    {"stage_workers", &Opt::stage_workers, OptionRow::RANGE, 1, ibdg_ctx::Staging::WORKERS},
    {"compact_tiles", &Opt::compact, OptionRow::RANGE, -1, 1, "-1 (never), 0 (auto) or 1 (always)"},
    {"finalize_in_next", &Opt::fin_next, OptionRow::RANGE, 0, 1, "0 or 1", OptionRow::JOIN_STREAMS},
    {"sum_dpp", &Opt::sum_dpp, OptionRow::RANGE, 0, 1, "0 or 1"},
    {"mx_counts", &Opt::mx_counts, OptionRow::RANGE, 0, 1, "0 or 1"},
    {"pair_sums", &Opt::pair_sums, OptionRow::RANGE, 0, 1, "0 or 1"},
    {"reserve_compact", &Opt::reserve_compact, OptionRow::RANGE, 0, 1, "0 or 1"},
    {"compact_density", &Opt::compact_density, OptionRow::RANGE, 1, 1000000},
    {"compact_targets", &Opt::compact_targets, OptionRow::RANGE, 1, 65536},
    {"site_results", &Opt::site_results, OptionRow::RANGE, 0, 1, "0 or 1"},
    {"log_windows", &Opt::log_windows, OptionRow::RANGE, 0, 1, "0 or 1"},
    {"rows_blocks_per_cu", &Opt::rows_blocks, OptionRow::RANGE, 0, 128},
    {"site_blocks_per_cu", &Opt::site_blocks, OptionRow::RANGE, 0, 128},
    {"recount_blocks_per_cu", &Opt::recount_blocks, OptionRow::RANGE, 0, 128},
    {"chunks_per_wave", &Opt::cpw, OptionRow::RANGE, 0, 5},
    {"waves_per_block", &Opt::waves, OptionRow::RANGE, 1, 8},
    {"ld_variant", &Opt::variant, OptionRow::RANGE, 0, 3, "0 (auto), 1 (strict), 2 (exponent counting) or 3 (reference order)"},
    {"ring_slots", &Opt::ring, OptionRow::SET, opt_set({2, 3, 4, 8}), 0, "2, 3, 4 or 8"},
    {"record_lds_bytes", &Opt::recbytes, OptionRow::RANGE, 1024, 96 * 1024},
    {"windows_per_wave", &Opt::wpg, OptionRow::RANGE, 1, 65536, nullptr, OptionRow::FIX_WPG},
};
