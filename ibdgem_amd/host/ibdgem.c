/*
 * ibdgem.c -- host program of the MI355X IBD-likelihood engine: the reference's
 * command line, input formats and output files, with the likelihood arithmetic done by
 * libibdgem_hip.so (include/ibdgem_hip.h).
 *
 * What stays on the CPU is what the north star leaves there: option parsing, text parsing
 * and the integer row filter chain of compare_impute (reference src/ibdgem.c:572-630).
 * What the reference computes per row and per window in that loop (:632-667, :669-722,
 * :736-756) is one ibdg_run per batch of comparison individuals.  On a machine without a HIP
 * device a non-LD run (BASELINE configs[0]: "plumbing, runs without a GPU") takes the per-row
 * values and the window products from the library's own host twins of the reference's math seam
 * (ibdg_pdg_table / ibdg_pdg_ibd0 / ibdg_pdg_ibd1, src/ibd-math.h:14-63) in the reference's
 * sequential order (host_nonld below); an --LD run without a device stops with the engine's
 * error -- the background-panel loop exists on the device only.
 *
 * Differences from the reference, all outside the BASELINE configs:
 *   - VCF input (-V) follows the IMPUTE semantics: any number of comparison individuals (the
 *     reference frees its genotype regex inside the per-individual loop, src/ibdgem.c:472, and
 *     crashes on the second one) and the -B background indexed by individual (the reference's VCF
 *     loop indexes genotypes by list position, src/ibdgem.c:374-375);
 *   - no 30720-byte line limit (src/file-io.h:10); .hap rows with a character other than
 *     '0'/'1' at an allele offset are counted as skipped instead of read as garbage;
 *   - the genotype files are read once, not once per comparison individual
 *     (src/ibdgem.c:771-772);
 *   - extra long option --plan: print, per comparison individual, the rows that pass the
 *     filter chain with their integer columns and the window boundaries, and exit.  It is the
 *     hook the CPU-only tests use to check the host logic against the reference's outputs.
 */
#define _GNU_SOURCE
#include <ctype.h>
#include <float.h>
#include <getopt.h>
#include <limits.h>
#include <math.h>
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#ifdef __GLIBC__
#include <malloc.h>
#include <sys/mman.h>
#endif
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <fcntl.h>
#include <errno.h>

#include "../../include/ibdgem_hip.h"
#include "hgpath.h"
#include "ingest.h"
#include "lineio.h"
#include "pileup.h"

/* ---- options (names and defaults: reference src/ibdgem.c:21-66) ------------------- */
static double opt_eps = 0.02, opt_min_qual = 0, opt_max_af = 1, opt_min_af = 0, opt_target_dp = 0;
static unsigned opt_max_cov = 20;
static int opt_window = 100;
static const char *opt_sq = "UNKWN";
static int opt_ld = 0, opt_plan = 0, opt_summary_only = 0, opt_ref_order = 0, in_impute = 0, in_vcf = 0;
static int has_S = 0, has_s = 0, has_B = 0, has_A = 0, has_p = 0, has_v = 0, has_D = 0;
static int opt_threads = 0;
static const char *cache_fn = NULL, *dump_panel_fn = NULL;
static int opt_stats_only = 0, has_arm = 0;
static int opt_log_summary = 0;          /* --log-summary: the summary's likelihoods as log2, from the engine's option "log_windows" */
static int opt_posteriors = 0;           /* --posteriors: with --log-stats --states, the forward-backward probabilities of the states beside the path */
static long opt_fit = 0;                 /* --fit-penalties N: with --log-stats --states, the update of --switches repeated at most N times over the kept log tables of all the pileup's individuals */
static int has_fit = 0;
static int opt_switches = 0;             /* --switches: with --log-stats --states, the probability of a switch at every step, the expected switches and the penalties they suggest */
static int opt_segments = 0;             /* --segments: with --log-stats --states, the path's segments with their scores and support */
static int has_chain_gap = 0;            /* --chain-gap BP: with --log-stats --states, a window more than BP behind the end of the one before starts a chain */
static unsigned long opt_chain_gap = 0;
static int has_switch_scale = 0;         /* --switch-scale X: with --log-stats --states, the penalties hold for two windows X apart; a step's switch weight scales with its distance */
static double opt_switch_scale = 0.0;
static const char *genetic_map_fn = NULL; /* --genetic-map FILE: the distances of --switch-scale in centimorgans along this map */
static double *gmap_pos = NULL, *gmap_cm = NULL;    /* ... its entries: position, cumulative cM */
static size_t gmap_n = 0;
static int has_sample_paths = 0;         /* --sample-paths K: with --log-stats --states, K paths per individual drawn from the posterior of the weights whose best path they find */
static unsigned long opt_sample_paths = 0;
static int has_seed = 0;                 /* --seed N: the seed of those draws (uint64) */
static uint64_t opt_seed = 1;
static int opt_log_stats = 0;            /* --log-stats: --arm-stats and --states from the log2 window table (no underflow), into log* files */
static int opt_states = 0, has_pen = 0;  /* --states: the IBD-state path of every comparison (hgpath.c), --p01/--p02/--p12 its penalties */
static double opt_p01 = HG_DEFAULT_P01, opt_p02 = HG_DEFAULT_P02, opt_p12 = HG_DEFAULT_P12;
static unsigned long arm_c0, arm_c1;     /* --arm-stats: the centromeric range [c0, c1] of the run's chromosome */

static struct option longopts[] = {
    {"LD", no_argument, &opt_ld, 1},
    {"plan", no_argument, &opt_plan, 1},
    {"summary-only", no_argument, &opt_summary_only, 1},
    {"stats-only", no_argument, &opt_stats_only, 1},
    {"arm-stats", required_argument, 0, 1006},
    {"states", no_argument, &opt_states, 1},
    {"log-summary", no_argument, &opt_log_summary, 1},
    {"log-stats", no_argument, &opt_log_stats, 1},
    {"posteriors", no_argument, &opt_posteriors, 1},
    {"segments", no_argument, &opt_segments, 1},
    {"switches", no_argument, &opt_switches, 1},
    {"fit-penalties", required_argument, 0, 1016},
    {"chain-gap", required_argument, 0, 1011},
    {"switch-scale", required_argument, 0, 1012},
    {"genetic-map", required_argument, 0, 1013},
    {"sample-paths", required_argument, 0, 1014},
    {"seed", required_argument, 0, 1015},
    {"p01", required_argument, 0, 1008},
    {"p02", required_argument, 0, 1009},
    {"p12", required_argument, 0, 1010},
    {"reference-order", no_argument, &opt_ref_order, 1},
    {"rand-stream", required_argument, 0, 1000},
    {"fmt-check", required_argument, 0, 1005},
    {"devices", required_argument, 0, 1001},
    {"threads", required_argument, 0, 1002},
    {"panel-cache", required_argument, 0, 1003},
    {"dump-panel", required_argument, 0, 1004},
    {"vcf", required_argument, 0, 'V'},
    {"hap", required_argument, 0, 'H'},
    {"legend", required_argument, 0, 'L'},
    {"indv", required_argument, 0, 'I'},
    {"pileup", required_argument, 0, 'P'},
    {"pileup-name", required_argument, 0, 'N'},
    {"pileup-list", required_argument, 0, 1007},
    {"window-size", required_argument, 0, 'w'},
    {"allele-freqs", required_argument, 0, 'A'},
    {"sample-list", required_argument, 0, 'S'},
    {"sample", required_argument, 0, 's'},
    {"background-list", required_argument, 0, 'B'},
    {"max-cov", required_argument, 0, 'M'},
    {"downsample-cov", required_argument, 0, 'D'},
    {"out-dir", required_argument, 0, 'O'},
    {"max-af", required_argument, 0, 'F'},
    {"min-af", required_argument, 0, 'f'},
    {"positions", required_argument, 0, 'p'},
    {"min-qual", required_argument, 0, 'q'},
    {"chromosome", required_argument, 0, 'c'},
    {"error-rate", required_argument, 0, 'e'},
    {"variable-sites-only", no_argument, 0, 'v'},
    {"help", no_argument, 0, 'h'},
    {0, 0, 0, 0}};

static void usage(int code)
{
    fputs("ibdgem (MI355X engine): likelihood that low-coverage reads (pileup) and a genotyped\n"
          "individual share 0, 1 or 2 chromosomes identical by descent, per SNP and per window.\n\n"
          "Usage: ibdgem [--LD] -H hap -L legend -I indv -P pileup [options]\n"
          "       ibdgem [--LD] -H hap -L legend -I indv --pileup-list FILE [options]\n"
          "  --LD                      background-panel (linkage-aware) window likelihoods\n"
          "  -H/--hap, -L/--legend, -I/--indv FILE   IMPUTE genotype input (plain or .gz)\n"
          "  -V/--vcf FILE             VCF genotype input (plain or .gz), biallelic SNP rows with 0/1 genotypes\n"
          "  -P/--pileup FILE          samtools pileup of the unknown sample (required)\n"
          "  -N/--pileup-name STR      name of the pileup sample (default UNKWN)\n"
          "  --pileup-list FILE        several pileups against the one panel in one run, instead of -P / -N: a line\n"
          "                            'NAME PATH' per pileup ('#' lines skipped); every pileup gets the files and\n"
          "                            messages `-P PATH -N NAME` would give it, in list order.  With --devices each\n"
          "                            context holds the whole panel and takes whole pileups from the list\n"
          "  -A/--allele-freqs FILE    CHROM POS AF table overriding the panel's own frequencies\n"
          "  -S/--sample-list FILE     individuals to compare against, one per line\n"
          "  -s/--sample STR           the same, comma separated\n"
          "  -B/--background-list FILE individuals forming the --LD background panel\n"
          "  -p/--positions FILE       restrict to these sites (CHROM POS or BED)\n"
          "  -q/--min-qual FLOAT       minimum QUAL (VCF input only)\n"
          "  -M/--max-cov INT          skip sites with more informative reads (default 20)\n"
          "  -F/--max-af, -f/--min-af FLOAT   alternate-allele frequency range (default 0..1)\n"
          "  -D/--downsample-cov FLOAT thin the reads to this mean depth\n"
          "  -w/--window-size INT      covered sites per summary window (default 100)\n"
          "  -O/--out-dir DIR          output directory (default: current directory)\n"
          "  -c/--chromosome STR       use only this chromosome of the pileup / -A / -p files\n"
          "  -e/--error-rate FLOAT     sequencing error rate (default 0.02)\n"
          "  -v/--variable-sites-only  skip sites where the compared individual is 0/0\n"
          "  --devices LIST            GPUs to spread the windows of each comparison over, e.g. 0,1,2,3\n"
          "                            (default 0); every GPU holds the whole panel, the windows are cut\n"
          "                            into contiguous ranges, one per GPU, and gathered on the host\n"
          "  --threads INT             host threads for reading the .hap file and writing the output files\n"
          "                            (default: the CPUs available to the process, at most 16)\n"
          "  --panel-cache FILE        keep the bit-packed panel of the .hap file in FILE and reuse it\n"
          "                            while the .hap file is unchanged\n"
          "  --summary-only            write the *.summary.txt files only (no per-site *.tab.txt files: the\n"
          "                            per-site values are neither copied back from the device nor formatted)\n"
          "  --arm-stats START,END     also write <out>/<pileup-name>.armstats.txt: per comparison individual the\n"
          "                            p-arm and q-arm sums of log2(LIBD2/LIBD0) and log2(LIBD1/LIBD0) over the\n"
          "                            summary windows, leaving out the centromeric range START..END (the\n"
          "                            reference's bin/chrarm-stats.py; summed on the device)\n"
          "  --states                  also write <out>/<pileup-name>.<individual>.hiddengem.txt: the most probable path\n"
          "                            of IBD0/1/2 states over the individual's summary windows, what `hiddengem -s`\n"
          "                            prints for its *.summary.txt; and <out>/<pileup-name>.ibdstates.txt: per\n"
          "                            individual the windows in each state and their fractions, then the totals\n"
          "                            (the reference's bin/sum-hiddengem.py).  Computed in the individual's output\n"
          "                            job on the host, beside the device's next batch\n"
          "  --log-summary             also write <out>/<pileup-name>.<individual>.logsummary.txt: the rows of the\n"
          "                            summary with LOG2_LIBD0 LOG2_LIBD1 LOG2_LIBD2 in place of the likelihoods, which\n"
          "                            leave the double range from moderate coverage on (0.000000e+00 in the summary);\n"
          "                            --LD columns from the exact exponents of the window products, on the device\n"
          "  --log-stats               with --arm-stats and/or --states: take the statistics from log2 of the window\n"
          "                            likelihoods (what --log-summary prints) instead of the likelihoods, which are 0 from\n"
          "                            moderate coverage on: <out>/<pileup-name>.logarmstats.txt (the sums of the logs\n"
          "                            themselves, no 2^-1074 in place of a 0), <pileup-name>.<individual>.loghiddengem.txt\n"
          "                            (the path with the largest sum of log2 emissions and penalties, in integers of\n"
          "                            2^-16 bit: nothing underflows, a window of zeros poisons nothing) and\n"
          "                            <pileup-name>.logibdstates.txt, in place of the three linear files; summed, and\n"
          "                            with --stats-only on one device also traced, on the device\n"
          "  --posteriors              with --log-stats --states: also the sum over ALL paths of the weights whose best path\n"
          "                            --log-stats finds (forward-backward, same --p01/--p02/--p12):\n"
          "                            <out>/<pileup-name>.<individual>.logposteriors.txt, per window the probability of\n"
          "                            IBD0/1/2 given all windows and the most probable state (the lowest on a tie); and\n"
          "                            <out>/<pileup-name>.logibdposteriors.txt, per individual the expected windows per\n"
          "                            state, their fractions and log2 of the paths' total weight, then the totals.  With\n"
          "                            --stats-only only the second file, on one device computed there\n"
          "  --segments                with --log-stats --states: also the level above the path, its segments (maximal runs of\n"
          "                            windows in one state): <out>/<pileup-name>.<individual>.logsegments.txt, per segment\n"
          "                            its state, first and last window, START of the first and END of the last, length,\n"
          "                            windows, sites, the sums of the three log2 emissions over it (exact, in bits) and the\n"
          "                            state's sum less the larger of the other two (Log2_LR); with --posteriors also the\n"
          "                            mean and the minimum of the state's probability inside it; and\n"
          "                            <out>/<pileup-name>.logibdsegments.txt, per individual and state the number of\n"
          "                            segments, the windows of the longest, the base pairs of all and of the longest, then\n"
          "                            the totals.  With --stats-only only the second file, on one device computed there\n"
          "  --chain-gap BP            with --log-stats --states: break the chain of windows wherever a window's START lies more\n"
          "                            than BP (an integer >= 1) behind the END of the window before it -- a centromere, a\n"
          "                            stretch without sites.  Such a window is entered like the first one: no switch penalty\n"
          "                            into it, and no segment (hence no base pair of a length) crosses the gap; the chains'\n"
          "                            paths, posteriors and segments are independent.  A gap inside a window breaks nothing.\n"
          "                            The files keep their formats; *.logsegments.txt gains a first column Chain (1-based)\n"
          "  --switch-scale X          with --log-stats --states: --p01, --p02 and --p12 hold for two windows whose centres\n"
          "                            ((START + END) / 2) lie X apart (a decimal > 0; base pairs, or centimorgans with\n"
          "                            --genetic-map); a step of distance D has its switch weights multiplied by D / X, capped\n"
          "                            at 1: switching costs more between close windows and less across sparse stretches.  In\n"
          "                            the path's integers: log2(D / X) * 65536, rounded, is added to the step's penalties.\n"
          "                            Combines with --chain-gap (a chain start stays free), --posteriors and --segments; no\n"
          "                            file changes its format\n"
          "  --genetic-map FILE        with --switch-scale: distances in centimorgans.  FILE: a header line, then lines of\n"
          "                            position, rate in cM/Mb (not read) and cumulative cM, positions strictly increasing;\n"
          "                            linear between two entries, the map's mean rate outside it\n"
          "  --sample-paths K          with --log-stats --states: also K (1 .. 65536) whole paths per individual drawn from the\n"
          "                            distribution over all paths that --posteriors sums (forward filtering, backward\n"
          "                            sampling), for what its per-window probabilities cannot say -- how sure a segment is,\n"
          "                            the range of the IBD1 base pairs, one long segment or five short ones:\n"
          "                            <out>/<pileup-name>.<individual>.logsamples.txt, per draw the windows, segments, base\n"
          "                            pairs and longest base pairs per state; and <out>/<pileup-name>.logibdsamples.txt, per\n"
          "                            individual and state the mean and the 2.5 %, 50 % and 97.5 % order statistics of the\n"
          "                            draws' windows, segments and base pairs and the share of draws with any IBD1 or IBD2\n"
          "                            segment, then the same of the draws' sums over the individuals.  A draw depends on\n"
          "                            --seed, the individual's place in the panel and its number, not on devices or batches.\n"
          "                            With --stats-only only the second file, on one device drawn there\n"
          "  --switches                with --log-stats --states: also, for every step from one window to the next, the\n"
          "                            probability given all windows that the state switches there, under the weights that\n"
          "                            --posteriors sums: <out>/<pileup-name>.<individual>.logswitches.txt, per window the\n"
          "                            probabilities of a 0<->1, 0<->2 and 1<->2 switch into it and their sum; and\n"
          "                            <out>/<pileup-name>.logibdswitches.txt, per individual the expected number of switches\n"
          "                            that pay each penalty, their totals, the same expectation under the penalties alone\n"
          "                            (# Prior), the steps counted, the penalties used and the penalties one multiplicative\n"
          "                            step p * total / (individuals * prior) suggests (# Next): running again with these\n"
          "                            repeats the step.  With --stats-only only the second file, on one device made there\n"
          "  --fit-penalties N         with --log-stats --states (not with -v or -D): keep the log2 window table of every\n"
          "                            comparison individual of the pileup's run and, after the last, repeat the step of\n"
          "                            --switches over all of them, starting from --p01, --p02, --p12: at most N times (1 ..\n"
          "                            1000), ending behind the first step that moves no penalty by more than 2^-16 bit (the\n"
          "                            resolution the penalties are read at).  <out>/<pileup-name>.logibdfit.txt has a row per\n"
          "                            iteration (the penalties used, the expected switches' totals, the prior, the steps\n"
          "                            counted, total / (individuals * prior)), then # Individuals, # Iterations with `stood`\n"
          "                            or `limit`, and # Fitted with 17 digits.  Every other file is made with the penalties\n"
          "                            given.  One device keeps the tables there (24 bytes per window and individual); several\n"
          "                            devices, or none, keep them on the host and iterate on --threads threads\n"
          "  --seed N                  with --sample-paths: the seed of the draws, 0 .. 2^64 - 1 (default 1)\n"
          "  --p01, --p02, --p12 FLOAT with --states: penalties for switching between IBD0 and IBD1, IBD0 and IBD2,\n"
          "                            IBD1 and IBD2 (defaults 1e-3, 1e-6, 1e-3, as hiddengem's)\n"
          "  --stats-only              with --arm-stats and/or --states: write the armstats / ibdstates file only (no\n"
          "                            *.tab.txt, no *.summary.txt, no *.hiddengem.txt; with --arm-stats alone the window\n"
          "                            tables stay on the device)\n"
          "  --reference-order         --LD: sum over the background panel serially in the reference's order\n"
          "                            (LIBD0/LIBD1 bit-identical to the reference; ~12x slower than the default,\n"
          "                            whose values agree to ~1e-15)\n"
          "  --plan                    print the filtered rows and windows only (no device needed)\n"
          "  -h/--help\n\n"
          "Outputs <out>/<pileup-name>.<individual>.tab.txt with columns\n"
          "CHR rsID POS REF ALT AF DP SQ_NREF SQ_NALT GT_A0 GT_A1 LIBD0 LIBD1 LIBD2\n"
          "and <out>/<pileup-name>.<individual>.summary.txt with columns\n"
          "SEGMENT START END LIBD0 LIBD1 LIBD2 NUM_SITES\n",
          stderr);
    exit(code);
}

/* ---- panel individuals -------------------------------------------------------------- */
typedef struct {
    char **names;
    size_t n;
} names_t;

static void chomp1(char *s)
{
    size_t n = strlen(s);
    if (n)
        s[n - 1] = '\0';               /* the reference drops the last character (the newline) */
}

static int read_names(const char *fn, names_t *out)
{
    line_src *ls = ls_open(fn);
    if (!ls)
        return 1;
    char *line;
    size_t cap = 0;
    out->n = 0;
    out->names = NULL;
    while ((line = ls_next(ls, NULL))) {
        chomp1(line);
        if (out->n == cap) {
            cap = cap ? cap * 2 : 256;
            out->names = ls_xrealloc(out->names, cap * sizeof *out->names);
        }
        out->names[out->n++] = strdup(line);
    }
    ls_close(ls);
    return 0;
}

static long find_name(const names_t *ids, const char *name)
{
    for (size_t i = 0; i < ids->n; ++i)
        if (strcmp(ids->names[i], name) == 0)
            return (long)i;
    return -1;
}

/* a list of panel individuals (by index) in list order, unknown names reported and dropped
 * (read_sf / read_rf, reference src/ibd-parse.c:176-219, :262-308) */
typedef struct {
    uint32_t *idx;
    size_t n;
} idlist_t;

static int read_idlist_file(const char *fn, const names_t *ids, const char *what_missing, const char *err_fn,
                            idlist_t *out)
{
    names_t l;
    if (read_names(fn, &l))
        return 1;
    out->idx = malloc((l.n ? l.n : 1) * sizeof *out->idx);
    out->n = 0;
    for (size_t i = 0; i < l.n; ++i) {
        long k = find_name(ids, l.names[i]);
        if (k < 0) {
            fprintf(stderr, what_missing, l.names[i]);
            continue;
        }
        out->idx[out->n++] = (uint32_t)k;
    }
    for (size_t i = 0; i < l.n; ++i)
        free(l.names[i]);
    free(l.names);
    if (out->n == 0) {
        fprintf(stderr, "[::] ERROR in %s(): No matching samples found in %s.\n", err_fn, fn);
        return 1;
    }
    return 0;
}

static int read_idlist_csv(const char *csv, const names_t *ids, idlist_t *out)
{
    char *buf = strdup(csv);
    out->idx = malloc((strlen(csv) / 2 + 2) * sizeof *out->idx);
    out->n = 0;
    /* strtok_r: the device contexts start on a thread of their own while this runs, and the runtime's start-up splits
     * strings with strtok too -- the two shared its hidden state, and every now and then the list ended early in one of
     * the runtime's strings ("Sample 00000000 not found ...", fewer comparisons than asked for, exit code 0) */
    char *save = NULL;
    for (char *tok = strtok_r(buf, ",", &save); tok; tok = strtok_r(NULL, ",", &save)) {
        long k = find_name(ids, tok);
        if (k < 0) {
            fprintf(stderr, "Sample %s not found in reference panel.\n", tok);
            continue;
        }
        out->idx[out->n++] = (uint32_t)k;
    }
    free(buf);
    if (out->n == 0) {
        fprintf(stderr, "[::] ERROR in read_scmd(): No matching samples found.\n");
        return 1;
    }
    return 0;
}

/* ---- -A and -p tables (reference src/ibd-parse.c:311-421) --------------------------- */
typedef struct {
    unsigned long pos;
    double f;
} af_rec;

static af_rec *af_tab;
static size_t af_n;
static unsigned long *pos_tab;
static size_t pos_n;

static int read_af_file(const char *fn, const char *chr)
{
    line_src *ls = ls_open(fn);
    if (!ls)
        return 1;
    size_t cap = 0;
    char *line, c[129];
    while ((line = ls_next(ls, NULL))) {
        af_rec r;
        if (sscanf(line, "%128s %lu %lf", c, &r.pos, &r.f) != 3)
            continue;
        if (chr && strcmp(c, chr) != 0)
            continue;
        if (af_n == cap) {
            cap = cap ? cap * 2 : 4096;
            af_tab = ls_xrealloc(af_tab, cap * sizeof *af_tab);
        }
        af_tab[af_n++] = r;
    }
    ls_close(ls);
    if (af_n == 0) {
        fprintf(stderr, "[::] ERROR in read_af(): Cannot parse lines from %s.\n", fn);
        return 1;
    }
    return 0;
}

static const af_rec *find_af(unsigned long pos)      /* bsearch over the (sorted) table */
{
    size_t lo = 0, hi = af_n;
    while (lo < hi) {
        size_t mid = lo + (hi - lo) / 2;
        if (af_tab[mid].pos == pos)
            return &af_tab[mid];
        if (af_tab[mid].pos < pos)
            lo = mid + 1;
        else
            hi = mid;
    }
    return NULL;
}

static int read_pos_file(const char *fn, const char *chr)
{
    line_src *ls = ls_open(fn);
    if (!ls)
        return 1;
    size_t cap = 0;
    char *line, c[129];
    while ((line = ls_next(ls, NULL))) {
        unsigned long p;
        /* BED (chr start end -> end) or chr pos */
        if (!(sscanf(line, "%128s %*d %lu", c, &p) == 2 || sscanf(line, "%128s %lu", c, &p) == 2))
            continue;
        if (chr && strcmp(c, chr) != 0)
            continue;
        if (pos_n == cap) {
            cap = cap ? cap * 2 : 4096;
            pos_tab = ls_xrealloc(pos_tab, cap * sizeof *pos_tab);
        }
        pos_tab[pos_n++] = p;
    }
    ls_close(ls);
    if (pos_n == 0) {
        fprintf(stderr, "[::] ERROR in read_pos(): Cannot parse lines from %s.\n", fn);
        return 1;
    }
    return 0;
}

static int cmp_ul(const void *a, const void *b)
{
    unsigned long x = *(const unsigned long *)a, y = *(const unsigned long *)b;
    return x < y ? -1 : x > y;
}

static int pos_listed(unsigned long pos)             /* membership (the reference scans linearly) */
{
    return bsearch(&pos, pos_tab, pos_n, sizeof *pos_tab, cmp_ul) != NULL;
}

/* ---- genotype rows -------------------------------------------------------------------- */
typedef struct {
    uint32_t id_off, ref_off, alt_off;   /* into the string arena */
    unsigned long pos;
    uint8_t legend_ok;                   /* the legend row had its 4 fields (src/ibdgem.c:589) */
    uint8_t hap_ok;                      /* the .hap row packed cleanly / the VCF row parsed, is biallelic, GTs ok */
    uint8_t gt_failed;                   /* VCF: a genotype field did not look like [01][/|][01] (message per run) */
    double qual;                         /* VCF QUAL column (-q) */
} row_t;

static row_t *rows;
static size_t n_rows;
static char *arena;
static size_t arena_len, arena_cap;
static uint64_t *packed;                /* the packed rows in host memory -- or, with a panel cache, NULL until something on the host
                                         * asks for a row (packed_rows): the engine takes the rows from the cache FILE */
static int packed_fd = -1;              /* the open panel cache and where its rows start */
static uint64_t packed_off;
static size_t packed_mapped_bytes;      /* > 0: `packed` is a mapping of the panel cache file of that many bytes */
static size_t packed_file_bytes;
static pthread_once_t packed_once = PTHREAD_ONCE_INIT;

static void packed_map(void)
{
    packed = ingest_cache_map(packed_fd, packed_off, packed_file_bytes);
    if (!packed) {
        fprintf(stderr, "[::] ERROR: cannot map the panel cache.\n");
        _exit(1);
    }
    packed_mapped_bytes = packed_file_bytes;
}

/* the packed rows for the few things the host itself reads them for (a row's alleles of the comparison individual in the
 * per-site table, -v, a run without a device): with a panel cache the file is mapped at the first such call.  Several
 * threads get here at once (formatters, shard and output threads, the contexts of a --pileup-list): with a cache, every
 * call goes through pthread_once, whose return orders the mapping's store before this load (`packed` is never read
 * unsynchronised while another thread may write it). */
static inline const uint64_t *packed_rows(void)
{
    if (packed_fd >= 0)
        pthread_once(&packed_once, packed_map);
    return packed;
}
static size_t row_words;
static uint32_t *alt_count_h;            /* alt alleles per panel row, counted on the host (ingest.c) or read from the cache */

static uint32_t arena_add(const char *s)
{
    size_t l = strlen(s) + 1;
    if (arena_len + l > arena_cap) {
        arena_cap = arena_cap ? arena_cap * 2 : (1 << 20);
        while (arena_len + l > arena_cap)
            arena_cap *= 2;
        arena = ls_xrealloc(arena, arena_cap);
    }
    memcpy(arena + arena_len, s, l);
    arena_len += l;
    return (uint32_t)(arena_len - l);
}

/* The legend rows (small text) are parsed on a thread of their own while the team of ingest.c
 * packs the .hap rows; both files advance together in the reference (src/ibdgem.c:573-578), so the
 * panel has as many rows as the shorter of the two. */
typedef struct {
    const char *fn;
    size_t n;
    int rc;
    int threads;
} legend_job;

/* one legend line into a row and a string arena (src/ibdgem.c:589) */
typedef struct {
    row_t *rows;
    size_t n, cap;
    char *arena;
    size_t arena_len, arena_cap;
} legend_part;

static uint32_t part_arena_add(legend_part *t, const char *s)
{
    const size_t l = strlen(s) + 1;
    if (t->arena_len + l > t->arena_cap) {
        t->arena_cap = t->arena_cap ? t->arena_cap * 2 : (1 << 20);
        while (t->arena_len + l > t->arena_cap)
            t->arena_cap *= 2;
        t->arena = ls_xrealloc(t->arena, t->arena_cap);
    }
    memcpy(t->arena + t->arena_len, s, l);
    t->arena_len += l;
    return (uint32_t)(t->arena_len - l);
}

static void part_add_legend_line(legend_part *t, const char *l)
{
    if (t->n == t->cap) {
        t->cap = t->cap ? t->cap * 2 : (1 << 16);
        t->rows = ls_xrealloc(t->rows, t->cap * sizeof *t->rows);
    }
    row_t *r = &t->rows[t->n++];
    memset(r, 0, sizeof *r);
    char id[129], ref[129], alt[129];
    if (sscanf(l, "%128s %lu %128s %128s", id, &r->pos, ref, alt) == 4) {
        r->legend_ok = 1;
        r->id_off = part_arena_add(t, id);
        r->ref_off = part_arena_add(t, ref);
        r->alt_off = part_arena_add(t, alt);
    }
}

/* A large plain legend is cut into byte ranges at line starts, one thread each.  Pass 1 counts the
 * lines of every range, so pass 2 can write its rows straight into their final places; the strings go
 * to an arena per thread, and once all sizes are known every thread copies its arena into the common
 * one and shifts the offsets of its own rows.  Small or gzip files go line by line. */
typedef struct {
    const char *base;
    size_t a, b;
    size_t lines;               /* pass 1 */
    size_t first;               /* pass 2: index of the range's first row */
    legend_part part;           /* .rows unused here: rows are written in place */
    size_t arena_base;          /* pass 3 */
} legend_range;

static void *legend_count(void *arg)
{
    legend_range *j = arg;
    size_t n = 0;
    for (const char *p = j->base + j->a, *e = j->base + j->b; p < e;) {
        const char *nl = memchr(p, '\n', (size_t)(e - p));
        ++n;
        if (!nl)
            break;
        p = nl + 1;
    }
    j->lines = n;
    return NULL;
}

static void *legend_parse(void *arg)
{
    legend_range *j = arg;
    char *buf = NULL;
    size_t cap = 0, n = j->first;
    for (size_t p = j->a; p < j->b;) {
        const char *nl = memchr(j->base + p, '\n', j->b - p);
        const size_t len = nl ? (size_t)(nl - (j->base + p)) + 1 : j->b - p;
        if (len + 1 > cap) {
            cap = (len + 1) * 2;
            buf = ls_xrealloc(buf, cap);
        }
        memcpy(buf, j->base + p, len);
        buf[len] = 0;
        row_t *r = &rows[n++];
        memset(r, 0, sizeof *r);
        char id[129], ref[129], alt[129];
        if (sscanf(buf, "%128s %lu %128s %128s", id, &r->pos, ref, alt) == 4) {
            r->legend_ok = 1;
            r->id_off = part_arena_add(&j->part, id);
            r->ref_off = part_arena_add(&j->part, ref);
            r->alt_off = part_arena_add(&j->part, alt);
        }
        p += len;
    }
    free(buf);
    return NULL;
}

static void *legend_place(void *arg)
{
    legend_range *j = arg;
    if (j->part.arena_len)
        memcpy(arena + j->arena_base, j->part.arena, j->part.arena_len);
    free(j->part.arena);
    const uint32_t shift = (uint32_t)j->arena_base;
    for (size_t i = j->first; i < j->first + j->lines; ++i)
        if (rows[i].legend_ok) {
            rows[i].id_off += shift;
            rows[i].ref_off += shift;
            rows[i].alt_off += shift;
        }
    return NULL;
}

static void team_run(void *(*fn)(void *), legend_range *rg, int T)
{
    pthread_t th[64];
    for (int t = 0; t < T; ++t)
        if (pthread_create(&th[t], NULL, fn, &rg[t]) != 0) {
            fn(&rg[t]);
            th[t] = pthread_self();
        }
    for (int t = 0; t < T; ++t)
        if (!pthread_equal(th[t], pthread_self()))
            pthread_join(th[t], NULL);
}

static void *read_legend(void *arg)
{
    legend_job *j = arg;
    size_t size = 0;
    const char *base = j->threads > 1 ? ls_map(j->fn, &size) : NULL;
    if (base && size >= ls_mt_min_bytes()) {
        const char *nl = memchr(base, '\n', size);              /* legend header (src/ibdgem.c:555) */
        const size_t from = nl ? (size_t)(nl - base) + 1 : size;
        const int T = j->threads > 64 ? 64 : j->threads;
        size_t cut[65];
        legend_range rg[64];
        ls_split_lines(base, size, from, T, cut);
        for (int t = 0; t < T; ++t) {
            memset(&rg[t], 0, sizeof rg[t]);
            rg[t].base = base;
            rg[t].a = cut[t];
            rg[t].b = cut[t + 1];
        }
        team_run(legend_count, rg, T);
        size_t total = 0;
        for (int t = 0; t < T; ++t) {
            rg[t].first = total;
            total += rg[t].lines;
        }
        rows = ls_xrealloc(rows, (total ? total : 1) * sizeof *rows);
        team_run(legend_parse, rg, T);
        size_t atotal = arena_len;
        for (int t = 0; t < T; ++t) {
            rg[t].arena_base = atotal;
            atotal += rg[t].part.arena_len;
        }
        if (atotal > arena_cap) {
            arena_cap = atotal;
            arena = ls_xrealloc(arena, arena_cap);
        }
        arena_len = atotal;
        team_run(legend_place, rg, T);
        ls_unmap(base, size);
        j->n = total;
        return NULL;
    }
    ls_unmap(base, size);
    line_src *leg = ls_open(j->fn);
    if (!leg) {
        j->rc = 1;
        return NULL;
    }
    legend_part t;
    memset(&t, 0, sizeof t);
    t.arena = arena;
    t.arena_len = arena_len;
    t.arena_cap = arena_cap;
    ls_next(leg, NULL);                                   /* legend header (src/ibdgem.c:555) */
    for (;;) {
        char *l = ls_next(leg, NULL);
        if (!l)
            break;
        part_add_legend_line(&t, l);
    }
    ls_close(leg);
    rows = t.rows;
    arena = t.arena;
    arena_len = t.arena_len;
    arena_cap = t.arena_cap;
    j->n = t.n;
    return NULL;
}

static int default_threads(void)
{
    cpu_set_t set;
    int n = 1;
    if (sched_getaffinity(0, sizeof set, &set) == 0)
        n = CPU_COUNT(&set);
    return n < 1 ? 1 : n > 16 ? 16 : n;
}

static int read_genotypes(const char *hap_fn, const char *legend_fn, unsigned n_ids)
{
    row_words = ibdg_row_words(n_ids);
    /* the .hap team and the legend team share the threads: the legend is ~1/400 of the text, but its rows
     * cost a sscanf each; with the packed-panel cache the legend is all there is to parse */
    legend_job lj = {legend_fn, 0, 0, opt_threads > 0 ? opt_threads : default_threads()};
    pthread_t lt;
    const int threaded = pthread_create(&lt, NULL, read_legend, &lj) == 0;
    if (!threaded)
        read_legend(&lj);
    uint8_t *ok = NULL;
    size_t n_hap = 0;
    int rc = 1;
    if (cache_fn)
        rc = ingest_cache_open(cache_fn, hap_fn, n_ids, &packed_fd, &packed_off, &ok, &alt_count_h, &n_hap);
    if (!rc) {
        packed_file_bytes = n_hap * (size_t)row_words * 8;
        if (getenv("IBDGEM_CACHE_MAP"))         /* measurement only: the rows as a mapping from the start, as until round 4 */
            (void)packed_rows();
    }
    if (rc) {
        packed_fd = -1;
        const int team = opt_threads > 0 ? opt_threads : default_threads();
        rc = ingest_hap(hap_fn, n_ids, team, &packed, &ok, &n_hap);
        if (!rc) {
            alt_count_h = malloc((n_hap ? n_hap : 1) * sizeof *alt_count_h);
            if (!alt_count_h)
                rc = 1;
            else
                ingest_alt_counts(packed, n_hap, n_ids, team, alt_count_h);
        }
        if (!rc && cache_fn && ingest_cache_store(cache_fn, hap_fn, n_ids, packed, ok, alt_count_h, n_hap))
            fprintf(stderr, "Could not write the panel cache %s (continuing without it).\n", cache_fn);
    }
    if (threaded)
        pthread_join(lt, NULL);
    if (rc || lj.rc) {
        fprintf(stderr, "[::] ERROR parsing hap/legend/indv data; make sure inputs are valid.\n");
        return 1;
    }
    n_rows = n_hap < lj.n ? n_hap : lj.n;
    for (size_t r = 0; r < n_rows; ++r)
        rows[r].hap_ok = ok[r];
    free(ok);
    if (dump_panel_fn) {
        FILE *f = fopen(dump_panel_fn, "wb");
        if (!f)
            return 1;
        for (size_t r = 0; r < n_rows; ++r)
            fputc(rows[r].hap_ok, f);
        fwrite(packed_rows(), 8, n_rows * row_words, f);
        fclose(f);
    }
    return 0;
}

/* VCF rows -> the same row table (restates the parsing of compare_vcf, reference
 * src/ibdgem.c:272-296, src/ibd-parse.c:113-173): sample names from the #CHROM line; per row the
 * eight fixed columns, FORMAT, then one field per sample whose first three characters must be
 * [01][/|][01].  Rows that do not split into the fixed columns, multi-allelic rows (comma in ALT)
 * and rows with an unparsable genotype are "skipped" rows. */
static int read_genotypes_vcf(const char *vcf_fn, names_t *ids)
{
    line_src *vcf = ls_open(vcf_fn);
    if (!vcf)
        return 1;
    char *line;
    while ((line = ls_next(vcf, NULL)) && strncmp(line, "##", 2) == 0)
        ;
    static const char hdr[] = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t";
    if (!line || strncmp(line, hdr, sizeof hdr - 1) != 0) {
        fprintf(stderr, "[::] ERROR parsing VCF header.\n");
        return 1;
    }
    {
        char *p = line + sizeof hdr - 1;
        p[strcspn(p, "\n")] = 0;
        size_t cap = 0;
        ids->n = 0;
        ids->names = NULL;
        char *save = NULL;
        for (char *tok = strtok_r(p, "\t", &save); tok; tok = strtok_r(NULL, "\t", &save)) {
            if (ids->n == cap) {
                cap = cap ? cap * 2 : 256;
                ids->names = ls_xrealloc(ids->names, cap * sizeof *ids->names);
            }
            ids->names[ids->n++] = strdup(tok);
        }
        if (ids->n == 0) {
            fprintf(stderr, "[::] ERROR: No samples found.\n");
            return 1;
        }
    }
    const unsigned n_ids = (unsigned)ids->n;
    row_words = ibdg_row_words(n_ids);
    uint8_t *alle = malloc(2 * (size_t)n_ids);
    size_t cap = 0;
    while ((line = ls_next(vcf, NULL))) {
        if (n_rows == cap) {
            cap = cap ? cap * 2 : (1 << 16);
            rows = ls_xrealloc(rows, cap * sizeof *rows);
            packed = ls_xrealloc(packed, cap * row_words * 8);
        }
        row_t *r = &rows[n_rows];
        memset(r, 0, sizeof *r);
        memset(packed + n_rows * row_words, 0, row_words * 8);
        n_rows++;
        line[strcspn(line, "\n")] = 0;
        char *f[9], *p = line;
        int nf = 0;
        while (nf < 9) {                                  /* CHROM POS ID REF ALT QUAL FILTER INFO FORMAT */
            char *t = strchr(p, '\t');
            if (!t)
                break;
            *t = 0;
            f[nf++] = p;
            p = t + 1;
        }
        char *endp;
        r->pos = strtoul(nf > 1 ? f[1] : "", &endp, 10);
        if (nf < 9 || endp == f[1] || !*p)
            continue;                                     /* the reference's sscanf != 8 branch */
        r->legend_ok = 1;
        r->id_off = arena_add(f[2]);
        r->ref_off = arena_add(f[3]);
        r->alt_off = arena_add(f[4]);
        r->qual = atof(f[5]);
        if (strchr(f[4], ','))
            continue;                                     /* not biallelic (src/ibdgem.c:275) */
        unsigned i = 0;
        for (char *tok = p; i < n_ids && tok; ++i) {
            char *t = strchr(tok, '\t');
            if (t)
                *t = 0;
            if (!((tok[0] == '0' || tok[0] == '1') && (tok[1] == '/' || tok[1] == '|') && (tok[2] == '0' || tok[2] == '1')))
                break;
            alle[2 * i] = (uint8_t)(tok[0] - '0');
            alle[2 * i + 1] = (uint8_t)(tok[2] - '0');
            tok = t ? t + 1 : NULL;
        }
        if (i < n_ids) {
            r->gt_failed = 1;
            continue;
        }
        ibdg_pack_alleles(alle, n_ids, packed + (n_rows - 1) * row_words);
        r->hap_ok = 1;
    }
    free(alle);
    ls_close(vcf);
    alt_count_h = malloc((n_rows ? n_rows : 1) * sizeof *alt_count_h);
    if (!alt_count_h)
        return 1;
    ingest_alt_counts(packed, n_rows, n_ids, 1, alt_count_h);
    return 0;
}

static int is_snp(const char *ref, const char *alt)   /* one of A C G T each (src/ibdgem.c:113-119) */
{
    return ref[0] && !ref[1] && strchr("ACGT", ref[0]) && alt[0] && !alt[1] && strchr("ACGT", alt[0]);
}

static inline unsigned row_allele(size_t r, unsigned indiv, unsigned hap)
{
    return (unsigned)(packed_rows()[r * row_words + 2 * (indiv >> 6) + hap] >> (indiv & 63)) & 1u;
}

/* The reference thins reads with libc rand(), never seeded (src/ibdgem.c:132), so its output
 * depends on glibc's default stream: the TYPE_3 additive-feedback generator of random_r.c
 * (r[i] = r[i-3] + r[i-31], state seeded from 1 with the Lehmer step 16807 mod 2^31-1, first
 * 310 values discarded, result = r >> 1).  The stream is restated here instead of calling
 * rand(): the HIP runtime inside this process draws from libc's global generator too, which
 * would shift the sequence.  tests/test_host_cli.py checks it against libc. */
static __thread uint32_t grand_state[34];     /* per thread: each pileup of a --pileup-list starts the stream afresh, */
static __thread int grand_f = 3, grand_r = 0, grand_ready = 0;   /* as a process of its own would (grand_seed(1)) */

static void grand_seed(uint32_t seed)
{
    int32_t w = (int32_t)(seed ? seed : 1);
    grand_state[0] = (uint32_t)w;
    for (int i = 1; i < 31; ++i) {
        const long hi = w / 127773, lo = w % 127773;
        w = (int32_t)(16807 * lo - 2836 * hi);
        if (w < 0)
            w += 2147483647;
        grand_state[i] = (uint32_t)w;
    }
    grand_f = 3;
    grand_r = 0;
    grand_ready = 1;
    for (int i = 0; i < 310; ++i) {
        grand_state[grand_f] += grand_state[grand_r];
        grand_f = (grand_f + 1) % 31;
        grand_r = (grand_r + 1) % 31;
    }
}

static int glibc_rand(void)
{
    if (!grand_ready)
        grand_seed(1);
    const uint32_t v = grand_state[grand_f] += grand_state[grand_r];
    grand_f = (grand_f + 1) % 31;
    grand_r = (grand_r + 1) % 31;
    return (int)(v >> 1);
}

/* cull_dp, reference src/ibdgem.c:126-137 */
static unsigned cull(unsigned count, double cull_p)
{
    if (cull_p == 1.0)
        return count;
    unsigned kept = 0;
    for (unsigned i = 0; i < count; ++i)
        if ((glibc_rand() / (double)2147483647) < cull_p)
            kept++;
    return kept;
}

/* ---- per-site rows of the tab file, formatted by a team of threads ---------------------------
 * The reference prints one fprintf per row (src/ibdgem.c:731-733): 4M rows x 14 columns per
 * comparison individual.  Here the rows are cut into contiguous ranges, every thread formats its
 * range into a buffer of its own with the same conversions (%lf, %e, %u, %lu through snprintf, so
 * the text is what printf would have written), and the buffers are written in order. */
/* ---- the reference's conversions without going through printf --------------------------------
 * 4M rows x (three %e + one %lf + six integers) per comparison individual is where a table-writing run
 * spends its host time.  These produce the very characters printf produces -- printf rounds the exact
 * binary value to nearest, ties to even -- and hand the rare case they cannot decide to sprintf:
 *   %lf of 0 <= f < 2^40: f * 10^6 exactly in 128-bit integer arithmetic (a double is m * 2^e);
 *   %e: a * 10^(6-E) as a 64 x 64 -> 128-bit integer product with a table of powers of ten (64-bit mantissas,
 *       made in long double); when the result lies within 1e-6 of a rounding boundary or 1e-5 of a power of
 *       ten, sprintf decides.  (Until round 3 the product was taken in long double itself: 62 ns per number
 *       in x87 code against 20 now -- frexp, floor and the control-word dance of the conversion were the time.)
 * `ibdgem --fmt-check N` compares them with sprintf on N random doubles (tests/test_host_cli.py). */
/* put_e6's table of powers of ten is made in long double and split into 64-bit mantissas */
_Static_assert(LDBL_MANT_DIG >= 64, "put_e6 needs a long double with a 64-bit mantissa (x86-64); elsewhere use sprintf");
static long double pow10_tab[700];           /* 10^(i-350) */
static uint64_t p10_m[700];                  /* the same as integers: pow10_tab[i] = p10_m[i] * 2^p10_e[i], top bit of p10_m set */
static int16_t p10_e[700];
static void fmt_init(void)
{
    static int done;
    if (done)
        return;
    pow10_tab[350] = 1.0L;
    for (int i = 1; i <= 349; ++i) {
        pow10_tab[350 + i] = pow10_tab[350 + i - 1] * 10.0L;      /* exact up to 10^27, 1 rounding per step after */
        pow10_tab[350 - i] = 1.0L / pow10_tab[350 + i];
    }
    for (int i = 1; i < 700; ++i) {
        int e;
        const long double m = frexpl(pow10_tab[i], &e);           /* [0.5, 1) */
        p10_m[i] = (uint64_t)ldexpl(m, 64);                       /* exact: the mantissa has 64 bits */
        p10_e[i] = (int16_t)(e - 64);
    }
    done = 1;
}

static char *put_str(char *d, const char *s)
{
    const size_t n = strlen(s);
    memcpy(d, s, n);
    return d + n;
}

static char *put_u64(char *d, unsigned long v)
{
    char t[24];
    int n = 0;
    do {
        t[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n)
        *d++ = t[--n];
    return d;
}

/* "%lf" (six decimals) */
static char *put_lf6(char *d, double f)
{
    if (!(f >= 0.0) || f >= 1099511627776.0 || (f == 0.0 && signbit(f)))
        return d + sprintf(d, "%lf", f);
    uint64_t bits;
    memcpy(&bits, &f, 8);
    const unsigned ex = (unsigned)(bits >> 52);            /* sign bit is clear */
    const int sh = 1075 - (int)ex;                         /* f = mi * 2^-sh exactly; f < 2^40 -> sh >= 13 */
    uint64_t q = 0;
    if (ex != 0 && sh < 127) {                             /* zero, subnormals and everything below 2^-54 * 10^6 round to 0 */
        const uint64_t mi = (bits & (((uint64_t)1 << 52) - 1)) | ((uint64_t)1 << 52);
        const unsigned __int128 p = (unsigned __int128)mi * 1000000u;   /* f * 10^6 = p / 2^sh; p < 2^73 */
        const unsigned __int128 q128 = p >> sh;            /* < 2^60 */
        const unsigned __int128 rem = p - (q128 << sh), half = (unsigned __int128)1 << (sh - 1);
        q = (uint64_t)q128;
        if (rem > half || (rem == half && (q & 1)))
            q += 1;
    }
    const unsigned long whole = (unsigned long)(q / 1000000u);
    unsigned long frac = (unsigned long)(q % 1000000u);
    d = put_u64(d, whole);
    *d++ = '.';
    for (int k = 5; k >= 0; --k) {
        d[k] = (char)('0' + frac % 10);
        frac /= 10;
    }
    return d + 6;
}

/* "%e" (six decimals, exponent of at least two digits).  v = mv * 2^ev with a 64-bit mv; q = v * 10^(6-E) as the
 * 128-bit product of mv and the table's 64-bit mantissa: its integer part is the seven digits, the next 64 bits
 * the fraction that decides the rounding.  The table entry is within 2^-56 of the power of ten (a rounding per
 * step of fmt_init), so q is off by less than 1e7 * 2^-56 < 2e-10: a fraction within 1e-6 of one half, or a q
 * within 1e-5 of a power of ten, goes to sprintf -- except for 1e-21 <= v < 1e7, where the power of ten is exact
 * and so is the product (most likelihoods; and exactly the values the guard band would catch most often: 1.0,
 * 0.5, 0.25 of rows without reads were 37 % of a table's numbers and all went to sprintf). */
static char *put_e6(char *d, double v)
{
    if (!isfinite(v))
        return d + sprintf(d, "%e", v);
    uint64_t bits;
    memcpy(&bits, &v, 8);
    if (bits >> 63) {
        *d++ = '-';
        bits &= ~((uint64_t)1 << 63);
        v = -v;
    }
    if (bits == 0) {
        memcpy(d, "0.000000e+00", 12);
        return d + 12;
    }
    const int ex = (int)(bits >> 52);
    if (ex == 0)                                           /* subnormal: printf's business */
        return d + sprintf(d, "%e", v);
    const uint64_t mv = ((bits & (((uint64_t)1 << 52) - 1)) | ((uint64_t)1 << 52)) << 11;
    const int ev = ex - 1075 - 11;
    const int b2 = ex - 1023;                              /* 2^b2 <= v < 2^(b2+1) */
    int E = (b2 * 78913) / 262144 - (b2 < 0);              /* floor(b2 * log10 2) or one off: settled below */
    uint64_t I = 0;
    unsigned __int128 prod = 0;
    int s = 0, settled = 0;
    for (int tries = 0; tries < 3 && !settled; ++tries) {
        const int k = 350 + 6 - E;
        if (k < 1 || k > 699)
            return d + sprintf(d, "%e", v);
        prod = (unsigned __int128)mv * p10_m[k];           /* q = prod * 2^-s */
        s = -(ev + p10_e[k]);
        if (s < 65 || s > 126)
            return d + sprintf(d, "%e", v);
        I = (uint64_t)(prod >> s);
        if (I >= 10000000u)
            ++E;
        else if (I < 1000000u)
            --E;
        else
            settled = 1;
    }
    if (!settled)
        return d + sprintf(d, "%e", v);
    unsigned long D;
    if (E <= 6 && E >= 6 - 27) {
        /* 10^0 .. 10^27 are exact in the table, so prod is q itself: round to nearest, ties to even, on all its bits
         * (1.0, 0.5, 0.25 -- rows without reads -- are exactly such ties or exact values) */
        const unsigned __int128 rem = prod & (((unsigned __int128)1 << s) - 1), half = (unsigned __int128)1 << (s - 1);
        D = I + ((rem > half || (rem == half && (I & 1))) ? 1u : 0u);
    } else {
        const uint64_t fr = (uint64_t)((prod << (128 - s)) >> 64);            /* the fraction, 0.64 fixed point */
        const uint64_t tol5 = 184467440737096ull, tol6 = 18446744073710ull, half = (uint64_t)1 << 63;   /* 1e-5, 1e-6 * 2^64 */
        if ((I == 1000000u && fr < tol5) || (I == 9999999u && fr > ~tol5))
            return d + sprintf(d, "%e", v);
        if (fr > half - tol6 && fr < half + tol6)
            return d + sprintf(d, "%e", v);
        D = I + (fr > half ? 1u : 0u);
    }
    if (D >= 10000000ul) {
        D /= 10;
        ++E;
    }
    char t[8];
    for (int k = 6; k >= 0; --k) {
        t[k] = (char)('0' + D % 10);
        D /= 10;
    }
    *d++ = t[0];
    *d++ = '.';
    memcpy(d, t + 1, 6);
    d += 6;
    *d++ = 'e';
    *d++ = E < 0 ? '-' : '+';
    unsigned a = (unsigned)(E < 0 ? -E : E);
    if (a >= 100) {
        *d++ = (char)('0' + a / 100);
        a %= 100;
    }
    *d++ = (char)('0' + a / 10);
    *d++ = (char)('0' + a % 10);
    return d;
}

static int fmt_ll(char *dst, double v, char sep)
{
    char *d = isnan(v) ? put_str(dst, "-nan") : put_e6(dst, v);        /* "-nan": x86 printf for 0/0 */
    *d++ = sep;
    return (int)(d - dst);
}

/* --fmt-check N: put_e6 / put_lf6 against sprintf on N random doubles (several distributions); prints the
 * number of differences (0 expected) and how many values took the sprintf way out */
static int fmt_check(long n)
{
    fmt_init();
    uint64_t x = 0x9E3779B97F4A7C15ull;
    long bad = 0, shown = 0;
    char a[400], b[400];
    for (long i = 0; i < n; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        double v;
        switch (i % 7) {
        case 0: { uint64_t bits = x; memcpy(&v, &bits, 8); break; }                       /* any bit pattern */
        case 1: v = (double)(x >> 11) / 9007199254740992.0; break;                         /* [0,1) */
        case 2: v = ldexp((double)(x >> 11) / 9007199254740992.0, -(int)(x % 1070)); break; /* likelihood-like */
        case 3: v = (double)(x % 20000001) / 1e7 * pow(10.0, (int)(x >> 40) % 40 - 20); break; /* short decimals */
        case 4: v = (double)(x % 2000001) / 128.0 / 15625.0; break;                         /* %lf ties: k/2^7 scaled */
        case 5: v = ((double)(1000000 + x % 9000000) + 0.5) / (double)(1u << ((x >> 32) % 3)); break; /* %e ties and near-ties */
        default: v = (double)((x >> 20) % 5009) / 5008.0; break;                           /* allele frequencies */
        }
        if (isnan(v))
            continue;
        *put_e6(a, v) = 0;
        sprintf(b, "%e", v);
        int diff = strcmp(a, b) != 0;
        *put_lf6(a, v) = 0;
        sprintf(b, "%lf", v);
        diff |= strcmp(a, b) != 0;
        if (diff) {
            ++bad;
            if (shown++ < 5)
                printf("DIFF %a: %s vs %s\n", v, a, b);
        }
    }
    printf("fmt-check: %ld values, %ld differences\n", n, bad);
    return bad != 0;
}

/* a row that passed the target-independent part of the filter chain */
typedef struct { uint32_t row; uint32_t pu; uint8_t n_ref, n_alt; double f; int f_is_override; } cand_t;
typedef struct {
    /* what a row is made of */
    const cand_t *cand;
    const uint32_t *s_cand;
    const pileup_t *pu;
    const double *site_ll;
    const uint8_t *s_nr, *s_na;
    unsigned tgt;
    int plan;
    /* columns 1-9 of every row as text, when somebody made them once for all comparison individuals (row_prefix_build) */
    const char *pre;
    const uint32_t *pre_off;       /* [n + 1] */
    /* this thread's rows and its text */
    size_t a, b;
    char *buf;
    size_t len, cap;
    int failed;
} fmt_job;

/* columns 1-9 of a row, "%s\t%s\t%lu\t%s\t%s\t%lf\t%u\t%u\t%u\t" (src/ibdgem.c:731-733): none of them depends on the
 * comparison individual */
static char *put_row_prefix(char *d, const pileup_t *pu, const cand_t *c, unsigned nr, unsigned na)
{
    const row_t *R = &rows[c->row];
    const pu_line *pl = &pu->lines[c->pu];
    d = put_str(d, pu->chr_names[pl->chr]); *d++ = '\t';
    d = put_str(d, arena + R->id_off); *d++ = '\t';
    d = put_u64(d, R->pos); *d++ = '\t';
    d = put_str(d, arena + R->ref_off); *d++ = '\t';
    d = put_str(d, arena + R->alt_off); *d++ = '\t';
    d = put_lf6(d, c->f); *d++ = '\t';          /* alt count / (2 N) or the -A value: the division the engine makes too */
    d = put_u64(d, pl->cov); *d++ = '\t';
    d = put_u64(d, nr); *d++ = '\t';
    d = put_u64(d, na); *d++ = '\t';
    return d;
}

static size_t row_prefix_room(const pileup_t *pu, const cand_t *c)
{
    const row_t *R = &rows[c->row];
    /* strings + 3 x %lu/%lf (<= 330 chars for the largest double) + 5 x %u + 3 x %e + separators */
    return strlen(pu->chr_names[pu->lines[c->pu].chr]) + strlen(arena + R->id_off) + strlen(arena + R->ref_off) +
           strlen(arena + R->alt_off) + 512;
}

static void *fmt_rows(void *arg)
{
    fmt_job *j = arg;
    j->failed = 0;
    for (size_t i = j->a; i < j->b; ++i) {
        const cand_t *c = &j->cand[j->s_cand[i]];
        const size_t room = j->pre ? (size_t)(j->pre_off[i + 1] - j->pre_off[i]) + 128 : row_prefix_room(j->pu, c);
        if (j->len + room > j->cap) {
            size_t nc = j->cap ? j->cap * 2 : ((size_t)1 << 20);
            while (j->len + room > nc)
                nc *= 2;
            char *nb = realloc(j->buf, nc);
            if (!nb) {
                j->failed = 1;
                return NULL;
            }
            j->buf = nb;
            j->cap = nc;
        }
        char *d = j->buf + j->len;
        /* "%s\t%s\t%lu\t%s\t%s\t%lf\t%u\t%u\t%u\t%u\t%u" (src/ibdgem.c:731-733) */
        if (j->pre) {
            const size_t len = j->pre_off[i + 1] - j->pre_off[i];
            memcpy(d, j->pre + j->pre_off[i], len);
            d += len;
        } else {
            d = put_row_prefix(d, j->pu, c, j->s_nr[i], j->s_na[i]);
        }
        d = put_u64(d, row_allele(c->row, j->tgt, 0)); *d++ = '\t';
        d = put_u64(d, row_allele(c->row, j->tgt, 1));
        if (j->plan) {
            *d++ = '\n';
        } else {
            *d++ = '\t';
            d += fmt_ll(d, j->site_ll[3 * i], '\t');
            d += fmt_ll(d, j->site_ll[3 * i + 1], '\t');
            d += fmt_ll(d, j->site_ll[3 * i + 2], '\n');
        }
        j->len = (size_t)(d - j->buf);
    }
    return NULL;
}

/* Columns 1-9 of all n rows once, for runs whose comparison individuals share the site list: a team formats contiguous
 * ranges into buffers of their own, which are then joined (offsets per row).  ~50 bytes per row; a table-writing thread
 * then copies a row's prefix instead of converting nine columns again (3 of the 6 conversions of a row that are not %e,
 * and all its string handling). */
typedef struct {
    fmt_job j;                     /* a, b, buf, len, cap as in fmt_rows */
    uint32_t *lens;                /* [n]: shared, every thread writes its own range */
    char *dst;                     /* the joined text (second step) */
    size_t dst_off;
} pre_job;

static void *pre_rows(void *arg)
{
    pre_job *p = arg;
    fmt_job *j = &p->j;
    j->failed = 0;
    for (size_t i = j->a; i < j->b; ++i) {
        const cand_t *c = &j->cand[j->s_cand[i]];
        const size_t room = row_prefix_room(j->pu, c);
        if (j->len + room > j->cap) {
            size_t nc = j->cap ? j->cap * 2 : ((size_t)1 << 20);
            while (j->len + room > nc)
                nc *= 2;
            char *nb = realloc(j->buf, nc);
            if (!nb) {
                j->failed = 1;
                return NULL;
            }
            j->buf = nb;
            j->cap = nc;
        }
        char *d = j->buf + j->len;
        char *e = put_row_prefix(d, j->pu, c, j->s_nr[i], j->s_na[i]);
        p->lens[i] = (uint32_t)(e - d);
        j->len += (size_t)(e - d);
    }
    return NULL;
}

static void *pre_join(void *arg)
{
    pre_job *p = arg;
    memcpy(p->dst + p->dst_off, p->j.buf, p->j.len);
    return NULL;
}

/* 0 on success: *pre_out (malloc'd text) and *off_out (malloc'd, n + 1 offsets); on any failure nothing is kept and the
 * tables are formatted row by row as before */
static int row_prefix_build(fmt_job proto, size_t n, int threads, char **pre_out, uint32_t **off_out)
{
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    pre_job jobs[64];
    pthread_t tid[64];
    int started[64] = {0};
    uint32_t *off = malloc((n + 1) * sizeof *off);
    if (!off)
        return 1;
    for (int t = 0; t < threads; ++t) {
        memset(&jobs[t], 0, sizeof jobs[t]);
        jobs[t].j = proto;
        jobs[t].j.buf = NULL;
        jobs[t].j.cap = jobs[t].j.len = 0;
        jobs[t].j.a = n * (size_t)t / (size_t)threads;
        jobs[t].j.b = n * (size_t)(t + 1) / (size_t)threads;
        jobs[t].lens = off;                                       /* lengths first, offsets after the scan below */
    }
    for (int t = 0; t + 1 < threads; ++t)
        started[t] = pthread_create(&tid[t], NULL, pre_rows, &jobs[t]) == 0;
    for (int t = 0; t < threads; ++t)
        if (!started[t])
            pre_rows(&jobs[t]);
    int bad = 0;
    size_t total = 0;
    for (int t = 0; t < threads; ++t) {
        if (started[t])
            pthread_join(tid[t], NULL);
        bad |= jobs[t].j.failed;
        jobs[t].dst_off = total;
        total += jobs[t].j.len;
    }
    char *pre = !bad && total < 0xffffffffu ? malloc(total ? total : 1) : NULL;
    if (pre) {
        for (int t = 0; t < threads; ++t) {
            jobs[t].dst = pre;
            started[t] = t + 1 < threads && pthread_create(&tid[t], NULL, pre_join, &jobs[t]) == 0;
        }
        for (int t = 0; t < threads; ++t)
            if (!started[t])
                pre_join(&jobs[t]);
        for (int t = 0; t < threads; ++t)
            if (started[t])
                pthread_join(tid[t], NULL);
        uint32_t run = 0;                                         /* lengths -> offsets */
        for (size_t i = 0; i < n; ++i) {
            const uint32_t len = off[i];
            off[i] = run;
            run += len;
        }
        off[n] = run;
    }
    for (int t = 0; t < threads; ++t)
        free(jobs[t].j.buf);
    if (!pre) {
        free(off);
        return 1;
    }
    *pre_out = pre;
    *off_out = off;
    return 0;
}

/* Rounds of 2^18 rows (bounds the text held in memory); the team formats round k+1 into a second set of buffers
 * while this thread writes round k -- a third of the phase was the copy into the page cache with the team idle. */
/* The rows in chunks of 2^14 (1.3 MB of text): a team of threads takes chunk numbers from a counter and formats each into
 * one of a ring of buffers; the calling thread writes the chunks in order as they become ready and hands the buffers back.
 * The team is started once per table and the writer never formats: putting ready text into the file (6 GB/s from one
 * thread, tools/write_floor.c) is the longer of the two jobs once sixteen threads format, so nothing may hold it up.
 * (Until round 3 a team was started per 2^18 rows and the caller wrote one round's text while the next was formatted.) */
typedef struct {
    fmt_job proto;
    size_t n, chunk_rows, n_chunks;
    int ring;                      /* buffers (a chunk uses buffer chunk % ring) */
    fmt_job *slot;                 /* [ring] */
    int *state;                    /* [ring]: 0 free, 1 being formatted, 2 ready */
    size_t next_chunk;             /* the next chunk a formatter takes */
    int failed;
    pthread_mutex_t mu;
    pthread_cond_t cv_ready, cv_free;
} row_pipe;

static void *row_pipe_worker(void *arg)
{
    row_pipe *P = arg;
    for (;;) {
        pthread_mutex_lock(&P->mu);
        size_t c;
        int b;
        for (;;) {
            c = P->next_chunk;
            if (c >= P->n_chunks || P->failed) {
                pthread_mutex_unlock(&P->mu);
                return NULL;
            }
            b = (int)(c % (size_t)P->ring);
            if (P->state[b] == 0)
                break;
            pthread_cond_wait(&P->cv_free, &P->mu);      /* the buffer's previous chunk is not written yet */
        }
        P->next_chunk = c + 1;
        P->state[b] = 1;
        pthread_mutex_unlock(&P->mu);
        fmt_job *j = &P->slot[b];
        j->a = c * P->chunk_rows;
        j->b = j->a + P->chunk_rows < P->n ? j->a + P->chunk_rows : P->n;
        j->len = 0;
        fmt_rows(j);
        pthread_mutex_lock(&P->mu);
        if (j->failed)
            P->failed = 1;
        P->state[b] = 2;
        pthread_cond_broadcast(&P->cv_ready);
        if (P->failed)
            pthread_cond_broadcast(&P->cv_free);
        pthread_mutex_unlock(&P->mu);
    }
}

/* format and write in turns (small tables, one thread, no thread to be had) */
static int write_rows_serial(FILE *tab, fmt_job proto, size_t n)
{
    fmt_job j = proto;
    j.buf = NULL;
    j.cap = 0;
    int rc = 0;
    for (size_t a = 0; a < n && !rc; a += 65536) {
        j.a = a;
        j.b = a + 65536 < n ? a + 65536 : n;
        j.len = 0;
        fmt_rows(&j);
        if (j.failed || fwrite(j.buf, 1, j.len, tab) != j.len)
            rc = 1;
    }
    free(j.buf);
    return rc;
}

static int write_rows_parallel(FILE *tab, fmt_job proto, size_t n, int threads)
{
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    /* (IBDGEM_MT_MIN_BYTES in the environment, the tests' switch for the threaded readers, also sends small tables through
     * the pipeline: chunks of 37 rows and a ring short enough that formatters wait for the writer) */
    const int tiny = ls_mt_min_bytes() < 4096;
    if (threads == 1 || (n < 8192 && !tiny))
        return write_rows_serial(tab, proto, n);
    row_pipe P;
    memset(&P, 0, sizeof P);
    P.proto = proto;
    P.n = n;
    P.chunk_rows = tiny ? 37 : 16384;
    P.n_chunks = (n + P.chunk_rows - 1) / P.chunk_rows;
    P.ring = tiny ? threads + 1 : 3 * threads;
    P.slot = calloc((size_t)P.ring, sizeof *P.slot);
    P.state = calloc((size_t)P.ring, sizeof *P.state);
    if (!P.slot || !P.state) {
        free(P.slot);
        free(P.state);
        return 1;
    }
    for (int b = 0; b < P.ring; ++b) {
        P.slot[b] = proto;
        P.slot[b].buf = NULL;
        P.slot[b].cap = 0;
    }
    pthread_mutex_init(&P.mu, NULL);
    pthread_cond_init(&P.cv_ready, NULL);
    pthread_cond_init(&P.cv_free, NULL);
    pthread_t tid[64];
    int n_started = 0;
    for (int t = 0; t < threads; ++t)
        if (pthread_create(&tid[n_started], NULL, row_pipe_worker, &P) == 0)
            ++n_started;
    int rc = 0;
    if (n_started == 0) {
        free(P.slot);
        free(P.state);
        pthread_mutex_destroy(&P.mu);
        pthread_cond_destroy(&P.cv_ready);
        pthread_cond_destroy(&P.cv_free);
        return write_rows_serial(tab, proto, n);
    }
    if (fflush(tab) != 0)
        rc = 1;
    const int fd = fileno(tab);
    for (size_t c = 0; c < P.n_chunks && !rc; ++c) {
        const int b = (int)(c % (size_t)P.ring);
        pthread_mutex_lock(&P.mu);
        while (P.state[b] != 2 && !P.failed)
            pthread_cond_wait(&P.cv_ready, &P.mu);
        const int bad = P.failed || P.state[b] != 2;
        pthread_mutex_unlock(&P.mu);
        if (bad) {
            rc = 1;
            break;
        }
        const fmt_job *j = &P.slot[b];
        for (size_t off = 0; off < j->len;) {        /* straight to the descriptor: stdio would copy 1.3 MB through its buffer */
            const ssize_t w = write(fd, j->buf + off, j->len - off);
            if (w < 0) {
                if (errno == EINTR)
                    continue;
                rc = 1;
                break;
            }
            off += (size_t)w;
        }
        pthread_mutex_lock(&P.mu);
        P.state[b] = 0;
        pthread_cond_broadcast(&P.cv_free);
        pthread_mutex_unlock(&P.mu);
    }
    if (rc) {
        pthread_mutex_lock(&P.mu);
        P.failed = 1;
        pthread_cond_broadcast(&P.cv_free);
        pthread_mutex_unlock(&P.mu);
    }
    for (int t = 0; t < n_started; ++t)
        pthread_join(tid[t], NULL);
    for (int b = 0; b < P.ring; ++b)
        free(P.slot[b].buf);
    free(P.slot);
    free(P.state);
    pthread_mutex_destroy(&P.mu);
    pthread_cond_destroy(&P.cv_ready);
    pthread_cond_destroy(&P.cv_free);
    return rc;
}

/* ---- the rows of the summary file (:751-756), formatted by the same team ---------------------- */
typedef struct {
    size_t a, b;                         /* windows [a, b) */
    const uint32_t *s_row, *w_first, *w_last, *w_ncov;
    const unsigned long *pos_first, *pos_last;   /* the windows' first and last positions, or NULL (looked up row by row) */
    const double *win_ll;
    int logs;                            /* the rows of the log summary: win_ll holds log2 values, printed %.6f, NaN as nan */
    char *buf;
    size_t len;
} sum_job;

static int fmt_log2(char *dst, double v, char sep)
{
    const int k = isnan(v) ? sprintf(dst, "nan") : sprintf(dst, "%.6f", v);
    dst[k] = sep;
    return k + 1;
}

static void *fmt_summary(void *arg)
{
    sum_job *j = arg;
    char *q = j->buf;
    for (size_t w = j->a; w < j->b; ++w) {
        q = put_u64(q, w + 1); *q++ = '\t';
        q = put_u64(q, j->pos_first ? j->pos_first[w] : rows[j->s_row[j->w_first[w]]].pos); *q++ = '\t';
        q = put_u64(q, j->pos_last ? j->pos_last[w] : rows[j->s_row[j->w_last[w]]].pos); *q++ = '\t';
        for (int k = 0; k < 3; ++k)
            q += j->logs ? fmt_log2(q, j->win_ll[3 * w + k], '\t') : fmt_ll(q, j->win_ll[3 * w + k], '\t');
        q = put_u64(q, j->w_ncov[w]); *q++ = '\n';
    }
    j->len = (size_t)(q - j->buf);
    return NULL;
}

/* 160 bytes hold any row: three integers of at most 20 digits, three numbers of at most 24 characters.
 * *buf / *cap: the caller's buffer, kept from one individual to the next (5.5 MB at 35 000 windows: allocated anew for every
 * individual it went back to the system each time -- a map, 600 page faults and an unmap per summary file). */
static int write_summary_parallel(FILE *sum, sum_job proto, size_t n_win, int threads, char **buf, size_t *cap)
{
    sum_job jobs[64];
    pthread_t tid[64];
    int started[64] = {0};
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    const int team = n_win < 2048 ? 1 : threads;
    if (*cap < n_win * 160 + 16) {
        free(*buf);
        *buf = malloc(n_win * 160 + 16);
        *cap = *buf ? n_win * 160 + 16 : 0;
    }
    char *all = *buf;
    if (!all)
        return 1;
    for (int t = 0; t < team; ++t) {
        jobs[t] = proto;
        jobs[t].a = n_win * (size_t)t / (size_t)team;
        jobs[t].b = n_win * (size_t)(t + 1) / (size_t)team;
        jobs[t].buf = all + jobs[t].a * 160;
        jobs[t].len = 0;
    }
    for (int t = 0; t + 1 < team; ++t)
        started[t] = pthread_create(&tid[t], NULL, fmt_summary, &jobs[t]) == 0;
    for (int t = 0; t < team; ++t)
        if (!started[t])
            fmt_summary(&jobs[t]);
    for (int t = 0; t + 1 < team; ++t)
        if (started[t])
            pthread_join(tid[t], NULL);
    /* straight to the descriptor (stdio would copy the 2.5 MB through its buffer); what stdio holds goes first */
    int rc = fflush(sum) != 0;
    const int fd = fileno(sum);
    for (int t = 0; t < team && !rc; ++t)
        for (size_t off = 0; off < jobs[t].len;) {
            const ssize_t w = write(fd, jobs[t].buf + off, jobs[t].len - off);
            if (w < 0) {
                if (errno == EINTR)
                    continue;
                rc = 1;
                break;
            }
            off += (size_t)w;
        }
    return rc;
}

/* ---- --arm-stats: chromosome-arm sums of the window log-likelihood ratios (reference bin/chrarm-stats.py) ----------
 * A window's terms are log2(L2') - log2(L0') and log2(L1') - log2(L0'), L' = L or 2^-1074 where L == 0, summed as
 * double-doubles: on the device by ibdg_window_llr_sums, here for runs without one and to add the parts of a range that
 * several devices summed, in device order.  The rounded sum then does not depend on the split. */
static void dd_add(double x[2], double hi, double lo)
{
    const double s = x[0] + hi, bb = s - x[0];
    double e = (x[0] - (s - bb)) + (hi - bb);       /* TwoSum: s + e == x[0] + hi exactly */
    e += x[1] + lo;
    x[0] = s + e;
    x[1] = e - (x[0] - s);
}

static double arm_log2(double v)
{
    return log2(v == 0.0 ? 0x1p-1074 : v);
}

/* the sums over windows [a, b) of a window table on the host: out = {IBD2/IBD0 hi, lo, IBD1/IBD0 hi, lo}; logs: the table
 * is the log2 table and its entries are the terms (--log-stats, ibdg_window_log2_llr_sums) */
static void llr_range_host(const double *win_ll, int logs, size_t a, size_t b, double out[4])
{
    out[0] = out[1] = out[2] = out[3] = 0.0;
    for (size_t w = a; w < b; ++w) {
        const double l0 = logs ? win_ll[3 * w] : arm_log2(win_ll[3 * w]), l1 = logs ? win_ll[3 * w + 1] : arm_log2(win_ll[3 * w + 1]),
                     l2 = logs ? win_ll[3 * w + 2] : arm_log2(win_ll[3 * w + 2]);
        dd_add(out, l2, 0.0);
        dd_add(out, -l0, 0.0);
        dd_add(out + 2, l1, 0.0);
        dd_add(out + 2, -l0, 0.0);
    }
}

/* The arms of a site list's n windows, from the START / END each summary row prints (fmt_summary's lookup):
 * p = [0, k), k the first window with END >= c0 (n if none), NaN when END_0 > c0 or n == 0;
 * q = [m, n), m the first window at or after k with START >= c1, NaN when there is none.
 * seg = {p first, p end, q first, q end}; ok[0], ok[1]: the arm has a value. */
static void arm_segments(const uint32_t *s_row, const uint32_t *w_first, const uint32_t *w_last, size_t n, uint32_t seg[4],
                         int ok[2])
{
    size_t k = 0;
    while (k < n && rows[s_row[w_last[k]]].pos < arm_c0)
        ++k;
    size_t m = k;
    while (m < n && rows[s_row[w_first[m]]].pos < arm_c1)
        ++m;
    ok[0] = n > 0 && rows[s_row[w_last[0]]].pos <= arm_c0;
    ok[1] = m < n;
    seg[0] = 0; seg[1] = (uint32_t)k;
    seg[2] = (uint32_t)(ok[1] ? m : n); seg[3] = (uint32_t)n;
}

/* "START,END": two decimal integers, END >= START; 0 when malformed */
static int parse_arm_range(const char *arg)
{
    char *e1, *e2;
    if (!isdigit((unsigned char)arg[0]))
        return 0;
    errno = 0;
    arm_c0 = strtoul(arg, &e1, 10);
    if (errno || *e1 != ',' || !isdigit((unsigned char)e1[1]))
        return 0;
    arm_c1 = strtoul(e1 + 1, &e2, 10);
    return !errno && *e2 == 0 && arm_c1 >= arm_c0;
}

/* windows of a site list: runs of `window` covered rows (:572, :657-663, :723-730); arrays of n_win + 1 entries.  The engine's
 * definition as well (ibdg_upload_sites: n_win = ceil(covered / window); ibdg_get_windows: first / last = the covered rows
 * w * window and min((w + 1) * window, covered) - 1): the host program cuts the --arm-stats arms from these before a run,
 * and checks them against the engine's whenever the window tables come back (see the gather below). */
static size_t host_windows(const uint8_t *nr, const uint8_t *na, size_t n, unsigned window, uint32_t **first, uint32_t **last,
                           uint32_t **ncov)
{
    size_t covered = 0;
    for (size_t i = 0; i < n; ++i)
        covered += (nr[i] + na[i]) > 0;
    const size_t n_win = (covered + window - 1) / window;
    uint32_t *w_first = malloc((n_win + 1) * 4), *w_last = malloc((n_win + 1) * 4), *w_ncov = calloc(n_win + 1, 4);
    if (!w_first || !w_last || !w_ncov) {
        fprintf(stderr, "[::] ERROR: out of memory for %zu windows.\n", n_win);
        exit(1);
    }
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        if (nr[i] + na[i] == 0) continue;
        const size_t w = k / window;
        if (k % window == 0) w_first[w] = (uint32_t)i;
        w_last[w] = (uint32_t)i;
        w_ncov[w]++;
        k++;
    }
    *first = w_first; *last = w_last; *ncov = w_ncov;
    return n_win;
}

/* a site list's windows: first and last site of each window and its covered rows, arrays of n_win + 1 entries */
typedef struct {
    size_t n_win;
    uint32_t *first, *last, *ncov;
} win_list;

static void win_list_free(win_list *l)
{
    free(l->first); free(l->last); free(l->ncov);
    memset(l, 0, sizeof *l);
}

/* 0: out of memory (and *l empty) */
static int win_list_alloc(win_list *l, size_t n_win)
{
    l->n_win = n_win;
    l->first = malloc((n_win + 1) * 4); l->last = malloc((n_win + 1) * 4); l->ncov = malloc((n_win + 1) * 4);
    if (l->first && l->last && l->ncov)
        return 1;
    win_list_free(l);
    return 0;
}

static int win_list_copy(win_list *to, const win_list *from)
{
    if (!win_list_alloc(to, from->n_win))
        return 0;
    memcpy(to->first, from->first, from->n_win * 4);
    memcpy(to->last, from->last, from->n_win * 4);
    memcpy(to->ncov, from->ncov, from->n_win * 4);
    return 1;
}

/* an individual's window table, owned by whoever holds the struct (a shard's job, the pileup's run, the individual's output
 * job: handed over by assignment, the giver's copy zeroed or dropped) */
typedef struct {
    win_list w;
    double *ll;                              /* LIBD0/1/2 per window, n_win + 1 rows */
    double *log;                             /* --log-summary: log2 of the same table, else NULL */
} win_table;

/* the log2 tables leave the engine / are made on the host: for --log-summary's files and --log-stats' statistics */
static int want_logs(void) { return opt_log_summary || opt_log_stats; }

static void win_table_free(win_table *t)
{
    win_list_free(&t->w);
    free(t->ll); free(t->log);
    memset(t, 0, sizeof *t);
}

/* 0: out of memory */
static int win_table_alloc_ll(win_table *t)
{
    t->ll = malloc((t->w.n_win + 1) * 24);
    t->log = want_logs() ? malloc((t->w.n_win + 1) * 24) : NULL;
    return t->ll && (t->log || !want_logs());
}

/* --chain-gap BP, for every route: window w >= 1 starts a chain iff its first position lies more than BP behind the last
 * position of window w - 1 (the START and END the summary prints); a gap inside a window starts nothing.  starts: room for n
 * entries; returns how many there are (strictly increasing, in [1, n): what ibdg_set_window_chains and the _chains_host twins
 * take).  Without the option: none. */
static size_t chain_gap_starts(const uint64_t *pos_first, const uint64_t *pos_last, size_t n, uint32_t *starts)
{
    size_t k = 0;
    for (size_t w = 1; has_chain_gap && w < n; ++w)
        if (pos_first[w] > pos_last[w - 1] && pos_first[w] - pos_last[w - 1] > opt_chain_gap)
            starts[k++] = (uint32_t)w;
    return k;
}

/* --genetic-map: g(x) in centimorgans.  Behind the map's last entry and before its first it continues at the map's mean rate;
 * else it is linear between the entry at or below x and the one above it. */
static double gmap_at(double x)
{
    const size_t n = gmap_n;
    const double mean = (gmap_cm[n - 1] - gmap_cm[0]) / (gmap_pos[n - 1] - gmap_pos[0]);
    if (x < gmap_pos[0])
        return gmap_cm[0] + (x - gmap_pos[0]) * mean;
    if (x >= gmap_pos[n - 1])
        return gmap_cm[n - 1] + (x - gmap_pos[n - 1]) * mean;
    size_t lo = 0, hi = n - 1;                   /* pos[lo] <= x < pos[hi] */
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (gmap_pos[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return gmap_cm[lo] + (x - gmap_pos[lo]) * ((gmap_cm[lo + 1] - gmap_cm[lo]) / (gmap_pos[lo + 1] - gmap_pos[lo]));
}

/* --genetic-map FILE is read once, before any pileup: exits with a message that names the line for anything but a header and
 * lines of three numbers with strictly increasing positions */
static void gmap_read(const char *fn)
{
    FILE *f = fopen(fn, "r");
    if (!f) {
        fprintf(stderr, "[::] ERROR: cannot open the genetic map (--genetic-map) %s.\n", fn);
        exit(1);
    }
    char line[1024];
    size_t cap = 0, ln = 1;
    if (!fgets(line, sizeof line, f)) {
        fprintf(stderr, "[::] ERROR: the genetic map (--genetic-map) %s is empty (a header line, then position, rate, cM).\n", fn);
        exit(1);
    }
    while (fgets(line, sizeof line, f)) {
        ++ln;
        double pos, rate, cm;
        char tail;
        if (line[strspn(line, " \t\r\n")] == 0)
            continue;
        if (sscanf(line, "%lf %lf %lf %c", &pos, &rate, &cm, &tail) != 3 || !isfinite(pos) || !isfinite(cm)) {
            fprintf(stderr, "[::] ERROR: genetic map (--genetic-map) %s, line %zu: not three numbers (position, rate in cM/Mb, cumulative cM).\n", fn, ln);
            exit(1);
        }
        if (gmap_n && !(pos > gmap_pos[gmap_n - 1])) {
            fprintf(stderr, "[::] ERROR: genetic map (--genetic-map) %s, line %zu: position %.17g does not lie above the %.17g of the entry before it (strictly increasing).\n",
                    fn, ln, pos, gmap_pos[gmap_n - 1]);
            exit(1);
        }
        if (gmap_n == cap) {
            cap = cap ? 2 * cap : 1024;
            gmap_pos = realloc(gmap_pos, cap * sizeof *gmap_pos);
            gmap_cm = realloc(gmap_cm, cap * sizeof *gmap_cm);
            if (!gmap_pos || !gmap_cm) {
                fprintf(stderr, "[::] ERROR: out of memory for the genetic map.\n");
                exit(1);
            }
        }
        gmap_pos[gmap_n] = pos, gmap_cm[gmap_n] = cm;
        ++gmap_n;
    }
    fclose(f);
    if (gmap_n < 2) {
        fprintf(stderr, "[::] ERROR: the genetic map (--genetic-map) %s has %zu entries; two make a rate.\n", fn, gmap_n);
        exit(1);
    }
}

/* --switch-scale X, for every route: the step shift of every window (what ibdg_set_window_steps and the _steps_host
 * twins take) from the positions the summary prints.  D_w is the distance of the centres of windows w - 1 and w -- the integer
 * difference of START + END first, then its half; with --genetic-map the difference of g at the two centres --, shift[w] =
 * llrint(log2(D_w / X) * 65536): one division, one log2, one product, one rounding, kept within +-2^30; -2^30 where D_w <= 0.
 * shift: room for n entries; shift[0] = 0 (not read). */
static void switch_scale_shifts(const uint64_t *pos_first, const uint64_t *pos_last, size_t n, int32_t *shift)
{
    const double lim = 1073741824.0;
    for (size_t w = 0; w < n; ++w) {
        double D = 0.0, v = -lim;
        if (w == 0) {
            shift[0] = 0;
            continue;
        }
        if (gmap_n)
            D = gmap_at((double)(pos_first[w] + pos_last[w]) * 0.5) - gmap_at((double)(pos_first[w - 1] + pos_last[w - 1]) * 0.5);
        else
            D = (double)(int64_t)((pos_first[w] + pos_last[w]) - (pos_first[w - 1] + pos_last[w - 1])) * 0.5;
        if (D > 0.0)
            v = log2(D / opt_switch_scale) * 65536.0;
        shift[w] = v >= lim ? (int32_t)lim : !(v > -lim) ? -(int32_t)lim : (int32_t)llrint(v);
    }
}

/* ---- --sample-paths: an individual's row of logibdsamples.txt, made when its draws are done, so that the K records of 120 bytes
 * need not be kept to the run's end: what stays per individual is the row's text, and per run K sums of nine numbers ---- */
enum { SMP_ROW_ROOM = 2048 };               /* 36 columns of at most 26 characters and the share */
static pthread_mutex_t g_smp_mu = PTHREAD_MUTEX_INITIALIZER;   /* a run's totals: its output jobs add to them side by side */

static int cmp_u64(const void *a, const void *b)
{
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}

/* What K draws say of one quantity, appended to buf: v[K] is sorted in place; the mean is the integer sum divided once, the
 * quantiles are the order statistics v[(K - 1) / 40], v[(K - 1) / 2] and v[(K - 1) - (K - 1) / 40] (integer division) */
static size_t sample_columns(char *buf, size_t len, uint64_t *v, size_t K)
{
    uint64_t sum = 0;
    for (size_t k = 0; k < K; ++k)
        sum += v[k];
    qsort(v, K, sizeof *v, cmp_u64);
    return len + (size_t)snprintf(buf + len, SMP_ROW_ROOM - len, "\t%.3f\t%llu\t%llu\t%llu", (double)sum / (double)K,
                                  (unsigned long long)v[(K - 1) / 40], (unsigned long long)v[(K - 1) / 2],
                                  (unsigned long long)v[(K - 1) - (K - 1) / 40]);
}

/* A row behind its ID, N_SEGMENTS and K, from K rows of nine numbers, v[k] = windows, segments and base pairs per state: per state
 * the three quantities' columns, then the share of draws with an IBD1 or IBD2 segment and the line's end.  buf [SMP_ROW_ROOM],
 * col [K]: scratch */
static void sample_row_tail(char *buf, const uint64_t (*v)[9], size_t K, uint64_t *col)
{
    size_t any = 0, len = 0;
    for (int s = 0; s < 3; ++s)
        for (int q = 0; q < 3; ++q) {
            for (size_t k = 0; k < K; ++k)
                col[k] = v[k][3 * q + s];
            len = sample_columns(buf, len, col, K);
        }
    for (size_t k = 0; k < K; ++k)
        any += v[k][3 + 1] + v[k][3 + 2] > 0;
    snprintf(buf + len, SMP_ROW_ROOM - len, "\t%.6f\n", (double)any / (double)K);
}

/* An individual's draws are done: rec [K][15] (ibdg_window_log2_samples / ibdg_log2_samples_host).  Its row's tail as text of its
 * own, and draw k added to the run's totals tot [K][9].  NULL: out of memory (nothing was added) */
static char *sample_individual_row(const uint64_t *rec, size_t K, uint64_t (*tot)[9])
{
    uint64_t (*nine)[9] = malloc(K * sizeof *nine), *col = malloc(K * sizeof *col);
    char *row = malloc(SMP_ROW_ROOM);
    if (nine && col && row) {
        for (size_t k = 0; k < K; ++k)
            for (int i = 0; i < 9; ++i)
                nine[k][i] = rec[15 * k + (i < 6 ? i : i + 3)];        /* windows [0..2], segments [3..5], base pairs [9..11] */
        pthread_mutex_lock(&g_smp_mu);
        for (size_t k = 0; k < K; ++k)
            for (int i = 0; i < 9; ++i)
                tot[k][i] += nine[k][i];
        pthread_mutex_unlock(&g_smp_mu);
        sample_row_tail(row, (const uint64_t (*)[9])nine, K, col);
    } else {
        free(row);
        row = NULL;
    }
    free(nine);
    free(col);
    return row;
}

/* ---- one comparison spread over several GPUs (window ranges, host-side gather) ------------ */
/* What the run's statistics files hold of one comparison individual, the same record from the device (or the individual's
 * output job) to the files: a shard's double-double arm sums (ibdg_window_llr_sums), of which the run keeps the four rounded
 * sums p20, q20, p10, q10 in arm[0..3]; its windows in IBD0, IBD1, IBD2; its expected windows per state and log2 Z; its line of
 * logibdsegments.txt (the summary of ibdg_window_log2_segments / ibdg_log2_segments_host); its row of
 * logibdsamples.txt behind the first three columns (sample_individual_row; its own allocation, freed with the run's records). */
typedef struct {
    double arm[8];
    uint64_t st[3];
    double po[4];
    uint64_t sg[12];
    char *smp_row;
    double sw[6];                            /* --switches: its expected switches, then the prior's of its site list */
    uint64_t swc[3];                         /* ... and the list's counted steps */
} ind_stats;

/* The host's conversation with ONE context about a pileup's comparison individuals, owned by the context's worker.  It has
 * three levels, each with a function of its own, called when the individual at hand starts that level (shards_fill decides):
 *   conv_list        a new site list: the context's slice of it goes up, what was kept of the list before is dropped;
 *   conv_batch       a new batch of individuals over that list (when the list does not depend on the individual -- no -v, no
 *                    -D -- up to TARGET_BATCH of them per engine call: groups share a workgroup of the --LD kernels; else the
 *                    individual alone): the run, its statistics, its tables where they come in one copy, the next batch queued;
 *   conv_individual  the individual's share of all that, or its own fetch.
 * The fields are grouped by the level that sets them. */
typedef struct {
    ibdg_ctx *eng;
    int idx;                                 /* which of the run's contexts, for messages */
    /* ---- the pileup's run (run_modes) ---- */
    FILE *err;                               /* where the pileup's messages go */
    const uint8_t *bg_count;
    int pu_id;
    int shared_list;                         /* the site list is the same for every comparison individual of the run */
    int list_on_device;                      /* -v lists made by the engine: it holds the individual's list already */
    int tables_stay;                         /* --stats-only: no window table leaves the device */
    int dev_states;                          /* --log-stats --states --stats-only on one context: the paths are found on the device */
    int reported;                            /* a failure was reported here already (not an engine error) */
    int fit_store;                           /* --fit-penalties on one context: every batch's log tables are kept in the engine's store, */
    size_t fit_reserve;                      /* ... which is sized for this many individuals, all of the run */
    /* ---- the slice [a, b) of the site list at hand (shards_fill) ---- */
    const uint32_t *row;                     /* the list's panel rows as this context counts them, */
    const uint32_t *s_row;                   /* ... and as the host does, for the windows' positions */
    const uint8_t *nr, *na;
    const double *fo;
    size_t a, b;
    const uint32_t *arm_seg;                 /* --arm-stats: {p first, p end, q first, q end} in the slice's window indices, or NULL */
    /* ---- the batch at hand and the one after it (NULL: none; window tables only, --summary-only), which is queued on the
     * device while the host goes through this one's tables ---- */
    const uint32_t *targets, *next;
    size_t n_targets, n_next;
    /* ---- kept from call to call ---- */
    win_list wl;                             /* the windows of the list at hand: the same for every individual over a shared list, */
    int wl_kept;                             /* ... fetched once then, not once per individual */
    /* a page-locked buffer through which an individual's window likelihoods come back at link speed (0.8 MB each at 35 000
     * windows: through pageable memory the copy took longer than the individual's share of the engine's run) */
    double *stage;
    size_t stage_cap;
    /* a batch's window tables, taken off the device in one copy, so that the next batch can run while the host goes through
     * them (one table at a time left the device idle for the 4 ms the host needs per batch of 30, beside 6 ms of running) */
    double *batch_ll;                        /* (page-locked) */
    double *batch_log;                       /* --log-summary: their logs, taken off the device with them */
    size_t batch_cap, batch_log_cap;
    const uint32_t *batch_of;                /* the batch (its targets) the tables belong to; NULL: none */
    const uint32_t *ahead_of;                /* the batch that has been queued ahead on the device; NULL: none */
    /* the statistics of the last run's individuals */
    double *arm_sums;                        /* --arm-stats: [T][2][4] */
    uint64_t *st_counts;                     /* --log-stats --states: the state counts, [T][3] */
    double *po_vals;                         /* --posteriors: expect [T][3], then log2 Z [T] */
    uint64_t *sg_vals;                       /* --segments: summary [T][12], then the counts [T] */
    uint64_t *sg_pos;                        /* ... the windows' first positions [n_win], then their last */
    uint32_t *ch_starts;                     /* --chain-gap: the chain starts of the list at hand */
    int32_t *sw_shift;                       /* --switch-scale: the step shifts of the list at hand */
    uint64_t *smp_vals;                      /* --sample-paths: the draws' records [T][K][15] */
    uint64_t *smp_stream;                    /* ... and the individuals' streams [T]: their indices in the panel */
    uint64_t (*smp_tot)[9];                  /* ... and the run's totals [K][9], which every individual's draws are added to (the run's) */
    double *swi_vals;                        /* --switches: the expected switches [T][3] */
    double swi_prior[3];                     /* ... the prior of the list at hand (made with the list's first batch) */
    uint64_t swi_counted[3];                 /* ... and its counted steps */
    int swi_have;
    size_t swi_cap;
    size_t arm_cap, st_cap, po_cap, sg_cap, sg_pos_cap, ch_cap, sw_cap, smp_cap, smp_stream_cap;
} dev_conv;

/* one comparison individual on one context: where it stands and what comes back for it */
enum { AT_INDIVIDUAL, AT_BATCH, AT_LIST };   /* the outermost level the individual starts (a list starts a batch) */
typedef struct {
    dev_conv *c;
    int level;
    size_t t_local;                          /* which of the batch it is */
    double *site_ll;                         /* out, per-site tables: the comparison-wide array, written at the slice's offset */
    win_table wt;                            /* out: slice-local arrays, window indices local */
    ind_stats out;                           /* out: its sums over the arms, and with dev_states its other statistics */
    int failed;
} shard_job;

/* room for `need` elements of `elt` bytes in a scratch array that only grows (its contents are not kept); 0: out of memory */
static int grow(void *ptr, size_t *cap, size_t need, size_t elt)
{
    void **p = ptr;
    if (*cap < need) {
        free(*p);
        *p = malloc(need * elt);
        *cap = *p ? need : 0;
    }
    return *p != NULL;
}

/* the same in page-locked memory (ibdg_host_alloc) */
static int grow_pinned(void *ptr, size_t *cap, size_t need, size_t elt)
{
    void **p = ptr;
    if (*cap < need) {
        if (*p)
            ibdg_host_free(*p);
        *p = ibdg_host_alloc(need * elt);
        *cap = *p ? need : 0;
    }
    return *p != NULL;
}

/* what a context's conversation holds, given back on the orderly way out */
static void conv_release(dev_conv *c)
{
    win_list_free(&c->wl);
    if (c->stage)
        ibdg_host_free(c->stage);
    if (c->batch_ll)
        ibdg_host_free(c->batch_ll);
    free(c->batch_log); free(c->arm_sums); free(c->st_counts); free(c->po_vals); free(c->sg_vals); free(c->sg_pos); free(c->ch_starts); free(c->sw_shift);
    free(c->smp_vals); free(c->smp_stream); free(c->swi_vals);
    memset(c, 0, sizeof *c);
}

/* a failure with a message of its own (every other one is the engine's: ibdg_last_error) */
static int conv_oom(dev_conv *c, size_t n_win)
{
    fprintf(c->err ? c->err : stderr, "[::] ERROR: out of memory for %zu windows.\n", n_win);
    c->reported = 1;
    return 1;
}

/* The windows of the list at hand on this context (n_win of them: ibdg_num_windows), in c->wl: fetched once per list when
 * the individuals share it, and every time otherwise.  NULL: failed. */
static const win_list *conv_windows(dev_conv *c, size_t n_win)
{
    if (c->wl_kept && c->wl.n_win == n_win)
        return &c->wl;
    win_list_free(&c->wl);
    c->wl_kept = 0;
    if (!win_list_alloc(&c->wl, n_win))
        return conv_oom(c, n_win), NULL;
    if (ibdg_get_windows(c->eng, c->wl.first, c->wl.last, c->wl.ncov))
        return NULL;
    c->wl_kept = c->shared_list;
    return &c->wl;
}

/* the positions of the windows of the list at hand in c->sg_pos: the first [n_win], then the last */
static int conv_positions(dev_conv *c, size_t n_win)
{
    const win_list *wl = conv_windows(c, n_win);
    if (!wl)
        return 1;
    if (!grow(&c->sg_pos, &c->sg_pos_cap, 2 * n_win + 1, sizeof(uint64_t)))
        return conv_oom(c, n_win);
    for (size_t w = 0; w < n_win; ++w) {
        c->sg_pos[w] = rows[c->s_row[c->a + wl->first[w]]].pos;
        c->sg_pos[n_win + w] = rows[c->s_row[c->a + wl->last[w]]].pos;
    }
    return 0;
}

/* --chain-gap where the paths are found on the device: the chain starts of a new site list go to the engine once, which keeps
 * them for every run over the list */
static int chains_on_device(dev_conv *c)
{
    if (!has_chain_gap || !(c->dev_states || c->fit_store))
        return 0;
    const size_t n_win = ibdg_num_windows(c->eng);
    if (conv_positions(c, n_win))
        return 1;
    if (!grow(&c->ch_starts, &c->ch_cap, n_win + 1, sizeof(uint32_t)))
        return conv_oom(c, n_win);
    return ibdg_set_window_chains(c->eng, c->ch_starts, chain_gap_starts(c->sg_pos, c->sg_pos + n_win, n_win, c->ch_starts));
}

/* --switch-scale where the paths are found on the device: likewise, the step shifts of a new site list */
static int steps_on_device(dev_conv *c)
{
    if (!has_switch_scale || !(c->dev_states || c->fit_store))
        return 0;
    const size_t n_win = ibdg_num_windows(c->eng);
    if (conv_positions(c, n_win))
        return 1;
    if (!grow(&c->sw_shift, &c->sw_cap, n_win + 1, sizeof(int32_t)))
        return conv_oom(c, n_win);
    switch_scale_shifts(c->sg_pos, c->sg_pos + n_win, n_win, c->sw_shift);
    return ibdg_set_window_steps(c->eng, c->sw_shift, n_win);
}

/* --segments where the tables stay on the device: the list's windows' positions go up with the call */
static int segments_on_device(dev_conv *c)
{
    const size_t n_win = ibdg_num_windows(c->eng), T = c->n_targets;
    if (conv_positions(c, n_win))
        return 1;
    if (!grow(&c->sg_vals, &c->sg_cap, T * 13, sizeof(uint64_t)))
        return conv_oom(c, n_win);
    return ibdg_window_log2_segments(c->eng, opt_p01, opt_p02, opt_p12, opt_posteriors, c->sg_pos, c->sg_pos + n_win,
                                     c->sg_vals + T * 12, c->sg_vals);
}

/* --sample-paths where the tables stay on the device: the positions go up with the call as the segments' do; a draw's stream is
 * the individual's index in the panel, so that no batch, slot or device shows in it */
static int samples_on_device(dev_conv *c)
{
    const size_t n_win = ibdg_num_windows(c->eng), T = c->n_targets, K = opt_sample_paths;
    if (conv_positions(c, n_win))
        return 1;
    if (!grow(&c->smp_vals, &c->smp_cap, T * K * 15, sizeof(uint64_t)) || !grow(&c->smp_stream, &c->smp_stream_cap, T + 1, sizeof(uint64_t)))
        return conv_oom(c, n_win);
    for (size_t t = 0; t < T; ++t)
        c->smp_stream[t] = c->targets[t];
    return ibdg_window_log2_samples(c->eng, opt_p01, opt_p02, opt_p12, K, opt_seed, c->smp_stream, c->sg_pos, c->sg_pos + n_win, c->smp_vals);
}

/* --switches where the tables stay on the device: the expectations alone come back; the prior is the twin's on the table that
 * says nothing under the context's chains and steps, once per site list.  (The last of the run's calls: it runs over the
 * posteriors' scratch.) */
static int switches_on_device(dev_conv *c)
{
    const size_t T = c->n_targets;
    if (!grow(&c->swi_vals, &c->swi_cap, T * 3, sizeof(double)))
        return conv_oom(c, 0);
    if (!c->swi_have && ibdg_window_log2_switches_prior(c->eng, opt_p01, opt_p02, opt_p12, c->swi_prior, c->swi_counted))
        return 1;
    c->swi_have = 1;
    return ibdg_window_log2_switches(c->eng, opt_p01, opt_p02, opt_p12, NULL, c->swi_vals);
}

/* the engine's last run must be the run of this very batch: its size says so (a diagnostic when it does not) */
static int same_run_size(dev_conv *c)
{
    const size_t have = ibdg_num_targets(c->eng);
    if (have == c->n_targets)
        return 1;
    fprintf(c->err ? c->err : stderr, "[::] ERROR: context %d holds the results of %zu comparison individuals, not the %zu of "
            "the batch at hand.\n", c->idx, have, c->n_targets);
    c->reported = 1;
    return 0;
}

/* The statistics of every individual of the run at once, before a look-ahead replaces the run's window tables: the arm sums,
 * and with dev_states the state counts, the posteriors' sums and the segments' summaries -- only these leave the device.  (On
 * one run the library finds the paths and the posteriors once for the three calls.) */
static int device_stats(dev_conv *c)
{
    const size_t T = c->n_targets;
    if (c->arm_seg) {
        const uint32_t sf[2] = {c->arm_seg[0], c->arm_seg[2]}, se[2] = {c->arm_seg[1], c->arm_seg[3]};
        if (!grow(&c->arm_sums, &c->arm_cap, T * 8, sizeof(double)))
            return conv_oom(c, 0);
        if (!same_run_size(c) || (opt_log_stats ? ibdg_window_log2_llr_sums : ibdg_window_llr_sums)(c->eng, sf, se, 2, c->arm_sums))
            return 1;
    }
    if (!c->dev_states)
        return 0;
    if (!grow(&c->st_counts, &c->st_cap, T * 3, sizeof(uint64_t)) || (opt_posteriors && !grow(&c->po_vals, &c->po_cap, T * 4, sizeof(double))))
        return conv_oom(c, 0);
    if (!same_run_size(c) || ibdg_window_log2_states(c->eng, opt_p01, opt_p02, opt_p12, NULL, NULL, c->st_counts))
        return 1;
    if (opt_posteriors && ibdg_window_log2_posteriors(c->eng, opt_p01, opt_p02, opt_p12, NULL, c->po_vals, c->po_vals + T * 3))
        return 1;
    return (opt_segments && segments_on_device(c)) || (has_sample_paths && samples_on_device(c)) || (opt_switches && switches_on_device(c));
}

/* ... and an individual's share in them (1: out of memory for its row of the samples file) */
static int device_stats_of(dev_conv *c, size_t t, ind_stats *out)
{
    if (c->arm_seg)
        memcpy(out->arm, c->arm_sums + t * 8, sizeof out->arm);
    if (!c->dev_states)
        return 0;
    memcpy(out->st, c->st_counts + t * 3, sizeof out->st);
    if (opt_posteriors) {
        memcpy(out->po, c->po_vals + t * 3, 3 * sizeof(double));
        out->po[3] = c->po_vals[c->n_targets * 3 + t];
    }
    if (opt_segments)
        memcpy(out->sg, c->sg_vals + t * 12, sizeof out->sg);
    if (has_sample_paths && !(out->smp_row = sample_individual_row(c->smp_vals + t * opt_sample_paths * 15, opt_sample_paths, c->smp_tot)))
        return conv_oom(c, 0);
    if (opt_switches) {
        memcpy(out->sw, c->swi_vals + t * 3, 3 * sizeof(double));
        memcpy(out->sw + 3, c->swi_prior, sizeof c->swi_prior);
        memcpy(out->swc, c->swi_counted, sizeof c->swi_counted);
    }
    return 0;
}

/* a new site list for this context: its slice goes up (unless the engine made the list itself) */
static int conv_list(dev_conv *c)
{
    c->wl_kept = 0;
    c->batch_of = NULL;
    c->swi_have = 0;
    if (!c->list_on_device && ibdg_upload_sites(c->eng, c->row + c->a, c->nr + c->a, c->na + c->a, c->fo ? c->fo + c->a : NULL,
                                                c->b - c->a, (unsigned)opt_window))
        return 1;
    if (chains_on_device(c) || steps_on_device(c))
        return 1;
    /* --fit-penalties: the store belongs to the site list, and is sized for all the run's individuals */
    return c->fit_store && ibdg_log2_store_reserve(c->eng, c->fit_reserve);
}

/* the next batch runs while the host goes on with this one's statistics and files */
static int queue_ahead(dev_conv *c)
{
    if (!c->next)
        return 0;
    if (ibdg_set_option(c->eng, "async", 1) || ibdg_run(c->eng, c->next, c->n_next, c->bg_count, c->pu_id, opt_ld) ||
        ibdg_set_option(c->eng, "async", 0))
        return 1;
    c->ahead_of = c->next;
    return 0;
}

/* A new batch: its run -- or the one queued ahead taken over --, the statistics of all its individuals, its window tables in
 * one copy where only these are wanted of more than one individual (--summary-only; with per-site values every individual
 * fetches its own, see conv_individual), then the next batch queued. */
static int conv_batch(dev_conv *c)
{
    c->batch_of = NULL;
    if (c->ahead_of != c->targets) {             /* not queued ahead (the first batch, or no look-ahead in this run) */
        if (c->ahead_of && ibdg_sync(c->eng))
            return 1;
        if (ibdg_run(c->eng, c->targets, c->n_targets, c->bg_count, c->pu_id, opt_ld))
            return 1;
    }
    c->ahead_of = NULL;
    if (device_stats(c))
        return 1;
    /* --fit-penalties: the batch's log tables onto the store's end, before a look-ahead replaces them */
    if (c->fit_store && (!same_run_size(c) || ibdg_log2_store_append(c->eng)))
        return 1;
    if (!c->tables_stay && (c->next || c->n_targets > 1)) {
        /* (the library is asked in runs with per-site tables too, as it always was: the calls a context sees are pinned) */
        const size_t nw = ibdg_num_windows(c->eng), need = c->n_targets * (nw + 1) * 3;
        if (opt_summary_only) {
            if (!grow_pinned(&c->batch_ll, &c->batch_cap, need, sizeof(double)) ||
                (want_logs() && !grow(&c->batch_log, &c->batch_log_cap, need, sizeof(double))))
                return conv_oom(c, nw);
            /* (the copy is as large as the LAST RUN's results: it must be the run of this very batch) */
            if (!same_run_size(c) || ibdg_get_window_ll_all(c->eng, c->batch_ll))                /* waits for the run */
                return 1;
            if (want_logs() && ibdg_get_window_log2_all(c->eng, c->batch_log))
                return 1;
            c->batch_of = c->targets;
        }
    }
    return queue_ahead(c);
}

/* the individual's share of the batch's statistics, its window table -- from the batch's copy, or fetched alone through the
 * staging buffer -- and its per-site values */
static int conv_individual(dev_conv *c, shard_job *j)
{
    const size_t t = j->t_local;
    win_table *wt = &j->wt;
    if (device_stats_of(c, t, &j->out))
        return 1;
    const size_t n_win = wt->w.n_win = ibdg_num_windows(c->eng);
    if (c->tables_stay)
        return 0;
    const win_list *wl = conv_windows(c, n_win);
    if (!wl)
        return 1;
    if (!c->wl_kept) {                           /* the individual's own list: its windows go with it */
        wt->w = c->wl;
        memset(&c->wl, 0, sizeof c->wl);
    } else if (!win_list_copy(&wt->w, wl))
        return conv_oom(c, n_win);
    if (!win_table_alloc_ll(wt))
        return conv_oom(c, n_win);
    if (c->batch_of == c->targets) {             /* (window tables only: no per-site values on this path) */
        memcpy(wt->ll, c->batch_ll + t * n_win * 3, n_win * 24);
        if (wt->log)
            memcpy(wt->log, c->batch_log + t * n_win * 3, n_win * 24);
        return 0;
    }
    /* (no page-locked memory to be had: straight into the table) */
    double *const via = grow_pinned(&c->stage, &c->stage_cap, (n_win + 1) * 3, sizeof(double)) ? c->stage : wt->ll;
    if (ibdg_get_window_ll(c->eng, t, via))
        return 1;
    if (via != wt->ll)
        memcpy(wt->ll, via, n_win * 24);
    if (wt->log && ibdg_get_window_log2(c->eng, t, wt->log))
        return 1;
    return !opt_summary_only && ibdg_get_site_ll(c->eng, t, j->site_ll + 3 * c->a);
}

/* an individual's call on one context (a thread per context when there are several) */
static void *shard_run(void *arg)
{
    shard_job *j = arg;
    dev_conv *c = j->c;
    j->failed = (j->level == AT_LIST && conv_list(c)) || (j->level >= AT_BATCH && conv_batch(c)) || conv_individual(c, j);
    return NULL;
}

/* cut points of a site list into `parts` contiguous pieces holding whole windows
 * (a window = `window` consecutive covered rows; uncovered rows stay with the open window) */
static void window_cuts(const uint8_t *nr, const uint8_t *na, size_t n, unsigned window, int parts, size_t *cuts)
{
    size_t covered = 0;
    for (size_t i = 0; i < n; ++i)
        covered += (nr[i] + na[i]) > 0;
    const size_t n_win = (covered + window - 1) / window;
    cuts[0] = 0;
    size_t seen = 0, i = 0;
    for (int p = 1; p < parts; ++p) {
        const size_t want = (n_win * (size_t)p / (size_t)parts) * window;    /* covered rows before this cut */
        while (i < n && seen < want)
            seen += (nr[i] + na[i]) > 0, ++i;
        cuts[p] = want >= covered ? n : i;
    }
    cuts[parts] = n;
}

/* IBDGEM_TIMING=1 in the environment: wall-clock seconds per phase on stderr ("## time <phase> <s>") */
static int timing_on = -1;
static __thread double timing_last;             /* per thread: the pileups of a --pileup-list are read beside the device work */
static __thread const char *timing_tag;         /* --pileup-list: the pileup the phases belong to ("## time [NAME] ...") */
static double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
static void phase(const char *name)
{
    if (timing_on < 0) {
        const char *e = getenv("IBDGEM_TIMING");
        timing_on = e && *e && *e != '0';
        timing_last = now_s();
        if (timing_on) {
            /* what the loader and the libraries' initialisers took before main: now (since boot) minus the start
             * time of the process (field 22 of /proc/self/stat, in clock ticks since boot) */
            FILE *f = fopen("/proc/self/stat", "r");
            char buf[1024];
            if (f && fgets(buf, sizeof buf, f)) {
                const char *p = strrchr(buf, ')');
                unsigned long long ticks = 0;
                int field = 2;
                for (p = p ? p + 1 : buf; *p && field < 22; ++p)
                    if (*p == ' ')
                        ++field;
                if (sscanf(p, "%llu", &ticks) == 1) {
                    struct timespec ts;
                    clock_gettime(CLOCK_BOOTTIME, &ts);
                    const double since = (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec - (double)ticks / (double)sysconf(_SC_CLK_TCK);
                    fprintf(stderr, "## time process start to main %.4f\n", since > 0 ? since : 0.0);
                }
            }
            if (f)
                fclose(f);
        }
        return;
    }
    if (!timing_on)
        return;
    const double t = now_s();
    if (timing_tag)
        fprintf(stderr, "## time [%s] %s %.4f\n", timing_tag, name, t - timing_last);
    else
        fprintf(stderr, "## time %s %.4f\n", name, t - timing_last);
    timing_last = t;
}

/* a thread's phases start here, tagged with the pileup they belong to (NULL: untagged, a single -P run) */
static void phase_begin(const char *tag)
{
    timing_last = now_s();
    timing_tag = tag;
}


/* the row filter chain up to the read counts (src/ibdgem.c:589-626) for the rows [a, b) */
typedef struct {
    size_t a, b;
    const pileup_t *pu;
    const uint32_t *alt_count;
    unsigned n_ids;
    int in_vcf, has_p, has_A;
    cand_t *cand;               /* this range's candidates, from its own start */
    size_t n;
    uint8_t *row_fate;
} filter_job;

static void *filter_rows(void *arg)
{
    filter_job *j = arg;
    for (size_t r = j->a; r < j->b; ++r) {
        const row_t *R = &rows[r];
        j->row_fate[r] = 2;
        if (!R->hap_ok) { j->row_fate[r] = 0; continue; }
        if (!R->legend_ok) continue;
        const char *ref = arena + R->ref_off, *alt = arena + R->alt_off;
        if (!is_snp(ref, alt)) continue;
        if (j->in_vcf && R->qual < opt_min_qual) continue;                /* -q (src/ibdgem.c:297) */
        const pu_line *pl = pileup_find(j->pu, R->pos);
        if (!pl) continue;
        if (j->has_p && !pos_listed(R->pos)) continue;
        double f = (double)j->alt_count[r] / (int)(j->n_ids * 2);
        int ovr = 0;
        if (j->has_A) {
            const af_rec *a = find_af(R->pos);
            if (a) { f = a->f; ovr = 1; }
        }
        if (f > opt_max_af || f < opt_min_af) continue;
        const unsigned nr = pileup_count(pl, ref[0]), na = pileup_count(pl, alt[0]);
        if (nr + na > opt_max_cov) continue;
        cand_t *c = &j->cand[j->n++];
        c->row = (uint32_t)r; c->pu = (uint32_t)(pl - j->pu->lines); c->n_ref = (uint8_t)nr; c->n_alt = (uint8_t)na;
        c->f = f; c->f_is_override = ovr;
        j->row_fate[r] = 1;
    }
    return NULL;
}

/* ---- a non-LD comparison without a device (BASELINE configs[0]) -----------------------------------
 * The per-row columns (src/ibdgem.c:632-651) from the library's host twins of find_pDgG / find_pDgf /
 * find_pDgIBD1 -- the operations and the bits of the device kernel k_site -- and the window products
 * multiplied in row order (:665-667), rows without reads left out (:657-663). */
typedef struct {
    size_t a, b;
    const cand_t *cand;
    const uint32_t *s_cand;
    const uint8_t *s_nr, *s_na;
    const double *pdg;          /* ibdg_pdg_table */
    unsigned tgt;
    double *site_ll;
} host_site_job;

static void *host_site_rows(void *arg)
{
    host_site_job *j = arg;
    const size_t d = (size_t)opt_max_cov + 1;
    for (size_t i = j->a; i < j->b; ++i) {
        const cand_t *c = &j->cand[j->s_cand[i]];
        const double *p = j->pdg + ((size_t)j->s_nr[i] * d + j->s_na[i]) * 3;
        const unsigned a0 = row_allele(c->row, j->tgt, 0), a1 = row_allele(c->row, j->tgt, 1);
        j->site_ll[3 * i] = ibdg_pdg_ibd0(c->f, p[0], p[1], p[2]);
        j->site_ll[3 * i + 1] = ibdg_pdg_ibd1(a0, a1, c->f, p[0], p[1], p[2]);
        j->site_ll[3 * i + 2] = p[a0 + a1];                                  /* :643-651 */
    }
    return NULL;
}

static void host_nonld(const cand_t *cand, const uint32_t *s_cand, const uint8_t *s_nr, const uint8_t *s_na, size_t n,
                       unsigned tgt, const double *pdg, int threads, double *site_ll,
                       const uint32_t *w_first, const uint32_t *w_last, size_t n_win, double *win_ll, double *win_log)
{
    host_site_job jobs[64];
    pthread_t th[64];
    int T = threads < 1 ? 1 : threads > 64 ? 64 : threads;
    if (n < 65536)
        T = 1;
    for (int t = 0; t < T; ++t) {
        host_site_job *j = &jobs[t];
        j->a = n * (size_t)t / (size_t)T; j->b = n * (size_t)(t + 1) / (size_t)T;
        j->cand = cand; j->s_cand = s_cand; j->s_nr = s_nr; j->s_na = s_na; j->pdg = pdg; j->tgt = tgt;
        j->site_ll = site_ll;
        if (T == 1 || pthread_create(&th[t], NULL, host_site_rows, j) != 0) {
            host_site_rows(j);
            th[t] = pthread_self();
        }
    }
    for (int t = 0; t < T; ++t)
        if (!pthread_equal(th[t], pthread_self()))
            pthread_join(th[t], NULL);
    for (size_t w = 0; w < n_win; ++w) {
        double s0 = 1.0, s1 = 1.0, s2 = 1.0;                                  /* :562 */
        for (size_t i = w_first[w]; i <= w_last[w]; ++i) {
            if (s_nr[i] + s_na[i] == 0)
                continue;
            s0 *= site_ll[3 * i]; s1 *= site_ll[3 * i + 1]; s2 *= site_ll[3 * i + 2];
        }
        win_ll[3 * w] = s0; win_ll[3 * w + 1] = s1; win_ll[3 * w + 2] = s2;
        if (win_log) {                                                        /* --log-summary: long-double sums of log2l */
            long double l[3] = {0, 0, 0};
            for (size_t i = w_first[w]; i <= w_last[w]; ++i)
                if (s_nr[i] + s_na[i] != 0)
                    for (int k = 0; k < 3; ++k)
                        l[k] += log2l((long double)site_ll[3 * i + k]);
            for (int k = 0; k < 3; ++k)
                win_log[3 * w + k] = (double)l[k];
        }
    }
}

/* ---- the panel's way to the device(s) ---------------------------------------------------------------
 * One thread per device, all at once.  With one site list for all comparison individuals (no -v, no -D)
 * and several devices, a device receives only the panel rows of its window range (windows are independent,
 * reference src/ibdgem.c:558-570) and its sites are numbered from the slice's first row;
 * otherwise every device receives the whole panel.  The copies overlap the host's filter chain: the -F/-f
 * filter takes its alt-allele counts from the host side (ingest.c), not from a device. */
typedef struct {
    ibdg_ctx *eng;
    size_t r0, n;                /* panel rows [r0, r0 + n) */
    unsigned n_ids;
    const uint32_t *bg_idx;      /* --reference-order: the -B list in file order */
    size_t bg_n;
    int ref_order, has_B;
    int n_uploads;               /* uploads running at the same time */
    size_t share_sites;          /* --LD comparison individuals that will run on ONE site list (0: each its own) */
    int failed;
    pthread_t th;
    int started;
} upload_job;

static void *upload_run(void *arg)
{
    upload_job *j = arg;
    j->failed = 1;
    /* the per-site table needs LIBD0/1/2 of every row (its AF column the host has itself); --summary-only needs
     * nothing per row: the engine then neither keeps nor computes per-row results beyond the IBD2 pick */
    if (ibdg_set_option(j->eng, "site_results", opt_summary_only ? 0 : 1))
        return NULL;
    if (want_logs() && ibdg_set_option(j->eng, "log_windows", 1))
        return NULL;
    /* the uploads of all devices run side by side: each staging team gets its share of the host's threads (and locks
     * as much less memory: two 8 MB buffers per thread) */
    if (j->n_uploads > 1 && ibdg_set_option(j->eng, "stage_workers", j->n_uploads >= 8 ? 1 : 8 / j->n_uploads))
        return NULL;
    /* that many individuals over one site list pay for its compacted tiles several times over: have them from the
     * first batch on (left alone, the engine gets there by itself once its runs have added up: nine batches) */
    if (j->share_sites >= 240 && ibdg_set_option(j->eng, "compact_tiles", 1))
        return NULL;
    /* with a panel cache the engine reads the rows from the file itself (no mapping of 2.56 GB on this side) -- decided
     * by packed_fd alone: `packed` may be mapped by another thread at this very moment */
    if (packed_fd >= 0
            ? ibdg_upload_panel_fd(j->eng, packed_fd, packed_off + (uint64_t)j->r0 * row_words * 8, j->n, j->n_ids)
            : ibdg_upload_panel(j->eng, packed_rows() + j->r0 * row_words, j->n, j->n_ids))
        return NULL;
    if (j->ref_order) {                                   /* background list in the -B file's order (:741) */
        if (ibdg_set_option(j->eng, "ld_variant", 3) || (j->has_B && ibdg_set_background_order(j->eng, j->bg_idx, j->bg_n)))
            return NULL;
    }
    j->failed = 0;
    return NULL;
}

static void uploads_start(upload_job *u, int n)
{
    for (int d = 0; d < n; ++d) {
        u[d].started = pthread_create(&u[d].th, NULL, upload_run, &u[d]) == 0;
        if (!u[d].started)
            upload_run(&u[d]);
    }
}

/* returns the first device whose upload failed, or -1 */
static int uploads_join(upload_job *u, int n)
{
    int bad = -1;
    for (int d = 0; d < n; ++d) {
        if (u[d].started) {
            pthread_join(u[d].th, NULL);
            u[d].started = 0;
        }
        if (u[d].failed && bad < 0)
            bad = d;
    }
    return bad;
}

/* engine contexts created on a thread of their own while the main thread parses the inputs */
typedef struct {
    int dev[64], n;
    double eps;
    unsigned max_cov;
    ibdg_ctx *eng[64];
    char *err[64];
} dev_job_t;

static pthread_t g_dev_thread;
static int g_dev_started;
/* the panel uploads that run beside the filter chain (one thread per device, inside the GPU runtime) */
static upload_job g_ups[64];
static int g_n_ups, g_uploads_pending;
static void outs_settle(int failing);

/* exit() while another thread is inside the GPU runtime -- its start-up, a panel upload -- is asking for trouble (the
 * runtime's exit handlers would run under live GPU threads), and so is leaving while output threads are still writing:
 * wait for every thread this program started first.  On a failing exit the output files that were opened but not
 * yet emptied are emptied, so that no complete-looking table of an earlier run survives a run that failed. */
static void quit(int code)
{
    if (g_dev_started) {
        g_dev_started = 0;
        pthread_join(g_dev_thread, NULL);
    }
    if (g_uploads_pending) {
        g_uploads_pending = 0;
        (void)uploads_join(g_ups, g_n_ups);
    }
    outs_settle(code != 0);
    exit(code);
}

typedef struct {
    dev_job_t *job;
    int d;
} dev_one_t;

static void *dev_start_one(void *arg)
{
    dev_one_t *o = arg;
    dev_job_t *j = o->job;
    j->eng[o->d] = ibdg_create(j->dev[o->d], j->eps, j->max_cov);
    return NULL;
}

/* The first context brings the runtime up; the others (one per further device: each device's own start-up takes
 * about as long again) are created side by side.  A failure is reported with the engine's message, which is
 * per process: with several failing devices it is one of theirs. */
static void *dev_start(void *arg)
{
    dev_job_t *j = arg;
    dev_one_t one[64];
    pthread_t th[64];
    int started[64] = {0};
    if (j->n < 1)
        return NULL;
    one[0].job = j;
    one[0].d = 0;
    dev_start_one(&one[0]);
    if (!j->eng[0]) {
        j->err[0] = strdup(ibdg_last_error(NULL));
        return NULL;
    }
    for (int d = 1; d < j->n; ++d) {
        one[d].job = j;
        one[d].d = d;
        started[d] = pthread_create(&th[d], NULL, dev_start_one, &one[d]) == 0;
        if (!started[d])
            dev_start_one(&one[d]);
    }
    for (int d = 1; d < j->n; ++d)
        if (started[d])
            pthread_join(th[d], NULL);
    for (int d = 1; d < j->n; ++d)
        if (!j->eng[d]) {
            j->err[d] = strdup(ibdg_last_error(NULL));
            break;
        }
    return NULL;
}

#define TARGET_BATCH 30      /* comparison individuals per engine call when their site lists coincide: two groups of k_ld_mfma */
#define DIE(...)                          \
    do {                                  \
        fprintf(stderr, __VA_ARGS__);     \
        quit(1);                          \
    } while (0)

/* <out>/<pileup-name>.<individual>.<kind>.txt: the files of one comparison individual, in the order they are opened (the run's
 * own are RUN_FILES, further down).  RULE: every file is a row here, and a row is all it needs.  Each is opened without
 * truncation by the loop (outputs_open: giving back the pages of an earlier run's 330 MB table takes tens of milliseconds,
 * which belong to the output job, not between two engine calls), emptied by the job that writes it (outs_empty) or, when the
 * run fails before that, by outs_settle_one, and closed by its writer (out_close) or the job's tail (outs_close). */
enum { F_TAB, F_SUM, F_LSUM, F_HG, F_LP, F_LS, F_LSMP, F_LSW, N_IND_FILES };
static const struct {
    const char *kind;
    const int *on;          /* the option that turns it on (NULL: always) */
    const int *to_null;     /* the option that puts /dev/null in its place: nothing to list or to empty */
    int log;                /* with --log-stats the kind is log<kind> */
} IND_FILES[N_IND_FILES] = {
    [F_TAB] = {"tab", .to_null = &opt_summary_only},
    [F_SUM] = {"summary"},
    [F_LSUM] = {"logsummary", &opt_log_summary},
    [F_HG] = {"hiddengem", &opt_states, .log = 1},
    [F_LP] = {"logposteriors", &opt_posteriors},
    [F_LS] = {"logsegments", &opt_segments},
    [F_LSMP] = {"logsamples", &has_sample_paths},
    [F_LSW] = {"logswitches", &opt_switches},
};
static int ind_file_on(int k) { return !IND_FILES[k].on || *IND_FILES[k].on; }
static int ind_file_null(int k) { return IND_FILES[k].to_null && *IND_FILES[k].to_null; }

/* ---- the output files of one comparison individual (src/ibdgem.c:144-152, :547-548, :731-733, :751-768) --------------
 * Everything the files are made of, so that they can be written while the next individual is on the device: with the
 * site list shared by all individuals (no -v, no -D) a default run of many of them is bound by its 330 MB tables, and
 * tables of different individuals go into different files, which take writers side by side (tools/write_floor.c: one
 * file 3-6 GB/s whatever the number of writers, eight files 22-32 GB/s). */
typedef struct {
    /* shared with every other individual of the run (read only while a job runs) */
    const char *out_dir, *user_cmd;
    const unsigned long *in_dist;
    double mean_cov, cull_p;
    const cand_t *cand;
    const uint32_t *s_cand, *s_row;
    const uint8_t *s_nr, *s_na;
    const pileup_t *pu;
    /* this individual */
    const char *tname;
    uint32_t tgt;
    size_t n;
    unsigned long processed, skipped, final_total, final_dist[128];
    const double *site_ll;                      /* per-row values (NULL with --summary-only) */
    const char *pre;                            /* columns 1-9 of every row as text (row_prefix_build), or NULL */
    const uint32_t *pre_off;
    FILE *file[N_IND_FILES];                    /* the files of IND_FILES that are open (tab and summary: stdout with --plan); closed by the job */
    win_table wt;                               /* owned: freed when the files are closed */
    int threads;
    /* when it runs beside the main thread */
    pthread_t th;
    int running, failed;
    int pending;                                /* the files are open and still hold whatever an earlier run left in them */
    const unsigned long *pos_first, *pos_last;  /* shared: the windows' first / last positions of the common site list, or NULL */
    char *sum_buf;                              /* the slot's buffer for the text of a summary file (kept between individuals) */
    size_t sum_cap;
    const char *sq;                             /* the pileup's name (-N) */
    FILE *err;                                  /* where the pileup's messages go */
    /* --states */
    ind_stats *res;                             /* the individual's lines of the run's statistics files: the twin's results go here */
    uint64_t (*smp_tot)[9];                     /* --sample-paths: the run's totals [K][9], which the individual's draws are added to */
    struct sw_prior *swp;                       /* --switches: the prior of the site list all individuals share, or NULL (each its own) */
    struct fit_keep *fit;                       /* --fit-penalties on the host: where the job leaves a copy of its log table, or NULL */
    size_t ti;                                  /* ... and which of the run's individuals it is */
    hg_path hgp;                                /* the slot's path arrays and text buffer (kept between individuals) */
    char *hg_buf;
    size_t hg_cap;
} out_job;

/* --switches: the prior and the counted steps of a site list that every individual of the run shares, made by the first output
 * job that needs them */
struct sw_prior {
    int have;
    double prior[3];
    uint64_t counted[3];
};
static pthread_mutex_t g_sw_prior_lock = PTHREAD_MUTEX_INITIALIZER;

/* --fit-penalties where no context holds every individual's whole table (windows spread over several devices, or no device):
 * the run keeps a copy of every individual's gathered log table, 24 bytes per window and individual on the host (2.08 GB at
 * 34 599 windows x 2504), left here by the output jobs, and the chain starts and step shifts of the site list they share, left
 * by the first job that has them. */
struct fit_keep {
    double **tabs;                              /* [individuals]: each a job's copy, owned here */
    size_t n_win;
    int have_lc;
    uint32_t *starts;
    size_t n_starts;
    int32_t *shift;
};
static pthread_mutex_t g_fit_keep_lock = PTHREAD_MUTEX_INITIALIZER;

enum { OUT_SLOTS = 12, MAX_WORKERS = 64 };
static out_job g_outs[MAX_WORKERS][OUT_SLOTS];  /* per worker (one per context with --pileup-list, else one) */
static int g_n_workers = 1;

/* every open file of the job emptied (a /dev/null in a file's place cannot be); how many could not be */
static int outs_empty(out_job *o)
{
    int bad = 0;
    o->pending = 0;
    for (int k = 0; k < N_IND_FILES; ++k)
        if (o->file[k] && !ind_file_null(k))
            bad += ftruncate(fileno(o->file[k]), 0) != 0;
    return bad;
}

/* a file of the individual's, where there is one: closed, and forgotten by its job; 1: the close failed */
static int out_close(FILE **f)
{
    const int bad = *f && *f != stdout && fclose(*f) != 0;      /* (stdout: --plan's, not the job's to close) */
    *f = NULL;
    return bad;
}

/* every file of the job that is still open */
static int outs_close(out_job *o)
{
    int bad = 0;
    for (int k = 0; k < N_IND_FILES; ++k)
        bad |= out_close(&o->file[k]);
    return bad;
}

/* join a worker's output threads; when its run is failing, empty the files nobody got to */
static void outs_settle_one(out_job *outs, int failing)
{
    for (int k = 0; k < OUT_SLOTS; ++k) {
        out_job *o = &outs[k];
        if (o->running) {
            o->running = 0;
            pthread_join(o->th, NULL);
        }
        if (failing && o->pending && !opt_plan) {
            for (int bad = outs_empty(o); bad > 0; --bad)
                fprintf(stderr, "[::] WARNING: could not empty an output file of %s.\n", o->tname);
            outs_close(o);
        }
    }
}

/* see quit(): every worker's (they have all been joined by then) */
static void outs_settle(int failing)
{
    for (int w = 0; w < g_n_workers; ++w)
        outs_settle_one(g_outs[w], failing);
}

/* ---- --states: the individual's IBD-state path (hgpath.c), inside its output job --------------------------------------
 * The path is the one `hiddengem -s` finds in the individual's *.summary.txt, so every likelihood enters the recurrence
 * as that program would read it back: through the summary's own conversion (fmt_ll: "%e", "-nan") and strtod.  Taken
 * from the doubles, not from the summary's text: the same holds where no summary is written (--stats-only).  No row of
 * a summary this program writes is one sscanf passes over (two integers, three numbers or nan / inf, an integer). */
static double summary_round_trip(double v)
{
    char t[48];
    if (v == 0.0 && !signbit(v))
        return 0.0;
    fmt_ll(t, v, 0);
    return strtod(t, NULL);
}

typedef struct {
    const hg_path *h;
    size_t a, b;
    char *buf;
    size_t len;
} hg_fmt_job;

static void *fmt_states(void *arg)
{
    hg_fmt_job *j = arg;
    j->len = hg_format_rows(j->h, j->a, j->b, j->buf);
    return NULL;
}

static int write_all(int fd, const char *buf, size_t len)
{
    for (size_t off = 0; off < len;) {
        const ssize_t w = write(fd, buf + off, len - off);
        if (w < 0) {
            if (errno == EINTR)
                continue;
            return 1;
        }
        off += (size_t)w;
    }
    return 0;
}

/* the table of a solved path, its rows formatted by the job's team (three "%.5Le" per window: 20 ms of printf at
 * 35 000 windows on one thread) */
static int write_states_parallel(FILE *f, const hg_path *h, int threads, char **buf, size_t *cap)
{
    hg_fmt_job jobs[64];
    pthread_t tid[64];
    int started[64] = {0};
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    /* (IBDGEM_MT_MIN_BYTES below its default sends short tables through the team too: the tests' switch, as for the readers) */
    const int team = h->n < (ls_mt_min_bytes() < ((size_t)1 << 20) ? 16 : 2048) ? 1 : threads;
    if (*cap < h->n * HG_ROW_ROOM + 256) {
        free(*buf);
        *buf = malloc(h->n * HG_ROW_ROOM + 256);
        *cap = *buf ? h->n * HG_ROW_ROOM + 256 : 0;
    }
    if (!*buf)
        return 1;
    for (int t = 0; t < team; ++t) {
        jobs[t].h = h;
        jobs[t].a = h->n * (size_t)t / (size_t)team;
        jobs[t].b = h->n * (size_t)(t + 1) / (size_t)team;
        jobs[t].buf = *buf + jobs[t].a * HG_ROW_ROOM;
        jobs[t].len = 0;
    }
    for (int t = 0; t + 1 < team; ++t)
        started[t] = pthread_create(&tid[t], NULL, fmt_states, &jobs[t]) == 0;
    for (int t = 0; t < team; ++t)
        if (!started[t])
            fmt_states(&jobs[t]);
    for (int t = 0; t + 1 < team; ++t)
        if (started[t])
            pthread_join(tid[t], NULL);
    int rc = fputs(hg_header, f) < 0 || fflush(f) != 0;
    const int fd = fileno(f);
    for (int t = 0; t < team && !rc; ++t)
        rc = write_all(fd, jobs[t].buf, jobs[t].len);
    char *tail = *buf + h->n * HG_ROW_ROOM;
    return rc || write_all(fd, tail, hg_format_tail(h, tail));
}

/* --log-stats: the path over the individual's log2 table in integers (ibdg_log2_states_host: the same bytes as the device's
 * ibdg_window_log2_states), its scores printed in bits */
static const char log_hg_header[] = "Segment\tIBD0_LogScore\tIBD1_LogScore\tIBD2_LogScore\tInferred_State\n";

/* what the three passes over an individual's log2 table share: the positions of its windows (first [n], then last; for
 * --segments, --chain-gap and --switch-scale, else NULL), its chain starts (--chain-gap; none without it) and its step shifts
 * (--switch-scale; NULL without it) */
typedef struct {
    uint64_t *pos;
    uint32_t *starts;
    size_t n_starts;
    int32_t *shift;
} log_chains;

/* --posteriors: the sum-product pass over the same table (ibdg_log2_posteriors_steps_host: the same bytes as the device's
 * ibdg_window_log2_posteriors) */
static int posteriors_individual(out_job *o, const log_chains *lc)
{
    if (!opt_posteriors)
        return 0;
    const size_t n = o->wt.w.n_win;
    FILE *const out = o->file[F_LP];
    double *post = out ? malloc((n ? n : 1) * 3 * sizeof *post) : NULL;
    int bad = out && !post;
    if (!bad && ibdg_log2_posteriors_steps_host(o->wt.log, n, opt_p01, opt_p02, opt_p12, post, o->res->po, o->res->po + 3, lc->starts,
                                                lc->n_starts, lc->shift)) {
        fprintf(o->err, "%s\n", ibdg_last_error(NULL));
        bad = 1;
    }
    if (!bad && out) {
        bad = fputs("Segment\tPost_IBD0\tPost_IBD1\tPost_IBD2\tMax_State\n", out) < 0;
        for (size_t w = 0; w < n && !bad; ++w) {
            const double *g = post + 3 * w;
            int m = g[1] > g[0] ? 1 : 0;
            m = g[2] > g[m] ? 2 : m;
            bad = fprintf(out, "%d\t%.6f\t%.6f\t%.6f\t%d\n", (int)(w + 1), g[0], g[1], g[2], m) < 0;
        }
    }
    bad = out_close(&o->file[F_LP]) || bad;
    free(post);
    return bad;
}

/* --segments: the path's segments over the same table (ibdg_log2_segments_steps_host: the same bytes as the device's
 * ibdg_window_log2_segments), with the positions and site counts of the individual's summary; with --chain-gap a first column
 * Chain (1-based), counted along lc->starts */
static const char log_seg_header[] = "Segment\tState\tFirst_Window\tLast_Window\tStart\tEnd\tLength\tNum_Windows\tNum_Sites\t"
                                     "IBD0_LogSum\tIBD1_LogSum\tIBD2_LogSum\tLog2_LR";

static int segments_individual(out_job *o, const log_chains *lc)
{
    if (!opt_segments)
        return 0;
    const size_t n = o->wt.w.n_win;
    const uint64_t *pos = lc->pos;
    uint64_t n_seg = 0;
    FILE *const out = o->file[F_LS];
    ibdg_segment *seg = out ? malloc((n ? n : 1) * sizeof *seg) : NULL;
    int bad = out && !seg;
    if (!bad && ibdg_log2_segments_steps_host(o->wt.log, n, opt_p01, opt_p02, opt_p12, opt_posteriors, pos, pos + n, seg, n, &n_seg,
                                              o->res->sg, lc->starts, lc->n_starts, lc->shift)) {
        fprintf(o->err, "%s\n", ibdg_last_error(NULL));
        bad = 1;
    }
    if (!bad && out) {
        size_t chain = 0;                        /* the starts at or before the segment at hand */
        bad = fprintf(out, "%s%s%s\n", has_chain_gap ? "Chain\t" : "", log_seg_header, opt_posteriors ? "\tPost_Mean\tPost_Min" : "") < 0;
        for (size_t k = 0; k < n_seg && !bad; ++k) {
            const ibdg_segment *g = &seg[k];
            const size_t f = g->first, l = f + g->n_win - 1;
            const int64_t own = g->e[g->state], a = g->e[(g->state + 1) % 3], b = g->e[(g->state + 2) % 3];
            unsigned long sites = 0;
            for (size_t w = f; w <= l; ++w)
                sites += o->wt.w.ncov[w];
            while (chain < lc->n_starts && lc->starts[chain] <= f)
                ++chain;
            bad = has_chain_gap && fprintf(out, "%zu\t", chain + 1) < 0;
            bad = bad || fprintf(out, "%zu\t%u\t%zu\t%zu\t%llu\t%llu\t%llu\t%u\t%lu\t%.4Lf\t%.4Lf\t%.4Lf\t%.4Lf", k + 1, g->state, f + 1,
                          l + 1, (unsigned long long)pos[f], (unsigned long long)pos[n + l],
                          (unsigned long long)(pos[n + l] - pos[f] + 1), g->n_win, sites, (long double)g->e[0] / 65536,
                          (long double)g->e[1] / 65536, (long double)g->e[2] / 65536,
                          (long double)(own - (a > b ? a : b)) / 65536) < 0;
            if (!bad && opt_posteriors)
                bad = fprintf(out, "\t%.6Lf\t%.6f", (long double)g->post_q / ((long double)g->n_win * 4294967296.0L), g->post_min) < 0;
            bad = bad || fputc('\n', out) == EOF;
        }
    }
    bad = out_close(&o->file[F_LS]) || bad;
    free(seg);
    return bad;
}

/* --sample-paths: K paths drawn from the posterior over the same table (ibdg_log2_samples_host: the same bytes as the device's
 * ibdg_window_log2_samples), keyed by the individual's index in the panel; one row per draw goes to the individual's file, the
 * individual's row of the run's file is made here and its draws are added to the run's totals (sample_individual_row): the records
 * themselves do not outlive the job */
static int samples_individual(out_job *o, const log_chains *lc)
{
    if (!has_sample_paths)
        return 0;
    const size_t n = o->wt.w.n_win, K = opt_sample_paths;
    FILE *const out = o->file[F_LSMP];
    uint64_t *rec = malloc(K * 15 * sizeof *rec);
    int bad = !rec;
    if (bad)
        fprintf(o->err, "[::] ERROR: out of memory for %zu draws.\n", K);
    if (!bad && ibdg_log2_samples_host(o->wt.log, n, opt_p01, opt_p02, opt_p12, lc->starts, lc->n_starts, lc->shift, K, opt_seed, o->tgt,
                                       lc->pos, lc->pos + n, NULL, rec)) {
        fprintf(o->err, "%s\n", ibdg_last_error(NULL));
        bad = 1;
    }
    if (!bad && out) {
        bad = fputs("Sample\tWIN_IBD0\tWIN_IBD1\tWIN_IBD2\tSEG_IBD0\tSEG_IBD1\tSEG_IBD2\tBP_IBD0\tBP_IBD1\tBP_IBD2\t"
                    "LONGEST_BP_IBD0\tLONGEST_BP_IBD1\tLONGEST_BP_IBD2\n", out) < 0;
        for (size_t k = 0; k < K && !bad; ++k) {
            const uint64_t *r = rec + 15 * k;
            bad = fprintf(out, "%zu", k + 1) < 0;
            for (int i = 0; i < 15 && !bad; ++i)
                if (i < 6 || i >= 9)                 /* (the windows of the longest segments are not in this file) */
                    bad = fprintf(out, "\t%llu", (unsigned long long)r[i]) < 0;
            bad = bad || fputc('\n', out) == EOF;
        }
    }
    if (!bad && !(o->res->smp_row = sample_individual_row(rec, K, o->smp_tot))) {
        fprintf(o->err, "[::] ERROR: out of memory for %zu draws.\n", K);
        bad = 1;
    }
    free(rec);
    return out_close(&o->file[F_LSMP]) || bad;
}

/* --switches: the pairwise pass over the same table (ibdg_log2_switches_host: the same bytes as the device's
 * ibdg_window_log2_switches), and the prior of the individual's site list from the same twin on the table that says nothing:
 * once per run where the individuals share the list (o->swp), else once per individual */
static int switches_individual(out_job *o, const log_chains *lc)
{
    if (!opt_switches)
        return 0;
    const size_t n = o->wt.w.n_win;
    FILE *const out = o->file[F_LSW];
    double *sw = out ? malloc((n ? n : 1) * 3 * sizeof *sw) : NULL;
    uint64_t counted[3];
    int bad = out && !sw;
    if (!bad && ibdg_log2_switches_host(o->wt.log, n, opt_p01, opt_p02, opt_p12, lc->starts, lc->n_starts, lc->shift, sw, o->res->sw, counted)) {
        fprintf(o->err, "%s\n", ibdg_last_error(NULL));
        bad = 1;
    }
    if (!bad) {
        struct sw_prior own = {0}, *p = o->swp ? o->swp : &own;
        if (o->swp)
            pthread_mutex_lock(&g_sw_prior_lock);
        if (!p->have) {
            if (ibdg_log2_switches_host(NULL, n, opt_p01, opt_p02, opt_p12, lc->starts, lc->n_starts, lc->shift, NULL, p->prior, p->counted)) {
                fprintf(o->err, "%s\n", ibdg_last_error(NULL));
                bad = 1;
            } else {
                p->have = 1;
            }
        }
        memcpy(o->res->sw + 3, p->prior, sizeof p->prior);
        memcpy(o->res->swc, p->counted, sizeof p->counted);
        if (o->swp)
            pthread_mutex_unlock(&g_sw_prior_lock);
    }
    if (!bad && out) {
        bad = fputs("Segment\tSw_01\tSw_02\tSw_12\tP_Switch\n", out) < 0;
        for (size_t w = 0; w < n && !bad; ++w) {
            const double *g = sw + 3 * w;
            bad = fprintf(out, "%d\t%.6f\t%.6f\t%.6f\t%.6f\n", (int)(w + 1), g[0], g[1], g[2], (g[0] + g[1]) + g[2]) < 0;
        }
    }
    bad = out_close(&o->file[F_LSW]) || bad;
    free(sw);
    return bad;
}

/* --fit-penalties on the host: a copy of the individual's log table stays with the run (the table itself goes with the job), and
 * the list's chain starts and step shifts with the first job to come by */
static int fit_keep_individual(out_job *o, const log_chains *lc)
{
    struct fit_keep *k = o->fit;
    if (!k)
        return 0;
    const size_t n = o->wt.w.n_win, bytes = (n ? n : 1) * 3 * sizeof(double);
    double *tab = malloc(bytes);
    if (!tab) {
        fprintf(o->err, "[::] ERROR: out of memory for the log table of %s that --fit-penalties keeps (%zu bytes: 24 per window and individual).\n",
                o->tname, bytes);
        return 1;
    }
    memcpy(tab, o->wt.log, n * 3 * sizeof(double));
    int bad = 0;
    pthread_mutex_lock(&g_fit_keep_lock);
    if (!k->have_lc) {                          /* the first job to come by: the list's chain starts and step shifts, both or neither */
        const size_t n_starts = lc->starts ? lc->n_starts : 0;
        uint32_t *starts = n_starts ? malloc(n_starts * sizeof *starts) : NULL;
        int32_t *shift = lc->shift ? malloc((n ? n : 1) * sizeof *shift) : NULL;
        if ((n_starts && !starts) || (lc->shift && !shift)) {
            fprintf(o->err, "[::] ERROR: out of memory for the %zu chain starts and %zu step shifts that --fit-penalties keeps.\n", n_starts,
                    lc->shift ? n : (size_t)0);
            free(starts);
            free(shift);
            bad = 1;
        } else {
            if (n_starts) memcpy(starts, lc->starts, n_starts * sizeof *starts);
            if (shift) memcpy(shift, lc->shift, n * sizeof *shift);
            k->n_win = n; k->starts = starts; k->n_starts = n_starts; k->shift = shift;
            k->have_lc = 1;
        }
    }
    if (!bad && k->n_win != n) {
        fprintf(o->err, "[::] ERROR: --fit-penalties: %s has %zu windows, not the %zu of the individuals before it.\n", o->tname, n, k->n_win);
        bad = 1;
    }
    pthread_mutex_unlock(&g_fit_keep_lock);
    if (bad)
        free(tab);
    else
        k->tabs[o->ti] = tab;                   /* (the individual's own slot: no other job writes it) */
    return bad;
}

static int log_states_individual(out_job *o)
{
    const size_t n = o->wt.w.n_win;
    uint64_t *const count = o->res->st;
    FILE *const out = o->file[F_HG];
    uint8_t *path = out ? malloc(n ? n : 1) : NULL;
    int64_t *score = out ? malloc((n ? n : 1) * 3 * sizeof *score) : NULL;
    const int want_pos = opt_segments || has_chain_gap || has_switch_scale || has_sample_paths;
    log_chains lc = {want_pos ? malloc((2 * n + 1) * sizeof *lc.pos) : NULL, has_chain_gap ? malloc((n + 1) * sizeof *lc.starts) : NULL, 0,
                     has_switch_scale ? malloc((n + 1) * sizeof *lc.shift) : NULL};
    int bad = (out && (!path || !score)) || (want_pos && !lc.pos) || (has_chain_gap && !lc.starts) || (has_switch_scale && !lc.shift);
    for (size_t w = 0; w < n && want_pos && !bad; ++w) {
        lc.pos[w] = o->pos_first ? o->pos_first[w] : rows[o->s_row[o->wt.w.first[w]]].pos;
        lc.pos[n + w] = o->pos_last ? o->pos_last[w] : rows[o->s_row[o->wt.w.last[w]]].pos;
    }
    if (!bad && has_chain_gap)
        lc.n_starts = chain_gap_starts(lc.pos, lc.pos + n, n, lc.starts);
    if (!bad && has_switch_scale)
        switch_scale_shifts(lc.pos, lc.pos + n, n, lc.shift);
    if (!bad && ibdg_log2_states_steps_host(o->wt.log, n, opt_p01, opt_p02, opt_p12, path, score, count, lc.starts, lc.n_starts, lc.shift)) {
        fprintf(o->err, "%s\n", ibdg_last_error(NULL));
        bad = 1;
    }
    if (!bad && out) {
        hg_path tail = {.n = n, .count = {(size_t)count[0], (size_t)count[1], (size_t)count[2]}};
        char buf[256];
        bad = fputs(log_hg_header, out) < 0;
        for (size_t w = 0; w < n && !bad; ++w)
            bad = fprintf(out, "%d\t%.4Lf\t%.4Lf\t%.4Lf\t%d\n", (int)(w + 1), (long double)score[3 * w] / 65536,
                          (long double)score[3 * w + 1] / 65536, (long double)score[3 * w + 2] / 65536, path[w]) < 0;
        bad = bad || fwrite(buf, 1, hg_format_tail(&tail, buf), out) == 0;
    }
    bad = out_close(&o->file[F_HG]) || bad;
    free(path);
    free(score);
    if ((!want_pos || lc.pos) && (!has_chain_gap || lc.starts) && (!has_switch_scale || lc.shift)) {    /* (else out of memory: the other files are closed as they are) */
        bad = posteriors_individual(o, &lc) || bad;
        bad = segments_individual(o, &lc) || bad;
        bad = samples_individual(o, &lc) || bad;
        bad = switches_individual(o, &lc) || bad;
        bad = fit_keep_individual(o, &lc) || bad;
    }
    free(lc.pos);
    free(lc.starts);
    free(lc.shift);
    return bad;
}

/* 0: the path is found, counted for ibdstates.txt and (with a file of F_HG open) written and its file closed */
static int states_individual(out_job *o)
{
    if (opt_log_stats)
        return log_states_individual(o);
    hg_path *h = &o->hgp;
    hg_reset(h);
    for (size_t w = 0; w < o->wt.w.n_win; ++w)
        if (hg_add(h, summary_round_trip(o->wt.ll[3 * w]), summary_round_trip(o->wt.ll[3 * w + 1]),
                   summary_round_trip(o->wt.ll[3 * w + 2])))
            return 1;
    if (hg_solve(h, opt_p01, opt_p02, opt_p12))
        return 1;
    for (int s = 0; s < 3; ++s)
        o->res->st[s] = h->count[s];
    if (!o->file[F_HG])
        return 0;
    const int bad = write_states_parallel(o->file[F_HG], h, o->threads, &o->hg_buf, &o->hg_cap);
    return out_close(&o->file[F_HG]) || bad;
}

/* The job is a sequence of stages over one out_job, each returning 0, or 1 after its own message to the pileup's stream, and
 * one way out (output_individual).  The files were opened by the loop's thread: a directory that cannot be written stops the
 * run at once. */
#define OFAIL(...) do { fprintf(o->err, __VA_ARGS__); return 1; } while (0)

/* the files emptied, the command line (--plan: its own line in their place) and the header block (:144-152, :547-548) */
static int out_begin(out_job *o)
{
    FILE *const tab = o->file[F_TAB];
    if (opt_plan)
        printf("## PLAN %s %s processed=%lu skipped=%lu windows=%zu cull_p=%f\n", o->sq, o->tname, o->processed, o->skipped,
               o->wt.w.n_win, o->cull_p);
    else if (outs_empty(o))
        OFAIL("[::] ERROR in compare_impute(): Cannot empty the output files of %s.\n", o->tname);
    else
        fprintf(tab, "# Entered command: %s\n\n", o->user_cmd);
    fprintf(tab, "# INPUT COVERAGE DISTRIBUTION:\n# COVERAGE N_SITES\n");
    for (unsigned c = 0; c <= opt_max_cov; ++c)
        fprintf(tab, "# %d %lu\n", c, o->in_dist[c]);
    fprintf(tab, "# MEAN DEPTH = %lf\n# CULL DEPTH RATIO = %lf\n", o->mean_cov, o->cull_p);
    fprintf(tab, "# CHR\trsID\tPOS\tREF\tALT\tAF\tDP\tSQ_NREF\tSQ_NALT\tGT_A0\tGT_A1\tLIBD0\tLIBD1\tLIBD2\n");
    if (!opt_plan)
        fprintf(o->file[F_SUM], "# SEGMENT\tSTART\tEND\tLIBD0\tLIBD1\tLIBD2\tNUM_SITES\n");
    return 0;
}

/* the per-site rows (:731-733) */
static int out_rows(out_job *o)
{
    const fmt_job proto = {.cand = o->cand, .s_cand = o->s_cand, .pu = o->pu, .site_ll = o->site_ll, .s_nr = o->s_nr, .s_na = o->s_na,
                           .tgt = o->tgt, .plan = opt_plan, .pre = o->pre, .pre_off = o->pre_off};
    if (!opt_summary_only && write_rows_parallel(o->file[F_TAB], proto, o->n, o->threads))
        OFAIL("[::] ERROR writing the per-site rows of %s.\n", o->tname);
    return 0;
}

/* the summary rows (:751-756) through the program's own conversions, by the team of threads: with many comparison
 * individuals per run the seven stdio calls per window were the longest item of an individual (25 ms of 33 at 35 000
 * windows); --plan: the windows' lines in their place */
static int out_summaries(out_job *o)
{
    sum_job sj = {.s_row = o->s_row, .w_first = o->wt.w.first, .w_last = o->wt.w.last, .w_ncov = o->wt.w.ncov, .win_ll = o->wt.ll,
                  .pos_first = o->pos_first, .pos_last = o->pos_last};
    if (opt_plan) {
        for (size_t w = 0; w < o->wt.w.n_win; ++w)
            printf("## WINDOW %zu\t%lu\t%lu\t%u\n", w + 1, rows[o->s_row[o->wt.w.first[w]]].pos, rows[o->s_row[o->wt.w.last[w]]].pos,
                   o->wt.w.ncov[w]);
        return 0;
    }
    if (write_summary_parallel(o->file[F_SUM], sj, o->wt.w.n_win, o->threads, &o->sum_buf, &o->sum_cap))
        OFAIL("[::] ERROR writing the summary rows of %s.\n", o->tname);
    if (!o->file[F_LSUM])
        return 0;
    /* the same rows with the three likelihoods as log2: columns 1-3 and 7 through the same conversions */
    fprintf(o->file[F_LSUM], "# SEGMENT\tSTART\tEND\tLOG2_LIBD0\tLOG2_LIBD1\tLOG2_LIBD2\tNUM_SITES\n");
    sj.win_ll = o->wt.log;
    sj.logs = 1;
    if (write_summary_parallel(o->file[F_LSUM], sj, o->wt.w.n_win, o->threads, &o->sum_buf, &o->sum_cap))
        OFAIL("[::] ERROR writing the log summary rows of %s.\n", o->tname);
    return 0;
}

/* footer (:761-768) */
static int out_footer(out_job *o)
{
    FILE *const tab = o->file[F_TAB];
    fprintf(tab, "# FINAL COVERAGE DISTRIBUTION:\n# COVERAGE N_SITES\n");
    for (unsigned c = 0; c <= opt_max_cov; ++c)
        fprintf(tab, "# %d %lu\n", c, o->final_dist[c]);
    fprintf(tab, "# FINAL MEAN DEPTH = %lf\n", (double)o->final_total / o->processed);
    fprintf(tab, "## Number of sites processed: %lu\n", o->processed);
    fprintf(tab, "## Number of sites skipped: %lu\n", o->skipped);
    return 0;
}

static void *output_individual(void *arg)
{
    out_job *o = arg;
    /* (--stats-only --states: the path's counts alone, no file of the individual's is open) */
    int bad = !opt_stats_only && (out_begin(o) || out_rows(o) || out_summaries(o) || out_footer(o));
    if (!bad && opt_states && states_individual(o)) {
        fprintf(o->err, opt_stats_only ? "[::] ERROR finding the IBD states of %s.\n" : "[::] ERROR writing the IBD-state path of %s.\n", o->tname);
        bad = 1;
    }
    /* the one way out, of a job that failed as well: whatever is still open is closed, the window table given back */
    bad = outs_close(o) || bad;
    win_table_free(&o->wt);
    o->failed = bad;
    return NULL;
}

/* ---- one pileup of the run: -P, or an entry of --pileup-list ----------------------------------------------------------
 * What belongs to the pileup -- its lines, coverage histogram and cull ratio, the target-independent part of the filter
 * chain, the site lists and output files of its comparisons -- lives in a pile_job; what belongs to the panel -- names,
 * genotype rows, the device contexts with the panel on them, alt counts -- is set up once by main.  A list is worked
 * through by one worker per context (one without a device); a worker reads and filters its next pileup on threads of
 * their own while it runs the one at hand, and no further ahead.  Every pileup's messages go to a buffer of its own,
 * printed in list order once it is done (a single -P run writes them to stderr as they come). */
typedef struct {
    const char *name, *path;       /* -N, -P */
    FILE *err;
    char *err_buf;
    size_t err_len;
    pileup_t *pu;
    long pu_id;                    /* the pileup's own name in the panel: left out of its background (:501-506) */
    unsigned long in_dist[128];
    double mean_cov, cull_p;
    cand_t *cand;                  /* the rows that passed the target-independent filters */
    uint8_t *row_fate;
    size_t n_cand;
    int rc;                        /* 0: fine so far; 1: failed; -1: not run (an earlier entry failed) */
    int done;
    char **files;                  /* --pileup-list: the output files it wrote */
    size_t n_files;
} pile_job;

static names_t g_ids;
static idlist_t g_targets;
static uint8_t *g_bg_count;
static const char *g_out_dir, *g_user_cmd, *g_uchr;
static int g_no_engine, g_host_math, g_list_mode;
static double *g_pdg_tab;

static struct {
    pile_job *jobs;
    size_t n;
    size_t next_take;              /* the next entry a worker takes */
    size_t next_print;             /* the next entry whose messages go to stderr */
    size_t fail_at;                /* the first entry that failed (n: none) */
    pthread_mutex_t mu;
} g_list = {NULL, 0, 0, 0, 0, PTHREAD_MUTEX_INITIALIZER};

/* host threads for one pileup's reading, filter chain and files: all of them, or with several contexts working through a list
 * side by side each worker's share of them */
static int g_thread_share;
static int all_threads(void)
{
    return g_thread_share > 0 ? g_thread_share : opt_threads > 0 ? opt_threads : default_threads();
}

/* --pileup-list FILE: "NAME PATH" per line, '#' lines and blank lines skipped.  Refusals exit(1) with one line. */
static void read_pileup_list(const char *fn, pile_job **out, size_t *n_out)
{
    FILE *f = fopen(fn, "r");
    if (!f) {
        fprintf(stderr, "[::] ERROR: Cannot open the pileup list '%s'.\n", fn);
        exit(1);
    }
    pile_job *jobs = NULL;
    size_t n = 0, cap = 0, ln = 0, lcap = 0;
    size_t *line_of = NULL;
    char *line = NULL;
    while (getline(&line, &lcap, f) >= 0) {
        ++ln;
        char *p = line;
        while (isspace((unsigned char)*p))
            ++p;
        if (!*p || *p == '#')
            continue;
        char *save = NULL, *name = strtok_r(p, " \t\r\n", &save), *path = strtok_r(NULL, " \t\r\n", &save);
        if (!name || !path || strtok_r(NULL, " \t\r\n", &save)) {
            fprintf(stderr, "[::] ERROR: Line %zu of the pileup list '%s' is not 'NAME PATH'.\n", ln, fn);
            exit(1);
        }
        for (size_t i = 0; i < n; ++i)
            if (strcmp(jobs[i].name, name) == 0) {
                fprintf(stderr, "[::] ERROR: Pileup name '%s' appears twice in the pileup list '%s' (lines %zu and %zu).\n", name,
                        fn, line_of[i], ln);
                exit(1);
            }
        if (n == cap) {
            cap = cap ? 2 * cap : 16;
            jobs = ls_xrealloc(jobs, cap * sizeof *jobs);
            line_of = ls_xrealloc(line_of, cap * sizeof *line_of);
        }
        memset(&jobs[n], 0, sizeof jobs[n]);
        jobs[n].name = strdup(name);
        jobs[n].path = strdup(path);
        line_of[n++] = ln;
    }
    free(line);
    free(line_of);
    fclose(f);
    if (n == 0) {
        fprintf(stderr, "[::] ERROR: The pileup list '%s' names no pileup.\n", fn);
        exit(1);
    }
    *out = jobs;
    *n_out = n;
}

/* the pileup itself (src/ibdgem.c:1001-1010) */
static void pj_read(pile_job *pj)
{
    pj->pu = pileup_read_mt_to(pj->path, g_uchr, all_threads(), pj->err);
    if (!pj->pu) {
        fprintf(pj->err, "[::] ERROR parsing Pileup data; make sure input is valid.\n");
        pj->rc = 1;
    }
}

/* input coverage distribution and cull ratio: find_cull_p (:83-106) */
static void pj_depth(pile_job *pj)
{
    const pileup_t *pu = pj->pu;
    unsigned long in_total = 0;
    memset(pj->in_dist, 0, sizeof pj->in_dist);
    for (size_t i = 0; i < pu->n_lines; ++i)
        if (pu->lines[i].cov <= opt_max_cov) {
            in_total += pu->lines[i].cov;
            pj->in_dist[pu->lines[i].cov]++;
        }
    pj->mean_cov = (double)in_total / pu->n_lines;
    pj->cull_p = 1;
    if (has_D) {
        if (opt_target_dp > pj->mean_cov)
            fprintf(pj->err, "Observed depth is lower than target depth -D. No culling will be done.\n");
        else
            pj->cull_p = opt_target_dp / pj->mean_cov;
    }
}

/* ---- target-independent part of the row filter chain (:589-626) -------------------
 * Rows are independent here: a team of threads takes contiguous row ranges, each fills its own part
 * of cand[] from the range's first row on, and the parts are closed up in order afterwards. */
static void pj_filter(pile_job *pj)
{
    pj->pu_id = find_name(&g_ids, pj->name);
    cand_t *cand = pj->cand = malloc((n_rows ? n_rows : 1) * sizeof *cand);
    uint8_t *row_fate = pj->row_fate = calloc(n_rows ? n_rows : 1, 1);   /* 0 skip-before-v, 1 candidate, 2 skipped after the -v test */
    if (!cand || !row_fate) {
        fprintf(pj->err, "[::] ERROR: out of memory for %zu rows.\n", n_rows);
        pj->rc = 1;
        return;
    }
    size_t n_cand = 0;
    int T = all_threads();
    if (T > 64) T = 64;
    if (n_rows * 64 < ls_mt_min_bytes()) T = 1;           /* small inputs (and the tests, unless they ask) on one thread */
    filter_job fj[64];
    pthread_t th[64];
    for (int t = 0; t < T; ++t) {
        filter_job *j = &fj[t];
        j->a = n_rows * (size_t)t / (size_t)T;
        j->b = n_rows * (size_t)(t + 1) / (size_t)T;
        j->pu = pj->pu; j->alt_count = alt_count_h; j->n_ids = (unsigned)g_ids.n; j->in_vcf = in_vcf; j->has_p = has_p;
        j->has_A = has_A;
        j->cand = cand + j->a; j->row_fate = row_fate; j->n = 0;
        if (T == 1 || pthread_create(&th[t], NULL, filter_rows, j) != 0) {
            filter_rows(j);
            th[t] = pthread_self();
        }
    }
    for (int t = 0; t < T; ++t) {
        if (!pthread_equal(th[t], pthread_self()))
            pthread_join(th[t], NULL);
        if (fj[t].cand != cand + n_cand)
            memmove(cand + n_cand, fj[t].cand, fj[t].n * sizeof *cand);
        n_cand += fj[t].n;
    }
    pj->n_cand = n_cand;
}

/* a list entry after the first: read and filtered on a thread of its own while its worker runs the entry before it */
static void *pj_prepare(void *arg)
{
    pile_job *pj = arg;
    phase_begin(pj->name);
    pj_read(pj);
    if (!pj->rc)
        pj_depth(pj);
    phase("pileup");
    if (!pj->rc)
        pj_filter(pj);
    phase("row filter chain");
    return NULL;
}

/* what a pileup holds once its files are written (a list keeps host memory to two pileups per worker) */
static void pj_release(pile_job *pj)
{
    pileup_free(pj->pu);
    free(pj->cand);
    free(pj->row_fate);
    pj->pu = NULL;
    pj->cand = NULL;
    pj->row_fate = NULL;
}

static void pj_add_file(pile_job *pj, const char *fn)
{
    if (!g_list_mode)
        return;
    pj->files = ls_xrealloc(pj->files, (pj->n_files + 1) * sizeof *pj->files);
    pj->files[pj->n_files++] = strdup(fn);
}

/* the next entry for a worker, -1 when there is none or an entry has failed */
static long list_take(void)
{
    pthread_mutex_lock(&g_list.mu);
    long i = -1;
    if (g_list.fail_at == g_list.n && g_list.next_take < g_list.n)
        i = (long)g_list.next_take++;
    pthread_mutex_unlock(&g_list.mu);
    return i;
}

static int list_failed_before(size_t i)
{
    pthread_mutex_lock(&g_list.mu);
    const int f = g_list.fail_at < i;
    pthread_mutex_unlock(&g_list.mu);
    return f;
}

/* an entry is done: its messages, and those of the done entries after it, go to stderr in list order (up to and including a
 * failed entry: nothing of the entries after it is printed) */
static void list_finish(size_t i, int rc)
{
    pthread_mutex_lock(&g_list.mu);
    pile_job *pj = &g_list.jobs[i];
    pj->rc = rc;
    pj->done = 1;
    if (rc > 0 && i < g_list.fail_at)
        g_list.fail_at = i;
    while (g_list.next_print < g_list.n && g_list.jobs[g_list.next_print].done && g_list.next_print <= g_list.fail_at) {
        pile_job *q = &g_list.jobs[g_list.next_print++];
        if (q->err != stderr) {
            fclose(q->err);                               /* (its output threads have all been joined) */
            q->err = NULL;
            if (q->err_len)
                fwrite(q->err_buf, 1, q->err_len, stderr);
            fflush(stderr);
            free(q->err_buf);
            q->err_buf = NULL;
        }
    }
    pthread_mutex_unlock(&g_list.mu);
}

/* a worker: the contexts it drives (all of them for a single -P run, one for a list), their panel uploads and its output slots */
typedef struct {
    dev_conv conv[64];             /* per context: the context and the conversation with it */
    int n_eng;
    upload_job *ups;
    int n_ups, ups_pending;
    int slice_mode;
    out_job *outs;
    long first;                    /* its first entry, handed out before any worker starts (-1: none) */
    int first_ready;               /* ... already read and filtered (by main) */
    pthread_t th;
    int started;
} worker_t;

/* ---- the run of one pileup over its comparison individuals (:522-773) -------------------------------------------------
 * pj_run is the loop; what it does is a sequence of stage functions over one pile_run, each returning 0, or 1 after its own
 * message to the pileup's stream.  The state is grouped by what replaces it:
 *   the pileup's run -- decided (run_modes) or set up (run_begin, candidates_to_device) once, given back by run_release;
 *   the site list at hand -- RULE: rebuilt exactly when the site list changes.  It changes for every comparison individual
 *     with -v or -D and for the first one alone otherwise (one_list).  site_list_reset drops the whole group, the site_list
 *     stage fills the list, and what is derived from it is made by its stage on first need and kept until the next reset;
 *   the comparison individual -- set by the loop, its window table handed to its output job. */
typedef struct {
    uint32_t *s_row, *s_cand;       /* the list: arrays of the pileup's candidate count (run_begin), n entries filled per list */
    uint8_t *s_nr, *s_na;
    double *s_fo;
    size_t n, n_gt_failed;
    unsigned long skipped, final_total, final_dist[128];
    int cuts_made;                  /* derived, engine path: the list cut into one window range per device (window_cuts) */
    size_t cuts[65];
    uint32_t *s_row_dev;            /* derived, slice_mode: the site list's rows counted from each device's first row */
    /* derived, --arm-stats on the engine path: the windows the arms were cut from (checked against the engine's), the windows
     * per device and the arms in each device's own window indices */
    uint32_t *arm_wfirst, *arm_wlast, arm_wcut[65], arm_local[64][4];
    size_t arm_nw;
    int arm_ok[2];
    /* derived: the positions a summary row names (:751-756) are the same for every individual over a common site list: looked
     * up once -- row by row they are two dependent loads into 160 MB of row records per window and individual */
    unsigned long *sum_pos_first, *sum_pos_last;
    size_t sum_pos_n;
    int sum_pos_made;
    char *row_pre;                  /* derived: columns 1-9 of every row as text, shared by all individuals' tables */
    uint32_t *row_pre_off;
} site_list;

enum { N_RUN_FILES = 6 };           /* RUN_FILES below */

typedef struct {
    /* ---- the pileup's run ---- */
    pile_job *pj;
    worker_t *w;
    FILE *err;
    int one_list;                   /* no -v, no -D: the site list does not depend on the comparison individual (:584, :627-628) */
    int overlap, dev_v, batchable, arm_on, tables_stay, dev_states, out_slots, out_threads_env;
    size_t n_site_out;              /* entries of an individual's per-site array */
    ind_stats *res;                 /* per individual, what the run's statistics files are written from (run_end) */
    struct sw_prior sw_prior;       /* --switches: the shared site list's prior, made by the first output job */
    /* --fit-penalties: on the device where one context holds every individual's whole table (fit_dev: its store), else over
     * the copies the output jobs leave in fit_keep; the iterations' rows and the verdict, made by run_end before the files */
    int fit_dev;
    struct fit_keep fit_keep;
    ibdg_fit_row *fit_rows;
    size_t fit_n;
    int fit_stood;
    double fitted[3];
    uint64_t (*smp_tot)[9], *smp_col;   /* --sample-paths: draw k summed over the individuals so far [K][9]; scratch [K] for their columns */
    FILE *run_file[N_RUN_FILES];    /* the files of RUN_FILES, open from run_begin to run_end */
    char *run_fn[N_RUN_FILES];
    double *site_slot[OUT_SLOTS];   /* the per-site array of each output slot */
    uint32_t *c_row;                /* dev_v: the candidates as the engine takes them */
    uint8_t *c_nr, *c_na;
    double *c_fo;
    size_t c_gt_failed;             /* ... and how many of the rows before the -v test have genotypes that did not parse */
    /* ---- the site list at hand ---- */
    site_list sl;
    /* ---- the comparison individual ---- */
    size_t ti;
    uint32_t tgt;
    const char *tname;
    int same_sites;                 /* it runs over the site list of the one before it */
    win_table wt;                   /* owned here until its output job takes it */
    double *site_ll;                /* its slot's per-site array */
} pile_run;

/* a stage's failing exit: its message to the pileup's stream, 1 to pj_run */
#define SFAIL(...) do { fprintf(r->err, __VA_ARGS__); return 1; } while (0)

static void run_modes(pile_run *r)
{
    const int no_engine = g_no_engine;
    r->one_list = !has_v && r->pj->cull_p == 1.0;
    r->batchable = !no_engine && r->one_list;
    /* the per-site values are only fetched for the per-site table: no 128 MB of page-locked memory for --summary-only */
    r->n_site_out = opt_summary_only && !no_engine ? 1 : (r->pj->n_cand ? r->pj->n_cand : 1);
    /* The files of up to out_slots individuals are written beside the main thread's work on the ones after them, each from
     * a per-row array of its own -- when the site list is the same for all of them (it is read by the writers), the rows go
     * to files (stdout keeps its order) and there is a table to write at all. */
    /* (--summary-only: the summary files alone, 2.5 MB each at 35 000 windows -- 1.5 ms per individual when written one
     * after the other, most of a whole-panel job whose engine time is 0.2 ms per individual) */
    r->overlap = r->one_list && !opt_plan && g_targets.n > 1;
    /* -v with one context and no -D: the rows that passed every filter but :584 are the pileup's; they go to the device once
     * (ibdg_upload_candidates) and every individual's list is cut from them there (ibdg_select_variable_sites) -- the host
     * walks the selected rows only: 3.5 ms per individual at 4M rows x 2504 where the scan of all rows took 58
     * (profiles/r09_variable_sites.txt).  (IBDGEM_VARSITES=host: the host's own scan, for the tests and for measurements.) */
    const char *vs_env = has_v ? getenv("IBDGEM_VARSITES") : NULL;
    r->dev_v = has_v && !no_engine && r->w->n_eng == 1 && g_n_ups == 1 && r->pj->cull_p == 1.0 && !(vs_env && !strcmp(vs_env, "host"));
    /* (--summary-only: 2.5 MB per individual instead of 330: twelve individuals at a time with four formatter threads each --
     * 0.52 ms per individual in a run of 960 against 0.65 with six and eight, 0.90 with four, tools/many_summaries.py) */
    r->out_slots = opt_summary_only ? 12 : 4;
    /* (IBDGEM_OUT_SLOTS=1..12, default 4, 12 with --summary-only: for the tests and for measurements) */
    if (getenv("IBDGEM_OUT_SLOTS") && atoi(getenv("IBDGEM_OUT_SLOTS")) >= 1 && atoi(getenv("IBDGEM_OUT_SLOTS")) <= OUT_SLOTS)
        r->out_slots = atoi(getenv("IBDGEM_OUT_SLOTS"));
    r->out_threads_env = getenv("IBDGEM_OUT_THREADS") ? atoi(getenv("IBDGEM_OUT_THREADS")) : 0;   /* (measurement switch) */
    r->arm_on = has_arm && !opt_plan;
    /* --stats-only keeps the window tables on the device unless the states are asked for: the path is found on the host */
    r->tables_stay = opt_stats_only && !opt_states;
    /* ... or in the log domain (--log-stats), where one context has the whole table and finds the paths itself */
    r->dev_states = opt_stats_only && opt_states && opt_log_stats && !no_engine && r->w->n_eng == 1;
    r->tables_stay = r->tables_stay || r->dev_states;
    /* --fit-penalties: one context holds every individual's whole table over the one site list (-v and -D are refused) and
     * keeps them in its store; windows spread over several contexts, or no device, leave the tables to the host */
    r->fit_dev = has_fit && !no_engine && r->w->n_eng == 1 && r->one_list;
    for (int d = 0; d < r->w->n_eng; ++d) {      /* what the conversation with each context takes from these */
        dev_conv *c = &r->w->conv[d];
        c->err = r->err; c->bg_count = g_bg_count; c->pu_id = (int)r->pj->pu_id; c->reported = 0;
        c->fit_store = r->fit_dev; c->fit_reserve = g_targets.n;
        c->shared_list = r->batchable; c->list_on_device = r->dev_v;
        c->tables_stay = r->tables_stay; c->dev_states = r->dev_states;
    }
}

/* ---- the statistics files a run writes once, after its last individual, from the individuals' records (r->res) ---- */

/* one line per comparison individual in the order of the summaries, as bin/sum-hiddengem.py prints a row, then its totals over
 * the pileup's individuals */
static void write_states_file(pile_run *r, FILE *f)
{
    size_t total[3] = {0, 0, 0};
    fprintf(f, "# ID\tN_SEGMENTS\tN_IBD0\tN_IBD1\tN_IBD2\tFRAC_IBD0\tFRAC_IBD1\tFRAC_IBD2\n");
    for (size_t ti = 0; ti < g_targets.n; ++ti) {
        const uint64_t *st = r->res[ti].st;
        const size_t count[3] = {(size_t)st[0], (size_t)st[1], (size_t)st[2]};
        hg_frac_row(f, g_ids.names[g_targets.idx[ti]], count);
        for (int k = 0; k < 3; ++k)
            total[k] += count[k];
    }
    hg_frac_totals(f, total);
}

/* likewise, laid out like the fractions file: the expected windows per state where that one has counts, and log2 Z */
static void write_posteriors_file(pile_run *r, FILE *f)
{
    double total[3] = {0.0, 0.0, 0.0};
    size_t total_n = 0;
    fprintf(f, "# ID\tN_SEGMENTS\tE_IBD0\tE_IBD1\tE_IBD2\tFRAC_IBD0\tFRAC_IBD1\tFRAC_IBD2\tLOG2_Z\n");
    for (size_t ti = 0; ti < g_targets.n; ++ti) {
        const double *e = r->res[ti].po;
        const size_t n = (size_t)(r->res[ti].st[0] + r->res[ti].st[1] + r->res[ti].st[2]);
        fprintf(f, "%s\t%zu\t%.3f\t%.3f\t%.3f", g_ids.names[g_targets.idx[ti]], n, e[0], e[1], e[2]);
        for (int k = 0; k < 3; ++k) {
            if (n)
                fprintf(f, "\t%.6f", e[k] / (double)n);
            else
                fputs("\tnan", f);
            total[k] += e[k];
        }
        fprintf(f, "\t%.6f\n", e[3]);
        total_n += n;
    }
    fprintf(f, "# Total segments = %zu\n", total_n);
    for (int k = 0; k < 3; ++k) {
        if (total_n)
            fprintf(f, "# Total E_IBD%d = %.3f (%.3f %%)\n", k, total[k], total[k] / (double)total_n * 100);
        else
            fprintf(f, "# Total E_IBD%d = %.3f (nan %%)\n", k, total[k]);
    }
}

/* likewise: per individual and state the four numbers of its segments, then the totals (sums of the counts and base pairs,
 * maxima of the two longest) */
static void write_segments_file(pile_run *r, FILE *f)
{
    static const char *const col[4] = {"N_SEG", "LONGEST_WIN", "TOTAL_BP", "LONGEST_BP"};
    uint64_t total[12] = {0};
    fputs("# ID", f);
    for (int s = 0; s < 3; ++s)
        for (int k = 0; k < 4; ++k)
            fprintf(f, "\tIBD%d_%s", s, col[k]);
    fputc('\n', f);
    for (size_t ti = 0; ti < g_targets.n; ++ti) {
        const uint64_t *g = r->res[ti].sg;
        fputs(g_ids.names[g_targets.idx[ti]], f);
        for (int s = 0; s < 3; ++s)
            for (int k = 0; k < 4; ++k) {
                const uint64_t v = g[3 * k + s];
                fprintf(f, "\t%llu", (unsigned long long)v);
                total[3 * k + s] = k & 1 ? (v > total[3 * k + s] ? v : total[3 * k + s]) : total[3 * k + s] + v;
            }
        fputc('\n', f);
    }
    for (int s = 0; s < 3; ++s)
        fprintf(f, "# Total IBD%d: N_SEG = %llu, LONGEST_WIN = %llu, TOTAL_BP = %llu, LONGEST_BP = %llu\n", s,
                (unsigned long long)total[s], (unsigned long long)total[3 + s], (unsigned long long)total[6 + s],
                (unsigned long long)total[9 + s]);
}

/* likewise: per individual its row -- its text was made when the individual's draws were done (sample_individual_row) --, then
 * the totals' from the run's sums of draw k over the individuals: the same statistics (the draws of different individuals are
 * independent) */
static void write_samples_file(pile_run *r, FILE *f)
{
    static const char *const what[3] = {"WIN", "SEG", "BP"}, *const stat[4] = {"MEAN", "Q025", "Q500", "Q975"};
    const size_t K = opt_sample_paths;
    char tail[SMP_ROW_ROOM];
    size_t total_n = 0;
    fputs("# ID\tN_SEGMENTS\tK", f);
    for (int s = 0; s < 3; ++s)
        for (int q = 0; q < 3; ++q)
            for (int k = 0; k < 4; ++k)
                fprintf(f, "\tIBD%d_%s_%s", s, what[q], stat[k]);
    fputs("\tP_ANY_IBD12\n", f);
    for (size_t ti = 0; ti < g_targets.n; ++ti) {
        const size_t n = (size_t)(r->res[ti].st[0] + r->res[ti].st[1] + r->res[ti].st[2]);
        if (!r->res[ti].smp_row)
            continue;                             /* (an individual whose job failed: the run is failing, and has said so) */
        fprintf(f, "%s\t%zu\t%zu%s", g_ids.names[g_targets.idx[ti]], n, K, r->res[ti].smp_row);
        total_n += n;
    }
    sample_row_tail(tail, (const uint64_t (*)[9])r->smp_tot, K, r->smp_col);
    fprintf(f, "# Total\t%zu\t%zu%s", total_n, K, tail);
}

/* likewise: per individual the expected switches that pay each penalty, their totals added in the order of the panel, the
 * expectation of one individual under the penalties alone, the steps counted, the penalties used and the ones the update
 * suggests (ibdg_switch_penalty_update over the file's individuals).  The prior and the counted steps belong to the site list:
 * with a list per individual (-v, -D) the prior shown is the individuals' sum in the order of the panel, the counted steps
 * likewise, and the update takes that sum as the prior of one. */
static void write_switches_file(pile_run *r, FILE *f)
{
    double total[3] = {0.0, 0.0, 0.0}, prior[3] = {0.0, 0.0, 0.0}, next[3];
    const double p[3] = {opt_p01, opt_p02, opt_p12};
    uint64_t counted[3] = {0, 0, 0};
    const size_t T = g_targets.n;
    int same = 1;
    fprintf(f, "# ID\tN_WIN\tE_SW01\tE_SW02\tE_SW12\n");
    for (size_t ti = 0; ti < T; ++ti) {
        const ind_stats *s = &r->res[ti];
        const size_t n = (size_t)(s->st[0] + s->st[1] + s->st[2]);
        fprintf(f, "%s\t%zu\t%.6f\t%.6f\t%.6f\n", g_ids.names[g_targets.idx[ti]], n, s->sw[0], s->sw[1], s->sw[2]);
        same = same && !memcmp(s->sw + 3, r->res[0].sw + 3, 3 * sizeof(double)) && !memcmp(s->swc, r->res[0].swc, sizeof s->swc);
        for (int k = 0; k < 3; ++k) {
            total[k] += s->sw[k];
            prior[k] += s->sw[3 + k];
            counted[k] += s->swc[k];
        }
    }
    if (same && T) {
        memcpy(prior, r->res[0].sw + 3, sizeof prior);
        memcpy(counted, r->res[0].swc, sizeof counted);
    }
    ibdg_switch_penalty_update(p, total, same ? T : 1, prior, next);
    fprintf(f, "# Total\t%.6f\t%.6f\t%.6f\n", total[0], total[1], total[2]);
    fprintf(f, "# Prior%s\t%.6f\t%.6f\t%.6f\n", same ? "" : " (sum over the individuals' own site lists)", prior[0], prior[1], prior[2]);
    fprintf(f, "# Counted\t%llu\t%llu\t%llu\n", (unsigned long long)counted[0], (unsigned long long)counted[1], (unsigned long long)counted[2]);
    fprintf(f, "# Penalties\t%.6e\t%.6e\t%.6e\n", p[0], p[1], p[2]);
    fprintf(f, "# Next\t%.6e\t%.6e\t%.6e\n", next[0], next[1], next[2]);
}

/* --fit-penalties: a row per iteration made (run_fit, before the files), with the penalties it used, the individuals' total, one
 * individual's prior, the counted steps and total / (T * prior) -- nan where the update keeps p --, then the verdict and the
 * fitted penalties with the digits that give the doubles back */
static void write_fit_file(pile_run *r, FILE *f)
{
    const size_t T = g_targets.n;
    fprintf(f, "# Iteration\tP01\tP02\tP12\tE_SW01\tE_SW02\tE_SW12\tPRIOR01\tPRIOR02\tPRIOR12\tCOUNTED01\tCOUNTED02\tCOUNTED12\tRATIO01\tRATIO02\tRATIO12\n");
    for (size_t i = 0; i < r->fit_n; ++i) {
        const ibdg_fit_row *w = &r->fit_rows[i];
        fprintf(f, "%zu\t%.6e\t%.6e\t%.6e\t%.6f\t%.6f\t%.6f\t%.6f\t%.6f\t%.6f\t%llu\t%llu\t%llu", i + 1, w->p[0], w->p[1], w->p[2], w->total[0],
                w->total[1], w->total[2], w->prior[0], w->prior[1], w->prior[2], (unsigned long long)w->counted[0],
                (unsigned long long)w->counted[1], (unsigned long long)w->counted[2]);
        for (int k = 0; k < 3; ++k) {
            const int ok = isfinite(w->total[k]) && isfinite(w->prior[k]) && w->total[k] > 0.0 && w->prior[k] > 0.0;
            if (ok)
                fprintf(f, "\t%.6f", w->total[k] / ((double)T * w->prior[k]));
            else
                fputs("\tnan", f);
        }
        fputc('\n', f);
    }
    fprintf(f, "# Individuals\t%zu\n", T);
    fprintf(f, "# Iterations\t%zu\t%s\n", r->fit_n, r->fit_stood ? "stood" : "limit");
    fprintf(f, "# Fitted\t%.17g\t%.17g\t%.17g\n", r->fitted[0], r->fitted[1], r->fitted[2]);
}

/* <out>/<pileup-name>.[log]<kind>.txt (the last five exist with --log-stats only), in the order they are opened and written.
 * armstats.txt is not among them: it is opened where it is written, in run_end. */
static const struct {
    const int *on;
    const char *kind, *phase;
    void (*write)(pile_run *, FILE *);
} RUN_FILES[N_RUN_FILES] = {
    {&opt_states, "ibdstates", "IBD-state fractions file", write_states_file},
    {&opt_posteriors, "ibdposteriors", "IBD-state posteriors file", write_posteriors_file},
    {&opt_segments, "ibdsegments", "IBD-state segments file", write_segments_file},
    {&has_sample_paths, "ibdsamples", "IBD-state samples file", write_samples_file},
    {&opt_switches, "ibdswitches", "IBD-state switches file", write_switches_file},
    {&has_fit, "ibdfit", "fitted switch penalties file", write_fit_file},
};

/* the run's arrays and its statistics files */
static int run_begin(pile_run *r)
{
    site_list *sl = &r->sl;
    const size_t room = r->pj->n_cand ? r->pj->n_cand : 1;
    /* Round 2 page-locked the arrays that cross the engine's boundary (ibdg_host_alloc).  Measured since: locking 128 MB costs 0.1 s, giving it
     * back at exit 0.2 s, and the copies it was meant to speed up (24 MB in, 96 MB out per comparison) run at the same
     * 56 GB/s from ordinary memory (bench.py results_to_host) -- so they are ordinary memory now (malloc / free). */
    sl->s_row = malloc(room * 4); sl->s_cand = malloc(room * 4);
    sl->s_nr = malloc(room); sl->s_na = malloc(room);
    sl->s_fo = has_A ? malloc(room * 8) : NULL;
    r->site_ll = r->site_slot[0] = malloc(r->n_site_out * 24);
    if (!sl->s_row || !sl->s_cand || !sl->s_nr || !sl->s_na || !r->site_ll)
        SFAIL("[::] ERROR: out of memory for %zu rows.\n", r->pj->n_cand);
    phase("result arrays");
    r->res = calloc(g_targets.n + 1, sizeof *r->res);
    if (!r->res)
        SFAIL("[::] ERROR: out of memory.\n");
    if (has_sample_paths) {
        r->smp_tot = calloc(opt_sample_paths, sizeof *r->smp_tot);
        r->smp_col = calloc(opt_sample_paths, sizeof *r->smp_col);
        if (!r->smp_tot || !r->smp_col)
            SFAIL("[::] ERROR: out of memory for %lu draws.\n", opt_sample_paths);
        for (int d = 0; d < r->w->n_eng; ++d)
            r->w->conv[d].smp_tot = r->smp_tot;
    }
    if (has_fit) {
        r->fit_rows = calloc((size_t)opt_fit, sizeof *r->fit_rows);
        if (!r->fit_dev)
            r->fit_keep.tabs = calloc(g_targets.n + 1, sizeof *r->fit_keep.tabs);
        if (!r->fit_rows || (!r->fit_dev && !r->fit_keep.tabs))
            SFAIL("[::] ERROR: out of memory for %ld iterations over %zu individuals.\n", opt_fit, g_targets.n);
    }
    /* opened before the run, like the individuals' files: a directory that cannot be written stops the run at once */
    for (int k = 0; k < N_RUN_FILES; ++k) {
        if (!*RUN_FILES[k].on)
            continue;
        if (asprintf(&r->run_fn[k], "%s/%s.%s%s.txt", g_out_dir, r->pj->name, opt_log_stats ? "log" : "", RUN_FILES[k].kind) < 0)
            return r->run_fn[k] = NULL, 1;
        if (!(r->run_file[k] = fopen(r->run_fn[k], "w")))
            SFAIL("[::] ERROR: Cannot open '%s' for writing.\n", r->run_fn[k]);
        pj_add_file(r->pj, r->run_fn[k]);
    }
    return 0;
}

/* overlap: the individual's output slot.  INVARIANT: a slot's previous output job is joined -- its files closed, its arrays
 * read for the last time -- before the slot's arrays are reused. */
static int output_slot_wait(pile_run *r)
{
    const size_t k = r->ti % (size_t)r->out_slots;
    out_job *prev = &r->w->outs[k];
    if (prev->running) {
        pthread_join(prev->th, NULL);
        prev->running = 0;
        if (prev->failed)
            return 1;
        phase("per individual: waiting for the output files of an earlier individual");
    }
    if (!r->site_slot[k] && !(r->site_slot[k] = malloc(r->n_site_out * 24)))
        SFAIL("[::] ERROR: out of memory for %zu rows.\n", r->pj->n_cand);
    r->site_ll = r->site_slot[k];
    return 0;
}

/* the worker's panel uploads, joined where the panel is first needed on the device */
static int join_uploads(pile_run *r)
{
    worker_t *w = r->w;
    if (!w->ups_pending)
        return 0;
    const int bad = uploads_join(w->ups, w->n_ups);
    w->ups_pending = 0;
    if (bad >= 0)
        SFAIL("%s\n", ibdg_last_error(w->ups[bad].eng));
    phase("panel upload (copy, alt counts, transposition; the part not hidden behind the filter chain)");
    return 0;
}

/* dev_v: the candidate arrays, once per pileup: cand[] holds the rows of fate 1 in row order */
static int candidates_to_device(pile_run *r)
{
    const cand_t *cand = r->pj->cand;
    const size_t n_cand = r->pj->n_cand, room = n_cand ? n_cand : 1;
    r->c_row = malloc(room * 4);
    r->c_nr = malloc(room);
    r->c_na = malloc(room);
    r->c_fo = has_A ? malloc(room * 8) : NULL;
    if (!r->c_row || !r->c_nr || !r->c_na || (has_A && !r->c_fo))
        SFAIL("[::] ERROR: out of memory for %zu rows.\n", n_cand);
    for (size_t i = 0; i < n_cand; ++i) {
        r->c_row[i] = cand[i].row; r->c_nr[i] = cand[i].n_ref; r->c_na[i] = cand[i].n_alt;
        if (r->c_fo) r->c_fo[i] = cand[i].f_is_override ? cand[i].f : NAN;
    }
    for (size_t row = 0; row < n_rows; ++row)
        r->c_gt_failed += r->pj->row_fate[row] == 0 && rows[row].gt_failed;
    if (join_uploads(r))                     /* (the candidates name rows of the panel: it must be there) */
        return 1;
    if (ibdg_upload_candidates(r->w->conv[0].eng, r->c_row, r->c_nr, r->c_na, r->c_fo, n_cand))
        SFAIL("%s\n", ibdg_last_error(r->w->conv[0].eng));
    phase("candidate rows of the pileup to the device");
    return 0;
}

/* ---- the site list: kept, cut on the device, or scanned on the host ---- */
static void site_list_reset(site_list *sl)
{
    const site_list empty = {.s_row = sl->s_row, .s_cand = sl->s_cand, .s_nr = sl->s_nr, .s_na = sl->s_na, .s_fo = sl->s_fo};
    /* (no output job reads these now: jobs run beside the loop only over a list that is never reset, see overlap) */
    free(sl->s_row_dev); free(sl->arm_wfirst); free(sl->arm_wlast);
    free(sl->sum_pos_first); free(sl->sum_pos_last); free(sl->row_pre); free(sl->row_pre_off);
    *sl = empty;
}

/* the reference's message for rows whose genotypes did not parse, repeated per individual as it prints it */
static void gt_failed_replay(const pile_run *r)
{
    for (size_t row = 0; row < n_rows && r->sl.n_gt_failed; ++row)
        if (r->pj->row_fate[row] == 0 && rows[row].gt_failed)
            fprintf(r->err, "Failed to parse genotype fields at %lu. Skipping to next site.\n", rows[row].pos);
}

/* every row is either skipped or on the list (:584-626): the rows not selected are the skipped ones */
static int site_list_from_device(pile_run *r)
{
    site_list *sl = &r->sl;
    ibdg_ctx *eng = r->w->conv[0].eng;
    sl->n_gt_failed = r->c_gt_failed;
    gt_failed_replay(r);
    if (ibdg_select_variable_sites(eng, r->tgt, (unsigned)opt_window))
        SFAIL("%s\n", ibdg_last_error(eng));
    const size_t n = sl->n = ibdg_num_sites(eng);
    if (n > r->pj->n_cand || ibdg_get_site_candidates(eng, sl->s_cand))
        SFAIL("%s\n", n > r->pj->n_cand ? "[::] ERROR: more sites selected than candidates." : ibdg_last_error(eng));
    for (size_t i = 0; i < n; ++i) {
        const size_t my = sl->s_cand[i];
        sl->s_row[i] = r->c_row[my]; sl->s_nr[i] = r->c_nr[my]; sl->s_na[i] = r->c_na[my];
        if (sl->s_fo) sl->s_fo[i] = r->c_fo[my];
        sl->final_total += (unsigned long)r->c_nr[my] + r->c_na[my];
        sl->final_dist[r->c_nr[my] + r->c_na[my]]++;
    }
    sl->skipped = n_rows - n;
    return 0;
}

/* the reference's own walk over every row (:584-628) */
static void site_list_host_scan(pile_run *r)
{
    site_list *sl = &r->sl;
    const cand_t *cand = r->pj->cand;
    const uint8_t *row_fate = r->pj->row_fate;
    const double cull_p = r->pj->cull_p;
    uint32_t *const s_row = sl->s_row, *const s_cand = sl->s_cand;    /* (locals: the byte stores below may alias *sl) */
    uint8_t *const s_nr = sl->s_nr, *const s_na = sl->s_na;
    double *const s_fo = sl->s_fo;
    unsigned long skipped = 0, final_total = 0;
    size_t n = 0;
    for (size_t row = 0, ci = 0; row < n_rows; ++row) {
        if (row_fate[row] == 0) {
            if (rows[row].gt_failed) {
                fprintf(r->err, "Failed to parse genotype fields at %lu. Skipping to next site.\n", rows[row].pos);
                sl->n_gt_failed++;
            }
            skipped++;
            continue;
        }
        const int is_cand = row_fate[row] == 1;
        const size_t my = ci;
        if (is_cand) ci++;
        if (has_v && row_allele(row, r->tgt, 0) == 0 && row_allele(row, r->tgt, 1) == 0) { skipped++; continue; }   /* :584 */
        if (!is_cand) { skipped++; continue; }
        const cand_t *c = &cand[my];
        const unsigned nr = cull(c->n_ref, cull_p), na = cull(c->n_alt, cull_p);                              /* :627-628 */
        final_total += nr + na;
        sl->final_dist[nr + na]++;
        s_row[n] = c->row; s_cand[n] = (uint32_t)my; s_nr[n] = (uint8_t)nr; s_na[n] = (uint8_t)na;
        if (s_fo) s_fo[n] = c->f_is_override ? c->f : NAN;
        n++;
    }
    sl->n = n; sl->skipped = skipped; sl->final_total = final_total;
}

/* Without -v and -D the site list does not depend on the comparison individual (:584, :627-628): it is built for the first
 * one and kept -- 9 ms per individual at 4M rows, more than its engine time. */
static int site_list_stage(pile_run *r)
{
    if (r->same_sites)
        gt_failed_replay(r);
    else {
        site_list_reset(&r->sl);
        if (!r->dev_v)
            site_list_host_scan(r);
        else if (site_list_from_device(r))
            return 1;
    }
    phase(r->dev_v ? "per individual: site list on the device" : "per individual: site list");
    return 0;
}

/* nine of a row's fourteen columns are the same for every comparison individual: their text is made once */
static void row_prefix_once(pile_run *r)
{
    site_list *sl = &r->sl;
    fmt_job pp;
    if (r->ti != 0 || !r->overlap || opt_summary_only || g_targets.n < 3 || sl->n == 0)
        return;
    memset(&pp, 0, sizeof pp);
    pp.cand = r->pj->cand; pp.s_cand = sl->s_cand; pp.pu = r->pj->pu; pp.s_nr = sl->s_nr; pp.s_na = sl->s_na;
    if (row_prefix_build(pp, sl->n, all_threads(), &sl->row_pre, &sl->row_pre_off)) {
        sl->row_pre = NULL;
        sl->row_pre_off = NULL;
    }
    phase("columns 1-9 of every row as text, once for all individuals");
}

/* ---- windows: runs of opt_window covered rows (:572, :657-663, :723-730) ---- */
/* no device: the windows, their likelihoods (non-LD) and the arm sums on the host */
static int windows_on_host(pile_run *r)
{
    const site_list *sl = &r->sl;
    win_table *t = &r->wt;
    t->w.n_win = host_windows(sl->s_nr, sl->s_na, sl->n, (unsigned)opt_window, &t->w.first, &t->w.last, &t->w.ncov);
    if (g_host_math) {
        if (!win_table_alloc_ll(t))
            SFAIL("[::] ERROR: out of memory for %zu windows.\n", t->w.n_win);
        host_nonld(r->pj->cand, sl->s_cand, sl->s_nr, sl->s_na, sl->n, r->tgt, g_pdg_tab, all_threads(), r->site_ll, t->w.first,
                   t->w.last, t->w.n_win, t->ll, t->log);
    }
    if (r->arm_on) {
        uint32_t seg[4];
        int ok[2];
        double p[4], q[4], *res = r->res[r->ti].arm;
        arm_segments(sl->s_row, t->w.first, t->w.last, t->w.n_win, seg, ok);
        const double *tab = opt_log_stats ? t->log : t->ll;
        llr_range_host(tab, opt_log_stats, seg[0], seg[1], p);
        llr_range_host(tab, opt_log_stats, seg[2], seg[3], q);
        res[0] = ok[0] ? p[0] : NAN; res[1] = ok[1] ? q[0] : NAN;
        res[2] = ok[0] ? p[2] : NAN; res[3] = ok[1] ? q[2] : NAN;
    }
    return 0;
}

/* the site list cut into one window range per device, and (--arm-stats) its arms in their global windows cut likewise */
static void site_cuts(pile_run *r)
{
    site_list *sl = &r->sl;
    const int n_eng = r->w->n_eng;
    uint32_t *an, seg[4];
    sl->cuts_made = 1;
    window_cuts(sl->s_nr, sl->s_na, sl->n, (unsigned)opt_window, n_eng, sl->cuts);
    if (!r->arm_on)
        return;
    const size_t nw = sl->arm_nw = host_windows(sl->s_nr, sl->s_na, sl->n, (unsigned)opt_window, &sl->arm_wfirst, &sl->arm_wlast, &an);
    arm_segments(sl->s_row, sl->arm_wfirst, sl->arm_wlast, nw, seg, sl->arm_ok);
    free(an);
    for (int d = 0; d <= n_eng; ++d)
        sl->arm_wcut[d] = (uint32_t)(nw * (size_t)d / (size_t)n_eng);     /* window_cuts' windows per device */
    for (int d = 0; d < n_eng; ++d)
        for (int k = 0; k < 4; ++k) {
            const uint32_t lo = sl->arm_wcut[d], hi = sl->arm_wcut[d + 1];
            sl->arm_local[d][k] = (seg[k] < lo ? lo : seg[k] > hi ? hi : seg[k]) - lo;
        }
}

/* slice_mode: every device gets the panel rows from its first site's row to its last site's row, and its sites are
 * numbered within that slice */
static int panel_slices(pile_run *r)
{
    site_list *sl = &r->sl;
    worker_t *w = r->w;
    if (!(sl->s_row_dev = malloc((sl->n ? sl->n : 1) * 4)))
        SFAIL("[::] ERROR: out of memory for %zu rows.\n", sl->n);
    for (int d = 0; d < w->n_eng; ++d) {
        upload_job *u = &w->ups[d];
        const size_t a = sl->cuts[d], b = sl->cuts[d + 1];
        u->r0 = a < b ? sl->s_row[a] : 0;
        u->n = a < b ? (size_t)sl->s_row[b - 1] + 1 - u->r0 : 0;
        for (size_t i = a; i < b; ++i)
            sl->s_row_dev[i] = sl->s_row[i] - (uint32_t)u->r0;
        if (timing_on > 0)
            fprintf(stderr, "## panel slice of device %d: rows %zu + %zu of %zu\n", d, u->r0, u->n, n_rows);
    }
    g_n_ups = w->n_eng;                      /* (a single -P run: this is the main thread; quit() joins them) */
    uploads_start(w->ups, w->n_eng);
    g_uploads_pending = 1;
    w->ups_pending = 1;
    return 0;
}

/* One contiguous window range per GPU.  Where the individual stands is decided here and nowhere else: it starts a list when
 * it does not run over the list of the one before it, a batch when it is the first of TARGET_BATCH over a shared list (on its
 * own list it is a batch of one), and otherwise only takes its share.  The next batch is named where it will be queued ahead:
 * window tables only (--summary-only). */
static void shards_fill(pile_run *r, shard_job *jobs)
{
    const site_list *sl = &r->sl;
    worker_t *w = r->w;
    const uint32_t *ids = g_targets.idx;
    const size_t n = g_targets.n, ti = r->ti, b0 = r->batchable ? ti - ti % TARGET_BATCH : ti, b1 = b0 + TARGET_BATCH;
    const int level = !r->same_sites ? AT_LIST : ti == b0 ? AT_BATCH : AT_INDIVIDUAL;
    for (int d = 0; d < w->n_eng; ++d) {
        dev_conv *c = &w->conv[d];
        shard_job *j = &jobs[d];
        if (level == AT_LIST) {
            c->row = w->slice_mode ? sl->s_row_dev : sl->s_row; c->s_row = sl->s_row;
            c->nr = sl->s_nr; c->na = sl->s_na; c->fo = sl->s_fo;
            c->a = sl->cuts[d]; c->b = sl->cuts[d + 1];
            c->arm_seg = r->arm_on ? sl->arm_local[d] : NULL;
        }
        if (level >= AT_BATCH) {
            c->targets = ids + b0;
            c->n_targets = !r->batchable ? 1 : n - b0 < TARGET_BATCH ? n - b0 : TARGET_BATCH;
            c->next = r->batchable && opt_summary_only && b1 < n ? ids + b1 : NULL;
            c->n_next = !c->next ? 0 : n - b1 < TARGET_BATCH ? n - b1 : TARGET_BATCH;
        }
        memset(j, 0, sizeof *j);
        j->c = c;
        j->level = level;
        j->t_local = ti - b0;
        j->site_ll = r->site_ll;
    }
}

/* ... evaluated concurrently.  INVARIANT: every shard thread of the individual is joined before any shard's failure is acted
 * on -- never exit() while other shard threads are inside the GPU runtime. */
static int shards_run(pile_run *r, shard_job *jobs)
{
    const int n_eng = r->w->n_eng;
    pthread_t th[64];
    int th_started[64] = {0}, shard_failed = -1;
    for (int d = 0; d < n_eng; ++d) {
        th_started[d] = n_eng > 1 && pthread_create(&th[d], NULL, shard_run, &jobs[d]) == 0;
        if (!th_started[d])                  /* (no thread to be had: the shard runs here) */
            shard_run(&jobs[d]);
    }
    for (int d = 0; d < n_eng; ++d) {
        if (th_started[d])
            pthread_join(th[d], NULL);
        if (jobs[d].failed && shard_failed < 0)
            shard_failed = d;
        r->wt.w.n_win += jobs[d].wt.w.n_win;
    }
    if (shard_failed >= 0 && !jobs[shard_failed].c->reported)
        fprintf(r->err, "%s\n", ibdg_last_error(jobs[shard_failed].c->eng));
    return shard_failed >= 0;
}

/* --arm-stats: each device's parts of the two arms, added in device order, then rounded */
static int arm_gather(pile_run *r, const shard_job *jobs)
{
    const site_list *sl = &r->sl;
    double acc[8] = {0}, *res = r->res[r->ti].arm;
    for (int d = 0; d < r->w->n_eng; ++d) {
        if (jobs[d].wt.w.n_win != sl->arm_wcut[d + 1] - sl->arm_wcut[d])
            SFAIL("[::] ERROR: device %d holds %zu windows, not the %u of its range.\n", d, jobs[d].wt.w.n_win,
                  sl->arm_wcut[d + 1] - sl->arm_wcut[d]);
        for (int k = 0; k < 4; ++k)
            dd_add(acc + 2 * k, jobs[d].out.arm[2 * k], jobs[d].out.arm[2 * k + 1]);
    }
    res[0] = sl->arm_ok[0] ? acc[0] + acc[1] : NAN; res[1] = sl->arm_ok[1] ? acc[4] + acc[5] : NAN;
    res[2] = sl->arm_ok[0] ? acc[2] + acc[3] : NAN; res[3] = sl->arm_ok[1] ? acc[6] + acc[7] : NAN;
    return 0;
}

/* the devices' window tables, gathered in order into the individual's */
static int tables_gather(pile_run *r, shard_job *jobs)
{
    win_table *t = &r->wt;
    if (r->w->n_eng == 1 && jobs[0].c->a == 0) {
        *t = jobs[0].wt;   /* one device, the whole site list: its arrays as they are (a copy of 1.2 MB per individual otherwise) */
        return 0;
    }
    const size_t n_win = t->w.n_win;
    if (!win_list_alloc(&t->w, n_win) || !win_table_alloc_ll(t)) {
        for (int d = 0; d < r->w->n_eng; ++d)
            win_table_free(&jobs[d].wt);
        SFAIL("[::] ERROR: out of memory for %zu windows.\n", n_win);
    }
    size_t wo = 0;
    for (int d = 0; d < r->w->n_eng; ++d) {
        win_table *s = &jobs[d].wt;
        const uint32_t a0 = (uint32_t)jobs[d].c->a;
        for (size_t wi = 0; wi < s->w.n_win; ++wi) {
            t->w.first[wo + wi] = s->w.first[wi] + a0;
            t->w.last[wo + wi] = s->w.last[wi] + a0;
        }
        memcpy(t->w.ncov + wo, s->w.ncov, s->w.n_win * 4);
        memcpy(t->ll + 3 * wo, s->ll, s->w.n_win * 24);
        if (t->log)
            memcpy(t->log + 3 * wo, s->log, s->w.n_win * 24);
        wo += s->w.n_win;
        win_table_free(s);
    }
    return 0;
}

static int windows_on_engine(pile_run *r)
{
    site_list *sl = &r->sl;
    win_table *t = &r->wt;
    shard_job jobs[64];
    if (!sl->cuts_made)
        site_cuts(r);
    if (r->w->slice_mode && r->ti == 0 && panel_slices(r))
        return 1;
    if (join_uploads(r))
        return 1;
    /* --pileup-list: what upload_run decides for a single run's contexts (share_sites), per pileup: whether this pileup's
     * individuals share one site list depends on its own cull ratio, so each pileup gets the layout choice its single run
     * makes ("auto" otherwise) */
    for (int d = 0; d < r->w->n_eng && g_list_mode && r->ti == 0; ++d)
        if (ibdg_set_option(r->w->conv[d].eng, "compact_tiles", r->batchable && opt_ld && !opt_ref_order && g_targets.n >= 240))
            SFAIL("%s\n", ibdg_last_error(r->w->conv[d].eng));
    shards_fill(r, jobs);
    if (shards_run(r, jobs))
        return 1;
    if (r->dev_states)
        r->res[r->ti] = jobs[0].out;         /* (one context: its record is the individual's; the arm sums follow) */
    if (r->arm_on && arm_gather(r, jobs))
        return 1;
    if (r->tables_stay)                      /* no window table left the device */
        return 0;
    if (tables_gather(r, jobs))
        return 1;
    if (r->arm_on && (t->w.n_win != sl->arm_nw || memcmp(t->w.first, sl->arm_wfirst, sl->arm_nw * 4) || memcmp(t->w.last, sl->arm_wlast, sl->arm_nw * 4)))
        SFAIL("[::] ERROR: the engine's windows are not the ones the chromosome arms were cut from.\n");
    return 0;
}

static void summary_positions(pile_run *r)
{
    site_list *sl = &r->sl;
    const win_list *t = &r->wt.w;
    if (!r->overlap || g_no_engine || (sl->sum_pos_made && sl->sum_pos_n == t->n_win))
        return;
    free(sl->sum_pos_first); free(sl->sum_pos_last);
    sl->sum_pos_first = malloc((t->n_win + 1) * sizeof *sl->sum_pos_first);
    sl->sum_pos_last = malloc((t->n_win + 1) * sizeof *sl->sum_pos_last);
    sl->sum_pos_n = t->n_win;
    sl->sum_pos_made = 1;
    for (size_t wi = 0; wi < t->n_win && sl->sum_pos_first && sl->sum_pos_last; ++wi) {
        sl->sum_pos_first[wi] = rows[sl->s_row[t->first[wi]]].pos;
        sl->sum_pos_last[wi] = rows[sl->s_row[t->last[wi]]].pos;
    }
}

/* ---- the individual's output job ---- */
/* File k of IND_FILES for the individual at hand, OUT/NAME.TARGET.KIND.txt: opened without truncation (see the table) and
 * listed among the pileup's files, with /dev/null in its place where its row says so.  NULL: not opened (fn NULL: no memory
 * for the name); the caller reports it. */
static FILE *out_file_open(pile_run *r, int k, const char *fn)
{
    const int fd = fn ? open(ind_file_null(k) ? "/dev/null" : fn, O_WRONLY | O_CREAT, 0666) : -1;
    FILE *f = fd >= 0 ? fdopen(fd, "w") : NULL;
    if (f && !ind_file_null(k))
        pj_add_file(r->pj, fn);
    return f;
}

/* The individual's files, opened in the table's order up to the first that cannot be.  The files after that one are not
 * opened, so no settle reaches them: where an earlier run left one it is emptied by name here (none is made), or it would
 * outlive this failing run looking complete. */
static int outputs_open(pile_run *r, out_job *o)
{
    char *fn[N_IND_FILES] = {NULL};
    int failed = -1;
    memset(o->file, 0, sizeof o->file);
    if (opt_plan || opt_stats_only) {         /* (--stats-only --states: the table is here for its path alone) */
        o->file[F_TAB] = o->file[F_SUM] = opt_plan ? stdout : NULL;
        return 0;
    }
    o->pending = 1;
    for (int k = 0; k < N_IND_FILES; ++k) {
        if (!ind_file_on(k))
            continue;
        if (asprintf(&fn[k], "%s/%s.%s.%s%s.txt", g_out_dir, r->pj->name, r->tname, IND_FILES[k].log && opt_log_stats ? "log" : "",
                     IND_FILES[k].kind) < 0)
            fn[k] = NULL;
        if (failed < 0 || k == F_SUM) {       /* (the summary is tried whatever became of the tab: one message names both) */
            if (!(o->file[k] = out_file_open(r, k, fn[k])) && failed < 0)
                failed = k;
        } else if (fn[k])
            (void)!truncate(fn[k], 0);
    }
    if (failed >= 0 && failed <= F_SUM && fn[F_TAB] && fn[F_SUM])
        fprintf(r->err, "[::] ERROR in compare_impute(): Cannot open '%s' and/or '%s' for writing.\n", fn[F_TAB], fn[F_SUM]);
    if (failed > F_SUM && fn[failed])
        fprintf(r->err, "[::] ERROR in compare_impute(): Cannot open '%s' for writing.\n", fn[failed]);
    for (int k = 0; k < N_IND_FILES; ++k)
        free(fn[k]);
    return failed >= 0;
}

/* everything the individual's files are made of goes to its slot's job, the window table with it; the job runs beside the
 * loop (overlap) or here */
static int output_start(pile_run *r)
{
    const site_list *sl = &r->sl;
    const pile_job *pj = r->pj;
    out_job *o = &r->w->outs[r->overlap ? r->ti % (size_t)r->out_slots : 0];
    o->pos_first = r->overlap && !g_no_engine && sl->sum_pos_first && sl->sum_pos_last ? sl->sum_pos_first : NULL;
    o->pos_last = o->pos_first ? sl->sum_pos_last : NULL;
    o->out_dir = g_out_dir; o->user_cmd = g_user_cmd; o->in_dist = pj->in_dist; o->mean_cov = pj->mean_cov; o->cull_p = pj->cull_p;
    o->cand = pj->cand; o->s_cand = sl->s_cand; o->s_row = sl->s_row; o->s_nr = sl->s_nr; o->s_na = sl->s_na; o->pu = pj->pu;
    o->tname = r->tname; o->tgt = r->tgt; o->n = sl->n;
    o->processed = sl->n; o->skipped = sl->skipped; o->final_total = sl->final_total;
    memcpy(o->final_dist, sl->final_dist, sizeof o->final_dist);
    o->site_ll = r->site_ll;
    o->pre = sl->row_pre; o->pre_off = sl->row_pre_off;
    o->wt = r->wt;
    memset(&r->wt, 0, sizeof r->wt);
    o->sq = pj->name; o->err = r->err;
    o->res = &r->res[r->ti];
    o->smp_tot = r->smp_tot;
    o->swp = r->one_list ? &r->sw_prior : NULL;
    o->fit = has_fit && !r->fit_dev ? &r->fit_keep : NULL;
    o->ti = r->ti;
    if (outputs_open(r, o))
        return 1;
    const int threads = all_threads();
    /* (tools/many_tables.py: files of 1 / 2 / 3 / 4 / 6 individuals at once with 8 threads each 73* / 66 / 57 / 47 / 54 ms per
     * individual, *16 threads; 4 x 4 threads 58, 3 x 16 threads 57) */
    o->threads = r->overlap && r->out_slots > 1 && threads > 3 ? (opt_summary_only ? (threads + 3) / 4 : threads / 2) : threads;
    if (r->overlap && r->out_threads_env > 0)
        o->threads = r->out_threads_env;
    o->running = r->overlap && pthread_create(&o->th, NULL, output_individual, o) == 0;
    if (!o->running)
        output_individual(o);
    return !o->running && o->failed;
}

/* ---- --fit-penalties: the iterations, after the run's last individual ---- */
/* the host route's share of one iteration: a thread's individuals (k, k + n, ...), each its own slot of expect */
typedef struct {
    const struct fit_keep *keep;
    const double *p;
    double *expect;                 /* [individuals][3] */
    size_t first, step, n_ind;
    int failed;
    pthread_t th;
} fit_part;

static void *fit_part_run(void *arg)
{
    fit_part *f = arg;
    const struct fit_keep *k = f->keep;
    uint64_t counted[3];
    for (size_t ti = f->first; ti < f->n_ind && !f->failed; ti += f->step)
        f->failed = ibdg_log2_switches_host(k->tabs[ti], k->n_win, f->p[0], f->p[1], f->p[2], k->starts, k->n_starts, k->shift, NULL,
                                            f->expect + 3 * ti, counted) != 0;
    return NULL;
}

/* The fit over the tables the output jobs kept: per iteration every individual's expectations on --threads threads (an
 * individual's are its own call's, whoever makes it), their sum in the order of the panel from 0.0, the prior from the table
 * that says nothing, ibdg_switch_fit_step -- the loop of ibdg_log2_fit_host, whose bytes these are for any number of threads. */
static int fit_on_host(pile_run *r)
{
    const struct fit_keep *k = &r->fit_keep;
    const size_t T = g_targets.n;
    const int n_th = all_threads() < 1 ? 1 : all_threads() > 64 ? 64 : all_threads();
    double cur[3] = {opt_p01, opt_p02, opt_p12}, *expect = malloc((T ? T : 1) * 3 * sizeof *expect);
    fit_part part[64];
    if (!expect)
        SFAIL("[::] ERROR: out of memory for the expectations of %zu individuals.\n", T);
    for (size_t ti = 0; ti < T; ++ti)
        if (!k->tabs[ti]) {
            free(expect);
            SFAIL("[::] ERROR: --fit-penalties: no log table was kept for %s.\n", g_ids.names[g_targets.idx[ti]]);
        }
    memcpy(r->fitted, cur, sizeof cur);
    for (long it = 0; T && it < opt_fit && !r->fit_stood; ++it) {
        double total[3] = {0.0, 0.0, 0.0}, prior[3], next[3];
        uint64_t counted[3];
        int bad = 0;
        int started[64] = {0};
        for (int t = 0; t < n_th; ++t) {
            part[t] = (fit_part){.keep = k, .p = cur, .expect = expect, .first = (size_t)t, .step = (size_t)n_th, .n_ind = T};
            started[t] = t < n_th - 1 && pthread_create(&part[t].th, NULL, fit_part_run, &part[t]) == 0;
        }
        for (int t = 0; t < n_th; ++t)
            if (!started[t])                     /* (the last share, or no thread to be had: it runs here) */
                fit_part_run(&part[t]);
        for (int t = 0; t < n_th; ++t) {
            if (started[t])
                pthread_join(part[t].th, NULL);
            bad |= part[t].failed;
        }
        for (size_t ti = 0; ti < T; ++ti)
            for (int s = 0; s < 3; ++s)
                total[s] += expect[3 * ti + s];
        bad = bad || ibdg_log2_switches_host(NULL, k->n_win, cur[0], cur[1], cur[2], k->starts, k->n_starts, k->shift, NULL, prior, counted) ||
              ibdg_switch_fit_step(cur, total, T, prior, counted, &r->fit_rows[it], next, &r->fit_stood);
        if (bad) {
            free(expect);
            SFAIL("%s\n", ibdg_last_error(NULL));
        }
        r->fit_n = (size_t)it + 1;
        memcpy(cur, next, sizeof cur);
        memcpy(r->fitted, next, sizeof next);
    }
    free(expect);
    return 0;
}

static int run_fit(pile_run *r)
{
    if (!has_fit)
        return 0;
    if (r->fit_dev) {
        ibdg_ctx *eng = r->w->conv[0].eng;
        const double p[3] = {opt_p01, opt_p02, opt_p12};
        if (ibdg_log2_store_count(eng) != g_targets.n)
            SFAIL("[::] ERROR: --fit-penalties: the device holds the log tables of %zu individuals, not of the run's %zu.\n",
                  ibdg_log2_store_count(eng), g_targets.n);
        if (ibdg_log2_store_fit(eng, p, (size_t)opt_fit, r->fit_rows, &r->fit_n, &r->fit_stood, r->fitted))
            SFAIL("%s\n", ibdg_last_error(eng));
    } else if (fit_on_host(r))
        return 1;
    phase("fit of the switch penalties (--fit-penalties)");
    return 0;
}

/* the files the run writes once, after its last individual */
static int run_end(pile_run *r)
{
    const idlist_t targets = g_targets;
    if (run_fit(r))
        return 1;
    if (r->arm_on) {
        /* one file for the run, written here once: the lines in comparison order, as bin/chrarm-stats.py prints them */
        char *arm_fn;
        const pileup_t *pu = r->pj->pu;
        const char *chrom = g_uchr ? g_uchr : pu->n_lines ? pu->chr_names[pu->lines[0].chr] : ".";
        if (asprintf(&arm_fn, "%s/%s.%s.txt", g_out_dir, r->pj->name, opt_log_stats ? "logarmstats" : "armstats") < 0)
            return 1;
        FILE *af = fopen(arm_fn, "w");
        if (!af)
            SFAIL("[::] ERROR: Cannot open '%s' for writing.\n", arm_fn);
        pj_add_file(r->pj, arm_fn);
        fprintf(af, "SAMPLE\tCHROM\tparm_IBD2/IBD0\tqarm_IBD2/IBD0\tparm_IBD1/IBD0\tqarm_IBD1/IBD0\n");
        for (size_t ti = 0; ti < targets.n; ++ti) {
            fprintf(af, "%s\t%s", g_ids.names[targets.idx[ti]], chrom);
            for (int k = 0; k < 4; ++k) {
                const double v = r->res[ti].arm[k];
                if (isnan(v))
                    fprintf(af, "\tnan");
                else
                    fprintf(af, "\t%.3e", v);
            }
            fputc('\n', af);
        }
        if (fclose(af) != 0)
            SFAIL("[::] ERROR writing '%s'.\n", arm_fn);
        free(arm_fn);
        phase("arm statistics file");
    }
    for (int k = 0; k < N_RUN_FILES; ++k) {
        FILE *f = r->run_file[k];
        if (!f)
            continue;
        RUN_FILES[k].write(r, f);
        r->run_file[k] = NULL;
        if (fclose(f) != 0)
            SFAIL("[::] ERROR writing '%s'.\n", r->run_fn[k]);
        phase(RUN_FILES[k].phase);
    }
    return 0;
}

/* What the run holds, after a failure as well (every thread that read it has been joined).  The small things always; the large
 * arrays for a list only, where the next pileup's take their place: a single -P run leaves them to the end of the process. */
static void run_release(pile_run *r)
{
    site_list *sl = &r->sl;
    for (int k = 0; k < N_RUN_FILES; ++k) {
        if (r->run_file[k])
            fclose(r->run_file[k]);           /* (a failed run's: opened empty, left empty) */
        free(r->run_fn[k]);
        r->run_file[k] = NULL, r->run_fn[k] = NULL;
    }
    for (size_t ti = 0; r->res && ti < g_targets.n; ++ti)
        free(r->res[ti].smp_row);
    free(r->res); free(sl->row_pre); free(sl->row_pre_off); free(r->smp_tot); free(r->smp_col);
    for (size_t ti = 0; r->fit_keep.tabs && ti < g_targets.n; ++ti)
        free(r->fit_keep.tabs[ti]);
    free(r->fit_keep.tabs); free(r->fit_keep.starts); free(r->fit_keep.shift); free(r->fit_rows);
    memset(&r->fit_keep, 0, sizeof r->fit_keep);
    r->fit_rows = NULL;
    r->res = NULL;
    r->smp_tot = NULL, r->smp_col = NULL;
    sl->row_pre = NULL;
    sl->row_pre_off = NULL;
    if (!g_list_mode)
        return;
    for (int k = 0; k < OUT_SLOTS; ++k)
        free(r->site_slot[k]);
    free(r->c_row); free(r->c_nr); free(r->c_na); free(r->c_fo);
    site_list_reset(sl);
    free(sl->s_row); free(sl->s_cand); free(sl->s_nr); free(sl->s_na); free(sl->s_fo);
}

static int pj_run(pile_job *pj, worker_t *w)
{
    pile_run r;
    out_job *const outs = w->outs;
    grand_seed(1);                  /* a fresh process's read-thinning stream (-D) */
    if (g_list_mode)
        timing_tag = pj->name;
    memset(&r, 0, sizeof r);
    r.pj = pj; r.w = w; r.err = pj->err;
    run_modes(&r);
    if (run_begin(&r))
        goto fail;
    for (r.ti = 0; r.ti < g_targets.n; ++r.ti) {
        r.tgt = g_targets.idx[r.ti];
        r.tname = g_ids.names[r.tgt];
        r.same_sites = r.one_list && r.ti > 0;
        memset(&r.wt, 0, sizeof r.wt);
        if (r.overlap && output_slot_wait(&r))
            goto fail;
        fprintf(r.err, "Running %s-vs-%s comparison...\n", pj->name, r.tname);
        if (r.dev_v && r.ti == 0 && candidates_to_device(&r))
            goto fail;
        if (site_list_stage(&r))
            goto fail;
        row_prefix_once(&r);
        if (g_no_engine ? windows_on_host(&r) : windows_on_engine(&r))
            goto fail;
        if (r.tables_stay) {
            win_table_free(&r.wt);
            phase("per individual: engine (upload, run, arm sums)");
            continue;
        }
        summary_positions(&r);
        phase("per individual: engine (upload, run, results)");
        if (output_start(&r))
            goto fail;
        phase("per individual: output files");
    }
    for (int k = 0; k < OUT_SLOTS; ++k) {     /* the output jobs still running */
        if (outs[k].running) {
            pthread_join(outs[k].th, NULL);
            outs[k].running = 0;
            if (outs[k].failed)
                goto fail;
        }
    }
    if (r.overlap)
        phase("output files of the last individuals (written beside the engine's work on the ones after them)");
    if (run_end(&r))
        goto fail;
    run_release(&r);
    return 0;
fail:
    outs_settle_one(outs, 1);
    run_release(&r);
    return 1;
}

/* a worker's loop over the list: entry i runs while entry i + 1 is read and filtered beside it */
static void *worker_main(void *arg)
{
    worker_t *w = arg;
    long cur = w->first;
    if (cur >= 0 && !w->first_ready) {
        pj_prepare(&g_list.jobs[cur]);
        phase_begin(NULL);
    }
    while (cur >= 0) {
        pile_job *pj = &g_list.jobs[cur];
        long nxt = -1;
        pthread_t pt;
        int prefetch = 0;
        if (!pj->rc && (nxt = list_take()) >= 0)
            prefetch = pthread_create(&pt, NULL, pj_prepare, &g_list.jobs[nxt]) == 0;
        int rc = pj->rc;
        if (!rc)
            rc = list_failed_before((size_t)cur) ? -1 : pj_run(pj, w);
        if (g_list_mode)
            pj_release(pj);
        list_finish((size_t)cur, rc);
        if (nxt >= 0) {
            if (prefetch)
                pthread_join(pt, NULL);
            else
                pj_prepare(&g_list.jobs[nxt]);
            phase_begin(NULL);
        }
        cur = nxt;
    }
    return NULL;
}

int main(int argc, char **argv)
{
    const clock_t t_start = clock();
    phase("start");
#ifdef __GLIBC__
    /* the per-individual arrays (window tables, 1.2 MB) and text buffers come and go once per comparison individual: kept in
     * the heap instead of a map, 300 page faults and an unmap each time (0.3 ms of an individual's 0.7 in a whole-panel run) */
    mallopt(M_MMAP_THRESHOLD, 256 << 20);
    mallopt(M_TRIM_THRESHOLD, 512 << 20);
#endif
    fmt_init();
    const char *hap_fn = NULL, *legend_fn = NULL, *indv_fn = NULL, *pu_fn = NULL, *vcf_fn = NULL;
    const char *sample_fn = NULL, *sample_csv = NULL, *bg_fn = NULL, *af_fn = NULL, *pos_fn = NULL;
    const char *uchr = NULL, *out_dir = NULL, *devices_arg = "0", *list_fn = NULL;
    int has_N = 0;
    char cwd[PATH_MAX];
    if (argc == 1)
        usage(0);
    out_dir = getcwd(cwd, sizeof cwd) ? cwd : "./";

    int o;
    while ((o = getopt_long(argc, argv, ":V:H:L:I:P:w:N:A:S:s:B:p:q:M:F:f:D:O:c:e:vh", longopts, NULL)) != -1) {
        switch (o) {
        case 0: break;
        case 'V': in_vcf = 1; vcf_fn = optarg; break;
        case 'H': in_impute = 1; hap_fn = optarg; break;
        case 'L': in_impute = 1; legend_fn = optarg; break;
        case 'I': in_impute = 1; indv_fn = optarg; break;
        case 'P': pu_fn = optarg; break;
        case 'w': opt_window = atoi(optarg); break;
        case 'N': opt_sq = optarg; has_N = 1; break;
        case 'S': has_S = 1; sample_fn = optarg; break;
        case 's': has_s = 1; sample_csv = optarg; break;
        case 'B': has_B = 1; bg_fn = optarg; break;
        case 'A': has_A = 1; af_fn = optarg; break;
        case 'M': opt_max_cov = (unsigned)atoi(optarg); break;
        case 'F': opt_max_af = atof(optarg); break;
        case 'f': opt_min_af = atof(optarg); break;
        case 'p': has_p = 1; pos_fn = optarg; break;
        case 'q': opt_min_qual = atof(optarg); break;
        case 'c': uchr = optarg; break;
        case 'e': opt_eps = atof(optarg); break;
        case 'O': out_dir = optarg; break;
        case 'D': opt_target_dp = atof(optarg); has_D = 1; break;
        case 'v': has_v = 1; break;
        case 'h': usage(0); break;
        case 1001: devices_arg = optarg; break;
        case 1002: opt_threads = atoi(optarg); break;
        case 1003: cache_fn = optarg; break;
        case 1004: dump_panel_fn = optarg; break;   /* test hook: the packed rows + clean flags as a binary file */
        case 1007: list_fn = optarg; break;         /* --pileup-list FILE: NAME PATH per pileup */
        case 1008: opt_p01 = atof(optarg); has_pen = 1; break;
        case 1009: opt_p02 = atof(optarg); has_pen = 1; break;
        case 1010: opt_p12 = atof(optarg); has_pen = 1; break;
        case 1011: {
            char *end = NULL;
            errno = 0;
            opt_chain_gap = strtoul(optarg, &end, 10);
            if (!isdigit((unsigned char)optarg[0]) || *end || errno || opt_chain_gap < 1) {
                fprintf(stderr, "[::] ERROR: Invalid chain gap (--chain-gap) '%s' (must be an integer >= 1, in base pairs).\n", optarg);
                exit(1);
            }
            has_chain_gap = 1;
            break;
        }
        case 1012: {
            char *end = NULL;
            errno = 0;
            opt_switch_scale = strtod(optarg, &end);
            if (end == optarg || *end || errno || !isfinite(opt_switch_scale) || !(opt_switch_scale > 0.0)) {
                fprintf(stderr, "[::] ERROR: Invalid switch scale (--switch-scale) '%s' (must be a decimal > 0: base pairs, or centimorgans with --genetic-map).\n", optarg);
                exit(1);
            }
            has_switch_scale = 1;
            break;
        }
        case 1013: genetic_map_fn = optarg; break;
        case 1014: {
            char *end = NULL;
            errno = 0;
            opt_sample_paths = strtoul(optarg, &end, 10);
            if (!isdigit((unsigned char)optarg[0]) || *end || errno || opt_sample_paths < 1 || opt_sample_paths > 65536) {
                fprintf(stderr, "[::] ERROR: Invalid number of draws (--sample-paths) '%s' (must be an integer in 1 .. 65536).\n", optarg);
                exit(1);
            }
            has_sample_paths = 1;
            break;
        }
        case 1015: {
            char *end = NULL;
            errno = 0;
            opt_seed = strtoull(optarg, &end, 10);
            if (!isdigit((unsigned char)optarg[0]) || *end || errno) {
                fprintf(stderr, "[::] ERROR: Invalid seed (--seed) '%s' (must be an integer in 0 .. 2^64 - 1).\n", optarg);
                exit(1);
            }
            has_seed = 1;
            break;
        }
        case 1016: {
            char *end = NULL;
            errno = 0;
            opt_fit = strtol(optarg, &end, 10);
            if (!isdigit((unsigned char)optarg[0]) || *end || errno || opt_fit < 1 || opt_fit > 1000) {
                fprintf(stderr, "[::] ERROR: Invalid number of iterations (--fit-penalties) '%s' (must be an integer in 1 .. 1000).\n", optarg);
                exit(1);
            }
            has_fit = 1;
            break;
        }
        case 1006:
            if (!parse_arm_range(optarg)) {
                fprintf(stderr, "[::] ERROR: Invalid centromeric range (--arm-stats) '%s' (must be START,END with START <= END).\n", optarg);
                exit(1);
            }
            has_arm = 1;
            break;
        case 1005: exit(fmt_check(atol(optarg)));   /* test hook: the number conversions against printf */
        case 1000:                                  /* test hook: the first N values of the read-thinning stream */
            for (long i = atol(optarg); i > 0; --i)
                printf("%d\n", glibc_rand());
            exit(0);
        case ':': fprintf(stderr, "Option -%c missing required argument.\n", optopt); exit(0);
        case '?':
            if (isprint(optopt))
                fprintf(stderr, "Invalid option -%c.\n", optopt);
            else
                fprintf(stderr, "Invalid option character.\n");
            break;
        default: fprintf(stderr, "[::] ERROR parsing command-line options.\n"); exit(0);
        }
    }
    for (int i = optind; i < argc; ++i)
        fprintf(stderr, "Given extra argument %s.\n", argv[i]);
    /* range checks, messages and exit codes of reference src/ibdgem.c:966-989 */
    if (has_D && opt_target_dp <= 0) { fprintf(stderr, "[::] ERROR: Invalid down-sample coverage (-D) of %.2f (must be > 0).\n", opt_target_dp); exit(0); }
    if (opt_min_af < 0) { fprintf(stderr, "[::] ERROR: Invalid minimum alternate allele frequency (-f) of %.2f (must be >= 0).\n", opt_min_af); exit(0); }
    if (opt_max_af > 1) { fprintf(stderr, "[::] ERROR: Invalid maximum alternate allele frequency (-F) of %.2f (must be <= 1).\n", opt_max_af); exit(0); }
    if (opt_max_cov < 1) { fprintf(stderr, "[::] ERROR: Invalid maximum estimated coverage (-M) of %u (must be >= 1).\n", opt_max_cov); exit(0); }
    if (opt_min_qual < 0) { fprintf(stderr, "[::] ERROR: Invalid genotype quality minimum (-q) of %.2f (must be >= 0).\n", opt_min_qual); exit(0); }
    if (opt_window < 2) { fprintf(stderr, "[::] ERROR: Invalid window size (-w) of %d (must be >= 2).\n", opt_window); exit(0); }
    if (opt_max_cov > 127) { fprintf(stderr, "[::] ERROR: Invalid maximum estimated coverage (-M) of %u (pileup lines hold at most 127 reads).\n", opt_max_cov); exit(0); }
    if (has_pen && !opt_states) { fprintf(stderr, "[::] ERROR: --p01, --p02 and --p12 are the penalties of --states.\n"); exit(1); }
    if (opt_states && opt_plan) { fprintf(stderr, "[::] ERROR: --states writes files --plan does not make; use one of them.\n"); exit(1); }
    if (opt_stats_only && !has_arm && !opt_states) { fprintf(stderr, "[::] ERROR: --stats-only needs --arm-stats START,END.\n"); exit(1); }
    if (opt_stats_only && opt_plan) { fprintf(stderr, "[::] ERROR: --stats-only writes a file --plan does not make; use one of them.\n"); exit(1); }
    if (opt_log_summary && opt_plan) { fprintf(stderr, "[::] ERROR: --log-summary writes files --plan does not make; use one of them.\n"); exit(1); }
    if (opt_log_summary && opt_stats_only) { fprintf(stderr, "[::] ERROR: --log-summary writes files --stats-only leaves out; use one of them.\n"); exit(1); }
    if (opt_log_stats && opt_plan) { fprintf(stderr, "[::] ERROR: --log-stats writes files --plan does not make; use one of them.\n"); exit(1); }
    if (opt_log_stats && !has_arm && !opt_states) { fprintf(stderr, "[::] ERROR: --log-stats needs --arm-stats START,END and/or --states: it says where their numbers come from.\n"); exit(1); }
    if (opt_posteriors && opt_plan) { fprintf(stderr, "[::] ERROR: --posteriors writes files --plan does not make; use one of them.\n"); exit(1); }
    if (opt_posteriors && (!opt_log_stats || !opt_states)) { fprintf(stderr, "[::] ERROR: --posteriors needs --log-stats and --states: it is the sum over all paths of the weights whose best path they find, with their --p01, --p02, --p12.\n"); exit(1); }
    if (opt_segments && opt_plan) { fprintf(stderr, "[::] ERROR: --segments writes files --plan does not make; use one of them.\n"); exit(1); }
    if (opt_segments && (!opt_log_stats || !opt_states)) { fprintf(stderr, "[::] ERROR: --segments needs --log-stats and --states: it cuts the path they find into its runs of one state and sums that path's own emissions over each.\n"); exit(1); }
    if (has_chain_gap && opt_plan) { fprintf(stderr, "[::] ERROR: --chain-gap changes files --plan does not make; use one of them.\n"); exit(1); }
    if (has_chain_gap && (!opt_log_stats || !opt_states)) { fprintf(stderr, "[::] ERROR: --chain-gap needs --log-stats and --states: it says where the chain of windows whose path they find is broken.\n"); exit(1); }
    if (has_switch_scale && opt_plan) { fprintf(stderr, "[::] ERROR: --switch-scale changes files --plan does not make; use one of them.\n"); exit(1); }
    if (has_switch_scale && (!opt_log_stats || !opt_states)) { fprintf(stderr, "[::] ERROR: --switch-scale needs --log-stats and --states: it scales the switch penalties of the chain of windows whose path they find.\n"); exit(1); }
    if (genetic_map_fn && opt_plan) { fprintf(stderr, "[::] ERROR: --genetic-map changes files --plan does not make; use one of them.\n"); exit(1); }
    if (genetic_map_fn && (!opt_log_stats || !opt_states)) { fprintf(stderr, "[::] ERROR: --genetic-map needs --log-stats and --states: it measures the distances their switch penalties are scaled by.\n"); exit(1); }
    if (genetic_map_fn && !has_switch_scale) { fprintf(stderr, "[::] ERROR: --genetic-map needs --switch-scale X: it says in which unit X and the distances between windows are measured.\n"); exit(1); }
    if (opt_switches && opt_plan) { fprintf(stderr, "[::] ERROR: --switches writes files --plan does not make; use one of them.\n"); exit(1); }
    if (opt_switches && (!opt_log_stats || !opt_states)) { fprintf(stderr, "[::] ERROR: --switches needs --log-stats and --states: it is the probability of a switch at every step under the weights whose best path they find, with their --p01, --p02, --p12.\n"); exit(1); }
    if (has_fit && opt_plan) { fprintf(stderr, "[::] ERROR: --fit-penalties writes a file --plan does not make; use one of them.\n"); exit(1); }
    if (has_fit && (!opt_log_stats || !opt_states)) { fprintf(stderr, "[::] ERROR: --fit-penalties needs --log-stats and --states: it fits the switch penalties of the weights whose best path they find, starting from their --p01, --p02, --p12.\n"); exit(1); }
    if (has_fit && (has_v || has_D)) { fprintf(stderr, "[::] ERROR: --fit-penalties cannot be combined with %s: every individual then has a site list of its own, and the fit is over the tables of one list.\n", has_v ? "-v" : "-D"); exit(1); }
    if (has_sample_paths && opt_plan) { fprintf(stderr, "[::] ERROR: --sample-paths writes files --plan does not make; use one of them.\n"); exit(1); }
    if (has_sample_paths && (!opt_log_stats || !opt_states)) { fprintf(stderr, "[::] ERROR: --sample-paths needs --log-stats and --states: it draws paths from the distribution over all paths of the weights whose best path they find, with their --p01, --p02, --p12.\n"); exit(1); }
    if (has_seed && !has_sample_paths) { fprintf(stderr, "[::] ERROR: --seed is the seed of --sample-paths K.\n"); exit(1); }
    if (genetic_map_fn)
        gmap_read(genetic_map_fn);
    if (opt_log_stats && opt_states) {
        const double pen[3] = {opt_p01, opt_p02, opt_p12};
        static const char *const pen_name[3] = {"--p01", "--p02", "--p12"};
        for (int k = 0; k < 3; ++k)
            if (!(pen[k] > 0.0 && pen[k] <= 1.0)) {
                fprintf(stderr, "[::] ERROR: --log-stats takes log2 of the penalties: %s of %g is not in (0, 1].\n", pen_name[k], pen[k]);
                exit(1);
            }
    }
    if (opt_stats_only)
        opt_summary_only = 1;                 /* (what the engine does for it: no per-site values, batches queued ahead) */

    /* the echoed command: argv joined by single spaces, with a trailing space (:992-997) */
    size_t cmd_len = 2;
    for (int i = 0; i < argc; ++i)
        cmd_len += strlen(argv[i]) + 1;
    char *user_cmd = malloc(cmd_len);
    user_cmd[0] = 0;
    for (int i = 0; i < argc; ++i) {
        strcat(user_cmd, argv[i]);
        strcat(user_cmd, " ");
    }

    /* the pileups of the run: -P / -N, or the entries of --pileup-list (refused with a line of its own before anything is read) */
    if (list_fn) {
        if (pu_fn || has_N) {
            fprintf(stderr, "[::] ERROR: --pileup-list names the pileups and their names; it does not go with -P or -N.\n");
            exit(1);
        }
        read_pileup_list(list_fn, &g_list.jobs, &g_list.n);
        g_list_mode = 1;
        for (size_t i = 0; i < g_list.n; ++i) {
            pile_job *pj = &g_list.jobs[i];
            pj->err = open_memstream(&pj->err_buf, &pj->err_len);
            if (!pj->err)
                pj->err = stderr;
        }
    } else {
        if (!pu_fn)
            DIE("[::] ERROR parsing Pileup data; make sure input is valid.\n");
        static pile_job one;
        one.name = opt_sq;
        one.path = pu_fn;
        one.err = stderr;
        g_list.jobs = &one;
        g_list.n = 1;
    }
    g_list.fail_at = g_list.n;
    g_uchr = uchr;
    g_out_dir = out_dir;
    g_user_cmd = user_cmd;
    pile_job *const p0 = &g_list.jobs[0];
    /* start the device(s) now: ibdg_create takes ~0.2 s of runtime start-up that needs none of the inputs */
    static dev_job_t dev_job;
    if (!opt_plan) {
        dev_job.eps = opt_eps;
        dev_job.max_cov = opt_max_cov;
        char *dl = strdup(devices_arg);
        char *save = NULL;
        for (char *tok = strtok_r(dl, ",", &save); tok && dev_job.n < 64; tok = strtok_r(NULL, ",", &save))
            dev_job.dev[dev_job.n++] = atoi(tok);
        free(dl);
        if (pthread_create(&g_dev_thread, NULL, dev_start, &dev_job) != 0)
            DIE("[::] ERROR: cannot start a worker thread.\n");
        g_dev_started = 1;
    }
    pj_read(p0);
    if (p0->rc) {
        list_finish(0, 1);
        quit(1);
    }
    if (has_A && read_af_file(af_fn, uchr))
        quit(1);
    if (has_p) {
        if (read_pos_file(pos_fn, uchr))
            quit(1);
        qsort(pos_tab, pos_n, sizeof *pos_tab, cmp_ul);
    }
    if (!in_vcf && !in_impute)
        DIE("[::] ERROR: Missing genotype files.\n");
    if (in_vcf && in_impute)
        DIE("[::] ERROR: 2 types of genotype inputs detected. Please choose either IMPUTE or VCF format.\n");
    if (in_impute && (!hap_fn || !legend_fn || !indv_fn))
        DIE("[::] ERROR parsing hap/legend/indv data; make sure inputs are valid.\n");

    names_t ids = {NULL, 0};
    if (in_vcf) {
        if (read_genotypes_vcf(vcf_fn, &ids))
            quit(1);
    } else {
        if (read_names(indv_fn, &ids))
            quit(1);
        if (ids.n == 0)
            DIE("[::] ERROR: No samples found in .indv file.\n");
    }
    const unsigned n_ids = (unsigned)ids.n;
    idlist_t targets = {NULL, 0}, bg = {NULL, 0};
    if (has_S) {                                            /* -S wins over -s (:1135-1155) */
        if (read_idlist_file(sample_fn, &ids, "Sample %s not found in reference panel.\n", "read_sf", &targets))
            quit(1);
    } else if (has_s) {
        if (read_idlist_csv(sample_csv, &ids, &targets))
            quit(1);
    } else {
        targets.n = n_ids;
        targets.idx = malloc(n_ids * sizeof *targets.idx);
        for (unsigned i = 0; i < n_ids; ++i)
            targets.idx[i] = i;
    }
    uint8_t *bg_count = NULL;
    if (has_B) {
        if (read_idlist_file(bg_fn, &ids, "Reference sample %s not found in input panel.\n", "read_rf", &bg))
            quit(1);
        bg_count = calloc(n_ids, 1);
        for (size_t i = 0; i < bg.n; ++i) {
            /* the engine takes one byte per individual: a list naming somebody 256 times is refused, not truncated */
            if (bg_count[bg.idx[i]] == 255)
                DIE("[::] ERROR: Reference sample %s is listed more than 255 times in %s.\n", ids.names[bg.idx[i]], bg_fn);
            bg_count[bg.idx[i]]++;
        }
    }
    g_ids = ids;
    g_targets = targets;
    g_bg_count = bg_count;
    phase("options, pileup, names");

    if (in_impute && read_genotypes(hap_fn, legend_fn, n_ids))
        quit(1);
    phase("genotypes (hap or cache, legend)");

    pj_depth(p0);

    /* ---- engine: panel upload, alt counts back for the AF filter ---------------------- */
    ibdg_ctx *engs[64];
    int n_eng = 0;
    int host_math = 0;              /* no device and a non-LD run: the library's host twins do the arithmetic */
    double *pdg_tab = NULL;
    if (!opt_plan) {
        /* the contexts were being created (device start-up, ~0.2 s) while the inputs were parsed */
        pthread_join(g_dev_thread, NULL);
        g_dev_started = 0;
        phase("device start (the part not hidden behind parsing)");
        if (dev_job.n > 0 && !dev_job.eng[0] && !opt_ld && ibdg_device_count() == 0) {
            const size_t d = (size_t)opt_max_cov + 1;
            pdg_tab = malloc(d * d * 3 * sizeof *pdg_tab);
            if (!pdg_tab || ibdg_pdg_table(opt_eps, opt_max_cov, pdg_tab))
                DIE("[::] ERROR: cannot build the P(D|G) table.\n");
            host_math = 1;
            g_pdg_tab = pdg_tab;
            dev_job.n = 0;
            fprintf(stderr, "No HIP device found: per-row and window likelihoods are computed on the host (non-LD runs only).\n");
        }
    }
    const int no_engine = opt_plan || host_math;
    g_no_engine = no_engine;
    g_host_math = host_math;
    upload_job *const ups = g_ups;
    /* the same rows for every comparison individual unless -v looks at its genotype or -D thins the
     * reads anew for each (src/ibdgem.c:584, :627-628) */
    const int batchable = !no_engine && !has_v && p0->cull_p == 1.0;
    /* several devices and one site list: every device holds its window range's rows only (a single pileup: with a list
     * every context holds the whole panel and takes whole pileups) */
    int slice_mode = 0;
    if (!no_engine) {
        for (int d = 0; d < dev_job.n; ++d) {
            ibdg_ctx *e = dev_job.eng[d];
            if (!e)
                DIE("%s\n", dev_job.err[d] ? dev_job.err[d] : "[::] ERROR in ibdg_create");
            engs[n_eng++] = e;
        }
        if (n_eng == 0)
            DIE("[::] ERROR: --devices needs at least one device index.\n");
        slice_mode = batchable && n_eng > 1 && !g_list_mode;
        for (int d = 0; d < n_eng; ++d) {
            memset(&ups[d], 0, sizeof ups[d]);
            ups[d].eng = engs[d]; ups[d].r0 = 0; ups[d].n = n_rows; ups[d].n_ids = n_ids;
            ups[d].ref_order = opt_ref_order; ups[d].has_B = has_B; ups[d].bg_idx = bg.idx; ups[d].bg_n = bg.n;
            ups[d].n_uploads = n_eng;
            /* (a list decides this per pileup, from each one's own cull ratio: pj_run) */
            ups[d].share_sites = batchable && opt_ld && !opt_ref_order && !g_list_mode ? targets.n : 0;
        }
        if (!slice_mode) {
            /* whole panel to every device, all copies at once, under the filter chain below */
            g_n_ups = n_eng;
            uploads_start(ups, n_eng);
            g_uploads_pending = 1;
        }
    }
    if (!alt_count_h)
        DIE("[::] ERROR: no genotype rows.\n");
    pj_filter(p0);
    phase("row filter chain");

    /* the workers: one per context with a list, else one for all of them; the main thread is the first */
    static worker_t workers[MAX_WORKERS];
    const int n_workers = g_list_mode && !no_engine ? (n_eng < MAX_WORKERS ? n_eng : MAX_WORKERS) : 1;
    for (int k = 0; k < n_workers; ++k) {
        worker_t *w = &workers[k];
        const int one = n_workers > 1 || g_list_mode;        /* a context of its own */
        w->n_eng = no_engine ? 0 : one ? 1 : n_eng;
        for (int d = 0; d < w->n_eng; ++d)
            w->conv[d].eng = engs[k + d], w->conv[d].idx = k + d;
        w->ups = ups + k;
        w->n_ups = w->n_eng;
        w->ups_pending = !no_engine && !slice_mode;
        w->slice_mode = slice_mode;
        w->outs = g_outs[k];
        /* every context's first entry is its own before any worker reads ahead: a read-ahead never takes an entry while
         * a context has none (with no more entries than contexts each entry has a context to itself) */
        w->first = (size_t)k < g_list.n ? k : -1;
        w->first_ready = k == 0;
    }
    g_list.next_take = (size_t)n_workers < g_list.n ? (size_t)n_workers : g_list.n;
    g_n_workers = n_workers;
    if (n_workers > 1) {
        /* the contexts share the host's threads: each worker reads, filters and writes with its part of them */
        const int total = opt_threads > 0 ? opt_threads : default_threads();
        g_thread_share = total / n_workers > 1 ? total / n_workers : 1;
    }
    for (int k = 1; k < n_workers; ++k)
        workers[k].started = pthread_create(&workers[k].th, NULL, worker_main, &workers[k]) == 0;
    worker_main(&workers[0]);
    for (int k = 1; k < n_workers; ++k)
        if (workers[k].started)
            pthread_join(workers[k].th, NULL);
        else
            worker_main(&workers[k]);       /* (no thread to be had: whatever is left, here) */
    /* every context's panel upload is joined before anything below can tear the runtime down -- a context that took no
     * entry never joined its own -- and a failed one is reported even when its context had nothing to do */
    int up_bad = -1;
    if (g_uploads_pending) {
        up_bad = uploads_join(g_ups, g_n_ups);
        g_uploads_pending = 0;
    }
    if (g_list.fail_at < g_list.n) {
        /* entries after the failing one that ran on another context leave no files behind */
        for (size_t i = g_list.fail_at + 1; i < g_list.n; ++i)
            for (size_t f = 0; f < g_list.jobs[i].n_files; ++f)
                unlink(g_list.jobs[i].files[f]);
        quit(1);
    }
    if (up_bad >= 0)
        DIE("%s\n", ibdg_last_error(g_ups[up_bad].eng));
#if !defined(__SANITIZE_ADDRESS__) && !defined(__SANITIZE_THREAD__)
    if (getenv("IBDGEM_EXIT_PROBE")) {       /* measurement only (tools/warm_phases.py): what of the process's end is the mapping */
        if (packed_mapped_bytes)
            munmap(packed, packed_mapped_bytes);
        phase("probe: munmap of the panel cache");
    }
    if (!getenv("IBDGEM_KEEP_TEARDOWN")) {
        /* every output file is closed: leave without tearing the device contexts and the runtime down -- the driver
         * reclaims the memory of a process that ends, and freeing 5 GB of it buffer by buffer plus the runtime's
         * own exit handlers cost ~0.06 s of a 0.6 s run (the sanitizer builds keep the orderly way out) */
        fprintf(stderr, "Run time: %f minutes.\n", ((double)(clock() - t_start) / CLOCKS_PER_SEC) / 60);
        fflush(NULL);
        _exit(EXIT_SUCCESS);
    }
#endif
    for (int k = 0; k < n_workers; ++k)
        for (int d = 0; d < workers[k].n_eng; ++d)
            conv_release(&workers[k].conv[d]);
    for (int d = 0; d < n_eng; ++d)
        ibdg_destroy(engs[d]);
    phase("engine shutdown");
    if (!g_list_mode)
        pileup_free(p0->pu);
    fprintf(stderr, "Run time: %f minutes.\n", ((double)(clock() - t_start) / CLOCKS_PER_SEC) / 60);
    return EXIT_SUCCESS;
}
