/* hiddengem.c -- most probable path of IBD0/IBD1/IBD2 states over the windows of a summary file.
 *
 * Own implementation with the command line, messages and output format of the reference's second
 * program (reference src/hiddengem.c: options :17-24/:192-237); the summary reader, the recurrence and
 * the table are hgpath.c, shared with `ibdgem --states`.  A three-state max-product recurrence over at
 * most a few ten thousand windows is host work.
 *
 * Differences from the reference, on purpose: any number of windows, an empty table prints the header
 * and the three percentage lines, a missing -s is an error message instead of an uninitialised file
 * name, and --summary-list: the paths of a list of summary files (one per chromosome, say) on several
 * threads, with the table of the reference's bin/sum-hiddengem.py over them (--fractions). */
#define _GNU_SOURCE
#include <ctype.h>
#include <getopt.h>
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "hgpath.h"
#include "lineio.h"

static double pen01 = HG_DEFAULT_P01, pen02 = HG_DEFAULT_P02, pen12 = HG_DEFAULT_P12;

static struct option longopts[] = {{"summary", required_argument, 0, 's'}, {"p01", required_argument, 0, 1},
                                   {"p02", required_argument, 0, 2},       {"p12", required_argument, 0, 3},
                                   {"summary-list", required_argument, 0, 4}, {"out-dir", required_argument, 0, 5},
                                   {"fractions", required_argument, 0, 6}, {"threads", required_argument, 0, 7},
                                   {"help", no_argument, 0, 'h'},          {0, 0, 0, 0}};

static void usage(int code)
{
    fputs("HIDDENGEM: Finds most probable path of IBD states across genomic segments.\n\n"
          "Usage: ./hiddengem -s [summary-file] [other options...] >[out-file]\n"
          "       ./hiddengem --summary-list [list-file] [--out-dir DIR] [--fractions FILE] [other options...]\n"
          "--summary, -s  FILE      Summary file from IBDGem likelihood calculation (*.summary.txt) (required)\n"
          "--p01  FLOAT             Penalty for switching between states IBD0 and IBD1 (default: 1e-3)\n"
          "--p02  FLOAT             Penalty for switching between states IBD0 and IBD2 (default: 1e-6)\n"
          "--p12  FLOAT             Penalty for switching between states IBD1 and IBD2 (default: 1e-3)\n"
          "--summary-list  FILE     Instead of -s: a line 'NAME PATH' per summary file (one per chromosome, say);\n"
          "                         writes DIR/NAME.hiddengem.txt for each, what -s PATH prints\n"
          "--out-dir  DIR           Where --summary-list writes its tables (default: current directory)\n"
          "--fractions  FILE        With --summary-list: per NAME the number of segments in each state and their\n"
          "                         fractions, then the totals over the list (the table of sum-hiddengem.py)\n"
          "--threads  INT           Threads working through a --summary-list (default: the CPUs available, at most 16)\n"
          "--help                   Show this help message and exit\n\n"
          "Format of output table is tab-delimited with columns:\n"
          "Segment, IBD0_Score, IBD1_Score, IBD2_Score, Inferred_State\n",
          stderr);
    exit(code);
}

/* ---- --summary-list ------------------------------------------------------------------------------------------- */
typedef struct {
    char *name, *path;
    size_t line;                   /* its line of the list file */
    size_t count[3];
    char *msg;                     /* what went wrong with it, or NULL */
} list_entry;

static struct {
    list_entry *e;
    size_t n, next;
    const char *out_dir;
    pthread_mutex_t mu;
} g_list = {NULL, 0, 0, ".", PTHREAD_MUTEX_INITIALIZER};

static void entry_run(list_entry *e, hg_path *h)
{
    char *msg = NULL, *out_fn = NULL;
    size_t msg_len = 0;
    FILE *err = open_memstream(&msg, &msg_len);
    if (!err)
        exit(1);
    int bad = hg_read_summary(h, e->path, err) || hg_solve(h, pen01, pen02, pen12);
    if (!bad) {
        FILE *f = asprintf(&out_fn, "%s/%s.hiddengem.txt", g_list.out_dir, e->name) < 0 ? NULL : fopen(out_fn, "w");
        if (!f) {
            fprintf(err, "Cannot open '%s' for writing.\n", out_fn ? out_fn : e->name);
            bad = 1;
        } else {
            bad = hg_write(f, h);
            bad = fclose(f) != 0 || bad;
            if (bad)
                fprintf(err, "Cannot write '%s'.\n", out_fn);
        }
        free(out_fn);
    }
    fclose(err);
    memcpy(e->count, h->count, sizeof e->count);
    if (bad)
        e->msg = msg;              /* (never empty: every failure above leaves a message) */
    else
        free(msg);
}

static void *list_worker(void *arg)
{
    hg_path h;
    memset(&h, 0, sizeof h);
    for (;;) {
        pthread_mutex_lock(&g_list.mu);
        const size_t i = g_list.next < g_list.n ? g_list.next++ : g_list.n;
        pthread_mutex_unlock(&g_list.mu);
        if (i == g_list.n)
            break;
        entry_run(&g_list.e[i], &h);
    }
    hg_free(&h);
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

/* "NAME<whitespace>PATH" per line (the reference's *.summary-list.txt).  Every refusal names the line. */
static int read_list(const char *fn)
{
    line_src *ls = ls_open(fn);
    if (!ls)
        return 1;
    size_t cap = 0, lineno = 0;
    for (char *line; (line = ls_next(ls, NULL));) {
        lineno++;
        char *save = NULL;
        const char *name = strtok_r(line, " \t\r\n", &save), *path = strtok_r(NULL, " \t\r\n", &save);
        if (!name || !path || strtok_r(NULL, " \t\r\n", &save)) {
            fprintf(stderr, "[::] ERROR: line %zu of '%s' is not 'NAME PATH'.\n", lineno, fn);
            return 1;
        }
        if (strchr(name, '/')) {
            fprintf(stderr, "[::] ERROR: line %zu of '%s': the name '%s' holds a '/'.\n", lineno, fn, name);
            return 1;
        }
        for (size_t k = 0; k < g_list.n; ++k)
            if (!strcmp(g_list.e[k].name, name)) {
                fprintf(stderr, "[::] ERROR: line %zu of '%s' repeats the name '%s' of line %zu.\n", lineno, fn, name,
                        g_list.e[k].line);
                return 1;
            }
        if (g_list.n == cap) {
            cap = cap ? cap * 2 : 64;
            g_list.e = ls_xrealloc(g_list.e, cap * sizeof *g_list.e);
        }
        list_entry *e = &g_list.e[g_list.n++];
        memset(e, 0, sizeof *e);
        e->name = strdup(name);
        e->path = strdup(path);
        e->line = lineno;
    }
    ls_close(ls);
    if (!g_list.n) {
        fprintf(stderr, "[::] ERROR: '%s' lists no summary file.\n", fn);
        return 1;
    }
    return 0;
}

static int run_list(const char *list_fn, const char *frac_fn, int threads)
{
    if (read_list(list_fn))
        return 1;
    if (threads < 1)
        threads = default_threads();
    if (threads > 16)
        threads = 16;
    if ((size_t)threads > g_list.n)
        threads = (int)g_list.n;
    pthread_t th[16];
    int started[16] = {0};
    for (int t = 1; t < threads; ++t)
        started[t] = pthread_create(&th[t], NULL, list_worker, NULL) == 0;
    list_worker(NULL);
    for (int t = 1; t < threads; ++t)
        if (started[t])
            pthread_join(th[t], NULL);
    int bad = 0;
    for (size_t i = 0; i < g_list.n; ++i)
        if (g_list.e[i].msg) {
            fprintf(stderr, "[::] ERROR: line %zu of '%s' (%s): %s", g_list.e[i].line, list_fn, g_list.e[i].name, g_list.e[i].msg);
            bad = 1;
        }
    if (!bad && frac_fn) {
        FILE *f = fopen(frac_fn, "w");
        if (!f) {
            fprintf(stderr, "[::] ERROR: Cannot open '%s' for writing.\n", frac_fn);
            bad = 1;
        } else {
            size_t total[3] = {0, 0, 0};
            fputs("CHROM\tN_SEGMENTS\tN_IBD0\tN_IBD1\tN_IBD2\tFRAC_IBD0\tFRAC_IBD1\tFRAC_IBD2\n", f);
            for (size_t i = 0; i < g_list.n; ++i) {
                hg_frac_row(f, g_list.e[i].name, g_list.e[i].count);
                for (int s = 0; s < 3; ++s)
                    total[s] += g_list.e[i].count[s];
            }
            hg_frac_totals(f, total);
            if (fclose(f) != 0) {
                fprintf(stderr, "[::] ERROR writing '%s'.\n", frac_fn);
                unlink(frac_fn);
                bad = 1;
            }
        }
    }
    for (size_t i = 0; i < g_list.n; ++i) {
        free(g_list.e[i].name);
        free(g_list.e[i].path);
        free(g_list.e[i].msg);
    }
    free(g_list.e);
    return bad;
}

int main(int argc, char **argv)
{
    const char *summary_fn = NULL, *list_fn = NULL, *frac_fn = NULL;
    int threads = 0, has_out_dir = 0, has_threads = 0;
    if (argc == 1)
        usage(0);
    int o;
    while ((o = getopt_long(argc, argv, ":s:h", longopts, NULL)) != -1) {
        switch (o) {
        case 's': summary_fn = optarg; break;
        case 1: pen01 = atof(optarg); break;
        case 2: pen02 = atof(optarg); break;
        case 3: pen12 = atof(optarg); break;
        case 4: list_fn = optarg; break;
        case 5: g_list.out_dir = optarg; has_out_dir = 1; break;
        case 6: frac_fn = optarg; break;
        case 7: threads = atoi(optarg); has_threads = 1; break;
        case 'h': usage(0); break;
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
    if (list_fn && summary_fn) {
        fprintf(stderr, "[::] ERROR: --summary-list takes the place of -s; use one of them.\n");
        return 1;
    }
    if (!list_fn && (has_out_dir || frac_fn || has_threads)) {
        fprintf(stderr, "[::] ERROR: --out-dir, --fractions and --threads belong to --summary-list.\n");
        return 1;
    }
    if (list_fn)
        return run_list(list_fn, frac_fn, threads);
    if (!summary_fn) {
        fprintf(stderr, "[::] ERROR parsing likelihood data; make sure input is valid.\n");
        return 1;
    }
    hg_path h;
    memset(&h, 0, sizeof h);
    if (hg_read_summary(&h, summary_fn, stderr) || hg_solve(&h, pen01, pen02, pen12))
        return 1;
    const int bad = hg_write(stdout, &h);
    hg_free(&h);
    return bad;
}
