/* hgpath.h -- the IBD-state path over the windows of one summary table: the max-product recurrence, the traceback
 * and the table `hiddengem` prints, shared by `hiddengem` (one summary file, or a list of them) and `ibdgem --states`
 * (every comparison individual of a run, inside its output job).  The arithmetic is the one place that decides the
 * printed text (hgpath.c); both programs feed it the three likelihoods of a window as a summary file presents them. */
#ifndef IBDG_HGPATH_H
#define IBDG_HGPATH_H
#include <stddef.h>
#include <stdio.h>

typedef struct {
    size_t n, cap;                 /* windows held / room (the arrays grow: no fixed limit) */
    double (*p)[3];                /* per window: l / ((l0 + l1) + l2), in double */
    long double (*score)[3];       /* hg_solve: best product over paths ending in state s at window i */
    unsigned char (*from)[3];      /* ... and the state at i - 1 on that path */
    int *path;                     /* ... the traceback */
    size_t count[3];               /* ... windows per state */
} hg_path;

#define HG_DEFAULT_P01 0.001
#define HG_DEFAULT_P02 0.000001
#define HG_DEFAULT_P12 0.001
#define HG_ROW_ROOM 96             /* bytes that hold any row of the table */

void hg_reset(hg_path *h);                                   /* n = 0; the arrays are kept */
int hg_add(hg_path *h, double l0, double l1, double l2);     /* append a window; 1: out of memory */
/* A row of a summary file (SEGMENT START END LIBD0 LIBD1 LIBD2 NUM_SITES): appended when it parses, passed over when
 * it does not.  1: out of memory. */
int hg_add_summary_line(hg_path *h, const char *line);
int hg_read_summary(hg_path *h, const char *fn, FILE *err);  /* a whole *.summary.txt (plain or .gz); 1: failed, message on err */
int hg_solve(hg_path *h, double p01, double p02, double p12);   /* 1: out of memory */
size_t hg_format_rows(const hg_path *h, size_t a, size_t b, char *buf);   /* rows [a, b) into buf (HG_ROW_ROOM each); bytes written */
size_t hg_format_tail(const hg_path *h, char *buf);          /* the three "#% IBDk" lines (256 bytes hold them) */
extern const char hg_header[];                               /* the table's first line */
int hg_write(FILE *f, const hg_path *h);                     /* header, rows, tail; 1: a write failed */
void hg_free(hg_path *h);

/* The table of bin/sum-hiddengem.py: one row per path (counts, fractions), then the totals. */
void hg_frac_row(FILE *f, const char *id, const size_t count[3]);
void hg_frac_totals(FILE *f, const size_t total[3]);
#endif
