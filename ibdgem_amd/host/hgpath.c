/* hgpath.c -- see hgpath.h.  Own implementation with the arithmetic and output format of the reference's second
 * program (reference src/hiddengem.c: summary reader :51-85, recurrence :103-147, traceback and output :246-283) and
 * the table of its bin/sum-hiddengem.py.
 *
 * Arithmetic follows the reference so that the printed scores are the same text: per window the three likelihoods
 * are normalised in double (l / ((l0+l1)+l2)); scores are products kept in long double; a transition multiplies
 * (previous score * window probability) * penalty, in that order; ties keep the lowest state (strict >).
 * Differences, on purpose: any number of windows (the reference holds 12288 in fixed arrays, src/hiddengem.c:8,27-33)
 * and an empty table prints the header and the three percentage lines instead of reading out of bounds. */
#include <stdlib.h>
#include <string.h>

#include "hgpath.h"
#include "lineio.h"

const char hg_header[] = "Segment\tIBD0_Score\tIBD1_Score\tIBD2_Score\tInferred_State\n";

void hg_reset(hg_path *h)
{
    h->n = 0;
    h->count[0] = h->count[1] = h->count[2] = 0;
}

void hg_free(hg_path *h)
{
    free(h->p);
    free(h->score);
    free(h->from);
    free(h->path);
    memset(h, 0, sizeof *h);
}

int hg_add(hg_path *h, double l0, double l1, double l2)
{
    if (h->n == h->cap) {
        const size_t cap = h->cap ? h->cap * 2 : 4096;
        void *p = realloc(h->p, cap * sizeof *h->p);
        if (!p)
            return 1;
        h->p = p;
        h->cap = cap;
    }
    double (*p)[3] = h->p;
    const size_t n = h->n;
    p[n][0] = l0 / (l0 + l1 + l2);
    p[n][1] = l1 / (l0 + l1 + l2);
    p[n][2] = l2 / (l0 + l1 + l2);
    h->n = n + 1;
    return 0;
}

int hg_add_summary_line(hg_path *h, const char *line)
{
    size_t start, end;
    double l0, l1, l2;
    int nsites;
    if (sscanf(line, "%*s\t%zu\t%zu\t%lf\t%lf\t%lf\t%d", &start, &end, &l0, &l1, &l2, &nsites) != 6)
        return 0;
    return hg_add(h, l0, l1, l2);
}

/* rows: SEGMENT START END LIBD0 LIBD1 LIBD2 NUM_SITES; leading '#' lines are the header, later lines that do not
 * parse are passed over (src/hiddengem.c:62-80) */
int hg_read_summary(hg_path *h, const char *fn, FILE *err)
{
    line_src *ls = ls_open_to(fn, err);
    if (!ls)
        return 1;
    hg_reset(h);
    int in_header = 1, rc = 0;
    for (char *line; !rc && (line = ls_next(ls, NULL));) {
        if (in_header && line[0] == '#')
            continue;
        in_header = 0;
        rc = hg_add_summary_line(h, line);
    }
    ls_close(ls);
    if (rc)
        fprintf(err, "[::] ERROR: out of memory for the windows of '%s'.\n", fn);
    return rc;
}

static int argmax3(const long double v[3])
{
    int m = 0;
    for (int i = 0; i < 3; ++i)
        if (v[i] > v[m])
            m = i;
    return m;
}

/* score[i][s] = best product of probabilities and switch penalties over paths ending in state s at window i;
 * from[i][s] = the state at i-1 on that path */
int hg_solve(hg_path *h, double pen01, double pen02, double pen12)
{
    const size_t n = h->n;
    void *a = realloc(h->score, (n ? n : 1) * sizeof *h->score);
    if (a)
        h->score = a;
    void *b = realloc(h->from, (n ? n : 1) * sizeof *h->from);
    if (b)
        h->from = b;
    void *c = realloc(h->path, (n ? n : 1) * sizeof *h->path);
    if (c)
        h->path = c;
    if (!a || !b || !c)
        return 1;
    double (*p)[3] = h->p;
    long double (*score)[3] = h->score;
    unsigned char (*from)[3] = h->from;
    int *path = h->path;
    const double pen[3][3] = {{1, pen01, pen02}, {pen01, 1, pen12}, {pen02, pen12, 1}};
    for (size_t i = 0; i < n; ++i) {
        for (int s = 0; s < 3; ++s) {
            if (i == 0) {
                score[0][s] = p[0][s];
                from[0][s] = (unsigned char)s;
                continue;
            }
            long double cand[3];
            for (int q = 0; q < 3; ++q) {
                cand[q] = score[i - 1][q] * p[i][s];
                if (q != s)
                    cand[q] = cand[q] * pen[q][s];
            }
            const int m = argmax3(cand);
            score[i][s] = cand[m];
            from[i][s] = (unsigned char)m;
        }
    }
    if (n) {
        path[n - 1] = argmax3(score[n - 1]);
        for (size_t i = n - 1; i > 0; --i)
            path[i - 1] = from[i][path[i]];
    }
    h->count[0] = h->count[1] = h->count[2] = 0;
    for (size_t i = 0; i < n; ++i)
        h->count[path[i]]++;
    return 0;
}

size_t hg_format_rows(const hg_path *h, size_t a, size_t b, char *buf)
{
    char *q = buf;
    for (size_t i = a; i < b; ++i)
        q += snprintf(q, HG_ROW_ROOM, "%d\t%.5Le\t%.5Le\t%.5Le\t%d\n", (int)(i + 1), h->score[i][0], h->score[i][1],
                      h->score[i][2], h->path[i]);
    return (size_t)(q - buf);
}

size_t hg_format_tail(const hg_path *h, char *buf)
{
    char *q = buf;
    for (int s = 0; s < 3; ++s) {
        const double count = (double)h->count[s];
        q += sprintf(q, "#%% IBD%d (n = %.0f): %.2f\n", s, count, (count / (int)h->n) * 100);
    }
    return (size_t)(q - buf);
}

int hg_write(FILE *f, const hg_path *h)
{
    enum { CHUNK = 256 };
    char buf[CHUNK * HG_ROW_ROOM];
    int bad = fputs(hg_header, f) < 0;
    for (size_t a = 0; a < h->n && !bad; a += CHUNK) {
        const size_t len = hg_format_rows(h, a, a + CHUNK < h->n ? a + CHUNK : h->n, buf);
        bad = fwrite(buf, 1, len, f) != len;
    }
    const size_t len = hg_format_tail(h, buf);
    bad = bad || fwrite(buf, 1, len, f) != len;
    return bad;
}

/* bin/sum-hiddengem.py:54 ("{1:d}" counts, "{5:.3f}" fractions of the path's windows); where the script would
 * divide by zero -- a path without windows -- the fractions are nan */
void hg_frac_row(FILE *f, const char *id, const size_t count[3])
{
    const size_t n = count[0] + count[1] + count[2];
    fprintf(f, "%s\t%zu\t%zu\t%zu\t%zu", id, n, count[0], count[1], count[2]);
    for (int s = 0; s < 3; ++s) {
        if (n)
            fprintf(f, "\t%.3f", (double)count[s] / (double)n);
        else
            fputs("\tnan", f);
    }
    fputc('\n', f);
}

void hg_frac_totals(FILE *f, const size_t total[3])
{
    const size_t n = total[0] + total[1] + total[2];
    fprintf(f, "# Total segments = %zu\n", n);
    for (int s = 0; s < 3; ++s) {
        if (n)
            fprintf(f, "# Total IBD%d (%%) = %.3f\n", s, ((double)total[s] / (double)n) * 100);
        else
            fprintf(f, "# Total IBD%d (%%) = nan\n", s);
    }
}
