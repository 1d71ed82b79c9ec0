/* The fit of the switch penalties (include/ibdgem_hip.h) for the recording stand-in of ibdg_stub.c: the host program
 * links against these names whether or not a run uses --fit-penalties.  The stand-in keeps a count and no table; its numbers
 * mean nothing: every step keeps the penalties and stands at once.  Nothing here is written to a trace (the traces on record
 * were made without the option, and these calls are not made without it). */
#include <string.h>
#include "../../include/ibdgem_hip.h"

static size_t store_cap, store_count;

int ibdg_switch_fit_step(const double p[3], const double total[3], size_t n_individuals, const double prior[3],
                         const uint64_t counted[3], ibdg_fit_row *row, double next[3], int *stood)
{
    for (int k = 0; k < 3; ++k)
        row->p[k] = next[k] = p[k], row->total[k] = total[k], row->prior[k] = prior[k], row->counted[k] = counted[k];
    *stood = 1;
    return 0;
}

int ibdg_log2_fit_host(const double *const *tabs, size_t n_individuals, size_t n_win, const double p[3], const uint32_t *starts,
                       size_t n_starts, const int32_t *shift, size_t max_iter, ibdg_fit_row *rows, size_t *n_rows, int *stood,
                       double fitted[3])
{
    const double zero[3] = {0.0, 0.0, 0.0}, one[3] = {1.0, 1.0, 1.0};
    const uint64_t counted[3] = {n_win ? n_win - 1 : 0, n_win ? n_win - 1 : 0, n_win ? n_win - 1 : 0};
    *n_rows = 0, *stood = 0;
    memcpy(fitted, p, 3 * sizeof *fitted);
    if (max_iter && n_individuals) {
        ibdg_switch_fit_step(p, zero, n_individuals, one, counted, &rows[0], fitted, stood);
        *n_rows = 1;
    }
    return 0;
}

int ibdg_log2_store_reserve(ibdg_ctx *c, size_t n_individuals)
{
    store_cap = n_individuals, store_count = 0;
    return 0;
}

int ibdg_log2_store_append(ibdg_ctx *c)
{
    if (store_count + ibdg_num_targets(c) > store_cap)
        return 1;
    store_count += ibdg_num_targets(c);
    return 0;
}

size_t ibdg_log2_store_count(ibdg_ctx *c) { return store_count; }

int ibdg_log2_store_switches(ibdg_ctx *c, double p01, double p02, double p12, double *expect)
{
    memset(expect, 0, store_count * 3 * sizeof *expect);
    return 0;
}

int ibdg_log2_store_fit(ibdg_ctx *c, const double p[3], size_t max_iter, ibdg_fit_row *rows, size_t *n_rows, int *stood, double fitted[3])
{
    return ibdg_log2_fit_host(NULL, store_count, ibdg_num_windows(c), p, NULL, 0, NULL, max_iter, rows, n_rows, stood, fitted);
}
