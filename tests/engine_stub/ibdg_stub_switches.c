/* The switches (include/ibdgem_hip.h) for the recording stand-in of ibdg_stub.c: the host program links against
 * these names whether or not a run uses --switches.  The stand-in's numbers mean nothing: no step switches, every step w >= 1 is
 * counted, the prior is one switch per pair.  Nothing here is written to a trace (the traces on record were made without the
 * option, and these calls are not made without it). */
#include <string.h>
#include "../../include/ibdgem_hip.h"

int ibdg_log2_switches_host(const double *tab, size_t n, double p01, double p02, double p12, const uint32_t *starts, size_t n_starts,
                            const int32_t *shift, double *sw, double expect[3], uint64_t counted[3])
{
    if (sw)
        memset(sw, 0, n * 3 * sizeof *sw);
    for (int k = 0; k < 3; ++k) {
        expect[k] = tab ? 0.0 : 1.0;
        counted[k] = n ? n - 1 : 0;
    }
    return 0;
}

int ibdg_window_log2_switches(ibdg_ctx *c, double p01, double p02, double p12, double *sw, double *expect)
{
    const size_t T = ibdg_num_targets(c), n = ibdg_num_windows(c);
    memset(expect, 0, T * 3 * sizeof *expect);
    if (sw)
        memset(sw, 0, T * n * 3 * sizeof *sw);
    return 0;
}

int ibdg_window_log2_switches_prior(ibdg_ctx *c, double p01, double p02, double p12, double expect[3], uint64_t counted[3])
{
    return ibdg_log2_switches_host(NULL, ibdg_num_windows(c), p01, p02, p12, NULL, 0, NULL, NULL, expect, counted);
}

int ibdg_switch_penalty_update(const double p[3], const double total[3], size_t n_individuals, const double prior[3], double next[3])
{
    for (int k = 0; k < 3; ++k) {
        const int ok = total[k] > 0.0 && prior[k] > 0.0 && total[k] - total[k] == 0.0 && prior[k] - prior[k] == 0.0;
        double x = ok ? p[k] * total[k] / ((double)n_individuals * prior[k]) : p[k];
        x = ok && x < 1e-300 ? 1e-300 : x;
        next[k] = ok && x > 1.0 ? 1.0 : x;
    }
    return 0;
}
