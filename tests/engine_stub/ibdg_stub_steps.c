/* The step shifts (include/ibdgem_hip.h) for the recording stand-in of ibdg_stub.c: the host program links
 * against these names whether or not a run uses --switch-scale.  The stand-in's numbers mean nothing, so the shifts change none
 * of them: the three twins are their namesakes without chains and shifts, the setter takes any array and keeps whether there is
 * one.  Nothing here is written to a trace (the traces on record were made without the option, and these calls are not made
 * without it). */
#include <pthread.h>
#include "../../include/ibdgem_hip.h"

static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;
static int g_steps;                      /* (of the last call on any context: the stand-in's contexts are opaque here) */

int ibdg_log2_states_steps_host(const double *tab, size_t n, double p01, double p02, double p12, uint8_t *path, int64_t *score,
                                uint64_t count[3], const uint32_t *starts, size_t n_starts, const int32_t *shift)
{
    return ibdg_log2_states_host(tab, n, p01, p02, p12, path, score, count);
}

int ibdg_log2_posteriors_steps_host(const double *tab, size_t n, double p01, double p02, double p12, double *post, double expect[3],
                                    double *log2_z, const uint32_t *starts, size_t n_starts, const int32_t *shift)
{
    return ibdg_log2_posteriors_host(tab, n, p01, p02, p12, post, expect, log2_z);
}

int ibdg_log2_segments_steps_host(const double *tab, size_t n, double p01, double p02, double p12, int with_post, const uint64_t *pf,
                                  const uint64_t *pl, ibdg_segment *seg, size_t cap, uint64_t *n_seg, uint64_t sum[12],
                                  const uint32_t *starts, size_t n_starts, const int32_t *shift)
{
    return ibdg_log2_segments_host(tab, n, p01, p02, p12, with_post, pf, pl, seg, cap, n_seg, sum);
}

int ibdg_set_window_steps(ibdg_ctx *c, const int32_t *shift, size_t n)
{
    pthread_mutex_lock(&g_mu);
    g_steps = n != 0;
    pthread_mutex_unlock(&g_mu);
    return 0;
}

int ibdg_has_window_steps(const ibdg_ctx *c)
{
    pthread_mutex_lock(&g_mu);
    const int r = g_steps;
    pthread_mutex_unlock(&g_mu);
    return r;
}
