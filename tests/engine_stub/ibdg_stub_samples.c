/* The sampled paths (include/ibdgem_hip.h) for the recording stand-in of ibdg_stub.c: the host program links
 * against these names whether or not a run uses --sample-paths.  The stand-in's numbers mean nothing: every draw puts all its
 * windows into IBD0, as one segment.  Nothing here is written to a trace (the traces on record were made without the option,
 * and these calls are not made without it). */
#include <string.h>
#include "../../include/ibdgem_hip.h"

int ibdg_log2_samples_host(const double *tab, size_t n, double p01, double p02, double p12, const uint32_t *starts, size_t n_starts,
                           const int32_t *shift, size_t n_samples, uint64_t seed, uint64_t stream, const uint64_t *pf,
                           const uint64_t *pl, uint8_t *paths, uint64_t *out)
{
    memset(out, 0, n_samples * 15 * sizeof *out);
    if (paths)
        memset(paths, 0, n_samples * n);
    for (size_t k = 0; k < n_samples && n; ++k) {
        uint64_t *r = out + 15 * k;
        r[0] = n, r[3] = 1, r[6] = n;
        r[9] = r[12] = pf ? pl[n - 1] - pf[0] + 1 : 0;
    }
    return 0;
}

int ibdg_window_log2_samples(ibdg_ctx *c, double p01, double p02, double p12, size_t n_samples, uint64_t seed, const uint64_t *stream,
                             const uint64_t *pf, const uint64_t *pl, uint64_t *out)
{
    const size_t T = ibdg_num_targets(c), n = ibdg_num_windows(c);
    for (size_t t = 0; t < T; ++t)
        ibdg_log2_samples_host(NULL, n, p01, p02, p12, NULL, 0, NULL, n_samples, seed, stream[t], pf, pl, NULL, out + t * n_samples * 15);
    return 0;
}

int ibdg_get_log2_sample_path(ibdg_ctx *c, size_t t, size_t k, uint8_t *path)
{
    memset(path, 0, ibdg_num_windows(c));
    return 0;
}
