"""The step-shift patterns that the host tests and the GPU tier share, by name."""
import numpy as np

import hp_post_ref as H

BIG = 1 << 30


def shift_sets(n):
    """{name: int32 [n]}: random shifts within +-20 bits that are no multiples of 256; +-2^30 (the sign alternates from border to
    border) on every block's first window w0 = k C, on w0 - 1 and on w0 + 1, 0 elsewhere; every window at -2^30."""
    C = H.blocking(n)[0]
    rng = np.random.default_rng(4099 * n)
    rnd = rng.integers(-20 * 65536, 20 * 65536, n)
    rnd += (rnd % 256 == 0)
    assert (rnd % 256 != 0).all() and np.abs(rnd).max() <= 20 * 65536
    sets = {"random": rnd}
    for name, d in (("w0", 0), ("w0-1", -1), ("w0+1", 1)):
        s = np.zeros(n, dtype=np.int64)
        for k, w0 in enumerate(range(C, n, C)):
            if 1 <= w0 + d < n:
                s[w0 + d] = BIG if k % 2 == 0 else -BIG
        sets[name] = s
    sets["all-min"] = np.full(n, -BIG)
    return {k: v.astype(np.int32) for k, v in sets.items()}


def finite_table(n, seed=0):
    """Random logs without NaN or infinities, the columns within +-8 bits: with every switch weight 0 (all-min) a state whose
    emission weight is 0 in one window would be dead for the whole table, and three such windows leave Z = 0."""
    rng = np.random.default_rng(577 * n + seed)
    return rng.normal(-300.0, 40.0, (n, 1)) + rng.uniform(-8.0, 8.0, (n, 3))
