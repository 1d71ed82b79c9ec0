"""The preconditions of tests/test_gpu_bg_edges.py, asserted from the arrays of tests/bg_cases.py alone (CPU tier): what every
case's name says about chunks, half chunks, groups of eight, lanes and multiplicities is counted here from the refids list,
independently of hp_ref.background, so a later edit of the cases cannot quietly lose it; the truths are normal doubles (or
NaN where the background is empty), the oracle agrees with them, and four wrong models of the exclusions each move some
case's truth: a kernel that made that mistake could not pass."""
import numpy as np
import pytest

import bg_cases as BC
import hp_ref as H

LD = H.LD
FORM_T = (1, 4, 5, 9, 15, 16, 31)
_TRUTH = {}


def counts(c):
    """Multiplicity per individual, counted from the list."""
    return np.bincount(c["refids"], minlength=c["n_ids"]) if len(c["refids"]) else np.zeros(c["n_ids"], dtype=np.int64)


def block_sums(weights, size):
    w = np.zeros(-(-len(weights) // size) * size, dtype=np.int64)
    w[:len(weights)] = weights
    return w.reshape(-1, size).sum(axis=1)


def weights_of(c, t):
    """The weights a run of comparison individual t sums with: the list's multiplicities, pu's and t's own zeroed."""
    w = counts(c).copy()
    w[t] = 0
    if c["pu"] >= 0:
        w[c["pu"]] = 0
    return w


def n_refpanel(c, t):
    """src/ibdgem.c:737-750: the list's length, one less for every entry that is the -N individual or the comparison one."""
    n = len(c["refids"])
    for idx in c["refids"].tolist():
        if idx == c["pu"] or idx == t:
            n -= 1
    return n


def checked_individuals(name):
    c = BC.make_case(name)
    out = []
    for T in FORM_T:
        for i in BC.checked(name, T):
            if c["targets"](T)[i] not in out:
                out.append(c["targets"](T)[i])
    return out


def truth(name, t):
    if (name, t) not in _TRUTH:
        c = BC.make_case(name)
        _TRUTH[name, t] = H.ld_truth(c["alle"], c["nr"], c["na"], t, c["W"], H.binomial_factors(c["eps"], c["M"]), c["refids"], c["pu"])
    return _TRUTH[name, t]


def test_shapes_windows_and_comparison_individuals():
    for name in BC.NAMES:
        c = BC.make_case(name)
        n = c["n_ids"]
        cov = c["nr"].astype(int) + c["na"]
        assert n == (520 if name.startswith("B-") else 130) and c["alle"].shape == (3 * 33 + 17, 2 * n), name
        assert c["eps"] == 0.02 and c["M"] == 20 and c["W"] == 33 and cov.min() >= 1 and cov.max() <= 20, name
        wins = H.windows(c["nr"], c["na"], c["W"])
        assert [len(r) for r in wins] == [33, 33, 33, 17], name
        assert all(r[0] // 32 != r[-1] // 32 for r in wins[:3]), name               # whole windows straddle the 32-row tiles
        m = counts(c)
        assert (m == c["mult"]).all() and m.max() <= 255 and (np.diff(c["refids"]) >= 0).all(), name
        full = c["targets"](31)
        assert len(set(full)) == 31 and full[0] == c["target"] and all(0 <= t < n for t in full), name
        for T in FORM_T:
            assert c["targets"](T) == full[:T] and T < n - 1, (name, T)             # (no form's group rule ever skips a case)
            assert BC.checked(name, T)[0] == 0 and BC.checked(name, T)[-1] == T - 1 and len(BC.checked(name, T)) <= 4
        if name != "pu-is-target":
            assert c["pu"] not in full, name
        assert BC.make_case(name) is c                                              # seeded and made once
    # three chunks, the last with two lanes, five half chunks with somebody in them; nine chunks = two chunk groups, whose 18
    # half chunks (the last one all padding) mfma_wg_sum adds up in groups of 8, 8 and 2
    assert len(block_sums(np.ones(130), 64)) == 3 and 130 - 128 == 2 and len(block_sums(np.ones(130), 32)) == 5
    assert len(block_sums(np.ones(520), 64)) == 9 and block_sums(np.ones(9), 8).tolist() == [8, 1]
    assert block_sums(np.ones(2 * 9), 8).tolist() == [8, 8, 2] and block_sums(np.ones(520), 32).tolist() == [32] * 16 + [8]


def test_every_claim_of_the_table():
    C = {name: BC.make_case(name) for name in BC.NAMES}
    M = {name: counts(C[name]) for name in BC.NAMES}
    W = {name: weights_of(C[name], C[name]["target"]) for name in BC.NAMES}         # what the target's own run sums with

    c, m = C["chunk-empty"], M["chunk-empty"]
    assert block_sums(m, 64).tolist() == [64, 0, 2] and c["target"] == 64 and (c["target"] >> 6, c["target"] & 63) == (1, 0)
    assert all(not 64 <= t < 128 for t in c["targets"](31)[1:]) and c["pu"] == -1

    c, m = C["own-chunk-otherwise-empty"], M["own-chunk-otherwise-empty"]
    assert c["target"] == 70 and m[70] == 2 and block_sums(m, 64).tolist() == [64, 2, 2]
    assert block_sums(W["own-chunk-otherwise-empty"], 64).tolist() == [64, 0, 2]  # the masked sum over the own chunk: 63 zeros

    m = M["half-chunks-empty"]
    assert block_sums(m, 32).tolist() == [32, 0, 0, 32, 2] and block_sums(m, 64).tolist() == [32, 32, 2]
    assert [int(m[t]) for t in C["half-chunks-empty"]["targets"](3)] == [1, 0, 1]

    c, m = C["one-lane-per-chunk"], M["one-lane-per-chunk"]
    assert np.flatnonzero(m).tolist() == [0, 127, 129] and block_sums(m, 64).tolist() == [1, 1, 1] and m.max() == 1
    assert block_sums(m, 32).tolist() == [1, 0, 0, 1, 1]                           # waves of k_ld_mfma with one weighted lane, and none
    assert all(m[t] == 0 for t in c["targets"](31))

    m = M["tail-only"]
    assert np.flatnonzero(m).tolist() == [128, 129] and block_sums(m, 64).tolist() == [0, 0, 2]
    assert C["tail-only"]["targets"](2)[1] == 128                                  # ... and a comparison individual inside it

    for name, only in (("single-first", 0), ("single-last", 129)):
        c, m = C[name], M[name]
        assert np.flatnonzero(m).tolist() == [only] and m[only] == 1 and only not in c["targets"](31) and c["pu"] == -1
        assert all(n_refpanel(c, t) == 1 for t in c["targets"](31))

    c, m = C["empty"], M["empty"]
    assert np.flatnonzero(m).tolist() == [c["target"]] and c["pu"] == -1 and n_refpanel(c, c["target"]) == 0
    assert all(n_refpanel(c, t) == 1 for t in c["targets"](31)[1:])

    c, m = C["empty-by-pu"], M["empty-by-pu"]
    assert sorted(np.flatnonzero(m).tolist()) == sorted([c["target"], c["pu"]]) and c["pu"] != c["target"] and c["pu"] >= 0
    assert n_refpanel(c, c["target"]) == 0 and len(c["refids"]) == 2               # either exclusion alone leaves one
    assert all(n_refpanel(c, t) == 1 for t in c["targets"](31)[1:])

    for name in ("mult-255", "B-mult-255"):
        c, m = C[name], M[name]
        n = c["n_ids"]
        assert all(m[i] == (255 if i % 7 == 0 else 0 if i % 11 == 0 else 1) for i in range(n)), name
        assert m[c["target"]] == 255 and m[c["pu"]] == 255 and c["pu"] != c["target"] and m.max() == 255
        assert [int(m[t]) for t in c["targets"](3)] == ([255, 0, 1] if n == 130 else [255, 255, 0])
        assert (block_sums(m, 64) > 0).all()
    assert n_refpanel(C["B-mult-255"], 70) == 255 * 73 + int((M["B-mult-255"] == 1).sum()) == 19019     # tens of thousands
    assert n_refpanel(C["mult-255"], 70) == 255 * 17 + int((M["mult-255"] == 1).sum()) == 4436

    c, m = C["mult-edges"], M["mult-edges"]
    at = [i for i in range(130) if i & 63 in (0, 31, 32, 63)]
    assert at == [0, 31, 32, 63, 64, 95, 96, 127, 128]
    assert [int(m[i]) for i in at] == [0, 1, 2, 3, 128, 255, 0, 1, 2] and (np.delete(m, at) == 1).all()
    assert set(int(m[i]) for i in at) == {0, 1, 2, 3, 128, 255} and [int(m[t]) for t in c["targets"](3)] == [255, 128, 0]

    c = C["pu-next-to-target"]
    assert c["pu"] == c["target"] + 1 and c["pu"] // 32 == c["target"] // 32 and (M["pu-next-to-target"] == 1).all()
    c = C["pu-lane63-other-chunk"]
    assert c["pu"] == 127 and c["pu"] & 63 == 63 and c["target"] >> 6 == 0 and (M["pu-lane63-other-chunk"] == 1).all()
    c = C["pu-in-tail"]
    assert c["pu"] == 129 and (M["pu-in-tail"] == 1).all()
    c, m = C["pu-unlisted"], M["pu-unlisted"]
    assert c["pu"] >= 0 and m[c["pu"]] == 0 and (np.delete(m, c["pu"]) == 1).all()
    c = C["pu-is-target"]
    assert c["pu"] == c["target"] == c["targets"](1)[0] and (M["pu-is-target"] == 1).all() and n_refpanel(c, c["target"]) == 129

    c, m = C["targets-unlisted"], M["targets-unlisted"]
    assert all(m[t] == 0 for t in c["targets"](31)) and np.flatnonzero(m == 0).tolist() == sorted(c["targets"](31))
    assert all(n_refpanel(c, t) == len(c["refids"]) for t in c["targets"](31)) and m.max() == 2 and c["pu"] == -1

    c, m = C["group-in-one-half"], M["group-in-one-half"]
    assert c["targets"](15) == list(range(64, 79)) and {t // 32 for t in c["targets"](15)} == {2}       # one wave of k_ld_mfma
    assert [int(m[t]) for t in range(64, 79)] == [1, 2, 3] * 5 and all(not 64 <= t < 96 for t in c["targets"](31)[15:])
    assert [c["targets"](15)[i] for i in BC.checked("group-in-one-half", 15)] == [64, 71, 78]

    c, m = C["B-first-group-empty"], M["B-first-group-empty"]
    assert block_sums(m, 64).tolist() == [0] * 8 + [8] and block_sums(m, 512).tolist() == [0, 8]        # chunk groups of eight
    assert block_sums(block_sums(m, 32), 8).tolist() == [0, 0, 8]                  # mfma_wg_sum: two whole groups of zeros
    assert np.flatnonzero(m).tolist() == list(range(512, 520)) and [int(m[t]) for t in c["targets"](3)] == [0, 1, 0]
    m = M["B-second-group-empty"]
    assert block_sums(m, 64).tolist() == [64] * 8 + [0] and block_sums(m, 512).tolist() == [512, 0]
    assert block_sums(block_sums(m, 32), 8).tolist() == [256, 256, 0] and C["B-second-group-empty"]["target"] >> 6 == 8

    # the largest multiplicity over all cases is the ABI's, and everything between an empty background and tens of thousands occurs
    assert max(int(M[name].max()) for name in BC.NAMES) == 255
    sizes = sorted({n_refpanel(C[name], C[name]["target"]) for name in BC.NAMES})
    assert sizes[:3] == [0, 1, 2] and sizes[-1] > 18000, sizes


@pytest.mark.parametrize("name", BC.NAMES)
def test_background_sizes_and_truths(oracle, name):
    """n_refpanel counted over the list as the reference counts it is the truth's n_bg; the sum of the weights agrees; every
    truth of a non-empty background is a normal double (the bounds' absolute term A 2^-1074 excuses nothing), an empty
    one gives NaN in both columns; the oracle is within 1e-10 of the truth, NaN where it is NaN."""
    c = BC.make_case(name)
    for t in checked_individuals(name):
        tr = truth(name, t)
        assert n_refpanel(c, t) == tr["n_bg"] == int(weights_of(c, t).sum()), (name, t)
        empty = name in BC.EMPTY and t == c["target"]
        assert (tr["n_bg"] == 0) == empty, (name, t)
        res = oracle.compare(c["alle"], c["nr"], c["na"], t, window=c["W"], eps=c["eps"], max_cov=c["M"], refids=c["refids"],
                             pu_id=c["pu"])["win"]
        assert res.shape == (4, 3) and np.isfinite(res[:, 2]).all()
        for col, key in ((0, "ibd0"), (1, "ibd1")):
            if empty:
                assert np.isnan(tr[key]).all() and np.isnan(res[:, col]).all(), (name, t, key)
                continue
            assert (tr[key] >= LD(2.0) ** -1022).all() and np.isfinite(tr[key]).all(), (name, t, key)
            rel = np.abs(res[:, col].astype(LD) - tr[key]) / tr[key]
            assert float(rel.max()) <= 1e-10, (name, t, key, float(rel.max()))
    lo = min(float(np.log2(truth(name, t)[k].min())) for t in checked_individuals(name) for k in ("ibd0", "ibd1")
             if truth(name, t)["n_bg"])
    print(f"{name}: {len(checked_individuals(name))} individuals, smallest truth 2^{lo:.0f}")


# --------------------------------------------------------------------------- teeth
def _moved(wrong, right):
    """Largest relative move of a window value (0 where both are NaN; inf where one is)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(wrong - right) / np.abs(right)
    rel = np.where(np.isnan(wrong) & np.isnan(right), LD(0), rel)
    return float(np.where(np.isnan(rel), LD(np.inf), rel).max())


def wrong_model(model, name, t):
    """The two columns a kernel with one mistake in the exclusions would give, from hp_ref.ld_truth.
      1  the comparison individual is not excluded: a twin of it (its haplotypes, a new index) takes its entries of the list;
      2  the background size is reduced by 1 instead of by the individual's multiplicity (k_target_weights: base_sum -
         base_w[tgt]): the right sums over the wrong size;
      3  pu is left out of the sum but not out of the size: the right sums over a size with pu's entries in it;
      4  a zero multiplicity is counted as one: everybody unlisted enters the list once."""
    c = BC.make_case(name)
    fac = H.binomial_factors(c["eps"], c["M"])
    right = truth(name, t)
    m = counts(c)
    if model == 1:
        n = c["n_ids"]
        alle = np.concatenate([c["alle"], c["alle"][:, 2 * t:2 * t + 2]], axis=1)
        refids = np.where(c["refids"] == t, n, c["refids"])
        tr = H.ld_truth(alle, c["nr"], c["na"], t, c["W"], fac, refids, c["pu"])
        return tr["ibd0"], tr["ibd1"]
    if model == 4:
        tr = H.ld_truth(c["alle"], c["nr"], c["na"], t, c["W"], fac, np.repeat(np.arange(c["n_ids"]), np.maximum(m, 1)), c["pu"])
        return tr["ibd0"], tr["ibd1"]
    base_sum = int(m.sum()) - (int(m[c["pu"]]) if c["pu"] >= 0 else 0)             # set_background (ibdg_api.cpp)
    if model == 2:
        size = base_sum - 1
    else:
        size = right["n_bg"] + (int(m[c["pu"]]) if c["pu"] >= 0 and c["pu"] != t else 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = LD(right["n_bg"]) / LD(size)
        return right["ibd0"] * scale, right["ibd1"] * scale


@pytest.mark.parametrize("model", [1, 2, 3, 4])
def test_a_wrong_exclusion_moves_some_case(model):
    caught = {}
    for name in BC.NAMES:
        c = BC.make_case(name)
        t = c["target"]
        right = truth(name, t)
        w0, w1 = wrong_model(model, name, t)
        move = max(_moved(w0, right["ibd0"]), _moved(w1, right["ibd1"]))
        if move > 1e-10:
            caught[name] = move
    print(f"wrong model {model}: moves the target's truth in {len(caught)} cases: "
          + ", ".join(f"{k} {v:.2g}" for k, v in caught.items()))
    # a move between numbers (not only a NaN that comes or goes) in at least one case
    assert max(v for v in caught.values() if np.isfinite(v)) >= 0.05, model
    expected = {1: "own-chunk-otherwise-empty", 2: "mult-255", 3: "pu-lane63-other-chunk", 4: "chunk-empty"}[model]
    assert expected in caught, (model, caught)
