"""Generates tests/golden/hotspot.npz: what independent code gives for the procedural cases of tests/spatial_reference.py
and tests/hotspot_reference.py (the inputs are regenerated from their seeds, so only results are stored).

    python tests/golden/gen_hotspot_goldens.py

Stored:
  ``<case>.<weights>.local_i / .lag / .gi_z``   the dense n x n W-matrix formulas (``hotspot_reference.dense_local``: I_i by
                               a matrix product with W, L_i with the binary matrix, Gi* as esda's ``G_Local(star=True)``
                               writes it from the raw values: (sum_j w*_ij x_j - W*_i xbar) / (s sqrt((n W*_i - W*_i^2) /
                               (n - 1))) with binary star weights), for univariate columns and two bivariate pairs, on the
                               STD-pruned graph with binary and with row-standardised weights.
  ``tail.z / .sf``             ``scipy.stats.norm.sf`` on a grid.
  ``draws.<seed>.<n>.<d>``     the draw tables of three (seed, n, d) triples, P = 6 draws each: a recording of the stated
                               function, so that a change of it cannot pass unnoticed.
  ``uniform.worst``            the largest deviation, in standard deviations, of a spot's frequency from d / (n - 1) on
                               n = 40, d = 8, P = 4000, seed 0.
  ``planted.*``                the planted-block case (``hotspot_reference.planted_case``) at alpha = 0.05, 199 draws, seed 0:
                               the interior spots of the block, how many of them the restatement labels HH, and how many
                               spots outside the block it labels HH.
  ``shuffle.*``                slide "mid" with a spot-shuffled copy (shuffle seed 1) as the prediction, 199 draws, seed 0:
                               the restatement's mean Pearson r of gi_z and mean Jaccard index of the HH sets.
esda and squidpy are not installed: parity with a release of either is unpinned."""
import os
import sys

import numpy as np
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hotspot_reference as hr  # noqa: E402
import spatial_reference as sr  # noqa: E402

BV_PAIRS = ((0, 3), (4, 1))
TAIL_Z = np.array([0.0, 0.3, 1.0, 1.41, 1.4143, 2.5, 5.0, 10.0, 20.0, 37.0])
DRAW_TRIPLES = ((0, 40, 8), (7, 9, 8), (123, 257, 3))
DRAW_P = 6
UNIFORM = dict(seed=0, n=40, d=8, P=4000)
SHUFFLE_SEED, N_PERMS = 1, 199


def dense_pairs(G):
    return np.concatenate([np.stack([np.arange(G), np.arange(G)], axis=1), np.asarray(BV_PAIRS)])


def uniformity(seed, n, d, P):
    """The largest |frequency - P d / (n - 1)| / sqrt(P q (1 - q)), q = d / (n - 1), over every (spot, other spot)."""
    tb = hr.draw_table(seed, P, n, np.full(n, d), d)
    q = d / (n - 1)
    worst = 0.0
    for i in range(n):
        cnt = np.bincount(tb[:, i, :].ravel(), minlength=n).astype(np.float64)
        assert cnt[i] == 0
        worst = max(worst, float(np.abs(np.delete(cnt, i) - P * q).max() / np.sqrt(P * q * (1 - q))))
    return worst


def shuffled(seed=SHUFFLE_SEED):
    c, x = sr.make_case("mid")
    return c, x, x[np.random.default_rng(seed).permutation(x.shape[0])]


def main():
    out = {}
    for name in ("small", "mid"):
        c, x = sr.make_case(name)
        for std in (False, True):
            g = sr.lattice(c, 8, "STD", std)
            d = hr.dense_local(x, g["nbr"], g["w"], dense_pairs(x.shape[1]))
            for key, v in d.items():
                out[f"{name}.{'r' if std else 'b'}.{key}"] = v
    out["tail.z"], out["tail.sf"] = TAIL_Z, stats.norm.sf(TAIL_Z)
    for seed, n, d in DRAW_TRIPLES:
        out[f"draws.{seed}.{n}.{d}"] = hr.draw_table(seed, DRAW_P, n, np.full(n, d), d).astype(np.int16)
    out["uniform.worst"] = np.float64(uniformity(**UNIFORM))
    c, x, interior, outside = hr.planted_case()
    g = sr.lattice(c, 8, "NA", True)
    r = hr.local_stats(x, g["nbr"], g["w"], n_perms=N_PERMS, seed=0, alpha=0.05)
    out["planted.interior"] = np.flatnonzero(interior)
    out["planted.interior_hh"] = np.int64((r["cluster"][interior, 0] == 1).sum())
    out["planted.outside_hh"] = np.int64((r["cluster"][outside, 0] == 1).sum())
    c, x, xs = shuffled()
    g = sr.lattice(c, 8, "NA", True)
    rt = hr.local_stats(x, g["nbr"], g["w"], n_perms=N_PERMS, seed=0)
    rp = hr.local_stats(xs, g["nbr"], g["w"], n_perms=N_PERMS, seed=0)
    rec = hr.recovery(rp, rt)
    out["shuffle.mean_pearson"] = np.float64(np.nanmean(rec["pearson"]))
    out["shuffle.mean_jaccard_hot"] = np.float64(np.nanmean(rec["jaccard_hot"]))
    out["shuffle.self_jaccard_hot"] = np.float64(np.nanmean(hr.recovery(rt, rt)["jaccard_hot"]))
    np.savez_compressed(hr.GOLDEN, **out)
    print(f"wrote {hr.GOLDEN}: {len(out)} arrays, {os.path.getsize(hr.GOLDEN)} bytes; uniform.worst = {out['uniform.worst']:.4f}, "
          f"planted {int(out['planted.interior_hh'])} / {int(interior.sum())} interior, {int(out['planted.outside_hh'])} outside; "
          f"shuffle Pearson {out['shuffle.mean_pearson']:.6f} Jaccard {out['shuffle.mean_jaccard_hot']:.6f}")


if __name__ == "__main__":
    main()
