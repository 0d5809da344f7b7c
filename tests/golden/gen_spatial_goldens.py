"""Generates tests/golden/spatial.npz: what independent code gives for the procedural cases of tests/spatial_reference.py
(``make_case`` regenerates the inputs from the seed, so only results are stored), and the restatement's own largest error
against each.

    python tests/golden/gen_spatial_goldens.py --reference <checkout of the reference project>

Stored:
  ``<case>.adj.<prune>.<k>``   the reference's own ``calcADJ(coords, k, 'euclidean', prune)`` (baselines/His2ST/
                               graph_construction.py, imported from the given checkout and only run, never copied), as
                               packed bits.  The coordinates obey a GAP CONDITION asserted here: in no row are the k-th and
                               (k + 1)-th nearest distances, a distance and the STD boundary, or a distance and 2.0 within
                               1e-9 relative of each other, so neither ``calcADJ``'s unstable ``argsort`` nor a rounding can
                               decide an edge, and the restatement must reproduce the adjacency exactly.
  ``lattice.nbr / .deg``       an exact integer lattice (every distance tied) by the restatement alone: pins the tie rule
                               "ascending (distance, index)", which ``calcADJ`` leaves to its sort.
  ``<case>.I / .C / .S``       the dense formulas: I = (n / S0) z'Wz / z'z by matrix products, C by explicit double loops,
                               S1 from W + W', S2 from the row and column sums (STD-pruned directed graph, both weightings).
  ``<case>.simI / .simC``      the same on ``x[perm]`` with numpy's own gather, for the recorded ``<case>.perms``.
  ``tail.*``                   ``scipy.stats.norm.sf`` on a grid, and mpmath's -log10 of both tails at |z| = 40 and 80.
  ``bh.*``                     ``scipy.stats.false_discovery_control``.
  ``*.err_*``                  the restatement's largest relative error against each of these, for the GPU bounds.
squidpy and esda are not installed: parity with a release of either is unpinned."""
import argparse
import importlib.util
import os
import sys

import mpmath
import numpy as np
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spatial_reference as sr  # noqa: E402

KS = (4, 8)
GAP = 1e-9
PERM_SEED, PERM_P = 7, 3
TAIL_Z = np.array([0.0, 0.3, 1.0, 1.41, 1.4143, 2.5, 5.0, 10.0, 20.0, 37.0])
TAIL_MP = (40.0, 80.0)
LATTICE = dict(gr=5, gc=6, seed=1)


def rel(a, b):
    with np.errstate(all="ignore"):
        r = np.abs(a - b) / np.abs(b)
    return float(np.nanmax(np.where(a == b, 0.0, r)))


def load_calcadj(reference):
    path = os.path.join(reference, "baselines", "His2ST", "graph_construction.py")
    spec = importlib.util.spec_from_file_location("reference_graph_construction", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.calcADJ


def gap_ok(coords, k):
    """The gap condition of the module docstring for one (coords, k)."""
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(axis=2))
    np.fill_diagonal(d, -1.0)
    s = np.sort(d, axis=1)[:, 1:]                                  # the other spots, ascending
    if (s[:, 0] <= 0).any():
        return False
    cut = (s[:, k] - s[:, k - 1]) > GAP * s[:, k]
    cand = s[:, :k]
    bound = cand.mean(axis=1) + cand.std(axis=1)
    std = (np.abs(cand - bound[:, None]) > GAP * bound[:, None]).all(axis=1)
    grid = (np.abs(cand - 2.0) > GAP * 2.0).all(axis=1)
    return bool(cut.all() and std.all() and grid.all())


def dense_stats(x, W):
    """I by matrix products, C by explicit double loops, from numpy's own mean."""
    n = x.shape[0]
    z = x - x.mean(axis=0)
    S0 = W.sum()
    den = (z * z).sum(axis=0)
    I = (n / S0) * np.einsum("ig,ij,jg->g", z, W, z) / den
    num = np.zeros(x.shape[1])
    for i in range(n):
        for j in np.flatnonzero(W[i]):
            num += W[i, j] * (z[i] - z[j]) ** 2
    C = ((n - 1) / (2 * S0)) * num / den
    return I, C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project (calcADJ is run from it)")
    args = ap.parse_args()
    calcADJ = load_calcadj(args.reference)
    mpmath.mp.dps = 50
    out = {}
    for name in sr.CASES:
        coords, x = sr.make_case(name)
        n = coords.shape[0]
        for k in KS:
            assert gap_ok(coords, k), f"{name}, k = {k}: the gap condition fails; pick another seed"
            for prune in sr.PRUNES:
                adj = calcADJ(coords, k, "euclidean", prune).numpy() != 0
                g = sr.lattice(coords, k, prune, False)
                assert np.array_equal(sr.dense(g["nbr"], g["w"]) != 0, adj), (name, k, prune)
                out[f"{name}.adj.{prune}.{k}"] = np.packbits(adj)
        errs = {"I": 0.0, "C": 0.0, "S": 0.0}
        for std in (False, True):
            g = sr.lattice(coords, 8, "STD", std)
            W = sr.dense(g["nbr"], g["w"])
            S = np.array([W.sum(), 0.5 * ((W + W.T) ** 2).sum(), ((W.sum(axis=1) + W.sum(axis=0)) ** 2).sum()])
            I, C = dense_stats(x, W)
            rI, rC = sr.statistics(x, g["nbr"], g["w"], g["S0"])
            tag = "r" if std else "b"
            out.update({f"{name}.I.{tag}": I, f"{name}.C.{tag}": C, f"{name}.S.{tag}": S})
            errs["I"] = max(errs["I"], float(np.max(np.abs(rI - I))))           # absolute: I passes through zero
            errs["C"] = max(errs["C"], rel(rC, C))
            errs["S"] = max(errs["S"], rel(np.array([g["S0"], g["S1"], g["S2"]]), S))
        perms = sr.permutations(PERM_SEED, PERM_P, n)
        assert np.array_equal(np.sort(perms, axis=1), np.broadcast_to(np.arange(n), perms.shape))
        simI = np.stack([dense_stats(x[p], W)[0] for p in perms])
        simC = np.stack([dense_stats(x[p], W)[1] for p in perms])
        rsI, rsC = sr.simulate(x, g["nbr"], g["w"], g["S0"], perms)
        out.update({f"{name}.perms": perms.astype(np.int16), f"{name}.simI": simI, f"{name}.simC": simC,
                    f"{name}.err_I": errs["I"], f"{name}.err_C": errs["C"], f"{name}.err_S": errs["S"],
                    f"{name}.err_simI": float(np.max(np.abs(rsI - simI))), f"{name}.err_simC": rel(rsC, simC)})
    # the tie rule on an exact lattice: the restatement alone
    lat = sr.make_coords(LATTICE["gr"], LATTICE["gc"], LATTICE["seed"], integer=True)
    g = sr.lattice(lat, 8, "Grid", True)
    out.update({"lattice.nbr": g["nbr"], "lattice.deg": g["deg"]})
    # the tails
    sf = stats.norm.sf(TAIL_Z)
    p1, nl1 = sr.normal_tail(TAIL_Z, False)
    p2, nl2 = sr.normal_tail(TAIL_Z, True)
    mp1 = np.array([float(-mpmath.log10(mpmath.erfc(mpmath.mpf(v) / mpmath.sqrt(2)) / 2)) for v in TAIL_MP])
    mp2 = np.array([float(-mpmath.log10(mpmath.erfc(mpmath.mpf(v) / mpmath.sqrt(2)))) for v in TAIL_MP])
    mpg = np.array([float(-mpmath.log10(mpmath.erfc(mpmath.mpf(float(v)) / mpmath.sqrt(2)) / 2)) for v in TAIL_Z])
    r1, r2 = sr.normal_tail(np.array(TAIL_MP), False)[1], sr.normal_tail(np.array(TAIL_MP), True)[1]
    out.update({"tail.z": TAIL_Z, "tail.sf": sf, "tail.nl_mp1": mp1, "tail.nl_mp2": mp2, "tail.nl_grid": mpg,
                "tail.err_sf": max(rel(p1, sf), rel(p2, 2 * sf)),
                "tail.err_nl": max(rel(r1, mp1), rel(r2, mp2), rel(nl1[1:], mpg[1:]))})
    # BH
    coords, x = sr.make_case("wide")
    r = sr.autocorr(x, coords, 8, "NA", True)
    p = np.concatenate([r["moran"]["pval_norm"], r["geary"]["pval_norm"], [0.5, 0.5, 1.0, 1e-300]])
    adj = stats.false_discovery_control(p, method="bh")
    out.update({"bh.p": p, "bh.adj": adj, "bh.err": rel(sr.bh(p), adj)})
    np.savez_compressed(sr.GOLDEN, **out)
    for key in sorted(out):
        if ".err" in key:
            print(f"{key}: {float(out[key]):.3e} ({float(out[key]) / sr.EPS:.1f} eps)")
    print(f"wrote {sr.GOLDEN}: {os.path.getsize(sr.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
