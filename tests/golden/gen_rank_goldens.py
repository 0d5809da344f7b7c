#!/usr/bin/env python3
"""Generate ``rank.npz``: inputs and scipy's results for the tests of mclstexp_amd.rank.

Every input is stored as int16 codes and one power-of-two scale (value = code * scale: exact in float32 and float64, so
one fixture serves every dtype combination; small codes give the ties expression data is full of).  Per case the file
holds ``scipy.stats.spearmanr`` and ``scipy.stats.kendalltau(method="asymptotic")`` vector by vector, and scipy's own
deviation from the exact-integer value (tests/rank_reference.py ``exact``: the same integers divided at 60 digits):

  batch   slides of n = 2, 3, 63, 64, 65, 257, 1025 spots, G = 33 genes; gene 0 zero-inflated (more than half exact
          zeros on both sides), gene 1 constant in the ground truth, gene 2 zeros only on the pred side of half the spots
          (the tests flip their sign), gene 3 pred = true, gene 4 pred = -true, even genes heavily tied, odd genes lightly
  spots   40 x 33, ranked row by row (get_R's dim=0)
  zi1500  n = 1500, G = 4: random and zero-inflated columns at the size the deviation was quoted for
  limit   one pair of 16384 elements with ties: the LDS plan at its edge; also its twelve integers (brute force)

Where /root/reference is present (the build container) ``ref.*`` holds the reference's own ``get_R(..., func=spearmanr)``
lifted from utils.py with ``ast`` and run unmodified on slide 4 of ``batch`` (dim=1) and on ``spots`` (dim=0).

    python tests/golden/gen_rank_goldens.py        # writes tests/golden/rank.npz
"""
import ast
import os
import sys
import warnings

import numpy as np
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rank_reference as rr  # noqa: E402

REF = "/root/reference"
SIZES = [2, 3, 63, 64, 65, 257, 1025]
G = 33
SCALE = 2.0 ** -6
REF_SLIDE = 4


def make_pair(rng, n, genes):
    """int16 codes (n, genes) of pred and true: even genes on a coarse grid, odd genes on a fine one."""
    base = rng.normal(size=(n, genes))
    noise = rng.normal(size=(n, genes))
    step = np.where(np.arange(genes) % 2 == 0, 8.0, 3000.0)
    true = np.round(np.maximum(base * 1.2 + 0.5, 0.0) * step)
    pred = np.round(np.maximum((base + 0.8 * noise) * 1.2 + 0.5, 0.0) * step)
    return pred.astype(np.int16), true.astype(np.int16)


def make_batch(rng):
    ps, ts = [], []
    for n in SIZES:
        p, t = make_pair(rng, n, G)
        p[rng.random(n) < 0.6, 0] = 0
        t[rng.random(n) < 0.6, 0] = 0
        t[:, 1] = 5
        p[::2, 2] = 0
        p[:, 3] = t[:, 3]
        p[:, 4] = -t[:, 4]
        ps.append(p), ts.append(t)
    return np.concatenate(ps), np.concatenate(ts), np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)


def scipy_pair(x, y):
    """(rho, rho_p, tau, tau_p) of scipy; Kendall's asymptotic p divides by zero at n = 2: NaN there."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sp = stats.spearmanr(x, y)
        try:
            kt = stats.kendalltau(x, y, method="asymptotic")
            tau, tau_p = kt.statistic, kt.pvalue
        except ZeroDivisionError:
            tau, tau_p = stats.kendalltau(x, y, method="exact").statistic, np.nan
    return float(sp.statistic), float(sp.pvalue), float(tau), float(tau_p)


def score(vectors):
    """scipy's four values per (x, y) and its largest deviation from the exact-integer rho / tau."""
    res = np.array([scipy_pair(x, y) for x, y in vectors])
    dev = np.zeros(2)
    for (x, y), row in zip(vectors, res):
        er, et = rr.exact(rr.integers(x, y))
        for k, (got, want) in enumerate(((row[0], er), (row[2], et))):
            assert np.isnan(got) == np.isnan(want)
            if not np.isnan(want):
                dev[k] = max(dev[k], abs(got - want))
    return res, dev


def lift_get_R():
    src = open(os.path.join(REF, "utils.py"), encoding="utf-8").read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "get_R")
    ns = {"np": np, "pearsonr": stats.pearsonr}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "utils.py", "exec"), ns)
    return ns["get_R"]


class _AnnDataX:
    def __init__(self, x):
        self.X = x
        self.shape = x.shape


def main():
    rng = np.random.default_rng(20250)
    out = {"scale": np.float64(SCALE)}

    def put(name, res, dev, shape):
        for k, key in enumerate(("rho", "rho_p", "tau", "tau_p")):
            out[f"{name}.{key}"] = res[:, k].reshape(shape)
        out[f"{name}.dev_rho"], out[f"{name}.dev_tau"] = dev
        print(name, shape, "scipy deviation from exact: rho %.3g tau %.3g" % tuple(dev))

    p, t, off = make_batch(rng)
    out.update({"batch.codes_p": p, "batch.codes_t": t, "batch.offsets": off})
    x, y = p * SCALE, t * SCALE
    vecs = [(x[off[s]:off[s + 1], g], y[off[s]:off[s + 1], g]) for s in range(len(SIZES)) for g in range(G)]
    put("batch", *score(vecs), (len(SIZES), G))

    p0, t0 = make_pair(rng, 40, G)
    out.update({"spots.codes_p": p0, "spots.codes_t": t0})
    put("spots", *score([(p0[i] * SCALE, t0[i] * SCALE) for i in range(40)]), (40,))

    pz, tz = make_pair(rng, 1500, 4)
    pz[rng.random(1500) < 0.7, 0] = 0
    tz[rng.random(1500) < 0.7, 0] = 0
    out.update({"zi1500.codes_p": pz, "zi1500.codes_t": tz})
    put("zi1500", *score([(pz[:, g] * SCALE, tz[:, g] * SCALE) for g in range(4)]), (4,))

    n = 16384
    base = rng.normal(size=n)
    tl = np.round(base * 900.0).astype(np.int16)
    pl = np.round((base + rng.normal(size=n)) * 900.0).astype(np.int16)
    out.update({"limit.codes_p": pl, "limit.codes_t": tl})
    put("limit", *score([(pl * SCALE, tl * SCALE)]), (1,))
    out["limit.ints"] = np.array(rr.integers(pl * SCALE, tl * SCALE), dtype=np.int64)

    if os.path.isdir(REF):
        get_R = lift_get_R()
        lo, hi = off[REF_SLIDE], off[REF_SLIDE + 1]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r1, p1 = get_R(_AnnDataX(x[lo:hi]), _AnnDataX(y[lo:hi]), dim=1, func=stats.spearmanr)
            r0, p0_ = get_R(_AnnDataX(p0 * SCALE), _AnnDataX(t0 * SCALE), dim=0, func=stats.spearmanr)
        out.update({"ref.slide": np.int64(REF_SLIDE), "ref.r1": r1, "ref.p1": p1, "ref.r0": r0, "ref.p0": p0_})
        print("reference get_R: dim=1", r1.shape, "dim=0", r0.shape)
    np.savez_compressed(os.path.join(HERE, "rank.npz"), **out)
    print("wrote rank.npz:", os.path.getsize(os.path.join(HERE, "rank.npz")), "bytes")


if __name__ == "__main__":
    main()
