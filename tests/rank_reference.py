"""numpy / Python-int restatement of the rank-agreement arithmetic (tests only), for the tests of mclstexp_amd.rank.

Spearman's rho and Kendall's tau-b of two vectors, stated as csrc/rank.hip computes them: every sum is an exact integer
(formed here with Python ints, which cannot overflow), and each statistic is then three correctly rounded conversions, two
square roots, one product and one division in fp64:

    a       = first + last + 2 of an element's tie run in the sorted vector: twice its 1-based average rank (-0.0 ties +0.0)
    Sxy     = sum a_x a_y
    T       = sum (t^3 - t),  tie = sum t(t-1)/2,  v0 = sum t(t-1)(t-2),  v1 = sum t(t-1)(2t+5)   over the tie runs t of a side
    joint   = the pairs i < j tied on both sides
    s       = sum_{i<j} sign(a_x[i] - a_x[j]) sign(a_y[i] - a_y[j])                                (brute force, O(n^2))
    rho     = (n Sxy - n^2 (n+1)^2) / (sqrt(d_x) sqrt(d_y)),  d = n (n^3 - n - T) / 3
    tau_b   = s / (sqrt(n0 - xtie) sqrt(n0 - ytie)),  n0 = n (n-1) / 2
              (both clipped to [-1, 1]; where numerator^2 = the product under the roots, perfect agreement, exactly +-1)
    var     = (m (2n+5) - x1 - y1) / 18 + 2 xtie ytie / m + x0 y0 / (9 m (n-2)),  m = n (n-1);  z = s / sqrt(var)

Spearman's p is Student's t with n - 2 degrees of freedom on rho: genes_reference.pearson_pvalue.  Kendall's p is the
two-sided normal tail of z (scipy.stats.kendalltau, method="asymptotic"): spatial_reference.normal_tail.  The exact
small-n Kendall p is not restated (the library does not compute it).

Pinned against scipy by tests/test_rank_host.py (tests/golden/rank.npz)."""
import math
import os

import numpy as np

from genes_reference import pearson_pvalue
from spatial_reference import normal_tail

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rank.npz")
INT_NAMES = ("n", "Sxy", "Tx", "Ty", "xtie", "ytie", "x0", "y0", "x1", "y1", "joint", "s")
EPS = 2.220446049250313e-16
P_FLOOR = 1e-290        # as tests/test_genes_host.py: below it p is 0 or next to it
T_P_REL = 1e-10         # tests/test_genes_host.py: the t-based p of the restatement against scipy's


def normal_p_bound(zs, want):
    """The normal-tail bound of tests/test_spatial_host.py: (2 z^2 + 16) eps p."""
    return (2 * zs * zs + 16) * EPS * want


def case_inputs(z, name):
    """(pred, true) of a fixture case as float64 (value = int16 code * scale: exact in float32 as well)."""
    scale = float(z["scale"])
    return z[f"{name}.codes_p"].astype(np.float64) * scale, z[f"{name}.codes_t"].astype(np.float64) * scale


def ranks2(v):
    """Twice the 1-based average rank of every element (int64), and the tie-run lengths > 1."""
    v = np.asarray(v)
    v = np.where(v == 0, 0.0, v)                             # -0.0 and +0.0 are one value
    order = np.argsort(v, kind="stable")
    sv = v[order]
    new = np.concatenate([[True], sv[1:] != sv[:-1]])
    first = np.flatnonzero(new)
    last = np.concatenate([first[1:], [v.size]]) - 1
    run = np.cumsum(new) - 1
    a = np.empty(v.size, dtype=np.int64)
    a[order] = first[run] + last[run] + 2
    t = last - first + 1
    return a, [int(x) for x in t[t > 1]]


def pair_sums(ax, ay, chunk=2048):
    """(s, joint) by brute force over all pairs i < j."""
    ax, ay = np.asarray(ax, dtype=np.int32), np.asarray(ay, dtype=np.int32)
    n, s, joint = ax.size, 0, 0
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        dx = np.sign(ax[lo:hi, None] - ax[None, :]).astype(np.int8)
        dy = np.sign(ay[lo:hi, None] - ay[None, :]).astype(np.int8)
        upper = np.arange(n)[None, :] > np.arange(lo, hi)[:, None]
        s += int((dx * dy)[upper].sum(dtype=np.int64))
        joint += int(((dx == 0) & (dy == 0) & upper).sum(dtype=np.int64))
    return s, joint


def integers(x, y, tau=True):
    """The twelve integers of one problem as Python ints, in the library's order (INT_NAMES)."""
    ax, tx = ranks2(x)
    ay, ty = ranks2(y)
    s, joint = pair_sums(ax, ay) if tau else (0, 0)
    out = {"n": len(ax), "Sxy": sum(int(p) * int(q) for p, q in zip(ax, ay))}
    for side, runs in (("x", tx), ("y", ty)):
        out["T" + side] = sum(t ** 3 - t for t in runs)
        out[side + "tie"] = sum(t * (t - 1) // 2 for t in runs)
        out[side + "0"] = sum(t * (t - 1) * (t - 2) for t in runs)
        out[side + "1"] = sum(t * (t - 1) * (2 * t + 5) for t in runs)
    out["joint"], out["s"] = joint, s
    return [out[k] for k in INT_NAMES]


def _clip(v):
    return 1.0 if v > 1.0 else (-1.0 if v < -1.0 else v)


def _ratio(num, a, b):
    """num / (sqrt(a) sqrt(b)) clipped; exactly +-1 where num^2 = a b (perfect agreement, decided on the integers)."""
    if num * num == a * b:
        return -1.0 if num < 0 else 1.0
    return _clip(float(num) / (math.sqrt(float(a)) * math.sqrt(float(b))))


def finish(ints, tau=True):
    """(rho, tau_b, z) of one problem from its integers; NaN where undefined (z also at n < 3)."""
    n, Sxy, Tx, Ty, xtie, ytie, x0, y0, x1, y1, _, s = (int(v) for v in ints)
    rho = tb = z = float("nan")
    if n < 2:
        return rho, tb, z
    num = n * Sxy - n * n * (n + 1) * (n + 1)
    dx, dy = n * (n ** 3 - n - Tx), n * (n ** 3 - n - Ty)
    assert dx % 3 == 0 and dy % 3 == 0
    dx, dy = dx // 3, dy // 3
    assert max(abs(num), dx, dy) < 2 ** 63
    if dx > 0 and dy > 0:
        rho = _ratio(num, dx, dy)
    if tau:
        n0 = n * (n - 1) // 2
        ex, ey = n0 - xtie, n0 - ytie
        if ex > 0 and ey > 0:
            tb = _ratio(s, ex, ey)
            if n >= 3:
                m = n * (n - 1)
                var = (float(m * (2 * n + 5) - x1 - y1) / 18.0 + float(2 * xtie * ytie) / float(m)) \
                    + (float(x0) * float(y0)) / float(9 * m * (n - 2))
                z = float(s) / math.sqrt(var)
    return rho, tb, z


def exact(ints):
    """(rho, tau_b) of the same integers at 60 significant digits, as floats: what scipy's own deviation is measured from."""
    from decimal import Decimal, getcontext
    getcontext().prec = 60
    n, Sxy, Tx, Ty, xtie, ytie, _, _, _, _, _, s = (int(v) for v in ints)
    num = n * Sxy - n * n * (n + 1) * (n + 1)
    dx, dy = n * (n ** 3 - n - Tx) // 3, n * (n ** 3 - n - Ty) // 3
    n0 = n * (n - 1) // 2
    rho = float(Decimal(num) / (Decimal(dx) * Decimal(dy)).sqrt()) if dx > 0 and dy > 0 else float("nan")
    ex, ey = n0 - xtie, n0 - ytie
    tb = float(Decimal(s) / (Decimal(ex) * Decimal(ey)).sqrt()) if ex > 0 and ey > 0 else float("nan")
    return rho, tb


def vector_stats(x, y, tau=True):
    """One problem: dict of ``ints`` (list of Python ints), ``rho``, ``rho_p``, ``rho_nl``, ``tau``, ``tau_p``, ``tau_nl``."""
    ints = integers(x, y, tau)
    rho, tb, z = finish(ints, tau)
    rp, rnl = pearson_pvalue(np.array([rho]), ints[0])
    tp, tnl = normal_tail(np.array([z]), True)
    return {"ints": ints, "rho": rho, "rho_p": float(rp[0]), "rho_nl": float(rnl[0]), "tau": tb, "tau_p": float(tp[0]),
            "tau_nl": float(tnl[0])}


def matrix_stats(pred, true, offsets=None, axis="genes", tau=True):
    """Every problem of row-stacked matrices: arrays of shape (S, G) for ``axis="genes"`` and (rows,) for ``"spots"``;
    ``ints`` carries a trailing axis of 12 (int64: every entry fits at n <= 16384)."""
    pred, true = np.asarray(pred), np.asarray(true)
    if axis == "spots":
        probs = [[(pred[i], true[i]) for i in range(pred.shape[0])]]
    else:
        off = [0, pred.shape[0]] if offsets is None else [int(o) for o in offsets]
        probs = [[(pred[off[s]:off[s + 1], g], true[off[s]:off[s + 1], g]) for g in range(pred.shape[1])]
                 for s in range(len(off) - 1)]
    res = [[vector_stats(x, y, tau) for x, y in row] for row in probs]
    out = {k: np.array([[r[k] for r in row] for row in res], dtype=np.int64 if k == "ints" else np.float64)
           for k in ("ints", "rho", "rho_p", "rho_nl", "tau", "tau_p", "tau_nl")}
    return {k: v[0] for k, v in out.items()} if axis == "spots" else out


def summary(rho, tau_b, heg):
    """(heg_rho, hvg_rho, heg_tau, hvg_tau, n_valid) of one slide, every sum taken gene by gene in index order."""
    member = np.zeros(len(rho), dtype=bool)
    member[np.asarray(heg)] = True
    out = []
    for v in (rho, tau_b):
        hs = av = 0.0
        cnt = 0
        for g, x in enumerate(v):
            if member[g]:
                hs = hs + float(x)
            if not math.isnan(x):
                av = av + float(x)
                cnt += 1
        out += [hs / float(len(heg)), av / float(cnt) if cnt else float("nan")]
    return out[0], out[1], out[2], out[3], int((~np.isnan(np.asarray(rho))).sum())
