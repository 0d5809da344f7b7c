"""torch.optim.Adam with L2-coupled weight decay (single tensor), restated in numpy: the float64 reference the Adam kernels
(csrc/adam.hip) are pinned to, the per-element error bounds derived for one fp32 step, and the inputs the CPU and the GPU
tests share.  numpy only.

One step from (p, g, m, v) at step number t:

    G = g + wd p;  M = m + (1 - b1)(G - m);  V = b2 v + (1 - b2) G^2
    bc1 = 1 - b1^t;  bc2 = 1 - b2^t;  P = p - (lr / bc1) M / (sqrt(V) / sqrt(bc2) + eps)

Bounds, per element, with u = 2^-23, a = |g| + wd |p| and K = 8; every input is the fp32 value widened to float64:

    |m_got - M| <= K u (|m_old| + a)
    |v_got - V| <= K u (b2 v_old + (1 - b2) a^2)
    |p_got - P'| <= u |P'| + 4 u |d'|,   d' = (lr / bc1) m_got / (sqrt(v_got) / sqrt(bc2) + eps),   P' = p_old - d'

The scales of m and v use a, not |G|: an fp32 implementation rounds wd p and the sum (or fuses them), so where g + wd p or
0.9 m + 0.1 g cancels the error stays of the size of the terms, not of the result.  p is judged against the implementation's
OWN new moments (teacher forcing): sqrt(V) is ill-conditioned where V cancels, and the moments are bounded separately.
Where a scale is exactly 0 the bound is 0 and the result must equal the reference exactly.

The bounds hold for normal fp32 numbers: an input set whose (1 - b2) g^2 underflows would need an absolute term.
planted_inputs keeps |g| >= 1e-6 wherever g != 0.
"""
import numpy as np

U = 2.0 ** -23
K = 8.0


def consts64(lr, b1, b2, eps, wd, t):
    """The eight values of the kernels' constants block, in struct order, in float64."""
    bc1 = 1.0 - float(b1) ** int(t)
    bc2 = 1.0 - float(b2) ** int(t)
    return np.array([lr / bc1, b1, b2, 1.0 - b1, 1.0 - b2, eps, wd, 1.0 / np.sqrt(bc2)], dtype=np.float64)


def step64(p, g, m, v, lr, b1, b2, eps, wd, t):
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    G = g + wd * p
    M = m + (1.0 - b1) * (G - m)
    V = b2 * v + (1.0 - b2) * (G * G)
    bc1 = 1.0 - float(b1) ** int(t)
    bc2 = 1.0 - float(b2) ** int(t)
    P = p - (lr / bc1) * M / (np.sqrt(V) / np.sqrt(bc2) + eps)
    return P, M, V


def step32(p, g, m, v, lr, b1, b2, eps, wd, t):
    """The same sequence in numpy float32: the constants rounded once from float64, then one rounding per operation and no
    fused multiply-add.  A CPU stand-in for "a correct fp32 implementation"."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    lr_bc1, _, b2f, omb1, omb2, epsf, wdf, rs2 = (f(x) for x in consts64(lr, b1, b2, eps, wd, t))
    G = g + wdf * p
    M = m + omb1 * (G - m)
    V = b2f * v + (omb2 * G) * G
    denom = np.sqrt(V) * rs2 + epsf
    P = p - lr_bc1 * (M / denom)
    assert P.dtype == f and M.dtype == f and V.dtype == f
    return P, M, V


def bounds(p, g, m, v, m_got, v_got, lr, b1, b2, eps, wd, t):
    """(M, V, P', d') and the three per-element bounds for one step from the fp32 state (p, g, m, v), given the implementation's
    new moments."""
    p, g, m, v, m_got, v_got = (np.asarray(x).astype(np.float64) for x in (p, g, m, v, m_got, v_got))
    _, M, V = step64(p, g, m, v, lr, b1, b2, eps, wd, t)
    a = np.abs(g) + wd * np.abs(p)
    bm = K * U * (np.abs(m) + a)
    bv = K * U * (b2 * v + (1.0 - b2) * a * a)
    bc1 = 1.0 - float(b1) ** int(t)
    bc2 = 1.0 - float(b2) ** int(t)
    with np.errstate(invalid="ignore"):          # non-finite or negative moments give a NaN bound: worst_ratio counts it as inf
        d = (lr / bc1) * m_got / (np.sqrt(v_got) / np.sqrt(bc2) + eps)
    Pt = p - d
    bp = U * np.abs(Pt) + 4.0 * U * np.abs(d)
    return (M, V, Pt, d), (bm, bv, bp)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; an error against a zero bound counts as inf, no error against a zero bound as 0.  An error
    or a bound that is not finite (a NaN or an infinity in the result, or in the moments the p bound is built from) counts
    as inf too: it can never be inside a bound."""
    err = np.abs(np.asarray(got).astype(np.float64) - ref)
    bound = np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isfinite(err) & np.isfinite(bound), r, np.inf)
    return float(r.max()) if r.size else 0.0


def within(r, limit=1.0):
    """Every ratio of r is at most limit (a NaN is not)."""
    return all(x <= limit for x in r)


def ratios(p, g, m, v, p_got, m_got, v_got, lr, b1, b2, eps, wd, t):
    """Worst |error| / bound of (p, m, v) for one step: each must be <= 1 (see within)."""
    (M, V, Pt, _), (bm, bv, bp) = bounds(p, g, m, v, m_got, v_got, lr, b1, b2, eps, wd, t)
    return worst_ratio(p_got, Pt, bp), worst_ratio(m_got, M, bm), worst_ratio(v_got, V, bv)


def planted_inputs(n, wd, seed=0):
    """fp32 (p, g, m, v) of n elements: g over eight decades with random sign, non-zero moments, and by position

        i % 7 == 0   g = 0                      i % 7 == 3 or i % 21 == 14   v = 0
        i % 7 == 1   g = -fl(wd p)              i % 11 == 0                  m = 0
        i % 7 == 2   m = -g / 9                 i % 13 == 6                  p = 0

    so that g + wd p cancels, 0.9 m + 0.1 g cancels, and (with wd = 0) elements whose m scale is exactly 0 (i % 77 == 0),
    whose v scale is (i % 21 == 14) and both (i % 231 == 77) exist.  The first five elements cover the four main classes,
    so the tiny sizes see them too."""
    rng = np.random.default_rng(seed)
    f = np.float32
    i = np.arange(n)
    p = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 0.5, n)).astype(f)
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 2, n)).astype(f)
    m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(f)
    v = (10.0 ** rng.uniform(-10, 2, n)).astype(f)
    p[i % 13 == 6] = 0
    g[i % 7 == 0] = 0
    k = i % 7 == 1
    g[k] = -(f(wd) * p[k])
    k = i % 7 == 2
    m[k] = -(g[k] / f(9))
    v[(i % 7 == 3) | (i % 21 == 14)] = 0
    m[i % 11 == 0] = 0
    return p, g, m, v
