"""Float64 restatement of the DenseNet dense-layer kernels (csrc/dense_conv.hip, conv3x3_rows.hip, dense_bwd.hip,
wrw_fused.hip, conv3x3_wrw_rows.hip), following the kernels' own rounding points, with a bound for every element of every
output derived from that element's own operands.  numpy only: no GPU, no torch.

Rounding points, as read from the code (``rounding=False`` switches every one of them off: plain real arithmetic):

  prologue (every kernel)   sc = fp32(gamma*rstd); sh = fmaf(-mean, sc, beta); t = fmaf(x, sc, sh); a = bf16_rne(max(t, 0));
                            the ReLU mask is [t > 0].  x*sc is exact in float64 (8 x 24 bits), so the sign of t is exact.
  forward                   z = bf16_rne(sum_k a*W1) (K terms), y = bf16_rne(sum a2*W2) (9*128 terms, taps outside the image
                            zero); the batch statistics are those of the STORED bf16 tensor.
  tail backward             da2 = 3x3 backward-data (9*32 terms); g2 = bf16_rne(da2*mask2), stored; dbeta2 = sum g2; dgamma2 =
                            sum g2*zhat; dz = bf16_rne(sc2*(g2 - c1 - zhat*c2)), c = the two sums / S.  The sums and dz are
                            restated from the kernel's own stored g2.
  head backward             da = dz W1 (128 terms); g = da*mask (fp32, never stored); dbeta = sum g; dgamma = rstd*(sum g*x -
                            mean*sum g); delta = bf16_rne(fmaf(sc, g, fmaf(ka, x, kb))); gbuf <- bf16_rne(gbuf + delta).

The reference VALUE of an output that is one rounding of an fp32 number is the UNROUNDED float64 number: the kernel's output
must lie within  e + half_ulp_bf16(|ref| + e)  of it, e being the bound of the fp32 number.

Bounds.  u = 2^-23 per fp32 operation (round to nearest is 2^-24; a truncating accumulate inside the matrix unit is 2^-23).  An
n-term accumulation gets e = n*u*sum|terms|; a value rounded to bf16 adds half_ulp_bf16(v) = 2^(floor(log2 v) - 8); later
roundings add their own half-ulp and propagated operands their own bound.  An element of a is AMBIGUOUS when the exact t lies
within 2^-22*|t| of the midpoint of two bf16 values: an output that consumes it gets |w|*ulp_bf16(a) more.  Nothing else is
excused.  (sh is rounded to fp32 once from the exact value of -mean*sc + beta: fma32.)"""
import numpy as np

U = 2.0 ** -23
AMB_REL = 2.0 ** -22
TINY = 2.0 ** -120          # floor under half_ulp_bf16's argument: inputs stay far from the denormals


# ------------------------------------------------------------------------------------------------------------------ bf16 / fp32
def bf16_bits(x):
    """bf16 bits (uint16) of float32(x), round to nearest even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_trunc_bits(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bits_to_f64(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16(x):
    """float64 value of bf16_rne(fp32(x))."""
    return bits_to_f64(bf16_bits(x))


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def fma32(a, b, c):
    """fp32(a*b + c) for fp32 values held in float64, rounded ONCE from the exact value: the product is exact in float64, the
    sum's float64 rounding error is recovered (TwoSum), and where it is not zero the fp32 neighbours are compared exactly."""
    from fractions import Fraction
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    p = a * b
    s = p + c
    bv = s - p
    err = (p - (s - bv)) + (c - bv)
    out = f32(s)
    for i in zip(*np.nonzero(err)):
        exact = Fraction(float(p[i])) + Fraction(float(c[i]))
        r = np.float32(out[i])
        cand = [np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf))]
        key = lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1)
        out[i] = float(min(cand, key=key))
    return out


def half_ulp_bf16(v):
    v = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), TINY)
    return np.exp2(np.floor(np.log2(v)) - 8.0)


def once_rounded(ref, e):
    """Bound of bf16_rne(f) against ref when |f - ref| <= e."""
    return half_ulp_bf16(np.abs(ref) + e) + e


def ratios(out, ref, bound):
    """|out - ref| / bound per element; a non-finite output counts as infinite, 0/0 as 0."""
    out = np.asarray(out, dtype=np.float64)
    err = np.abs(out - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return np.where(np.isfinite(out) & ~np.isnan(r), r, np.inf)


def worst(out, ref, bound):
    """(worst ratio, its index tuple)."""
    r = ratios(out, ref, bound)
    if r.size == 0:
        return 0.0, ()
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), tuple(int(v) for v in i)


def bias(out, ref):
    """mean of sign(ref)*(out - ref)/half_ulp_bf16(ref) over the elements with ref != 0: 0 for round-to-nearest, -1 for
    truncation.  Returns (bias, N, allowed) with allowed = max(0.05, 6*0.5774/sqrt(N)) (the error in half-ulps is uniform on
    [-1, 1]: standard deviation 1/sqrt(3) = 0.5774)."""
    out = np.asarray(out, dtype=np.float64)
    m = ref != 0.0
    n = int(m.sum())
    if n == 0:
        return 0.0, 0, 1.0
    b = float(np.mean(np.sign(ref[m]) * (out[m] - ref[m]) / half_ulp_bf16(ref[m])))
    return b, n, max(0.05, 6 * 0.5774 / np.sqrt(n))


# ------------------------------------------------------------------------------------------------------------------ prologue
class Prologue:
    """a = relu(bn(x)) as the kernels form it.  x: (S, C) float64 holding bf16 values; gamma .. rstd: fp32 values."""

    def __init__(self, x, gamma, beta, mean, rstd, rounding=True):
        x = np.asarray(x, dtype=np.float64)
        g, b, m, r = (np.asarray(v, dtype=np.float64) for v in (gamma, beta, mean, rstd))
        self.mean, self.rstd = m, r
        if rounding:
            self.sc = f32(g * r)                         # exact product, one rounding
            self.sh = fma32(-m, self.sc, b)              # fmaf: one rounding of the exact value
        else:
            self.sc = g * r
            self.sh = b - m * self.sc
        self.t = x * self.sc + self.sh                   # x*sc exact; the sum carries 2^-53
        self.mask = self.t > 0.0
        tp = np.maximum(self.t, 0.0)
        if rounding:
            self.a = bf16(tp)                            # fp32 (fmaf), then bf16, both to nearest even
            lo = bits_to_f64(bf16_trunc_bits(f32(tp)))   # the bf16 value at or below t
            ulp = 2.0 * half_ulp_bf16(np.maximum(lo, TINY))
            mid = lo + 0.5 * ulp
            self.ulp = np.where(self.mask, ulp, 0.0)
            self.amb = self.mask & (np.abs(tp - mid) <= AMB_REL * tp)
        else:
            self.a = tp
            self.ulp = np.zeros_like(tp)
            self.amb = np.zeros(tp.shape, dtype=bool)
        self.amb_w = np.where(self.amb, self.ulp, 0.0)   # what an ambiguous element may move by

    @property
    def amb_share(self):
        return float(self.amb.mean()) if self.amb.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ forward
def conv1x1_fwd(x, gamma, beta, mean, rstd, W1, rounding=True):
    """z[s][n] = sum_k a[s][k]*W1[n][k].  Returns (ref unrounded, bound of the stored bf16 z, prologue)."""
    p = Prologue(x, gamma, beta, mean, rstd, rounding)
    W1 = np.asarray(W1, dtype=np.float64)
    ref = p.a @ W1.T
    e = W1.shape[1] * U * (np.abs(p.a) @ np.abs(W1).T) + p.amb_w @ np.abs(W1).T
    return ref, once_rounded(ref, e), p


def _taps(H, W):
    for ky in range(3):
        for kx in range(3):
            yield ky, kx, slice(ky, ky + H), slice(kx, kx + W)


def _pad(a, B, H, W):
    return np.pad(a.reshape(B, H, W, a.shape[-1]), ((0, 0), (1, 1), (1, 1), (0, 0)))


def conv3x3_fwd(z, B, H, W, gamma, beta, mean, rstd, W2, rounding=True):
    """y[p][co] = sum_{ky,kx,ci} a2[p + (ky-1, kx-1)][ci]*W2[co][ky][kx][ci], zero outside the image.  z: (B*H*W, 128),
    W2: (32, 3, 3, 128).  Returns (ref, bound, prologue)."""
    p = Prologue(z, gamma, beta, mean, rstd, rounding)
    W2 = np.asarray(W2, dtype=np.float64)
    ap, aa, am = _pad(p.a, B, H, W), _pad(np.abs(p.a), B, H, W), _pad(p.amb_w, B, H, W)
    S, Co = B * H * W, W2.shape[0]
    ref, mag, amb = np.zeros((S, Co)), np.zeros((S, Co)), np.zeros((S, Co))
    for ky, kx, sy, sx in _taps(H, W):
        w = W2[:, ky, kx, :].T
        ref += ap[:, sy, sx, :].reshape(S, -1) @ w
        mag += aa[:, sy, sx, :].reshape(S, -1) @ np.abs(w)
        amb += am[:, sy, sx, :].reshape(S, -1) @ np.abs(w)
    e = 9 * W2.shape[3] * U * mag + amb
    return ref, once_rounded(ref, e), p


def border_pixels(B, H, W):
    """Flat indices of the pixels with at least one tap outside the image."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    edge = ((yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1)).reshape(-1)
    return np.nonzero(np.tile(edge, B))[0]


# ------------------------------------------------------------------------------------------------------------------ statistics
def stats_ref(v, eps):
    v = np.asarray(v, dtype=np.float64)
    m = v.mean(axis=0)
    var = ((v - m) ** 2).mean(axis=0)
    return m, var, 1.0 / np.sqrt(var + eps)


def _rstd_bound(var, e_var, eps):
    r = 1.0 / np.sqrt(var + eps)
    lo = 1.0 / np.sqrt(np.maximum(var - e_var, 0.0) + eps)
    hi = 1.0 / np.sqrt(var + e_var + eps)
    return np.maximum(lo - r, r - hi) + U * r          # the cast to fp32 (2^-24) and float(eps) vs eps


def stats_tiles(v, eps, bm):
    """mean / biased variance / rstd of the stored tensor v (S, C) with the bounds of the tile scheme (conv1x1_fwd_kernel,
    conv3x3_fwd_kernel + tile_stats_finalize_kernel): per tile of bm rows, fp32 sums of d = v - v[first row of the tile] and of
    d^2; the tile's sum = fmaf(n, shift, s1) and M2 = s2 - s1^2/n in fp32; Chan's merge in double (exact at this scale).
    Returns ((mean, var, rstd), (bounds))."""
    v = np.asarray(v, dtype=np.float64)
    S, C = v.shape
    m, var, rstd = stats_ref(v, eps)
    e_sum, e_var = np.zeros(C), np.zeros(C)
    for r0 in range(0, S, bm):
        t = v[r0:r0 + bm]
        n = t.shape[0]
        d = t - t[0]
        a1, s1, s2 = np.abs(d).sum(0), d.sum(0), (d * d).sum(0)
        e_s1 = (n + 1) * U * a1                          # n adds, and the rounding of d itself
        tsum = t.sum(0)
        e_t = e_s1 + U * np.abs(tsum)                    # fmaf(n, shift, s1)
        e_s2 = (n + 3) * U * s2                          # n fmas; d's rounding enters d^2 twice
        e_m2 = e_s2 + 2 * np.abs(s1) * e_s1 / n + e_s1 ** 2 / n + 2 * U * s1 * s1 / n + U * (s2 + s1 * s1 / n)
        e_sum += e_t
        e_var += e_m2 + 2 * np.abs(tsum / n - m) * e_t + e_t ** 2 / n
    e_mean = e_sum / S + U * np.abs(m)
    e_var = e_var / S + (e_sum / S) ** 2 + U * var
    return (m, var, rstd), (e_mean, e_var, _rstd_bound(var, e_var, eps))


def stats_sums(v, eps, nmax):
    """The same for the raw-sums scheme of the row-walking 3x3 forward (conv3x3_fwd_rows_kernel + sums_finalize_kernel): per
    unit of at most nmax pixels fp32 sums of v and v^2, added in double; var = (q - sum^2/S)/S."""
    v = np.asarray(v, dtype=np.float64)
    S, C = v.shape
    m, var, rstd = stats_ref(v, eps)
    e_sum = nmax * U * np.abs(v).sum(0)
    e_q = nmax * U * (v * v).sum(0)
    e_mean = e_sum / S + U * np.abs(m)
    e_var = (e_q + 2 * np.abs(m) * e_sum + e_sum ** 2 / S) / S + U * var
    return (m, var, rstd), (e_mean, e_var, _rstd_bound(var, e_var, eps))


def rows_applicable(H, W):
    return 17 <= W <= 150


def fwd_rows_unit_pixels(B, H, W):
    """Pixels per unit of the row-walking forward: rc output rows of a 32-column strip (rows_plan in conv3x3_rows.hip)."""
    rc = min(max((H * B * ((W + 31) // 32)) // 2048, 2), H)
    return rc * 32


def bwd_rows_unit_pixels(B, H, W):
    rc = min(max((H * B * ((W + 31) // 32) * 4) // 2048, 2), H)
    return rc * 32


# ------------------------------------------------------------------------------------------------------------------ tail backward
def conv3x3_bwd_data(dy, B, H, W, W2):
    """da2[p][ci] = sum_{ky,kx,co} dy[p - (ky-1, kx-1)][co]*W2[co][ky][kx][ci].  Returns (value, sum of |terms|)."""
    dy = np.asarray(dy, dtype=np.float64)
    W2 = np.asarray(W2, dtype=np.float64)
    S, Ci = B * H * W, W2.shape[3]
    dp, da = _pad(dy, B, H, W), _pad(np.abs(dy), B, H, W)
    ref, mag = np.zeros((S, Ci)), np.zeros((S, Ci))
    for ky, kx, _, _ in _taps(H, W):
        sy, sx = slice(2 - ky, 2 - ky + H), slice(2 - kx, 2 - kx + W)
        w = W2[:, ky, kx, :]
        ref += dp[:, sy, sx, :].reshape(S, -1) @ w
        mag += da[:, sy, sx, :].reshape(S, -1) @ np.abs(w)
    return ref, mag


def tail_g2(dy, B, H, W, W2, z, gamma, beta, mean, rstd, rounding=True):
    """g2 = da2*[bn2(z) > 0]: (ref unrounded, bound of the stored bf16 g2, prologue of z)."""
    p = Prologue(z, gamma, beta, mean, rstd, rounding)
    da, mag = conv3x3_bwd_data(dy, B, H, W, W2)
    ref = np.where(p.mask, da, 0.0)
    e = np.where(p.mask, 9 * np.asarray(W2).shape[0] * U * mag, 0.0)
    bound = np.where(p.mask, once_rounded(ref, e), 0.0)          # a masked element is exactly zero
    return ref, bound, p


def tail_from_g2(g2, z, gamma, mean, rstd, nmax, rows_form, rounding=True):
    """dbeta2, dgamma2 and dz restated from the STORED g2 (S, 128).  nmax = pixels per fp32 partial sum (128: flat tile; the
    unit of the row-walking form).  flat form: dgamma2 = sum g2*((z - mean)*rstd); row-walking form: rstd*fmaf(-mean, sum g2,
    sum g2*z) per unit.  Returns dict name -> (ref, bound); dz's ref is unrounded."""
    g2, z = np.asarray(g2, dtype=np.float64), np.asarray(z, dtype=np.float64)
    gam, mu, rs = (np.asarray(v, dtype=np.float64) for v in (gamma, mean, rstd))
    S = g2.shape[0]
    zh = (z - mu) * rs
    db, dg = g2.sum(0), (g2 * zh).sum(0)
    if not rounding:
        sc = gam * rs
        return {"dbeta": (db, 0.0), "dgamma": (dg, 0.0), "dz": (sc * (g2 - db / S - zh * dg / S), 0.0)}
    e_db = nmax * U * np.abs(g2).sum(0)
    if rows_form:
        e_dg = rs * (nmax + 2) * U * (np.abs(g2 * z).sum(0) + np.abs(mu) * np.abs(g2).sum(0))
    else:
        e_dg = (nmax + 2) * U * np.abs(g2 * zh).sum(0)           # zhat carries two fp32 roundings
    c1, c2 = db / S, dg / S
    e_c1, e_c2 = e_db / S + U * np.abs(c1), e_dg / S + U * np.abs(c2)
    sc = f32(gam * rs)
    dz = sc * (g2 - c1 - zh * c2)
    # bn2_dz_kernel: sc*(g - c1 - (z - mu)*rs*c2), six fp32 operations (contraction to fma only removes roundings)
    e_dz = np.abs(sc) * (6 * U * (np.abs(g2) + np.abs(c1) + np.abs(zh * c2)) + e_c1 + np.abs(zh) * e_c2)
    return {"dbeta": (db, e_db + U * np.abs(db)), "dgamma": (dg, e_dg + U * np.abs(dg)), "dz": (dz, once_rounded(dz, e_dz))}


def tail_from_unstored_g2(gref, gbound, z, gamma, mean, rstd, nmax):
    """The same where g2 itself is not kept (the persistent block backward holds it in LDS): the stored g2 is only known to lie
    within gbound of gref, and that bound is carried into the two sums, their means and dz (flat form)."""
    z = np.asarray(z, dtype=np.float64)
    gam, mu, rs = (np.asarray(v, dtype=np.float64) for v in (gamma, mean, rstd))
    S = z.shape[0]
    zh = (z - mu) * rs
    ga = np.abs(gref) + gbound
    db, dg = gref.sum(0), (gref * zh).sum(0)
    e_db = gbound.sum(0) + nmax * U * ga.sum(0)
    e_dg = (gbound * np.abs(zh)).sum(0) + (nmax + 2) * U * (ga * np.abs(zh)).sum(0)
    c1, c2 = db / S, dg / S
    e_c1, e_c2 = e_db / S + U * np.abs(c1), e_dg / S + U * np.abs(c2)
    sc = f32(gam * rs)
    dz = sc * (gref - c1 - zh * c2)
    e_dz = np.abs(sc) * (gbound + 6 * U * (ga + np.abs(c1) + np.abs(zh * c2)) + e_c1 + np.abs(zh) * e_c2)
    return {"dbeta": (db, e_db + U * np.abs(db)), "dgamma": (dg, e_dg + U * np.abs(dg)), "dz": (dz, once_rounded(dz, e_dz))}


# ------------------------------------------------------------------------------------------------------------------ head backward
class Head:
    """g = (dz W1)*[bn1(x) > 0] with its per-element bound, and the two BatchNorm-backward sums as bn1_bwd_kernel<0> +
    bn1_bwd_finalize_kernel form them: per 64-row tile fp32 sums s1 = sum g, s2 = rstd*fmaf(-mean, s1, sum g*x); tiles added in
    double."""
    TILE = 64

    def __init__(self, dz, W1, x, gamma, beta, mean, rstd, rounding=True):
        self.p = p = Prologue(x, gamma, beta, mean, rstd, rounding)
        dz, W1 = np.asarray(dz, dtype=np.float64), np.asarray(W1, dtype=np.float64)
        self.x = x = np.asarray(x, dtype=np.float64)
        self.S = S = x.shape[0]
        mu, rs = p.mean, p.rstd
        da = dz @ W1
        self.g = g = np.where(p.mask, da, 0.0)
        self.e_g = e_g = np.where(p.mask, W1.shape[0] * U * (np.abs(dz) @ np.abs(W1)), 0.0) if rounding else np.zeros_like(g)
        n = self.TILE
        self.dbeta = g.sum(0)
        self.dgamma = rs * ((g * x).sum(0) - mu * self.dbeta)
        if rounding:
            self.e_db = e_g.sum(0) + n * U * np.abs(g).sum(0)
            self.e_dg = rs * ((e_g * np.abs(x)).sum(0) + (n + 2) * U * np.abs(g * x).sum(0)
                              + np.abs(mu) * (e_g.sum(0) + (n + 2) * U * np.abs(g).sum(0)))
        else:
            self.e_db = self.e_dg = np.zeros_like(self.dbeta)
        self.c1, self.c2 = self.dbeta / S, self.dgamma / S
        self.e_c1 = self.e_db / S + (U * np.abs(self.c1) if rounding else 0.0)
        self.e_c2 = self.e_dg / S + (U * np.abs(self.c2) if rounding else 0.0)
        self.rounding = rounding

    def param_grads(self):
        """dgamma, dbeta as written (one cast to fp32 more)."""
        return {"dbeta": (self.dbeta, self.e_db + U * np.abs(self.dbeta)),
                "dgamma": (self.dgamma, self.e_dg + U * np.abs(self.dgamma))}

    def delta(self, c1=None, c2=None, e_c1=None, e_c2=None, premultiplied=False):
        """delta = fmaf(sc, g, fmaf(ka, x, kb)) before its rounding to bf16: (ref, bound e of the fp32 value).
        MODE 1 (premultiplied False): ka = -sc*c2*rstd, kb = fmaf(-ka, mean, -sc*c1) with c = (mean g, mean g*xhat).
        MODE 2 (premultiplied True):  ka = -c2*rstd,    kb = fmaf(-ka, mean, -c1)    with c = sc*(means) of the previous pass."""
        p, x = self.p, self.x
        c1 = self.c1 if c1 is None else c1
        c2 = self.c2 if c2 is None else c2
        e_c1 = self.e_c1 if e_c1 is None else e_c1
        e_c2 = self.e_c2 if e_c2 is None else e_c2
        mu, rs, sc = p.mean, p.rstd, p.sc
        s = np.ones_like(sc) if premultiplied else sc
        ka = -s * c2 * rs
        kb = -ka * mu - s * c1
        ref = sc * self.g + ka * x + kb
        if not self.rounding:
            return ref, np.zeros_like(ref)
        e_ka = np.abs(s * rs) * e_c2 + 2 * U * np.abs(ka)
        e_kb = e_ka * np.abs(mu) + np.abs(s) * e_c1 + 2 * U * (np.abs(ka * mu) + np.abs(s * c1))
        e = (np.abs(sc) * self.e_g + e_ka * np.abs(x) + e_kb + U * (np.abs(ka * x) + np.abs(kb))
             + U * (np.abs(sc * self.g) + np.abs(ka * x + kb)))
        return ref, e


def head_kacc(h, gamma):
    """bn1_bwd_finalize_kernel's single-pass output kacc[c] = (float)(gamma*rstd*(sum g, sum g*xhat)/S), the product
    gamma*rstd formed in double (NOT the fp32 sc of the prologue).  (C, 2) reference and bound."""
    scv = np.asarray(gamma, dtype=np.float64) * h.p.rstd
    k = np.stack([scv * h.dbeta / h.S, scv * h.dgamma / h.S], 1)
    e = np.stack([np.abs(scv) * h.e_db / h.S, np.abs(scv) * h.e_dg / h.S], 1) + U * np.abs(k)
    return k, e


def pair_delta(hA, cA, hB, cB, C):
    """bn1_dx_pair_kernel: fmaf(scA, gA, fmaf(scB, gB, fmaf(kaA + kaB, x, kbA + kbB))) on the C channels both layers read, the
    coefficients (C, 2) given.  hA: Head of the later layer (C + 32 input channels), hB: of the earlier one.  The sum is rounded to
    bf16 ONCE and then added to gbuf like any delta (gbuf_add)."""
    z = np.zeros(hA.p.sc.shape[0])
    rA, eA = hA.delta(np.pad(cA[:, 0], (0, z.size - C)), np.pad(cA[:, 1], (0, z.size - C)), z, z)
    rB, eB = hB.delta(cB[:, 0], cB[:, 1], 0.0, 0.0)
    rA, eA = rA[:, :C], eA[:, :C]
    return rA + rB, eA + eB + U * (np.abs(rA) + np.abs(rB))


def bn1_wrw(dz, W1, x, gamma, beta, mean, rstd, nterms):
    """mcl_dense_bn1_wrw (wrw_partial_kernel<1> + wrw_merge_kernel): the Gram form.  Per pixel slab, in fp32 on the matrix
    unit, R = dz^T mask and Qx = dz^T (mask*x) (exact operands); then per slab Q = rstd*fmaf(-mean, R, Qx), the weight-gradient
    partial fmaf(gamma, Q, beta*R) and the partial sums sum_m W1*R, sum_m W1*Q; the slabs are added in fp32.  So dW1 here is
    dz^T of the UNROUNDED a = mask*(gamma*xhat + beta) with gamma, rstd used apart -- not of bf16(a) as in the forward and in
    mcl_conv1x1_wrw_det (a rounding point that differs between the two weight-gradient forms).  nterms = fp32 additions along
    the longest path (pixels of a slab + slabs + the epilogue).  Every bound is nterms*u*(the same expression on absolute
    values).  Returns dict name -> (ref, bound): dW (128, C), dgamma, dbeta (C,), coef (C, 2)."""
    p = Prologue(x, gamma, beta, mean, rstd)
    dz, W1, x = (np.asarray(v, dtype=np.float64) for v in (dz, W1, x))
    g, b, mu, rs = (np.asarray(v, dtype=np.float64) for v in (gamma, beta, mean, rstd))
    S = x.shape[0]
    m = p.mask.astype(np.float64)
    R, Qx = dz.T @ m, dz.T @ (m * x)
    aR, aQx = np.abs(dz).T @ m, np.abs(dz).T @ (m * np.abs(x))
    Q = rs * (Qx - mu * R)
    aQ = rs * (aQx + np.abs(mu) * aR)
    nu = nterms * U
    dW, e_dW = g * Q + b * R, nu * (np.abs(g) * aQ + np.abs(b) * aR)
    db, e_db = (W1 * R).sum(0), (nterms + 128) * U * (np.abs(W1) * aR).sum(0)
    dg, e_dg = (W1 * Q).sum(0), (nterms + 128) * U * (np.abs(W1) * aQ).sum(0)
    coef = np.stack([db, dg], 1) / S
    e_coef = np.stack([e_db, e_dg], 1) / S + 2 * U * np.abs(coef)          # v * (1.0f / (float)S): two roundings
    return {"dW": (dW, e_dW), "dbeta": (db, e_db), "dgamma": (dg, e_dg), "coef": (coef, e_coef)}


def wrw_slab_terms(S):
    """fp32 additions along the longest path of wrw_partial_kernel + wrw_merge_kernel: at most the S pixels (a slab holds
    fewer; the rows that pad it to whole tiles are zeros), at most ceil(S / 128) slabs (plan() in wrw_fused.hip keeps 128
    pixels or more per slab), and the epilogue's few operations."""
    return S + -(-S // 128) + 8


def wrw3_terms(S):
    """The same for mcl_dense_conv3x3_wrw_det: S pixels over at most 256 partials (88 pixel groups in the kernel-row form, one
    per workgroup in the row-walking form), merged in fp32."""
    return S + min(256, S) + 8


def gbuf_add(gbuf_old, delta_ref, e_delta, e_g=0.0):
    """gbuf <- bf16_rne(gbuf + bf16_rne(delta)): two roundings.  e_g: what the incoming gbuf may be off by (a chain of passes
    whose intermediate buffers are not kept).  (ref unrounded = gbuf + delta, bound)."""
    gbuf_old = np.asarray(gbuf_old, dtype=np.float64)
    b1 = once_rounded(delta_ref, e_delta) + e_g                    # the stored bf16 delta
    ref = gbuf_old + delta_ref
    return ref, half_ulp_bf16(np.abs(ref) + b1) + b1 + U * np.abs(ref)   # one fp32 add of two bf16 values, then bf16


def gbuf_add_once(gbuf_old, delta_ref, e_delta):
    """The pair form: the deltas are added in fp32 and the sum with gbuf is rounded to bf16 once more (delta rounded once)."""
    return gbuf_add(gbuf_old, delta_ref, e_delta)


def bn1_fix(gbuf_old, x, c0, nc, mean, rstd, kacc, e_k1=0.0, e_k2=0.0, e_g=0.0):
    """bn1_fix_kernel: gbuf[:, c] <- bf16_rne(gbuf - fmaf(ka, x, kb)), ka = k2*rstd, kb = fmaf(-ka, mean, k1), on the channels
    [c0, c0 + nc); kacc: (C, 2) = (k1, k2) already offset to channel 0 of x / gbuf; e_k1 / e_k2 (per channel of the window) and
    e_g (per element of the window): what kacc and the incoming gbuf may be off by.  (ref unrounded, bound)."""
    g, x = np.asarray(gbuf_old, dtype=np.float64)[:, c0:c0 + nc], np.asarray(x, dtype=np.float64)[:, c0:c0 + nc]
    mu, rs = np.asarray(mean, dtype=np.float64)[c0:c0 + nc], np.asarray(rstd, dtype=np.float64)[c0:c0 + nc]
    k1, k2 = np.asarray(kacc, dtype=np.float64)[c0:c0 + nc, 0], np.asarray(kacc, dtype=np.float64)[c0:c0 + nc, 1]
    ka = k2 * rs
    kb = k1 - ka * mu
    ref = g - (ka * x + kb)
    e_ka = rs * e_k2 + U * np.abs(ka)
    e_kb = e_ka * np.abs(mu) + e_k1 + U * (np.abs(ka * mu) + np.abs(k1))
    e = e_ka * np.abs(x) + e_kb + U * (np.abs(ka * x) + np.abs(kb)) + U * np.abs(ref) + e_g
    return ref, once_rounded(ref, e)


# ------------------------------------------------------------------------------------------------------------------ weight gradients
def _acc(ref, e, prior):
    """Overwrite (prior None) or accumulate semantics of an fp32 output: one more fp32 add, one store."""
    if prior is None:
        return ref, e + U * np.abs(ref)
    tot = np.asarray(prior, dtype=np.float64) + ref
    return tot, e + U * (np.abs(ref) + np.abs(tot))


def conv1x1_wrw(dz, a, prior=None, e_a=None, nterms=None):
    """dW[m][n] = sum_s dz[s][m]*a[s][n] in fp32 (slab partials merged in fixed order: nterms additions along the longest
    path, default S).  e_a: what an element of a may move by (ambiguous prologue elements)."""
    dz, a = np.asarray(dz, dtype=np.float64), np.asarray(a, dtype=np.float64)
    ref = dz.T @ a
    e = (nterms or dz.shape[0]) * U * (np.abs(dz).T @ np.abs(a))
    if e_a is not None:
        e = e + np.abs(dz).T @ e_a
    return _acc(ref, e, prior)


def conv3x3_wrw(dy, a2, B, H, W, prior=None, e_a=None, nterms=None):
    """dW2[co][ky][kx][ci] = sum_p dy[p][co]*a2[p + (ky-1, kx-1)][ci] over the taps inside the image: (32, 3, 3, 128)."""
    dy, a2 = np.asarray(dy, dtype=np.float64), np.asarray(a2, dtype=np.float64)
    S = B * H * W
    ap, aa = _pad(a2, B, H, W), _pad(np.abs(a2), B, H, W)
    ae = _pad(e_a, B, H, W) if e_a is not None else None
    ref = np.zeros((dy.shape[1], 3, 3, a2.shape[1]))
    e = np.zeros_like(ref)
    for ky, kx, sy, sx in _taps(H, W):
        ref[:, ky, kx, :] = dy.T @ ap[:, sy, sx, :].reshape(S, -1)
        e[:, ky, kx, :] = (nterms or S) * U * (np.abs(dy).T @ aa[:, sy, sx, :].reshape(S, -1))
        if ae is not None:
            e[:, ky, kx, :] += np.abs(dy).T @ ae[:, sy, sx, :].reshape(S, -1)
    return _acc(ref, e, prior)


# ------------------------------------------------------------------------------------------------------------------ inputs
def layer_params(C, seed, spread=True):
    """BatchNorm operands of C channels (fp32 values as float64): one negative gamma (channel 1) and one dead channel
    (channel 2: relu(bn(x)) == 0 everywhere); mean / rstd plausible for data of per-channel location loc and scale."""
    rng = np.random.default_rng(seed)
    loc, scale = rng.normal(0.0, 1.0, C), rng.uniform(0.5, 2.0, C)
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.normal(0.0, 0.3, C)
    if C > 1:
        gamma[1] = -0.7
    if C > 2:
        gamma[2], beta[2] = 0.1, -50.0
    mean = loc + 0.1 * scale * rng.normal(size=C)
    rstd = rng.uniform(0.8, 1.2, C) / scale
    return dict(loc=loc, scale=scale, gamma=f32(gamma), beta=f32(beta), mean=f32(mean), rstd=f32(rstd))


def activations(S, C, prm, seed):
    rng = np.random.default_rng(seed)
    return bf16(rng.normal(size=(S, C)) * prm["scale"] + prm["loc"])


def weights(shape, fan_in, seed, positive_row=None):
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, 1.0 / np.sqrt(fan_in), shape)
    if positive_row is not None:
        w[positive_row] = np.abs(w[positive_row])        # |mean| / std of that output channel ~ sqrt(fan_in)
    return bf16(w)


def gradients(shape, seed, scale=1e-2):
    rng = np.random.default_rng(seed)
    return bf16(rng.normal(0.0, scale, shape))


def bn(p):
    return p["gamma"], p["beta"], p["mean"], p["rstd"]


def conv1x1_case(S, K):
    prm = layer_params(K, 100 + K)
    return prm, activations(S, K, prm, 200 + K), weights((128, K), K, 300 + K, positive_row=5)


def tail_case(B, H, W):
    prm = layer_params(128, 400 + H * W)
    S = B * H * W
    return (prm, activations(S, 128, prm, 500 + S), weights((32, 3, 3, 128), 1152, 600 + S, positive_row=5),
            gradients((S, 32), 700 + S))


def head_case(S, C):
    prm = layer_params(C, 800 + C)
    return (prm, activations(S, C, prm, 900 + C), weights((128, C), C, 1000 + C),
            bf16(gradients((S, 128), 1100 + C) + 1e-3), gradients((S, C), 1200 + C))


def pair_case(S, C):
    """Two layers on one buffer: A reads C + 32 channels, B the first C; the statistics are the channels'."""
    C2 = C + 32
    prmA = layer_params(C2, 2100 + C)
    prmB = {k: v[:C] for k, v in dict(prmA, **{k: layer_params(C2, 2200 + C)[k] for k in ("gamma", "beta")}).items()}
    x = activations(S, C2, prmA, 2300 + C)
    gb = gradients((S, C2), 2400 + C)
    dzA, dzB = (bf16(gradients((S, 128), 2500 + C + i) + 1e-3) for i in range(2))
    return prmA, prmB, x, gb, dzA, dzB, weights((128, C2), C2, 2600 + C), weights((128, C), C, 2700 + C)


def wrw1_case(S, M, N):
    prm = layer_params(N, 2800 + N)
    return prm, activations(S, N, prm, 2900 + N), bf16(gradients((S, M), 3000 + M) + 1e-3)


# the shapes of the GPU tests (tests/test_dense_exact_gpu.py); the host tests run the fp32 emulation on the same ones
CONV1X1_SHAPES = [(65, 8, 16), (300, 96, 96), (129, 992, 1024), (70, 1024, 1024), (32768, 64, 256), (32805, 72, 80)]  # S, K, ldx
CONV3X3_FLAT = [(1, 1, 1, 32), (1, 5, 3, 32), (3, 10, 6, 64), (5, 7, 7, 1024), (1, 14, 14, 32), (1, 1, 16, 32)]       # B, H, W, ld
CONV3X3_ROWS = [(1, 1, 17, 32), (1, 3, 32, 64), (2, 5, 33, 96), (1, 3, 97, 64), (2, 2, 150, 32), (3, 9, 17, 64)]
HEAD_SHAPES = [(63, 8, 8), (300, 96, 96), (129, 128, 512), (129, 136, 512), (257, 264, 512)]                          # S, C, ld
PAIR_SHAPES = [(300, 96, 160), (129, 136, 512)]
WRW3_SHAPES = [(3, 10, 6), (1, 1, 40), (2, 5, 33), (7, 2, 20)]                                                        # B, H, W
WRW1_SHAPES = [(300, 256, 512), (31, 128, 992), (777, 128, 160)]                                                      # S, M, N
AMB_CAP = 1e-3
