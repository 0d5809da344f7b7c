"""Float64 restatement of the kernels AROUND the dense layers of the DenseNet backbone -- conv0 (csrc/dense_conv.hip), the
BatchNorm(+ReLU) passes of the stem and the transitions (csrc/bnrelu.hip), the pools (csrc/pool.hip), norm5 + global pool
(csrc/step_misc.hip) and the transition's data gradient (csrc/gemm_bf16.hip) -- in the style of tests/dense_reference.py, whose
primitives it imports.  numpy only: no GPU, no torch.  Per entry point EITHER the exact bits of the output (the code leaves the
compiler no freedom: single fp32 operations, explicit fmaf, fixed-order adds) OR the float64 value with a bound for every
element derived from that element's own operands (accumulation order or contraction is free).  ``rounding=False`` switches
every rounding point off: plain real arithmetic, checked against fp64 autograd in tests/test_stem_reference_host.py.

Rounding points, as read from the code:

  prologue (every BatchNorm kernel)   sc = fp32(gamma*rstd) (one multiply); sh = fmaf(-mean, sc, beta); t = fmaf(x, sc, sh).  The
        ReLU mask of every backward pass is [t > 0] (the kernels test ``t <= 0``); the sign of a correctly rounded fmaf is the
        sign of the exact value, and x*sc is exact in float64, so the mask is EXACT.
  mcl_bn_act_fwd        y = t or fmaxf(t, 0), stored as fp32 or bf16_rne: EXACT, both dtypes.
  mcl_bn_act_avgpool_fwd   v = fmaxf(t, 0) per pixel; y = bf16_rne(0.25f*((va + vb) + (vc + vd))), every add rounded to fp32,
        windows of floor(H/2) x floor(W/2): EXACT.
  mcl_avgpool2_nhwc_bf16   forward the same sum on the raw bf16 values; backward bf16_rne(0.25f*dy): EXACT.
  mcl_maxpool3s2_nhwc_bf16_fwd / mcl_bn_act_maxpool_fwd   the nine taps in row-major window order, taps outside the map skipped,
        ``v > m`` strict from m = -inf: the FIRST maximum wins and -0.0 does not beat +0.0.  With BatchNorm v = fmaxf(t, 0) in
        fp32 and the arg-max is decided on that fp32 value; y = bf16_rne(max).  y and idx EXACT.
  mcl_maxpool3s2_nhwc_bf16_bwd_ld   dx = bf16_rne(sum of dy over the at most four windows (ay, ax) in {0,1}^2 order whose recorded
        arg-max is this pixel), fp32 adds from 0 in that order: EXACT (generic and quad kernels alike).
  mcl_bn_stats          per thread fp32 shifted sums d = x - x[row 0] (one rounding), s1 += d, s2 = fmaf(d, d, s2) over
        ceil(rows_per_block / rpi) rows; rpi threads merged in fp32 through LDS; the finalize adds groups of up to 4 partials in
        fp32, then double.  mean = fp32(x[0] + a/S), var = fp32(max(b/S - (a/S)^2, 0)), rstd = fp32(1/sqrt(var + eps)) in
        double.  BOUND with the chain length L = rows per thread + rpi + 4 of plan(), restated here.  copy_out EXACT (a copy).
  mcl_bn_act_bwd / mcl_bn_act_avgpool_bwd   g = dy (pool: 0.25f*dp[window], exact; 0 on the unpaired last row / column of an odd
        map) times the mask; s1 += g, s2 = fmaf(g, fp32(fp32(x - mean)*rstd), s2), the same merge scheme; dbeta = fp32(a),
        dgamma = fp32(b) (accumulate_params: += in fp32), coef = fp32(a/S), fp32(b/S) with S ALL pixels: BOUND.  dx =
        sc*(g - c1 - xhat*c2) (+ dx) from the kernel's own coef: xhat*c2 may be contracted into the subtraction and sc*(..) into
        the accumulate, so BOUND: g and c1 pass three roundings, xhat*c2 five, then the add, then one bf16 rounding (bf16 dtype).
  mcl_conv0_fwd         y = bf16_rne(147-term fp32 accumulation on the matrix unit, taps outside the image zero): BOUND.  The
        statistics are those of the STORED y: per tile of 2*OW pixels unshifted fp32 sums of v and v^2, M2 = s2 - s1*s1/n in
        fp32, merged by Chan's method in double: BOUND.
  mcl_conv0_wrw         dW = sum_p dy*x in fp32 over the pixels of a workgroup's tiles (rows padded to 16 pixels with zeros), the
        workgroups merged in fixed order in fp32 (32 groups of eight accumulators); accumulate: one more add: BOUND.
  mcl_bn_gap_fwd        m = fp32(fp32 sum over HW in four interleaved chains, merged (0+1)+(2+3)) * fp32(1/HW); out = fmaf(m -
        mean, sc, beta): BOUND for out and xmean.
  mcl_bn_gap_bwd        from the kernel's own xmean: a = sum_b g, q = sum_b g*fp32(fp32(xm - mean)*rstd) in double; dbeta, dgamma,
        coef cast to fp32; dx = bf16_rne(gamma*rstd*(g*fp32(1/HW) - c1 - (x - mean)*rstd*c2)) from the kernel's own coef, the
        roundings counted per term (six, four, six): BOUND.
  mcl_gemm_bf16 as TransitionFn.backward calls it   dp = bf16_rne(sum_co dy*W), Co terms in fp32: BOUND.
  the transition's forward conv1x1 is mcl_dense_conv1x1_fwd with the identity prologue: dense_reference.conv1x1_fwd / stats_tiles.

Bounds follow dense_reference.py: U = 2^-23 per fp32 operation (twice the round-to-nearest error, so second-order terms are
covered), n*U*sum|terms| for an n-term fp32 chain in any order, once_rounded() for one bf16 rounding, propagated bounds for
operands the kernel computed itself.  Nothing is tuned."""
import numpy as np

from dense_reference import U, bf16, bf16_bits, f32, fma32, once_rounded, _rstd_bound, stats_ref
import dense_reference as dr

NTH = 256


# ------------------------------------------------------------------------------------------------------------------ primitives
def fma32v(a, b, c):
    """fma32 for whole tensors: fp32(a*b + c) rounded once.  The product is exact in float64; the float64 sum is made STICKY
    (rounded to odd: where it is inexact and its last bit is even it moves one float64 towards the exact value), and a value
    rounded to odd at 53 bits rounds to 24 bits like the exact one.  Equal to dense_reference.fma32 (checked on the host)."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    p = a * b
    s = p + c
    bv = s - p
    err = (p - (s - bv)) + (c - bv)
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    fix = (err != 0.0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return f32(s)


def add32(a, b):
    """fp32(a + b), rounded once (the float64 sum of two fp32 values far apart is itself rounded: made sticky like fma32v)."""
    return fma32v(a, 1.0, b)


def f32_bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64).astype(np.float32)).view(np.uint32)


def _p(prm):
    return tuple(np.asarray(prm[k], dtype=np.float64) for k in ("gamma", "beta", "mean", "rstd"))


def prologue(prm, rounding=True):
    """(sc, sh) as every kernel forms them."""
    g, b, m, r = _p(prm)
    if not rounding:
        return g * r, b - m * g * r
    sc = f32(g * r)
    return sc, fma32(-m, sc, b)


def bn_t(x, prm, rounding=True):
    """t = fmaf(x, sc, sh): the fp32 value (rounding) or the real one."""
    sc, sh = prologue(prm, rounding)
    x = np.asarray(x, dtype=np.float64)
    return fma32v(x, sc, sh) if rounding else x * sc + sh


def relu_mask(x, prm, rounding=True):
    """[t > 0], exact: x*sc is exact in float64 and the float64 sum keeps the sign of the exact one."""
    sc, sh = prologue(prm, rounding)
    return np.asarray(x, dtype=np.float64) * sc + sh > 0.0


def store_bits(v, dtype):
    """The bits a kernel stores for the fp32 value v: dtype 1 bf16 (round to nearest even), dtype 0 fp32."""
    return bf16_bits(v) if dtype == 1 else f32_bits(v)


# ------------------------------------------------------------------------------------------------------------------ exact: forward passes
def bn_act_fwd(x, prm, relu, rounding=True):
    """mcl_bn_act_fwd: the fp32 value before the store (store_bits gives the bits)."""
    t = bn_t(x, prm, rounding)
    return np.maximum(t, 0.0) if relu else t


def _win4(v, H, W):
    """The four pixels of every 2x2 window (floor pooling) of v (N, H, W, C)."""
    h2, w2 = 2 * (H // 2), 2 * (W // 2)
    return v[:, 0:h2:2, 0:w2:2], v[:, 0:h2:2, 1:w2:2], v[:, 1:h2:2, 0:w2:2], v[:, 1:h2:2, 1:w2:2]


def avgpool_fwd(v, rounding=True):
    """0.25f*((a + b) + (c + d)), every add rounded to fp32.  v: (N, H, W, C) fp32 values.  The fp32 value before the store."""
    N, H, W, C = v.shape
    a, b, c, d = _win4(np.asarray(v, dtype=np.float64), H, W)
    if not rounding:
        return 0.25 * (a + b + c + d)
    return 0.25 * add32(add32(a, b), add32(c, d))            # 0.25f* is exact


def bn_act_avgpool_fwd(x, prm, rounding=True):
    """mcl_bn_act_avgpool_fwd on x (N, H, W, C)."""
    return avgpool_fwd(np.maximum(bn_t(x, prm, rounding), 0.0), rounding)


def avgpool_bwd(dy, H, W, drop_quarter=False):
    """mcl_avgpool2_nhwc_bf16 backward / the gradient reaching pixel (y, x) through the pool: 0.25f*dy[y/2, x/2] (exact in fp32),
    zero on the unpaired last row / column of an odd map.  dy: (N, H/2, W/2, C)."""
    dy = np.asarray(dy, dtype=np.float64)
    g = np.zeros((dy.shape[0], H, W, dy.shape[3]))
    h2, w2 = 2 * (H // 2), 2 * (W // 2)
    g[:, :h2, :w2] = np.repeat(np.repeat(dy, 2, axis=1), 2, axis=2) * (1.0 if drop_quarter else 0.25)
    return g


def maxpool_fwd(v, last_wins=False):
    """MaxPool2d(3, 2, 1) of v (N, H, W, C): (max, idx) with idx = ky*3 + kx of the FIRST maximum in row-major window order, taps
    outside the map skipped (-inf padding never passes the strict comparison)."""
    v = np.asarray(v, dtype=np.float64)
    N, H, W, C = v.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    vp = np.pad(v, ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=-np.inf)
    m = np.full((N, OH, OW, C), -np.inf)
    am = np.zeros((N, OH, OW, C), dtype=np.uint8)
    for t in range(9):
        ky, kx = divmod(t, 3)
        sl = vp[:, ky:ky + 2 * OH - 1:2, kx:kx + 2 * OW - 1:2]
        take = (sl >= m) & np.isfinite(sl) if last_wins else sl > m
        m = np.where(take, sl, m)
        am = np.where(take, np.uint8(t), am)
    return m, am


def bn_act_maxpool_fwd(x, prm, rounding=True):
    """mcl_bn_act_maxpool_fwd: the arg-max decided on the fp32 value fmaxf(t, 0); y is its bf16 rounding."""
    return maxpool_fwd(np.maximum(bn_t(x, prm, rounding), 0.0))


def maxpool_bwd(idx, dy, H, W, rounding=True):
    """mcl_maxpool3s2_nhwc_bf16_bwd_ld: per input pixel the fp32 sum, in window order (ay, ax) = (0,0), (0,1), (1,0), (1,1), of
    dy over the windows whose recorded arg-max is this pixel.  idx, dy: (N, OH, OW, C).  The fp32 value before the store."""
    idx, dy = np.asarray(idx), np.asarray(dy, dtype=np.float64)
    N, OH, OW, C = dy.shape
    iy, ix = np.arange(H), np.arange(W)
    acc = np.zeros((N, H, W, C))
    for w in range(4):
        ay, ax = w >> 1, w & 1
        oy, ox = iy // 2 + ay, ix // 2 + ax
        vy = ((ay == 0) | (iy & 1 == 1)) & (oy < OH)
        vx = ((ax == 0) | (ix & 1 == 1)) & (ox < OW)
        me = (iy - (2 * oy - 1))[:, None] * 3 + (ix - (2 * ox - 1))[None, :]
        oyc, oxc = np.minimum(oy, OH - 1), np.minimum(ox, OW - 1)
        g = dy[:, oyc][:, :, oxc]
        hit = (vy[:, None] & vx[None, :])[None, :, :, None] & (idx[:, oyc][:, :, oxc] == me[None, :, :, None])
        acc = np.where(hit, add32(acc, g) if rounding else acc + g, acc)
    return acc


# ------------------------------------------------------------------------------------------------------------------ plan()
def plan(S, C, dtype):
    """plan() of csrc/bnrelu.hip: (row blocks, rows per block, channel tiles)."""
    V = 8 if dtype == 1 else 4
    cvn_all = C // V
    cvn = min(cvn_all, NTH)
    rpi = NTH // cvn
    rpb = rpi * 8
    nb = -(-S // rpb)
    if nb > 1024:
        nb = 1024
        rpb = -(-S // nb)
        rpb = -(-rpb // rpi) * rpi
        nb = -(-S // rpb)
    return nb, rpb, -(-cvn_all // NTH)


def chain(S, C, dtype):
    """Per channel, the fp32 additions along the longest path of a per-channel sum: the rows one thread walks, the rpi threads
    merged through LDS, a group of 4 partials in the finalize (everything after that is double)."""
    V = 8 if dtype == 1 else 4
    nb, rpb, tiles = plan(S, C, dtype)
    L = np.zeros(C)
    for t in range(tiles):
        cvn = min(C // V - t * NTH, NTH)
        rpi = NTH // cvn
        L[t * NTH * V:(t * NTH + cvn) * V] = -(-min(rpb, S) // rpi) + rpi + 4
    return L


# ------------------------------------------------------------------------------------------------------------------ bounded: BatchNorm
def bn_stats(x, eps, dtype):
    """mcl_bn_stats of x (S, C): ((mean, var, rstd), (bounds)), the shifted-sum scheme with plan()'s chain lengths."""
    x = np.asarray(x, dtype=np.float64)
    S, C = x.shape
    L = chain(S, C, dtype)
    d = x - x[0]
    a, b = d.sum(0), (d * d).sum(0)
    e_a = (L + 1) * U * np.abs(d).sum(0)                    # the rounding of d itself, then L additions
    e_b = (L + 3) * U * b                                   # d's rounding enters d^2 twice
    m = a / S
    mean = x[0] + m
    var = np.maximum(b / S - m * m, 0.0)
    e_mean = e_a / S + U * np.abs(mean)
    e_var = e_b / S + 2 * np.abs(m) * e_a / S + (e_a / S) ** 2 + U * var
    return (mean, var, 1.0 / np.sqrt(var + eps)), (e_mean, e_var, _rstd_bound(var, e_var, eps))


def bn_bwd_sums(g, x, prm, L, prior=(None, None), S_coef=None):
    """dbeta, dgamma, coef from the masked gradient g (S, C) (already 0 where the ReLU is off): name -> (ref, bound).  L: chain
    lengths; prior: (dgamma, dbeta) before the call when accumulate_params; S_coef: what coef divides by (default: all rows)."""
    g, x = np.asarray(g, dtype=np.float64), np.asarray(x, dtype=np.float64)
    _, _, mu, rs = _p(prm)
    S = g.shape[0] if S_coef is None else S_coef
    xh = (x - mu) * rs
    db, dg = g.sum(0), (g * xh).sum(0)
    e_db = L * U * np.abs(g).sum(0)
    e_dg = (L + 2) * U * np.abs(g * xh).sum(0)              # xhat carries two fp32 roundings
    out = {"coef": (np.stack([db / S, dg / S], 1), np.stack([e_db / S + U * np.abs(db / S), e_dg / S + U * np.abs(dg / S)], 1))}
    for nm, v, e, pr in (("dgamma", dg, e_dg, prior[0]), ("dbeta", db, e_db, prior[1])):
        e = e + U * np.abs(v)                               # the cast to fp32
        if pr is not None:
            v = np.asarray(pr, dtype=np.float64) + v
            e = e + U * np.abs(v)                           # += in fp32
        out[nm] = (v, e)
    return out


def bn_bwd_dx(g, x, prm, coef, dtype, prior=None, rounding=True):
    """dx = sc*(g - c1 - xhat*c2) (+ prior) from the given coef (C, 2) (the kernel's own): (ref unrounded, bound of the stored
    value).  d = sc*((g - c1) - xhat*c2): g and c1 pass three roundings (the two subtractions, *sc), xhat*c2 five (x - mean,
    *rstd, *c2, the second subtraction, *sc); contraction only removes roundings."""
    g, x = np.asarray(g, dtype=np.float64), np.asarray(x, dtype=np.float64)
    _, _, mu, rs = _p(prm)
    sc, _ = prologue(prm, rounding)
    c1, c2 = np.asarray(coef, dtype=np.float64)[:, 0], np.asarray(coef, dtype=np.float64)[:, 1]
    xh = (x - mu) * rs
    d = sc * (g - c1 - xh * c2)
    if not rounding:
        return (d if prior is None else prior + d), 0.0
    e = np.abs(sc) * U * (3 * (np.abs(g) + np.abs(c1)) + 5 * np.abs(xh * c2))
    ref = d
    if prior is not None:
        ref = np.asarray(prior, dtype=np.float64) + d
        e = e + U * np.abs(ref)
    return ref, (once_rounded(ref, e) if dtype == 1 else e)


def pool_gradient(dp, x, prm, H, W, to_unpaired=False, drop_quarter=False, rounding=True):
    """The masked gradient of mcl_bn_act_avgpool_bwd: (N*H*W, C) from dp (N, H/2, W/2, C) and x (N, H, W, C).  to_unpaired
    (mutant): the last row / column of an odd map takes the gradient of the window beside it."""
    g = avgpool_bwd(dp, H, W, drop_quarter)
    if to_unpaired:
        if H & 1:
            g[:, H - 1] = g[:, H - 2]
        if W & 1:
            g[:, :, W - 1] = g[:, :, W - 2]
    C = g.shape[3]
    return np.where(relu_mask(x, prm, rounding), g, 0.0).reshape(-1, C)


# ------------------------------------------------------------------------------------------------------------------ bounded: conv0
def conv0_patches(x, top_reads_row0=False):
    """im2col of the 7x7 stride-2 pad-3 stem convolution: x (N, H, W, 3) -> (N*OH*OW, 147) in (ky, kx, c) order.  top_reads_row0
    (mutant): tap ky = 0 of the first output row reads input row 0 instead of the zero padding."""
    x = np.asarray(x, dtype=np.float64)
    N, H, W, _ = x.shape
    OH, OW = H // 2, W // 2
    xp = np.pad(x, ((0, 0), (3, 3), (3, 3), (0, 0)))
    cols = []
    for ky in range(7):
        for kx in range(7):
            t = xp[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2].copy()
            if top_reads_row0 and ky == 0:
                t[:, 0] = xp[:, 3, kx:kx + 2 * OW:2]
            cols.append(t)
    return np.stack(cols, 3).reshape(N * OH * OW, 147)


def conv0_fwd(x, Wt):
    """(ref unrounded (P, 64), bound of the stored bf16 y).  Wt: (64, 7, 7, 3)."""
    A, Wm = conv0_patches(x), np.asarray(Wt, dtype=np.float64).reshape(64, 147)
    ref = A @ Wm.T
    return ref, once_rounded(ref, 147 * U * (np.abs(A) @ np.abs(Wm).T))


def conv0_border(N, H, W):
    """Flat indices of the output pixels with at least one tap outside the image."""
    OH, OW = H // 2, W // 2
    oy, ox = np.meshgrid(np.arange(OH), np.arange(OW), indexing="ij")
    edge = ((2 * oy - 3 < 0) | (2 * oy + 3 >= H) | (2 * ox - 3 < 0) | (2 * ox + 3 >= W)).reshape(-1)
    return np.nonzero(np.tile(edge, N))[0]


def stats_tiles_unshifted(v, eps, n):
    """mean / var / rstd of the stored v (P, C), P a multiple of n, under conv0_fwd_kernel's scheme: per tile of n pixels fp32 sums
    of v and v^2 (any order: n*U*sum|terms|), M2 = s2 - s1*s1/n in fp32, Chan's merge in double."""
    v = np.asarray(v, dtype=np.float64)
    P, C = v.shape
    m, var, rstd = stats_ref(v, eps)
    t = v.reshape(P // n, n, C)
    a1, s1, s2 = np.abs(t).sum(1), t.sum(1), (t * t).sum(1)
    e_s1, e_s2 = n * U * a1, n * U * s2
    e_m2 = e_s2 + 2 * np.abs(s1) * e_s1 / n + e_s1 ** 2 / n + 2 * U * s1 * s1 / n + U * (s2 + s1 * s1 / n)
    e_sum = e_s1.sum(0)
    e_var = (e_m2 + 2 * np.abs(s1 / n - m) * e_s1 + e_s1 ** 2 / n).sum(0)
    e_mean = e_sum / P + U * np.abs(m)
    e_var = e_var / P + (e_sum / P) ** 2 + U * var
    return (m, var, rstd), (e_mean, e_var, _rstd_bound(var, e_var, eps))


def conv0_wrw_terms(N, H, W):
    """fp32 additions along the longest path of mcl_conv0_wrw.  The 2*OW pixels of each of a workgroup's tiles (the columns that
    pad a row to 16 pixels are zeros: no rounding); then wrw_merge_kernel over the grid workgroups: 32 groups, each its slabs
    g, g + 32, .. over eight accumulators (ceil(grid / 256) terms each, a tree of three adds), the groups added in order (31)."""
    ntile = N * (H // 4)
    grid = min(ntile, 768)
    return -(-ntile // grid) * 2 * (W // 2) + min(grid, -(-grid // 256) + 34)


def conv0_wrw(x, dy, N, H, W, prior=None):
    """dW (64, 147) = dy^T patches: (ref, bound), overwrite or accumulate."""
    A, dy = conv0_patches(x), np.asarray(dy, dtype=np.float64)
    ref = dy.T @ A
    return dr._acc(ref, conv0_wrw_terms(N, H, W) * U * (np.abs(dy).T @ np.abs(A)), prior)


# ------------------------------------------------------------------------------------------------------------------ bounded: norm5 + pool
def bn_gap_fwd(x, prm, rounding=True):
    """x (B, HW, C): {"out": (ref, bound), "xmean": (ref, bound)}."""
    x = np.asarray(x, dtype=np.float64)
    B, HW, C = x.shape
    _, beta, mu, _ = _p(prm)
    sc, _ = prologue(prm, rounding)
    m = x.mean(1)
    out = (m - mu) * sc + beta
    if not rounding:
        return {"out": (out, 0.0), "xmean": (m, 0.0)}
    e_m = (-(-HW // 4) + 2) * U * np.abs(x).sum(1) / HW + 2 * U * np.abs(m)        # the chains, fp32(1/HW) and the multiply
    e_out = np.abs(sc) * (e_m + U * np.abs(m - mu)) + U * np.abs(out)               # m - mean, then the fmaf
    return {"out": (out, e_out), "xmean": (m, e_m)}


def bn_gap_bwd_sums(g, xm, prm, HW, prior=(None, None)):
    """From g (B, C) fp32 and the kernel's own xmean (B, C): dbeta, dgamma, coef -> (ref, bound).  The sums run in double."""
    g, xm = np.asarray(g, dtype=np.float64), np.asarray(xm, dtype=np.float64)
    _, _, mu, rs = _p(prm)
    S = g.shape[0] * HW
    xh = (xm - mu) * rs
    a, q = g.sum(0), (g * xh).sum(0)
    e_a, e_q = 2.0 ** -45 * np.abs(g).sum(0), 2 * U * np.abs(g * xh).sum(0)
    out = {"coef": (np.stack([a / S, q / S], 1), np.stack([e_a / S + U * np.abs(a / S), e_q / S + U * np.abs(q / S)], 1))}
    for nm, v, e, pr in (("dgamma", q, e_q, prior[0]), ("dbeta", a, e_a, prior[1])):
        e = e + U * np.abs(v)
        if pr is not None:
            v = np.asarray(pr, dtype=np.float64) + v
            e = e + U * np.abs(v)
        out[nm] = (v, e)
    return out


def bn_gap_bwd_dx(g, x, prm, coef, rounding=True):
    """dx (B, HW, C) = (gamma*rstd)*((g*fp32(1/HW) - c1) - ((x - mean)*rstd)*c2) from the given coef: (ref unrounded, bound of the
    stored bf16).  Roundings per term: g six (1/HW, its product, two subtractions, the last product, gamma*rstd), c1 four,
    xhat*c2 six (x - mean, *rstd, *c2, one subtraction, the last product, gamma*rstd)."""
    g, x = np.asarray(g, dtype=np.float64), np.asarray(x, dtype=np.float64)
    gam, _, mu, rs = _p(prm)
    HW = x.shape[1]
    c1, c2 = np.asarray(coef, dtype=np.float64)[:, 0], np.asarray(coef, dtype=np.float64)[:, 1]
    xh = (x - mu) * rs
    gh = g[:, None, :] / HW
    ref = gam * rs * (gh - c1 - xh * c2)
    if not rounding:
        return ref, 0.0
    e = np.abs(gam * rs) * U * (6 * np.abs(gh) + 4 * np.abs(c1) + 6 * np.abs(xh * c2))
    return ref, once_rounded(ref, e)


# ------------------------------------------------------------------------------------------------------------------ bounded: transition dp
def transition_dp(dy, Wt):
    """dp = dy . W as TransitionFn.backward asks mcl_gemm_bf16 for it: dy (Sq, Co), W (Co, C): (ref, bound of the stored bf16)."""
    dy, Wt = np.asarray(dy, dtype=np.float64), np.asarray(Wt, dtype=np.float64)
    ref = dy @ Wt
    return ref, once_rounded(ref, Wt.shape[0] * U * (np.abs(dy) @ np.abs(Wt)))


# ------------------------------------------------------------------------------------------------------------------ inputs
def stem_params(C, seed):
    """BatchNorm operands of C channels, after dense_reference.layer_params: channel 1 has a negative gamma, channel 2 is dead
    (beta far below zero), channel 3 has |mean|/std ~ 1e3, channel 4 (TIE) has gamma = rstd = 1, beta = 0, mean = 1 on data in
    {0, 1, 2, 3}: t == 0 exactly where x == 1, the case that tells ``t <= 0`` from ``t < 0``."""
    p = dr.layer_params(C, seed)
    if C > 3:
        p["loc"][3] = 1e3 * p["scale"][3]
        p["mean"][3] = f32(p["loc"][3] * (1 + 1e-5))
    if C > 4:
        for k, v in (("gamma", 1.0), ("beta", 0.0), ("mean", 1.0), ("rstd", 1.0)):
            p[k][4] = v
    return p


def stem_activations(shape, prm, seed, dtype=1):
    """Activations of shape (..., C): bf16 values (dtype 1) or fp32 values (dtype 0)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=shape) * prm["scale"] + prm["loc"]
    if shape[-1] > 4:
        x[..., 4] = rng.integers(0, 4, shape[:-1])
    return bf16(x) if dtype == 1 else f32(x)


def bn_case(dtype, S, C):
    """(parameters, activations, gradient) of the BatchNorm cases, host and GPU tests alike."""
    prm = stem_params(C, 11 + C)
    return prm, stem_activations((S, C), prm, 12 + S, dtype), stem_gradients((S, C), 13 + S, dtype)


def stem_gradients(shape, seed, dtype=1, scale=1e-2, offset=2e-3):
    """A gradient with a non-zero mean (as in training), so that the mean terms of the BatchNorm backward matter."""
    g = np.random.default_rng(seed).normal(offset, scale, shape)
    return bf16(g) if dtype == 1 else f32(g)


def conv0_case(N, H, W, seed=0):
    """Image (N, H, W, 3) and weight (64, 7, 7, 3), bf16 values; output channel 5 has all-positive weights and the image a
    positive mean, so that channel's |mean|/std is large."""
    rng = np.random.default_rng(1000 * N + 10 * H + W + seed)
    x = bf16(rng.normal(0.4, 1.0, (N, H, W, 3)))
    return x, dr.weights((64, 7, 7, 3), 147, 77 + seed, positive_row=5)


# the shapes of the GPU tests (tests/test_stem_exact_gpu.py); the host tests run the fp32 emulations on the small ones
BN_SHAPES = [(1, 1, 8, 8), (1, 777, 40, 256), (0, 333, 1028, 1032), (1, 50, 2056, 2056), (0, 8400, 1000, 1000)]   # dtype, S, C, ld
AVGPOOL_BN_SHAPES = [(2, 4, 2, 40), (3, 5, 9, 64), (2, 7, 7, 256), (1, 14, 14, 1024)]                             # N, H, W, C
AVGPOOL_SHAPES = [(2, 2, 2, 8), (3, 6, 10, 40)]
MAXPOOL_SHAPES = [(1, 1, 1, 8, 8), (2, 1, 5, 8, 8), (3, 17, 9, 64, 64), (2, 6, 10, 40, 40), (2, 16, 16, 64, 96),
                  (1, 2, 2, 8, 8)]                                                                                # N, H, W, C, lddy
# conv0: (155, 20, 8) has 775 tiles > 768 (a second tile per workgroup).  tile_stats_finalize_kernel takes the LAST tile apart
# (nfull = tiles - 1) and a thread walks t0 = tid, tid + 2048, .. < nfull: at 2049 tiles nfull = 2048 and every thread still
# makes one trip (tile 2048 is the last one, taken by thread 0 outside the loop); the second trip needs nfull > 2048, i.e. 2050
# tiles or more.  2060 tiles: threads 0 .. 10 make it (tiles 2048 .. 2058, their other seven loads clamped and zeroed), thread 11
# takes the last tile.
CONV0_SHAPES = [(1, 4, 8), (2, 8, 72), (3, 12, 40), (1, 4, 256), (155, 20, 8), (2049, 4, 8), (2060, 4, 8)]        # N, H, W
CONV0_WRW_SHAPES = CONV0_SHAPES[:5]
GAP_SHAPES = [(5, 1, 8, 8), (2, 50, 64, 96), (3, 9, 520, 544), (4, 49, 1024, 1024)]                               # B, HW, C, ld
DP_SHAPES = [(98, 256, 128), (300, 96, 128)]                                                                      # Sq, C, Co
