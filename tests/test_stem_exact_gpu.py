"""Every kernel entry point AROUND the dense layers -- conv0, the stem's and the transitions' BatchNorm passes, the pools, norm5 +
global pool, the transition's convolution and data gradient -- called through ctypes and held element by element to the
restatement in tests/stem_reference.py: identical bits where the code leaves the compiler no freedom, a derived per-element
bound elsewhere.  As in test_dense_exact_gpu.py every buffer sits between guard words and every region a kernel may not use
(the columns of a wide buffer outside its channel slice, outputs and workspace before the call) holds a NaN sentinel; after the
call guards, inputs and untouched columns must be bit-unchanged and every output finite.  Every case has one negative gamma,
one dead channel, one channel with |mean|/std ~ 1e3 and one whose fmaf is exactly zero on a quarter of its pixels; each case
prints the worst share of a bound it uses.  Left out: the grid-stride second trip of the pool kernels (more than 4.19 M
chunks, reached by no shape of the workload), csrc/pool_generic.hip, the running-statistics and image-conversion kernels."""
import numpy as np
import pytest
import torch

import dense_reference as dr
import stem_reference as sr
from exact_harness import EPS, Mat, vec, out_vec, _st, _check, _within, _bits_equal, _bias, _stats

pytestmark = pytest.mark.gpu

KIND = {0: "f32", 1: "bf16"}


@pytest.fixture(scope="module")
def L():
    from mclstexp_amd import _lib
    return _lib.lib()           # must load: no fallback


def _bn_vecs(prm):
    return [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]


def _ptrs(bufs):
    return [b.ptr() for b in bufs]


def _c0(ld, C, V):
    """Column of the slice inside a buffer ld wide: 8 where there is room, 16-byte aligned."""
    return min(8, (ld - C) // V * V)


def _prior(shape, seed, dtype=0, scale=0.5):
    """What an accumulating output holds before the call.  scale: that of what is added to it, so that the bound (the rounding
    of the sum) stays as sharp as in the overwriting case."""
    return sr.stem_gradients(shape, seed, dtype, scale=scale, offset=0.0)


def _all_unchanged(bufs, what="input"):
    for b in bufs:
        b.unchanged(what)


# ------------------------------------------------------------------------------------------------------------ BatchNorm passes
_bn_case = sr.bn_case


@pytest.mark.parametrize("dtype,S,C,ld", sr.BN_SHAPES)
def test_bn_stats(L, dtype, S, C, ld):
    """mcl_bn_stats with copy_out: the statistics within the bounds of the shifted-sum scheme at plan()'s chain lengths (var = 0
    at S = 1, the second channel tile, the capped plan), the copy bit for bit beside NaN columns."""
    V = 8 if dtype == 1 else 4
    prm, x, _ = _bn_case(dtype, S, C)
    c0, ldo = _c0(ld, C, V), C + 2 * V
    xb = Mat(S, ld, KIND[dtype]).set(c0, x).freeze()
    cb = Mat(S, ldo, KIND[dtype]).freeze()
    ws = Mat(1, int(L.mcl_bn_workspace_floats(S, C, dtype)), "f32").freeze()
    so = [out_vec(C).freeze() for _ in range(3)]
    _check(L.mcl_bn_stats(xb.ptr(c0), ld, S, C, dtype, cb.ptr(V), ldo, ws.ptr(), EPS, *_ptrs(so), _st()), "mcl_bn_stats")
    torch.cuda.synchronize()
    xb.unchanged("x")
    cb.unchanged("copy_out", V, C)
    ws.unchanged("workspace", 0, ws.ld)
    rep = []
    _bits_equal("copy_out", cb.bits(V, C), xb.bits(c0, C), rep)
    refs, bounds = sr.bn_stats(x, EPS, dtype)
    _stats("", [s.get()[0] for s in so], refs, bounds, rep)
    if S == 1:
        assert (so[1].get()[0] == 0.0).all(), "var of a single row is not zero"
    print(f"bn_stats dtype={dtype} S={S} C={C} ld={ld}: " + ", ".join(rep))


@pytest.mark.parametrize("dtype,S,C,ld", sr.BN_SHAPES)
def test_bn_act_fwd(L, dtype, S, C, ld):
    """mcl_bn_act_fwd, relu 0 and 1, both dtypes: identical bits."""
    V = 8 if dtype == 1 else 4
    prm, x, _ = _bn_case(dtype, S, C)
    c0 = _c0(ld, C, V)
    xb = Mat(S, ld, KIND[dtype]).set(c0, x).freeze()
    pv = _bn_vecs(prm)
    rep = []
    for relu in (0, 1):
        yb = Mat(S, ld, KIND[dtype]).freeze()
        _check(L.mcl_bn_act_fwd(xb.ptr(c0), ld, S, C, dtype, *_ptrs(pv), relu, yb.ptr(c0), ld, _st()), "mcl_bn_act_fwd")
        torch.cuda.synchronize()
        _all_unchanged([xb] + pv)
        yb.unchanged("y", c0, C)
        _bits_equal(f"y(relu={relu})", yb.bits(c0, C), sr.store_bits(sr.bn_act_fwd(x, prm, relu), dtype), rep)
    print(f"bn_act_fwd dtype={dtype} S={S} C={C} ld={ld}: " + ", ".join(rep))


def _run_bn_bwd(L, dtype, S, C, ld, relu, acc, accp, in_place=False, case=None, dyb=None, c0=None):
    """One mcl_bn_act_bwd call checked against the restatement.  dyb given: the gradient already lies on the device (the stem
    backward: what mcl_maxpool3s2_nhwc_bf16_bwd_ld left), dx then goes in place."""
    V = 8 if dtype == 1 else 4
    prm, x, dy = case or _bn_case(dtype, S, C)
    c0 = _c0(ld, C, V) if c0 is None else c0
    xb = Mat(S, ld, KIND[dtype]).set(c0, x).freeze()
    if dyb is None:
        dyb = Mat(S, ld, KIND[dtype]).set(c0, dy)
    dyb.freeze()
    prior_dx = _prior((S, C), 15 + S, dtype, scale=1e-2) if acc else None       # the gradient's own scale
    if in_place:
        dxb = dyb
    else:
        dxb = Mat(S, ld, KIND[dtype])
        if acc:
            dxb.set(c0, prior_dx)
        dxb.freeze()
    ws = Mat(1, int(L.mcl_bn_workspace_floats(S, C, dtype)), "f32").freeze()
    pv = _bn_vecs(prm)
    prior = [dr.f32(_prior((C,), 16 + i)) for i in range(2)] if accp else [None, None]
    dgb, dbb = [(vec(p) if accp else out_vec(C)).freeze() for p in prior]
    _check(L.mcl_bn_act_bwd(dyb.ptr(c0), ld, xb.ptr(c0), ld, S, C, dtype, *_ptrs(pv), relu, ws.ptr(), dgb.ptr(), dbb.ptr(), accp,
                            dxb.ptr(c0), ld, acc, _st()), "mcl_bn_act_bwd")
    torch.cuda.synchronize()
    _all_unchanged([xb] + pv)
    if not in_place:
        dyb.unchanged("dy")
    dxb.unchanged("dx", c0, C)
    ws.unchanged("workspace", 0, ws.ld)
    dgb.unchanged("dgamma", 0, C)
    dbb.unchanged("dbeta", 0, C)
    gm = np.where(sr.relu_mask(x, prm), dy, 0.0) if relu else dy
    s = sr.bn_bwd_sums(gm, x, prm, sr.chain(S, C, dtype), prior=prior)
    rep = []
    _within("dgamma", dgb.get()[0], *s["dgamma"], rep)
    _within("dbeta", dbb.get()[0], *s["dbeta"], rep)
    coef = ws.get()[0][-2 * C:].reshape(C, 2)              # the kernel's own: the last 2C floats of the workspace
    _within("coef", coef, *s["coef"], rep)
    ref, bound = sr.bn_bwd_dx(gm, x, prm, coef, dtype, prior=prior_dx)
    dx = dxb.get(c0, C)
    _within("dx", dx, ref, bound, rep)
    if dtype == 1:                                         # one bf16 rounding of an fp32 value, accumulating or not
        _bias("dx", dx, ref, rep)
    return rep


@pytest.mark.parametrize("accp", [0, 1])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dtype,S,C,ld", sr.BN_SHAPES[:4])
def test_bn_act_bwd(L, dtype, S, C, ld, relu, acc, accp):
    """mcl_bn_act_bwd: dgamma, dbeta, coef within the bounds of the merge scheme; dx restated from the kernel's own coef."""
    rep = _run_bn_bwd(L, dtype, S, C, ld, relu, acc, accp)
    print(f"bn_act_bwd dtype={dtype} S={S} C={C} ld={ld} relu={relu} accumulate={acc} accumulate_params={accp}: " + ", ".join(rep))


def test_bn_act_bwd_capped_plan(L):
    """The capped branch of plan() (1050 row blocks -> 934 of 9 rows): one case, 8.4 M elements."""
    dtype, S, C, ld = sr.BN_SHAPES[4]
    rep = _run_bn_bwd(L, dtype, S, C, ld, 1, 1, 1)
    print(f"bn_act_bwd dtype={dtype} S={S} C={C} ld={ld} relu=1 accumulate=1 accumulate_params=1: " + ", ".join(rep))


@pytest.mark.parametrize("dtype,S,C,ld", sr.BN_SHAPES[:4])
def test_bn_act_bwd_in_place(L, dtype, S, C, ld):
    """dx == dy, as StemTailFn.backward runs it."""
    rep = _run_bn_bwd(L, dtype, S, C, ld, 1, 0, 0, in_place=True)
    print(f"bn_act_bwd in place dtype={dtype} S={S} C={C} ld={ld}: " + ", ".join(rep))


# ------------------------------------------------------------------------------------------------------------ transitions: BatchNorm + average pool
@pytest.mark.parametrize("accp", [0, 1])
@pytest.mark.parametrize("N,H,W,C", sr.AVGPOOL_BN_SHAPES)
def test_bn_act_avgpool(L, N, H, W, C, accp):
    """mcl_bn_act_avgpool_fwd (bits) and mcl_bn_act_avgpool_bwd (bounds; dx from the kernel's own coef), every leading dimension
    wider than C; odd maps pool with floor and their unpaired last row / column receives no gradient through the pool."""
    prm = sr.stem_params(C, 21 + C)
    x = sr.stem_activations((N, H, W, C), prm, 22 + H)
    S, SP = N * H * W, N * (H // 2) * (W // 2)
    dp = sr.stem_gradients((N, H // 2, W // 2, C), 23 + W)
    ldx, ldy, lddp, lddx = C + 16, C + 8, C + 24, C + 8
    xb = Mat(S, ldx).set(8, x.reshape(S, C)).freeze()
    yb = Mat(SP, ldy).freeze()
    pv = _bn_vecs(prm)
    _check(L.mcl_bn_act_avgpool_fwd(xb.ptr(8), ldx, N, H, W, C, *_ptrs(pv), yb.ptr(0), ldy, _st()), "mcl_bn_act_avgpool_fwd")
    torch.cuda.synchronize()
    _all_unchanged([xb] + pv)
    yb.unchanged("p", 0, C)
    rep = []
    _bits_equal("p", yb.bits(0, C), dr.bf16_bits(sr.bn_act_avgpool_fwd(x, prm)).reshape(SP, C), rep)
    dpb = Mat(SP, lddp).set(16, dp.reshape(SP, C)).freeze()
    dxb = Mat(S, lddx).freeze()
    ws = Mat(1, int(L.mcl_bn_workspace_floats(S, C, 1)), "f32").freeze()
    prior = [dr.f32(_prior((C,), 26 + i)) for i in range(2)] if accp else [None, None]
    dgb, dbb = [(vec(p) if accp else out_vec(C)).freeze() for p in prior]
    _check(L.mcl_bn_act_avgpool_bwd(dpb.ptr(16), lddp, xb.ptr(8), ldx, N, H, W, C, *_ptrs(pv), ws.ptr(), dgb.ptr(), dbb.ptr(), accp,
                                    dxb.ptr(8), lddx, _st()), "mcl_bn_act_avgpool_bwd")
    torch.cuda.synchronize()
    _all_unchanged([xb, dpb] + pv)
    dxb.unchanged("dx", 8, C)
    ws.unchanged("workspace", 0, ws.ld)
    dgb.unchanged("dgamma", 0, C)
    dbb.unchanged("dbeta", 0, C)
    gi = sr.pool_gradient(dp, x, prm, H, W)
    x2 = x.reshape(S, C)
    s = sr.bn_bwd_sums(gi, x2, prm, sr.chain(S, C, 1), prior=prior)
    _within("dgamma", dgb.get()[0], *s["dgamma"], rep)
    _within("dbeta", dbb.get()[0], *s["dbeta"], rep)
    coef = ws.get()[0][-2 * C:].reshape(C, 2)
    _within("coef", coef, *s["coef"], rep)
    ref, bound = sr.bn_bwd_dx(gi, x2, prm, coef, 1)
    dx = dxb.get(8, C)
    _within("dx", dx, ref, bound, rep)
    _bias("dx", dx, ref, rep)
    print(f"bn_act_avgpool N={N} H={H} W={W} C={C} accumulate_params={accp}: " + ", ".join(rep))


@pytest.mark.parametrize("N,H,W,C", sr.AVGPOOL_SHAPES)
def test_avgpool2(L, N, H, W, C):
    """mcl_avgpool2_nhwc_bf16, both directions: identical bits."""
    prm = sr.stem_params(C, 27 + C)
    x = sr.stem_activations((N, H, W, C), prm, 28 + H)
    S, SP = N * H * W, N * (H // 2) * (W // 2)
    xb, yb = Mat(S, C).set(0, x.reshape(S, C)).freeze(), Mat(SP, C).freeze()
    _check(L.mcl_avgpool2_nhwc_bf16(xb.ptr(), yb.ptr(), N, H, W, C, 0, _st()), "mcl_avgpool2_nhwc_bf16")
    dy = sr.stem_gradients((N, H // 2, W // 2, C), 29 + W)
    dyb, dxb = Mat(SP, C).set(0, dy.reshape(SP, C)).freeze(), Mat(S, C).freeze()
    _check(L.mcl_avgpool2_nhwc_bf16(dyb.ptr(), dxb.ptr(), N, H, W, C, 1, _st()), "mcl_avgpool2_nhwc_bf16 (backward)")
    torch.cuda.synchronize()
    _all_unchanged([xb, dyb])
    yb.unchanged("y", 0, C)
    dxb.unchanged("dx", 0, C)
    rep = []
    _bits_equal("y", yb.bits(), dr.bf16_bits(sr.avgpool_fwd(x)).reshape(SP, C), rep)
    _bits_equal("dx", dxb.bits(), dr.bf16_bits(sr.avgpool_bwd(dy, H, W)).reshape(S, C), rep)
    print(f"avgpool2 N={N} H={H} W={W} C={C}: " + ", ".join(rep))


# ------------------------------------------------------------------------------------------------------------ stem: max pool
@pytest.mark.parametrize("N,H,W,C,lddy", sr.MAXPOOL_SHAPES)
def test_maxpool_and_stem_backward(L, N, H, W, C, lddy):
    """mcl_maxpool3s2_nhwc_bf16_fwd and mcl_bn_act_maxpool_fwd (y and idx bit for bit: the first maximum wins, windows full of
    ReLU zeros and zeros of both signs tie), then the stem backward as StemTailFn drives it: mcl_maxpool3s2_nhwc_bf16_bwd_ld
    from a channel slice of a wider buffer into g (bits; the generic kernel on odd maps, the quad kernel on even ones), then
    mcl_bn_act_bwd in place on g, restated from the g the first launch left."""
    prm = sr.stem_params(C, 31 + C)
    x = sr.stem_activations((N, H, W, C), prm, 32 + H * W)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    S, SP = N * H * W, N * OH * OW
    rep = []
    # the plain pool, on data with zeros of both signs in channel 2
    xz = x.copy()
    xz[..., 2] = np.where(np.random.default_rng(1).random(x.shape[:-1]) < 0.5, -0.0, 0.0)
    xb, yb, ib = Mat(S, C).set(0, xz.reshape(S, C)).freeze(), Mat(SP, C).freeze(), Mat(SP, C, "u8").freeze()
    _check(L.mcl_maxpool3s2_nhwc_bf16_fwd(xb.ptr(), yb.ptr(), ib.ptr(), N, H, W, C, _st()), "mcl_maxpool3s2_nhwc_bf16_fwd")
    torch.cuda.synchronize()
    xb.unchanged("x")
    yb.unchanged("y", 0, C)
    ib.unchanged("idx", 0, C)
    m, idx = sr.maxpool_fwd(xz)
    _bits_equal("maxpool y", yb.bits(), dr.bf16_bits(m).reshape(SP, C), rep)
    _bits_equal("maxpool idx", ib.bits(), idx.reshape(SP, C), rep)
    # norm0 -> relu0 -> pool0
    xb, yb, ib = Mat(S, C).set(0, x.reshape(S, C)).freeze(), Mat(SP, C).freeze(), Mat(SP, C, "u8").freeze()
    pv = _bn_vecs(prm)
    _check(L.mcl_bn_act_maxpool_fwd(xb.ptr(), N, H, W, C, *_ptrs(pv), yb.ptr(), ib.ptr(), _st()), "mcl_bn_act_maxpool_fwd")
    torch.cuda.synchronize()
    _all_unchanged([xb] + pv)
    yb.unchanged("y", 0, C)
    ib.unchanged("idx", 0, C)
    m, idx = sr.bn_act_maxpool_fwd(x, prm)
    _bits_equal("bn y", yb.bits(), dr.bf16_bits(m).reshape(SP, C), rep)
    _bits_equal("bn idx", ib.bits(), idx.reshape(SP, C), rep)
    assert (m[..., 2] == 0.0).all(), "the dead channel is not dead"            # every window of it ties at zero
    # the backward: dy is a channel slice of a wider gradient buffer
    c0 = (lddy - C) // 8 * 8
    dy = sr.stem_gradients((N, OH, OW, C), 33 + W)
    dyb = Mat(SP, lddy).set(c0, dy.reshape(SP, C)).freeze()
    gb = Mat(S, C)
    gb.freeze()
    ib.freeze()
    _check(L.mcl_maxpool3s2_nhwc_bf16_bwd_ld(ib.ptr(), dyb.ptr(c0), lddy, gb.ptr(), N, H, W, C, _st()),
           "mcl_maxpool3s2_nhwc_bf16_bwd_ld")
    torch.cuda.synchronize()
    _all_unchanged([dyb, ib])
    gb.unchanged("g", 0, C)
    _bits_equal("g", gb.bits(), dr.bf16_bits(sr.maxpool_bwd(idx, dy, H, W)).reshape(S, C), rep)
    g = gb.get()
    rep += _run_bn_bwd(L, 1, S, C, C, 1, 0, 0, in_place=True, case=(prm, x.reshape(S, C), g), dyb=gb, c0=0)
    print(f"maxpool + stem backward N={N} H={H} W={W} C={C} lddy={lddy}: " + ", ".join(rep))


# ------------------------------------------------------------------------------------------------------------ conv0
@pytest.mark.parametrize("N,H,W", sr.CONV0_SHAPES)
def test_conv0_fwd(L, N, H, W):
    """mcl_conv0_fwd with and without statistics, twice (bit-reproducible): y within the 147-term bound, the border pixels on
    their own, the statistics of the stored y within the bounds of the tile scheme.  (155, 20, 8) has 775 tiles > 768: workgroups
    0..6 take a second tile at another row position of another image, over a slab that held other rows, rows outside the image
    among them.  tile_stats_finalize_kernel sets the last tile apart, so its threads take a second trip from 2050 tiles on:
    (2049, 4, 8) is the last shape of one trip each, (2060, 4, 8) gives threads 0 .. 10 a second one (stem_reference.py)."""
    x, Wt = sr.conv0_case(N, H, W)
    P = N * (H // 2) * (W // 2)
    xb, wb = Mat(1, N * H * W * 3).set(0, x.reshape(1, -1)).freeze(), Mat(64, 147).set(0, Wt.reshape(64, 147)).freeze()
    ref, bound = sr.conv0_fwd(x, Wt)
    bp = sr.conv0_border(N, H, W)
    rep, ys, sts = [], [], []
    for stats in (1, 1, 0):
        yb = Mat(P, 64).freeze()
        ws = Mat(1, int(L.mcl_conv0_workspace_floats(N, H, W)), "f32").freeze()
        so = [out_vec(64).freeze() for _ in range(3)]
        sp = _ptrs(so) if stats else [None, None, None]
        _check(L.mcl_conv0_fwd(xb.ptr(), N, H, W, wb.ptr(), yb.ptr(), ws.ptr(), EPS, *sp, _st()), "mcl_conv0_fwd")
        torch.cuda.synchronize()
        _all_unchanged([xb, wb])
        yb.unchanged("y", 0, 64)
        ws.unchanged("workspace", 0, ws.ld)
        for s in so:
            s.unchanged("statistics", 0, 64 if stats else 0)
        ys.append(yb.bits())
        if stats:
            sts.append(np.stack([s.bits() for s in so]))
    y = dr.bits_to_f64(ys[0])
    _within("y", y, ref, bound, rep)
    _bias("y", y, ref, rep)
    wbp, at = dr.worst(y[bp], ref[bp], bound[bp])
    assert wbp <= 1.0, f"border pixel {bp[at[0]]}, channel {at[1]}: {wbp:.3f} of its bound"
    refs, bounds = sr.stats_tiles_unshifted(y, EPS, W)
    _stats("y", [s.view(np.float32).astype(np.float64)[0] for s in sts[0]], refs, bounds, rep)
    _bits_equal("second run y", ys[1], ys[0], rep)
    _bits_equal("second run statistics", sts[1], sts[0], rep)
    _bits_equal("y without statistics", ys[2], ys[0], rep)
    print(f"conv0_fwd N={N} H={H} W={W}: " + ", ".join(rep) + f", border pixels {bp.size}: worst {wbp:.3f}")


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("N,H,W", sr.CONV0_WRW_SHAPES)
def test_conv0_wrw(L, N, H, W, acc):
    """mcl_conv0_wrw, overwrite and accumulate, twice (bit-reproducible)."""
    x, _ = sr.conv0_case(N, H, W)
    P = N * (H // 2) * (W // 2)
    dy = sr.stem_gradients((P, 64), 41 + W)
    xb, dyb = Mat(1, N * H * W * 3).set(0, x.reshape(1, -1)).freeze(), Mat(P, 64).set(0, dy).freeze()
    prior = dr.f32(_prior((64, 147), 42, scale=1e-2 * np.sqrt(P))) if acc else None      # the scale of a sum over P pixels
    outs, rep = [], []
    for _ in range(2):
        ws = Mat(1, int(L.mcl_conv0_wrw_workspace_floats(N, H, W)), "f32").freeze()
        dWb = (Mat(64, 147, "f32").set(0, prior) if acc else Mat(64, 147, "f32")).freeze()
        _check(L.mcl_conv0_wrw(xb.ptr(), N, H, W, dyb.ptr(), ws.ptr(), dWb.ptr(), acc, _st()), "mcl_conv0_wrw")
        torch.cuda.synchronize()
        _all_unchanged([xb, dyb])
        ws.unchanged("workspace", 0, ws.ld)
        dWb.unchanged("dW", 0, 147)
        outs.append(dWb.bits())
    _within("dW", outs[0].view(np.float32).astype(np.float64), *sr.conv0_wrw(x, dy, N, H, W, prior=prior), rep)
    _bits_equal("second run", outs[1], outs[0], rep)
    print(f"conv0_wrw N={N} H={H} W={W} accumulate={acc}: " + ", ".join(rep))


# ------------------------------------------------------------------------------------------------------------ norm5 + global pool
@pytest.mark.parametrize("accp", [0, 1])
@pytest.mark.parametrize("B,HW,C,ld", sr.GAP_SHAPES)
def test_bn_gap(L, B, HW, C, ld, accp):
    """mcl_bn_gap_fwd with and without xmean, mcl_bn_gap_bwd restated from the kernel's own xmean and coef."""
    prm = sr.stem_params(C, 51 + C)
    x = sr.stem_activations((B, HW, C), prm, 52 + HW)
    g = dr.f32(np.random.default_rng(53).normal(1e-3, 1e-2, (B, C)))
    S = B * HW
    xb = Mat(S, ld).set(0, x.reshape(S, C)).freeze()
    pv = _bn_vecs(prm)
    rep = []
    f = sr.bn_gap_fwd(x, prm)
    outs = []
    for with_xm in (1, 0):
        ob, mb = Mat(B, C, "f32").freeze(), Mat(B, C, "f32").freeze()
        _check(L.mcl_bn_gap_fwd(xb.ptr(), ld, B, HW, C, *_ptrs(pv), ob.ptr(), mb.ptr() if with_xm else None, _st()), "mcl_bn_gap_fwd")
        torch.cuda.synchronize()
        _all_unchanged([xb] + pv)
        ob.unchanged("out", 0, C)
        mb.unchanged("xmean", 0, C if with_xm else 0)
        outs.append(ob.bits())
        if with_xm:
            _within("out", ob.get(), *f["out"], rep)
            xm = mb.get()
            _within("xmean", xm, *f["xmean"], rep)
            xmb = mb
    _bits_equal("out without xmean", outs[1], outs[0], rep)
    gb = Mat(B, C, "f32").set(0, g).freeze()
    xmb.freeze()
    coefb = out_vec(2 * C).freeze()
    prior = [dr.f32(_prior((C,), 56 + i)) for i in range(2)] if accp else [None, None]
    dgb, dbb = [(vec(p) if accp else out_vec(C)).freeze() for p in prior]
    dxb = Mat(S, ld).freeze()
    _check(L.mcl_bn_gap_bwd(gb.ptr(), xmb.ptr(), xb.ptr(), ld, B, HW, C, pv[0].ptr(), pv[2].ptr(), pv[3].ptr(), coefb.ptr(), dgb.ptr(),
                            dbb.ptr(), accp, dxb.ptr(), ld, _st()), "mcl_bn_gap_bwd")
    torch.cuda.synchronize()
    _all_unchanged([xb, gb, xmb] + pv)
    dxb.unchanged("dx", 0, C)
    for b, n in ((coefb, 2 * C), (dgb, C), (dbb, C)):
        b.unchanged("output", 0, n)
    s = sr.bn_gap_bwd_sums(g, xm, prm, HW, prior=prior)
    _within("dgamma", dgb.get()[0], *s["dgamma"], rep)
    _within("dbeta", dbb.get()[0], *s["dbeta"], rep)
    coef = coefb.get()[0].reshape(C, 2)
    _within("coef", coef, *s["coef"], rep)
    ref, bound = sr.bn_gap_bwd_dx(g, x, prm, coef)
    dx = dxb.get(0, C).reshape(B, HW, C)
    _within("dx", dx, ref, bound, rep)
    _bias("dx", dx, ref, rep)
    print(f"bn_gap B={B} HW={HW} C={C} ld={ld} accumulate_params={accp}: " + ", ".join(rep))


# ------------------------------------------------------------------------------------------------------------ transition convolution
def test_transition_conv_fwd(L):
    """The transition's convolution as pooled_conv1x1_fwd issues it: mcl_dense_conv1x1_fwd with the identity prologue, Co = 256 as
    two launches -- weights at row offset 128, output at column offset 128 of a buffer 320 wide, statistics at + 128."""
    S, C, Co, ldz = 300, 96, 256, 320
    rng = np.random.default_rng(61)
    p = dr.bf16(np.abs(rng.normal(0.3, 0.5, (S, C))))
    Wt = dr.weights((Co, C), C, 62, positive_row=5)
    ident = dict(gamma=np.ones(C), beta=np.zeros(C), mean=np.zeros(C), rstd=np.ones(C))
    pb, wb = Mat(S, C).set(0, p).freeze(), Mat(Co, C).set(0, Wt).freeze()
    pv = _bn_vecs(ident)
    zb = Mat(S, ldz).freeze()
    ws = Mat(1, int(L.mcl_dense_conv1x1_workspace_floats(S)), "f32").freeze()
    so = [out_vec(Co).freeze() for _ in range(3)]
    for n0 in (0, 128):
        _check(L.mcl_dense_conv1x1_fwd(pb.ptr(), C, S, C, *_ptrs(pv), wb.ptr(n0 * C), zb.ptr(n0), ldz, ws.ptr(), EPS,
                                       *[s.ptr(n0) for s in so], _st()), "mcl_dense_conv1x1_fwd")
    torch.cuda.synchronize()
    _all_unchanged([pb, wb] + pv)
    zb.unchanged("z", 0, Co)
    ws.unchanged("workspace", 0, ws.ld)
    ref, bound, pr = dr.conv1x1_fwd(p, *dr.bn(ident), Wt)
    assert np.array_equal(pr.a, p) and pr.amb_share == 0.0
    z = zb.get(0, Co)
    rep = []
    _within("z", z, ref, bound, rep)
    _bias("z", z, ref, rep)
    refs, bounds = dr.stats_tiles(z, EPS, 64)
    _stats("z", [s.get()[0] for s in so], refs, bounds, rep)
    print(f"transition conv1x1 forward S={S} C={C} Co={Co}: " + ", ".join(rep))


@pytest.mark.parametrize("Sq,C,Co", sr.DP_SHAPES)
def test_transition_dp(L, Sq, C, Co):
    """dp = dy . W through mcl_gemm_bf16 exactly as TransitionFn.backward calls it, dy the first Co columns of a wider buffer."""
    dy, Wt = sr.stem_gradients((Sq, Co), 61), dr.weights((Co, C), C, 62)
    lddy = Co + 32
    dyb, wb, dpb = Mat(Sq, lddy).set(0, dy).freeze(), Mat(Co, C).set(0, Wt).freeze(), Mat(Sq, C).freeze()
    _check(L.mcl_gemm_bf16(dyb.ptr(), lddy, 0, wb.ptr(), C, 0, dpb.ptr(), C, 0, Sq, C, Co, 1, 1, 0, 0, 0, 1.0, 2, None, None, 0, 0,
                           None, 0, None, 0, 1, None, 0, _st()), "mcl_gemm_bf16")
    torch.cuda.synchronize()
    _all_unchanged([dyb, wb])
    dpb.unchanged("dp", 0, C)
    ref, bound = sr.transition_dp(dy, Wt)
    dp = dpb.get()
    rep = []
    _within("dp", dp, ref, bound, rep)
    _bias("dp", dp, ref, rep)
    print(f"transition dp Sq={Sq} C={C} Co={Co}: " + ", ".join(rep))
