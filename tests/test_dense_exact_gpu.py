"""Every dense-layer kernel entry point, called through ctypes, element by element against the float64 restatement in
tests/dense_reference.py.  Every buffer sits between guard words; every region a kernel may not use -- the columns of a wide
buffer outside its channel slice, the outputs and the workspace before the call -- holds a NaN sentinel.  After the call the
guards and the untouched regions must be bit-unchanged, every output finite, and every element within its own derived bound
(a non-finite value counts as infinitely far).  The tensors that are ONE rounding of an fp32 value (z, y, g2, dz) also pass a
bias check: truncation instead of round-to-nearest-even gives -1 there.  The bounds are derived in dense_reference.py, not
tuned; each case prints how much of them it uses."""
import numpy as np
import pytest
import torch

import dense_reference as dr
from exact_harness import DEV, EPS, Mat, vec, out_vec, _st, _check, _within, _bias, _bias_ok, _stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from mclstexp_amd import _lib
    return _lib.lib()           # must load: no fallback


# ------------------------------------------------------------------------------------------------------------ conv1x1 forward
@pytest.mark.parametrize("S,K,ldx", dr.CONV1X1_SHAPES)
def test_conv1x1_fwd(L, S, K, ldx):
    """mcl_dense_conv1x1_fwd: the four-wave form (S < 32768) and the <2, 64, 0> form; K tails (K % 64 != 0) beside NaN columns;
    one negative gamma, one dead channel; output channel 5 has all-positive weights (|mean|/std ~ sqrt(K) for the shifted sums)."""
    prm, x, W1 = dr.conv1x1_case(S, K)
    ldz = 160
    xb = Mat(S, ldx).set(0, x).freeze()
    wb = Mat(128, K).set(0, W1).freeze()
    zb = Mat(S, ldz).freeze()
    ws = Mat(1, int(L.mcl_dense_conv1x1_workspace_floats(S)), "f32").freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    so = [out_vec(128).freeze() for _ in range(3)]
    _check(L.mcl_dense_conv1x1_fwd(xb.ptr(), ldx, S, K, *[p.ptr() for p in pv], wb.ptr(), zb.ptr(), ldz, ws.ptr(), EPS,
                                   *[s.ptr() for s in so], _st()), "mcl_dense_conv1x1_fwd")
    torch.cuda.synchronize()
    for b, nm in [(xb, "x"), (wb, "W1")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    zb.unchanged("z", 0, 128)
    ws.unchanged("workspace", 0, ws.ld)
    for s in so:
        s.unchanged("statistics", 0, 128)
    ref, bound, p = dr.conv1x1_fwd(x, *dr.bn(prm), W1)
    assert p.amb_share <= dr.AMB_CAP
    z = zb.get(0, 128)
    rep = []
    _within("z", z, ref, bound, rep)
    _bias("z", z, ref, rep)
    refs, bounds = dr.stats_tiles(z, EPS, 128 if S >= 32768 else 64)
    _stats("z", [s.get()[0] for s in so], refs, bounds, rep)
    print(f"conv1x1_fwd S={S} K={K} ldx={ldx}: " + ", ".join(rep) + f", ambiguous share {p.amb_share:.2e}")


# ------------------------------------------------------------------------------------------------------------ conv3x3 forward
def _slice0(ld):
    return (ld - 32) // 2 // 8 * 8


_tail_inputs = dr.tail_case


@pytest.mark.parametrize("B,H,W,ldo", dr.CONV3X3_FLAT + dr.CONV3X3_ROWS)
def test_conv3x3_fwd(L, B, H, W, ldo):
    """mcl_dense_conv3x3_fwd, flat-tile form (W < 17: tiles span images, ragged last tile) and row-walking form (17 <= W <= 150),
    written into a 32-channel slice of a wider buffer whose other columns hold NaN; the border pixels stated on their own."""
    S = B * H * W
    prm, z, W2, _ = _tail_inputs(B, H, W)
    c0 = _slice0(ldo)
    zb = Mat(S, 128).set(0, z).freeze()
    wb = Mat(32, 1152).set(0, W2.reshape(32, -1)).freeze()
    ob = Mat(S, ldo).freeze()
    ws = Mat(1, int(L.mcl_dense_conv3x3_workspace_floats(S)), "f32").freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    so = [out_vec(32).freeze() for _ in range(3)]
    _check(L.mcl_dense_conv3x3_fwd(zb.ptr(), S, H, W, *[p.ptr() for p in pv], wb.ptr(), ob.ptr(c0), ldo, ws.ptr(), EPS,
                                   *[s.ptr() for s in so], _st()), "mcl_dense_conv3x3_fwd")
    torch.cuda.synchronize()
    for b, nm in [(zb, "z"), (wb, "W2")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    ob.unchanged("out", c0, 32)
    ws.unchanged("workspace", 0, ws.ld)
    ref, bound, p = dr.conv3x3_fwd(z, B, H, W, *dr.bn(prm), W2)
    assert p.amb_share <= dr.AMB_CAP
    y = ob.get(c0, 32)
    rep = []
    _within("y", y, ref, bound, rep)
    _bias("y", y, ref, rep)
    bp = dr.border_pixels(B, H, W)
    wb_, at = dr.worst(y[bp], ref[bp], bound[bp])
    assert wb_ <= 1.0, f"border pixel {bp[at[0]]}, channel {at[1]}: {wb_:.3f} of its bound"
    if dr.rows_applicable(H, W):
        refs, bounds = dr.stats_sums(y, EPS, dr.fwd_rows_unit_pixels(B, H, W))
    else:
        refs, bounds = dr.stats_tiles(y, EPS, 128)
    _stats("y", [s.get()[0] for s in so], refs, bounds, rep)
    print(f"conv3x3_fwd B={B} H={H} W={W} ldo={ldo}: " + ", ".join(rep) + f", border pixels {bp.size}: worst {wb_:.3f}, "
          f"ambiguous share {p.amb_share:.2e}")


# ------------------------------------------------------------------------------------------------------------ tail backward
TAIL_LD = {32: 32, 64: 64, 96: 1024, 1024: 1024}     # lddy in {32, 64, 1024} over the same (B, H, W) lists


def _run_tail(L, B, H, W, lddy, acc, fix):
    S = B * H * W
    prm, z, W2, dy = _tail_inputs(B, H, W)
    c0 = _slice0(lddy)
    rep = []
    db_ = Mat(S, lddy).set(c0, dy).freeze()
    zb = Mat(S, 128).set(0, z).freeze()
    wb = Mat(32, 1152).set(0, W2.reshape(32, -1)).freeze()
    g2b, dzb = Mat(S, 128).freeze(), Mat(S, 128).freeze()
    ws = Mat(1, int(L.mcl_dense_conv3x3_bwd_workspace_floats(S)), "f32").freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    rng = np.random.default_rng(S + acc)
    prior = [dr.f32(rng.normal(0, 0.5, 128)) for _ in range(2)] if acc else [None, None]
    dgb, dbb = [(vec(p) if acc else out_vec(128)).freeze() for p in prior]
    if fix:
        fp = dr.layer_params(32, 1300 + S)
        xf = dr.activations(S, 32, fp, 1400 + S)
        fk = dr.f32(rng.normal(0, 2e-3, (32, 2)))
        ldxf = lddy
        xfb = Mat(S, ldxf).set(c0, xf).freeze()
        fv = [vec(fp["mean"]).freeze(), vec(fp["rstd"]).freeze(), vec(fk.reshape(-1)).freeze()]
        dycb = Mat(S, 32).freeze()
        _check(L.mcl_dense_conv3x3_bwd_fix(db_.ptr(c0), lddy, S, H, W, wb.ptr(), zb.ptr(), *[p.ptr() for p in pv], ws.ptr(),
                                           dgb.ptr(), dbb.ptr(), acc, g2b.ptr(), dzb.ptr(), xfb.ptr(c0), ldxf,
                                           *[v.ptr() for v in fv], dycb.ptr(), _st()), "mcl_dense_conv3x3_bwd_fix")
    else:
        _check(L.mcl_dense_conv3x3_bwd(db_.ptr(c0), lddy, S, H, W, wb.ptr(), zb.ptr(), *[p.ptr() for p in pv], ws.ptr(),
                                       dgb.ptr(), dbb.ptr(), acc, g2b.ptr(), dzb.ptr(), _st()), "mcl_dense_conv3x3_bwd")
    torch.cuda.synchronize()
    for b, nm in [(db_, "dy"), (zb, "z"), (wb, "W2")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    for b, nm in [(g2b, "g2"), (dzb, "dz")]:
        b.unchanged(nm, 0, 128)
    ws.unchanged("workspace", 0, ws.ld)
    dgb.unchanged("dgamma2", 0, 128)
    dbb.unchanged("dbeta2", 0, 128)
    if fix:
        for b in [xfb] + fv:
            b.unchanged("fix operand")
        dycb.unchanged("dyc", 0, 32)
        cref, cbound = dr.bn1_fix(dy, xf, 0, 32, fp["mean"], fp["rstd"], fk)
        dy = dycb.get()
        _within("dyc", dy, cref, cbound, rep)
    rows = dr.rows_applicable(H, W)
    gref, gbound, p = dr.tail_g2(dy, B, H, W, W2, z, *dr.bn(prm))           # (fix form: from the kernel's own stored dyc)
    g2 = g2b.get()
    _within("g2", g2, gref, gbound, rep)
    t = dr.tail_from_g2(g2, z, prm["gamma"], prm["mean"], prm["rstd"], dr.bwd_rows_unit_pixels(B, H, W) if rows else 128, rows)
    dz = dzb.get()
    _within("dz", dz, *t["dz"], rep)
    _bias("g2", g2, gref, rep)
    _bias("dz", dz, t["dz"][0], rep)
    for nm, buf, pr in (("dgamma", dgb, prior[0]), ("dbeta", dbb, prior[1])):
        ref, e = t[nm]
        if pr is not None:
            ref, e = pr + ref, e + dr.U * np.abs(pr + ref)
        _within(nm + "2", buf.get()[0], ref, e, rep)
    print(f"conv3x3_bwd{'_fix' if fix else ''} B={B} H={H} W={W} lddy={lddy} accumulate={acc}: " + ", ".join(rep))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("B,H,W,ld", dr.CONV3X3_FLAT + dr.CONV3X3_ROWS)
def test_conv3x3_bwd(L, B, H, W, ld, acc):
    """mcl_dense_conv3x3_bwd, flat-tile and row-walking forms: g2 against the restatement, then dz, dgamma2, dbeta2 restated
    from the kernel's own stored g2; dy read in place from a 32-channel slice between NaN columns."""
    _run_tail(L, B, H, W, TAIL_LD[ld], acc, fix=False)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("B,H,W,ld", dr.CONV3X3_FLAT)
def test_conv3x3_bwd_fix(L, B, H, W, ld, acc):
    """mcl_dense_conv3x3_bwd_fix: the corrected dy (dyc) against the restatement of bn1_fix, then everything else from the
    kernel's own dyc."""
    _run_tail(L, B, H, W, TAIL_LD[ld], acc, fix=True)


# ------------------------------------------------------------------------------------------------------------ head backward
_head_inputs = dr.head_case


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("S,C,ld", dr.HEAD_SHAPES)
def test_bn1_bwd(L, S, C, ld, acc):
    """mcl_dense_bn1_bwd (bn1_bwd_kernel<0>, finalize, bn1_bwd_kernel<1>): gbuf (two roundings), dgamma, dbeta; x and gbuf are
    the first C columns of wider buffers whose other columns hold NaN."""
    prm, x, W1, dz, gb = _head_inputs(S, C)
    xb = Mat(S, ld).set(0, x).freeze()
    gbb = Mat(S, ld).set(0, gb).freeze()
    dzb = Mat(S, 128).set(0, dz).freeze()
    wb = Mat(128, C).set(0, W1).freeze()
    ws = Mat(1, int(L.mcl_dense_bn1_bwd_workspace_floats(S, C)), "f32").freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    rng = np.random.default_rng(S + acc)
    prior = [dr.f32(rng.normal(0, 0.5, C)) for _ in range(2)] if acc else [None, None]
    dgb, dbb = [(vec(p) if acc else out_vec(C)).freeze() for p in prior]
    _check(L.mcl_dense_bn1_bwd(dzb.ptr(), wb.ptr(), C, xb.ptr(), ld, S, *[p.ptr() for p in pv], ws.ptr(), dgb.ptr(), dbb.ptr(),
                               acc, gbb.ptr(), ld, _st()), "mcl_dense_bn1_bwd")
    torch.cuda.synchronize()
    for b, nm in [(xb, "x"), (dzb, "dz"), (wb, "W1")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    gbb.unchanged("gbuf", 0, C)
    ws.unchanged("workspace", 0, ws.ld)
    dgb.unchanged("dgamma", 0, C)
    dbb.unchanged("dbeta", 0, C)
    h = dr.Head(dz, W1, x, *dr.bn(prm))
    assert h.p.amb_share <= dr.AMB_CAP
    rep = []
    _within("gbuf", gbb.get(0, C), *dr.gbuf_add(gb, *h.delta()), rep)
    pg = h.param_grads()
    for nm, buf, pr in (("dgamma", dgb, prior[0]), ("dbeta", dbb, prior[1])):
        ref, e = pg[nm]
        if pr is not None:
            ref, e = pr + ref, e + dr.U * np.abs(pr + ref)
        _within(nm, buf.get()[0], ref, e, rep)
    print(f"bn1_bwd S={S} C={C} ld={ld} accumulate={acc}: " + ", ".join(rep))


@pytest.mark.parametrize("S,C,ld", dr.HEAD_SHAPES)
def test_bn1_single_pass_sequence(L, S, C, ld):
    """mcl_dense_bn1_dx_sums + mcl_dense_bn1_fix as DenseBlockFn.backward drives them for two layers of one block: layer B reads
    [0, C + 32), layer A reads [0, C) (the buffers are widened to hold C + 32 channels where the listed ld is narrower).  Each of
    the four launches is restated from the buffers the launch before it left (gbuf and kprev read back in between): B's pass
    without previous terms, the fix of [C, C + 32), A's pass subtracting B's terms one pass late, the fix of [0, C)."""
    C2 = C + 32
    ld = max(ld, (C2 + 7) // 8 * 8)
    prmB = dr.layer_params(C2, 1500 + C)
    prmA = dict(prmB, **{k: dr.layer_params(C, 1600 + C)[k] for k in ("gamma", "beta")})     # the statistics are the channels'
    prmA = {k: v[:C] if k in ("mean", "rstd", "loc", "scale") else v for k, v in prmA.items()}
    x = dr.activations(S, C2, prmB, 1700 + C)
    gb0 = dr.gradients((S, C2), 1800 + C)
    xb = Mat(S, ld).set(0, x).freeze()
    gbb = Mat(S, ld).set(0, gb0)
    kprev = out_vec(2 * C2).freeze()                       # never initialised by the host
    mv, rv = vec(prmB["mean"]).freeze(), vec(prmB["rstd"]).freeze()
    rep = []
    cur = gb0
    for name, Cl, prm, have_prev in (("B", C2, prmB, 0), ("A", C, prmA, 1)):
        dz = dr.bf16(dr.gradients((S, 128), 1900 + Cl) + 1e-3)
        W1 = dr.weights((128, Cl), Cl, 2000 + Cl)
        dzb, wb = Mat(S, 128).set(0, dz).freeze(), Mat(128, Cl).set(0, W1).freeze()
        gv, bv = vec(prm["gamma"]).freeze(), vec(prm["beta"]).freeze()
        ws = Mat(1, int(L.mcl_dense_bn1_bwd_workspace_floats(S, Cl)), "f32").freeze()
        prior = [dr.f32(np.full(Cl, 0.5)), dr.f32(np.full(Cl, -0.25))]
        dgb, dbb = vec(prior[0]).freeze(), vec(prior[1]).freeze()
        kin = kprev.get()[0].reshape(C2, 2)
        gbb.freeze()
        kprev.freeze()
        _check(L.mcl_dense_bn1_dx_sums(dzb.ptr(), wb.ptr(), Cl, xb.ptr(), ld, S, gv.ptr(), bv.ptr(), mv.ptr(), rv.ptr(), ws.ptr(),
                                       dgb.ptr(), dbb.ptr(), 1, kprev.ptr(), have_prev, gbb.ptr(), ld, _st()),
               "mcl_dense_bn1_dx_sums")
        torch.cuda.synchronize()
        for b, nm in ((xb, "x"), (dzb, "dz"), (wb, "W1"), (gv, "gamma"), (bv, "beta"), (mv, "mean"), (rv, "rstd")):
            b.unchanged(nm)
        gbb.unchanged("gbuf", 0, Cl)
        ws.unchanged("workspace", 0, ws.ld)
        kprev.unchanged("kprev", 0, 2 * Cl)
        h = dr.Head(dz, W1, x[:, :Cl], prm["gamma"], prm["beta"], prmB["mean"][:Cl], prmB["rstd"][:Cl])
        assert h.p.amb_share <= dr.AMB_CAP
        z = np.zeros(Cl)
        d = h.delta(kin[:Cl, 0] if have_prev else z, kin[:Cl, 1] if have_prev else z, z, z, premultiplied=True)
        out = gbb.get(0, C2)
        _within(f"{name}: gbuf", out[:, :Cl], *dr.gbuf_add(cur[:, :Cl], *d), rep)
        pg = h.param_grads()
        for nm, buf, pr in (("dgamma", dgb, prior[0]), ("dbeta", dbb, prior[1])):
            ref, e = pg[nm]
            _within(f"{name}: {nm}", buf.get()[0], pr + ref, e + dr.U * np.abs(pr + ref), rep)
        kref, ke = dr.head_kacc(h, prm["gamma"])
        kout = kprev.get()[0].reshape(C2, 2)
        _within(f"{name}: kacc", kout[:Cl], kref, ke, rep)
        cur = out
        # the mean terms of this pass on the channels the next pass does not cover
        c0, nc = (C, 32) if name == "B" else (0, C)
        gbb.freeze()
        kprev.freeze()
        _check(L.mcl_dense_bn1_fix(xb.ptr(), ld, gbb.ptr(), ld, S, c0, nc, mv.ptr(), rv.ptr(), kprev.ptr(), _st()),
               "mcl_dense_bn1_fix")
        torch.cuda.synchronize()
        gbb.unchanged("gbuf (fix)", c0, nc)
        xb.unchanged("x")
        kprev.unchanged("kprev (fix)")
        out = gbb.get(0, C2)
        _within(f"{name}: fix", out[:, c0:c0 + nc], *dr.bn1_fix(cur, x, c0, nc, prmB["mean"], prmB["rstd"], kout), rep)
        cur = out
    print(f"bn1 single pass S={S} C={C} ld={ld}: " + ", ".join(rep))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("S,C,ld", dr.HEAD_SHAPES)
def test_bn1_wrw_then_dx(L, S, C, ld, acc):
    """mcl_dense_bn1_wrw (the Gram form: dW1, dgamma, dbeta and the two means from one pass) against its restatement, then
    mcl_dense_bn1_dx with the kernel's own means."""
    prm, x, W1, dz, gb = _head_inputs(S, C)
    xb, gbb = Mat(S, ld).set(0, x).freeze(), Mat(S, ld).set(0, gb).freeze()
    dzb, wb = Mat(S, 128).set(0, dz).freeze(), Mat(128, C).set(0, W1).freeze()
    ws = Mat(1, int(L.mcl_wrw_workspace_floats(S, 128, C)), "f32").freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    rng = np.random.default_rng(S + C + acc)
    prior = [dr.f32(rng.normal(0, 0.5, (128, C))), dr.f32(rng.normal(0, 0.5, C)), dr.f32(rng.normal(0, 0.5, C))]
    outs = [(Mat(128, C, "f32").set(0, prior[0]) if acc else Mat(128, C, "f32")).freeze()]
    outs += [(vec(p) if acc else out_vec(C)).freeze() for p in prior[1:]]
    dWb, dgb, dbb = outs
    coefb = out_vec(2 * C).freeze()
    _check(L.mcl_dense_bn1_wrw(dzb.ptr(), wb.ptr(), C, xb.ptr(), ld, S, *[p.ptr() for p in pv], ws.ptr(), dWb.ptr(), acc,
                               dgb.ptr(), dbb.ptr(), acc, coefb.ptr(), _st()), "mcl_dense_bn1_wrw")
    torch.cuda.synchronize()
    for b, nm in [(xb, "x"), (gbb, "gbuf"), (dzb, "dz"), (wb, "W1")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    for b, n in ((ws, ws.ld), (dWb, C), (dgb, C), (dbb, C), (coefb, 2 * C)):
        b.unchanged("output", 0, n)
    r = dr.bn1_wrw(dz, W1, x, *dr.bn(prm), dr.wrw_slab_terms(S))
    rep = []
    for nm, buf, pr in (("dW", dWb, prior[0]), ("dgamma", dgb, prior[1]), ("dbeta", dbb, prior[2])):
        ref, e = r[nm]
        out = buf.get() if nm == "dW" else buf.get()[0]
        ref, e = (pr + ref, e + dr.U * (np.abs(ref) + np.abs(pr + ref))) if acc else (ref, e + dr.U * np.abs(ref))
        _within(nm, out, ref, e, rep)
    coef = coefb.get()[0].reshape(C, 2)
    _within("coef", coef, *r["coef"], rep)
    _check(L.mcl_dense_bn1_dx(dzb.ptr(), wb.ptr(), C, xb.ptr(), ld, S, *[p.ptr() for p in pv], coefb.ptr(), gbb.ptr(), ld,
                              _st()), "mcl_dense_bn1_dx")
    torch.cuda.synchronize()
    gbb.unchanged("gbuf", 0, C)
    coefb.freeze().unchanged("coef")
    h = dr.Head(dz, W1, x, *dr.bn(prm))
    z = np.zeros(C)
    _within("gbuf", gbb.get(0, C), *dr.gbuf_add(gb, *h.delta(coef[:, 0], coef[:, 1], z, z)), rep)
    print(f"bn1_wrw + bn1_dx S={S} C={C} ld={ld} accumulate={acc}: " + ", ".join(rep))


@pytest.mark.parametrize("S,C,ld", dr.PAIR_SHAPES)
def test_bn1_dx_window_and_pair(L, S, C, ld):
    """mcl_dense_bn1_dx_window (layer A's term on its last 32 input channels) and mcl_dense_bn1_dx_pair (both layers' terms on the
    C channels both read, added in fp32, rounded to bf16 once, then added to gbuf) against the restatement."""
    C2 = C + 32
    prmA, prmB, x, gb, dzA, dzB, W1A, W1B = dr.pair_case(S, C)
    hA = dr.Head(dzA, W1A, x, *dr.bn(prmA))
    hB = dr.Head(dzB, W1B, x[:, :C], *dr.bn(prmB))
    coefA, coefB = (dr.f32(np.stack([h.c1, h.c2], 1)) for h in (hA, hB))
    xb, gbb = Mat(S, ld).set(0, x).freeze(), Mat(S, ld).set(0, gb).freeze()
    bufs = dict(dzA=Mat(S, 128).set(0, dzA), dzB=Mat(S, 128).set(0, dzB), WA=Mat(128, C2).set(0, W1A), WB=Mat(128, C).set(0, W1B),
                gA=vec(prmA["gamma"]), bA=vec(prmA["beta"]), gB=vec(prmB["gamma"]), bB=vec(prmB["beta"]),
                mu=vec(prmA["mean"]), rs=vec(prmA["rstd"]), cA=vec(coefA.reshape(-1)), cB=vec(coefB.reshape(-1)))
    for b in bufs.values():
        b.freeze()
    P = {k: b.ptr() for k, b in bufs.items()}
    _check(L.mcl_dense_bn1_dx_window(P["dzA"], P["WA"], C2, C, 32, xb.ptr(), ld, S, P["gA"], P["bA"], P["mu"], P["rs"], P["cA"],
                                     gbb.ptr(), ld, _st()), "mcl_dense_bn1_dx_window")
    torch.cuda.synchronize()
    gbb.unchanged("gbuf (window)", C, 32)
    rep = []
    z = np.zeros(C2)
    dA = hA.delta(coefA[:, 0], coefA[:, 1], z, z)
    _within("window", gbb.get(C, 32), *dr.gbuf_add(gb[:, C:], dA[0][:, C:], dA[1][:, C:]), rep)
    gbb.freeze()
    _check(L.mcl_dense_bn1_dx_pair(P["dzA"], P["WA"], C2, P["gA"], P["bA"], P["cA"], P["dzB"], P["WB"], P["gB"], P["bB"], P["cB"],
                                   C, xb.ptr(), ld, S, P["mu"], P["rs"], gbb.ptr(), ld, _st()), "mcl_dense_bn1_dx_pair")
    torch.cuda.synchronize()
    gbb.unchanged("gbuf (pair)", 0, C)
    xb.unchanged("x")
    for k, b in bufs.items():
        b.unchanged(k)
    _within("pair", gbb.get(0, C), *dr.gbuf_add(gb[:, :C], *dr.pair_delta(hA, coefA[:C], hB, coefB, C)), rep)
    print(f"bn1_dx_window + bn1_dx_pair S={S} C={C} ld={ld}: " + ", ".join(rep))


# ------------------------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("B,H,W", dr.WRW3_SHAPES)
def test_conv3x3_wrw(L, B, H, W, acc):
    """mcl_dense_conv3x3_wrw_det (kernel-row form and, for 17 <= W, the row-walking form), overwrite and accumulate."""
    S = B * H * W
    prm, z, _, dy = _tail_inputs(B, H, W)
    dy = dr.bf16(dy + 2e-3)
    lddy, c0 = 64, 16
    dyb, zb = Mat(S, lddy).set(c0, dy).freeze(), Mat(S, 128).set(0, z).freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    ws = Mat(1, int(L.mcl_dense_conv3x3_wrw_workspace_floats(S)), "f32").freeze()
    prior = dr.f32(np.random.default_rng(S).normal(0, 0.5, (32, 1152))) if acc else None
    dWb = (Mat(32, 1152, "f32").set(0, prior) if acc else Mat(32, 1152, "f32")).freeze()
    _check(L.mcl_dense_conv3x3_wrw_det(dyb.ptr(c0), lddy, zb.ptr(), S, H, W, *[p.ptr() for p in pv], ws.ptr(), dWb.ptr(), acc,
                                       _st()), "mcl_dense_conv3x3_wrw_det")
    torch.cuda.synchronize()
    for b, nm in [(dyb, "dy"), (zb, "z")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    ws.unchanged("workspace", 0, ws.ld)
    dWb.unchanged("dW2", 0, 1152)
    p = dr.Prologue(z, *dr.bn(prm))
    ref, e = dr.conv3x3_wrw(dy, p.a, B, H, W, prior=None if prior is None else prior.reshape(32, 3, 3, 128), e_a=p.amb_w,
                            nterms=dr.wrw3_terms(S))
    rep = []
    _within("dW2", dWb.get().reshape(32, 3, 3, 128), ref, e, rep)
    print(f"conv3x3_wrw B={B} H={H} W={W} accumulate={acc}: " + ", ".join(rep))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("S,M,N", dr.WRW1_SHAPES)
def test_conv1x1_wrw_det(L, S, M, N, acc):
    """mcl_conv1x1_wrw_det with the BatchNorm + ReLU prologue (a rounded to bf16, as in the forward), M up to 256 output
    channels (two passes of 128), ragged channel tiles, overwrite and accumulate."""
    prm, a, dz = dr.wrw1_case(S, M, N)
    lda = (N + 32 + 7) // 8 * 8
    ab, dzb = Mat(S, lda).set(0, a).freeze(), Mat(S, M).set(0, dz).freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    ws = Mat(1, int(L.mcl_wrw_workspace_floats(S, min(M, 128), N)), "f32").freeze()
    prior = dr.f32(np.random.default_rng(S).normal(0, 0.5, (M, N))) if acc else None
    dWb = (Mat(M, N, "f32").set(0, prior) if acc else Mat(M, N, "f32")).freeze()
    _check(L.mcl_conv1x1_wrw_det(dzb.ptr(), M, ab.ptr(), lda, *[p.ptr() for p in pv], ws.ptr(), dWb.ptr(), acc, S, M, N, _st()),
           "mcl_conv1x1_wrw_det")
    torch.cuda.synchronize()
    for b, nm in [(ab, "a"), (dzb, "dz")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    ws.unchanged("workspace", 0, ws.ld)
    dWb.unchanged("dW", 0, N)
    p = dr.Prologue(a, *dr.bn(prm))
    assert p.amb_share <= dr.AMB_CAP
    rep = []
    _within("dW", dWb.get(), *dr.conv1x1_wrw(dz, p.a, prior=prior, e_a=p.amb_w, nterms=dr.wrw_slab_terms(S)), rep)
    print(f"conv1x1_wrw_det S={S} M={M} N={N} accumulate={acc}: " + ", ".join(rep))


# ------------------------------------------------------------------------------------------------------------ persistent block
def _nhwc(t):
    """(B, C, H, W) tensor -> (B*H*W, C) float64 pixels."""
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().cpu().numpy()


def _dense_block4():
    from mclstexp_amd.backbones import densenet121_features_module
    torch.manual_seed(0)
    blk = densenet121_features_module().denseblock4
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif "norm" in n:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return blk.to(DEV).train()


def _block_input(B):
    x = torch.randn(B, 512, 7, 7, generator=torch.Generator().manual_seed(3)).mul_(1.5).add_(0.2)
    return x.to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("B", [1, 5, 33])
def test_persistent_block_backward(B, monkeypatch):
    """dense_block_bwd_kernel (csrc/dense_block.hip) against float64, teacher-forced layer by layer (last layer first) from the
    tensors the launch itself wrote (every layer's dz and the dy' it consumed) and the parameter gradients:
      dy'      the layer's 32 channels of the gradient buffer minus the mean terms the pass before left pending (bn1_fix).  The
               buffer between the passes lives in LDS only, so it is restated as a chain from the incoming gradient -- every
               pass gbuf <- bf16(gbuf + bf16(delta)) in MODE 2 order, the mean terms one pass late -- and the bound of every link
               is carried to the next; the mean terms (kacc) are not kept either and carry the bound of their sums;
      dz       from the stored dy'; g2 is not kept, so its rounding bound is carried into dz and into dgamma2 / dbeta2;
      dgamma1, dbeta1 from the stored dz; dW1 from the stored dz, dW2 from the stored dy';
      the block-input gradient: the end of the chain after the last fix."""
    from mclstexp_amd import densenet_fused as dn
    blk = _dense_block4()
    x = _block_input(B)
    calls = []
    real = dn.dense_block_bwd_persistent
    monkeypatch.setattr(dn, "dense_block_bwd_persistent", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(dn, "USE_BLOCK_PERSISTENT", True)
    monkeypatch.setattr(dn, "USE_BLOCK_PERSISTENT_BWD", True)
    monkeypatch.setattr(dn, "CAPTURE_BLOCKS", [])
    for p in blk.parameters():
        p.grad = None
    gout = torch.randn(B, 1024, 7, 7, generator=torch.Generator().manual_seed(13)).to(DEV).to(torch.bfloat16)
    gout = gout.contiguous(memory_format=torch.channels_last)
    xi = x.clone().requires_grad_(True)
    buf, stats = dn.dense_block(blk, xi, dn._RunningStats(), force_join=True)
    buf.backward(gout.clone())
    torch.cuda.synchronize()
    assert calls == [1], "the persistent backward launch did not run"
    assert not dn.block_persistent_error(x.device)
    cap = dn.CAPTURE_BLOCKS[0]
    S = B * 49
    bufd, gin = _nhwc(buf), _nhwc(cap["gin"])
    mean, rstd = (t.double().cpu().numpy() for t in (stats.mean, stats.rstd))
    f64 = lambda t: t.detach().double().cpu().numpy()
    worst = {}

    def note(name, out, ref, bound, l):
        out = np.asarray(out)
        assert np.isfinite(out).all(), f"layer {l} {name}: non-finite"
        w, at = dr.worst(out, ref, bound)
        worst[name] = max(worst.get(name, 0.0), w)
        assert w <= 1.0, f"layer {l} {name}: element {at} is {w:.3f} of its bound"

    R, E = gin.copy(), np.zeros_like(gin)          # the gradient buffer as restated, and what the real one may be off by
    kP = eP = None                                 # (K1, K2) of the pass before and their bounds
    layers = list(blk.values())
    for l in range(15, -1, -1):
        ly = layers[l]
        cin = 512 + 32 * l
        W1 = f64(cap["wcast"][2 * l]).reshape(128, cin)
        W2 = f64(cap["wcast"][2 * l + 1].permute(0, 2, 3, 1))
        z, dyc, dz = _nhwc(cap["z"][l]), _nhwc(cap["dyc"][l]), _nhwc(cap["dz"][l])
        m2, _, r2 = (f64(t) for t in cap["bn2"][l])
        g2w, b2w = f64(ly.norm2.weight), f64(ly.norm2.bias)
        if kP is None:
            assert np.array_equal(dyc, gin[:, cin:cin + 32]), "the last layer consumed something else than the incoming gradient"
        else:
            note("dy'", dyc, *dr.bn1_fix(R, bufd, cin, 32, mean, rstd, kP, eP[cin:cin + 32, 0], eP[cin:cin + 32, 1],
                                         E[:, cin:cin + 32]), l)
        gref, gbound, p2 = dr.tail_g2(dyc, B, 7, 7, W2, z, g2w, b2w, m2, r2)
        t = dr.tail_from_unstored_g2(gref, gbound, z, g2w, m2, r2, 64)
        note("dz", dz, *t["dz"], l)
        note("dgamma2", f64(ly.norm2.weight.grad), *t["dgamma"], l)
        note("dbeta2", f64(ly.norm2.bias.grad), *t["dbeta"], l)
        note("dW2", f64(ly.conv2.weight.grad.permute(0, 2, 3, 1)),
             *dr.conv3x3_wrw(dyc, p2.a, B, 7, 7, e_a=p2.amb_w, nterms=dr.wrw3_terms(S)), l)
        g1w, b1w = f64(ly.norm1.weight), f64(ly.norm1.bias)
        h = dr.Head(dz, W1, bufd[:, :cin], g1w, b1w, mean[:cin], rstd[:cin])
        pg = h.param_grads()
        note("dgamma1", f64(ly.norm1.weight.grad), *pg["dgamma"], l)
        note("dbeta1", f64(ly.norm1.bias.grad), *pg["dbeta"], l)
        note("dW1", f64(ly.conv1.weight.grad).reshape(128, cin),
             *dr.conv1x1_wrw(dz, h.p.a, e_a=h.p.amb_w, nterms=dr.wrw_slab_terms(S)), l)
        zc = np.zeros(cin)
        if kP is None:
            d = h.delta(zc, zc, zc, zc, premultiplied=True)
        else:
            d = h.delta(kP[:cin, 0], kP[:cin, 1], eP[:cin, 0], eP[:cin, 1], premultiplied=True)
        R[:, :cin], E[:, :cin] = dr.gbuf_add(R[:, :cin], *d, e_g=E[:, :cin])
        kP, eP = dr.head_kacc(h, g1w)
    gx = _nhwc(xi.grad)
    note("block-input gradient", gx, *dr.bn1_fix(R, bufd, 0, 512, mean, rstd, kP, eP[:512, 0], eP[:512, 1], E[:, :512]), 0)
    share = float(np.median(E[:, :512] / (dr.half_ulp_bf16(R[:, :512]) + 1e-300)))
    print(f"persistent block backward B={B}, worst over 16 layers: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; the block-input chain's carried bound is {share:.1f} bf16 half-ulps of the value (median)")


@pytest.mark.parametrize("B", [1, 5, 33])
def test_persistent_block_forward(B, monkeypatch):
    """dense_block_fwd_kernel (csrc/dense_block.hip), a whole 7 x 7 dense block in one launch: all 16 layers teacher-forced from
    the tensors the launch itself produced -- z and y element by element, both batch statistics with the bounds of its scheme
    (per image an fp32 shifted sum over the 49 pixels, the images merged in double)."""
    from mclstexp_amd import densenet_fused as dn
    blk = _dense_block4()
    x = _block_input(B)
    calls = []
    real = dn.dense_block_fwd_persistent
    monkeypatch.setattr(dn, "dense_block_fwd_persistent", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(dn, "USE_BLOCK_PERSISTENT", True)
    monkeypatch.setattr(dn, "CAPTURE_BLOCKS", [])
    with torch.enable_grad():
        buf, stats = dn.dense_block(blk, x.clone().requires_grad_(True), dn._RunningStats())
    torch.cuda.synchronize()
    assert calls == [1], "the persistent launch did not run"
    assert not dn.block_persistent_error(x.device)
    cap = dn.CAPTURE_BLOCKS[0]
    bufd = _nhwc(buf)
    assert np.isfinite(bufd).all()
    mean, var, rstd = (t.double().cpu().numpy() for t in (stats.mean, stats.var, stats.rstd))
    worst = {}
    amb = 0.0

    def note(name, out, ref, bound, l):
        w, at = dr.worst(np.asarray(out), ref, bound)
        worst[name] = max(worst.get(name, 0.0), w)
        assert w <= 1.0, f"layer {l} {name}: element {at} is {w:.3f} of its bound"

    bz, by = [], []
    for l, ly in enumerate(blk.values()):
        cin = 512 + 32 * l
        f64 = lambda t: t.detach().double().cpu().numpy()
        W1 = f64(cap["wcast"][2 * l]).reshape(128, cin)
        W2 = f64(cap["wcast"][2 * l + 1].permute(0, 2, 3, 1))
        ref, bound, p = dr.conv1x1_fwd(bufd[:, :cin], f64(ly.norm1.weight), f64(ly.norm1.bias), mean[:cin], rstd[:cin], W1)
        amb = max(amb, p.amb_share)
        z = _nhwc(cap["z"][l])
        note("z", z, ref, bound, l)
        bz.append(_bias_ok(f"layer {l} z", z, ref))
        m2, v2, r2 = (f64(t) for t in cap["bn2"][l])
        refs, bounds = dr.stats_tiles(z, ly.norm2.eps, 49)
        for nm, o, r, b in zip(("zmean", "zvar", "zrstd"), (m2, v2, r2), refs, bounds):
            note(nm, o, r, b, l)
        ref, bound, p = dr.conv3x3_fwd(z, B, 7, 7, f64(ly.norm2.weight), f64(ly.norm2.bias), m2, r2, W2)
        amb = max(amb, p.amb_share)
        y = bufd[:, cin:cin + 32]
        note("y", y, ref, bound, l)
        by.append(_bias_ok(f"layer {l} y", y, ref))
        refs, bounds = dr.stats_tiles(y, ly.norm1.eps, 49)
        for nm, o, r, b in zip(("ymean", "yvar", "yrstd"), (mean[cin:cin + 32], var[cin:cin + 32], rstd[cin:cin + 32]), refs, bounds):
            note(nm, o, r, b, l)
    print(f"persistent block forward B={B}, worst over 16 layers: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f", worst |bias| of a layer z {max(bz):.4f} y {max(by):.4f}, ambiguous share <= {amb:.2e}")
    assert amb <= dr.AMB_CAP
