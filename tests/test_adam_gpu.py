"""Every Adam kernel path of csrc/adam.hip, called through ctypes, one step at a time against the float64 restatement in
tests/adam_reference.py: the flat kernels (vector body, scalar tail, second grid-stride trip, unaligned fallback, bf16 shadow),
the device-side constants kernel with its history ring, the dense table kernels (4-row groups with missing rows, padded
gradient rows, both forms) and the lazy table kernel called directly (clamped and duplicate positions, owner < 0, one and two
tables, materialisation, the non-vector form) bit for bit against the dense kernel stepped every step.

Every buffer sits between guard words filled with a sentinel (a quiet NaN when read as a float); the guards must be bit-unchanged
after every call.  The bounds are derived in adam_reference.py, not tuned; each case prints how much of them it uses."""
import numpy as np
import pytest
import torch

import adam_reference as ar

pytestmark = pytest.mark.gpu

DEV = "cuda"
B1, B2, EPS = 0.9, 0.999, 1e-8
GUARD = 64                       # guard words (4 bytes each) on either side of every buffer
SENT = 0x7FC0DEAD                # a quiet NaN as fp32, a huge step number as int32
MCL_EINVAL, MCL_EUNSUPPORTED = -1, -2
HYPERS = [(1e-4, 1e-3), (1e-2, 0.0)]


@pytest.fixture(scope="module")
def L():
    from mclstexp_amd import _lib
    return _lib.lib()           # must load: no fallback


def _st():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """A device buffer of 4- or 8-byte elements between sentinel guards.  off shifts the payload by whole floats (an
    unaligned base pointer); tail widens the guard behind it."""

    def __init__(self, host, off=0, tail=GUARD):
        host = np.ascontiguousarray(host)
        assert host.dtype.itemsize in (4, 8)
        words = host.reshape(-1).view(np.int32)
        self.dtype, self.shape, self.n, self.lo = host.dtype, host.shape, words.size, GUARD + off
        self.base = torch.full((self.lo + self.n + tail,), SENT, dtype=torch.int32, device=DEV)
        self.set(host)

    @property
    def ptr(self):
        return self.base.data_ptr() + 4 * self.lo

    def set(self, host):
        words = np.ascontiguousarray(host, dtype=self.dtype).reshape(-1).view(np.int32)
        assert words.size == self.n
        self.base[self.lo:self.lo + self.n].copy_(torch.from_numpy(words.copy()))

    def get(self):
        return self.base[self.lo:self.lo + self.n].cpu().numpy().view(self.dtype).reshape(self.shape)

    def dev(self):
        return self.base[self.lo:self.lo + self.n]

    def bits(self):
        return self.dev().cpu().numpy()

    def guards_ok(self):
        b = self.base
        return bool((b[:self.lo] == SENT).all().item() and (b[self.lo + self.n:] == SENT).all().item())


def _guards(*bufs):
    for i, b in enumerate(bufs):
        assert b.guards_ok(), f"guard words of buffer {i} were overwritten"


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def _check(code, what):
    assert code == 0, f"{what} returned {code}"


def _dev_consts(L, lr, wd, t, hist=None, hist_len=0):
    """The device form's constants for step t: counter at t - 1, one call of the constants kernel."""
    step = Buf(np.array([t - 1], dtype=np.int64))
    consts = Buf(np.zeros(8, dtype=np.float32))
    hyper = Buf(np.array([lr, B1, B2, EPS, wd], dtype=np.float64))
    if hist is None:
        _check(L.mcl_adam_consts_update(step.ptr, consts.ptr, hyper.ptr, _st()), "mcl_adam_consts_update")
    else:
        _check(L.mcl_adam_consts_update_hist(step.ptr, consts.ptr, hyper.ptr, hist.ptr, hist_len, _st()),
               "mcl_adam_consts_update_hist")
    assert int(step.get()[0]) == t
    _guards(step, consts, hyper)
    return step, consts, hyper


def _bf16_rne(x):
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------- flat kernels
def _run_flat(L, form, data, lr, wd, t, offs=(0, 0, 0, 0)):
    """One step of one entry point on fresh guarded copies of data = (p, g, m, v).  Returns (code, [p, g, m, v] buffers, shadow
    buffer or None)."""
    n = data[0].size
    bufs = [Buf(x, off=o) for x, o in zip(data, offs)]
    pb, gb, mb, vb = bufs
    shadow = None
    if form == "host":
        code = L.mcl_adam_step(pb.ptr, gb.ptr, mb.ptr, vb.ptr, n, lr, B1, B2, EPS, wd, 1 - B1 ** t, 1 - B2 ** t, _st())
    else:
        _, consts, _ = _dev_consts(L, lr, wd, t)
        if form == "dev":
            code = L.mcl_adam_step_dev(pb.ptr, gb.ptr, mb.ptr, vb.ptr, n, consts.ptr, _st())
        else:
            # bf16 pairs in 4-byte words; an odd n leaves half a word that the kernel must not touch
            shadow = Buf(np.full((n + 1) // 2 * 2, 0xBEEF, dtype=np.uint16).view(np.int32))
            code = L.mcl_adam_step_dev_shadow(pb.ptr, gb.ptr, mb.ptr, vb.ptr, n, consts.ptr, shadow.ptr, _st())
        _guards(consts)
    _guards(*bufs)
    if shadow is not None:
        _guards(shadow)
    return code, bufs, shadow


FLAT_N = [1, 3, 4, 5, 1023, 100003, 2097152 + 4099]     # the last: above the 2048-workgroup cap of 2 097 152 elements, so the
#                                                         vector body takes a second grid-stride trip and the 3-element scalar
#                                                         tail is seen by every workgroup


@pytest.mark.parametrize("n", FLAT_N)
def test_flat_step_within_bounds_all_forms(L, n):
    """mcl_adam_step against float64 within the bounds for p, m and v; mcl_adam_step_dev with constants from the constants
    kernel bit-identical to it; mcl_adam_step_dev_shadow bit-identical too, its shadow the bf16 round-to-nearest-even of the
    new p.  One step from a non-trivial state, so nothing accumulates."""
    worst = np.zeros(3)
    for t in (1, 2, 1000):
        for lr, wd in HYPERS:
            data = ar.planted_inputs(n, wd, seed=n % 1000 + t)
            p, g, m, v = data
            code, (pb, gb, mb, vb), _ = _run_flat(L, "host", data, lr, wd, t)
            _check(code, "mcl_adam_step")
            P, M, V = pb.get(), mb.get(), vb.get()
            assert _same_bits(gb.get(), g), "the gradient was written"
            r = ar.ratios(p, g, m, v, P, M, V, lr, B1, B2, EPS, wd, t)
            print(f"flat n={n} t={t} lr={lr} wd={wd}: worst ratio p {r[0]:.3f} m {r[1]:.3f} v {r[2]:.3f}")
            assert ar.within(r), f"n={n} t={t} lr={lr} wd={wd}: (p, m, v) use {r} of their bounds"
            worst = np.maximum(worst, r)
            for form in ("dev", "shadow"):
                code, (pb2, gb2, mb2, vb2), sh = _run_flat(L, form, data, lr, wd, t)
                _check(code, form)
                assert _same_bits(pb2.get(), P) and _same_bits(mb2.get(), M) and _same_bits(vb2.get(), V), \
                    f"{form} form differs from mcl_adam_step at n={n} t={t} lr={lr} wd={wd}"
                assert _same_bits(gb2.get(), g)
                if sh is not None:
                    s = sh.get().view(np.uint16)
                    assert np.array_equal(s[:n], _bf16_rne(P)), "shadow != bf16 round-to-nearest-even of the new p"
                    assert np.all(s[n:] == 0xBEEF), "the shadow was written past n"
    print(f"flat n={n} (host = dev = shadow, bit-identical): worst ratio p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")


@pytest.mark.parametrize("n", [5, 100003])
def test_flat_unaligned_pointers(L, n):
    """A base pointer off by one float selects adam_kernel_scalar: bit-identical to the aligned run of the same data and inside
    the bounds.  The shadow form has no scalar fallback: MCL_EUNSUPPORTED, and no byte of any buffer changes."""
    t = 2
    worst = np.zeros(3)
    for lr, wd in HYPERS:
        data = ar.planted_inputs(n, wd, seed=n % 1000 + 17)
        p, g, m, v = data
        ref = {}
        for form in ("host", "dev"):
            code, (pb, _, mb, vb), _ = _run_flat(L, form, data, lr, wd, t)
            _check(code, form)
            ref[form] = (pb.get(), mb.get(), vb.get())
        r = ar.ratios(p, g, m, v, *ref["host"], lr, B1, B2, EPS, wd, t)
        assert ar.within(r)
        for offs in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)):
            for form in ("host", "dev"):
                code, (pb, gb, mb, vb), _ = _run_flat(L, form, data, lr, wd, t, offs=offs)
                _check(code, form)
                got = (pb.get(), mb.get(), vb.get())
                assert all(_same_bits(a, b) for a, b in zip(got, ref[form])), \
                    f"unaligned {offs} {form} form differs from the aligned run at n={n}"
                assert _same_bits(gb.get(), g)
                r = ar.ratios(p, g, m, v, *got, lr, B1, B2, EPS, wd, t)
                assert ar.within(r), f"unaligned {offs} {form}: (p, m, v) use {r} of their bounds"
                worst = np.maximum(worst, r)
            code, bufs, sh = _run_flat(L, "shadow", data, lr, wd, t, offs=offs)
            assert code == MCL_EUNSUPPORTED, f"shadow form with offsets {offs} returned {code}"
            for b, x in zip(bufs, data):
                assert _same_bits(b.get(), x), "a refused call changed a buffer"
            assert np.all(sh.get().view(np.uint16) == 0xBEEF), "a refused call wrote the shadow"
    print(f"flat unaligned n={n}: worst ratio p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")


# ------------------------------------------------------------------------------------------------------------ constants kernel
@pytest.mark.parametrize("t", [1, 2, 3, 10, 1000, 8191, 8192, 8193, 100000])
def test_consts_kernel(L, t):
    """adam_consts_kernel from a counter at t - 1: the counter becomes t, the eight constants are within one fp32 ulp of the
    float64 closed forms (those that do not depend on t exactly the rounded value), ring slot t & 15 holds the same eight words
    and no other slot is touched; new hyper-parameters on the device are used by the next call; the form without a ring
    gives the same constants."""
    lr, wd, hl = 1e-4, 1e-3, 16
    f = np.float32

    def verify(got, lr, wd, t):
        want = ar.consts64(lr, B1, B2, EPS, wd, t)
        want32 = want.astype(f)
        ulps = np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
        print(f"consts t={t} lr={lr} wd={wd}: ulps from float32(consts64) {np.round(ulps, 3).tolist()}")
        assert np.all(ulps <= 1.0), f"t={t}: constants {got} vs {want32}"
        assert _same_bits(got[1:7], want32[1:7]), f"t={t}: step-independent constants {got[1:7]} vs {want32[1:7]}"

    hist = Buf(np.full(8 * hl, SENT, dtype=np.int32))
    step, consts, hyper = _dev_consts(L, lr, wd, t, hist=hist, hist_len=hl)
    c = consts.get()
    verify(c, lr, wd, t)
    ring = hist.bits().reshape(hl, 8)
    assert np.array_equal(ring[t & (hl - 1)], c.view(np.int32)), "ring slot t & 15 != the constants"
    others = np.delete(ring, t & (hl - 1), axis=0)
    assert np.all(others == SENT), "another ring slot was written"
    _guards(hist)
    # no ring: the same eight floats
    _, c2, _ = _dev_consts(L, lr, wd, t)
    assert _same_bits(c2.get(), c)
    # hyper-parameters are read from device memory: overwrite lr and wd there, step again
    lr2, wd2 = 3e-5, 5e-2
    hyper.set(np.array([lr2, B1, B2, EPS, wd2], dtype=np.float64))
    _check(L.mcl_adam_consts_update_hist(step.ptr, consts.ptr, hyper.ptr, hist.ptr, hl, _st()), "mcl_adam_consts_update_hist")
    assert int(step.get()[0]) == t + 1
    c3 = consts.get()
    verify(c3, lr2, wd2, t + 1)
    ring = hist.bits().reshape(hl, 8)
    assert np.array_equal(ring[(t + 1) & (hl - 1)], c3.view(np.int32)) and np.array_equal(ring[t & (hl - 1)], c.view(np.int32))
    assert np.all(np.delete(ring, [t & (hl - 1), (t + 1) & (hl - 1)], axis=0) == SENT)
    _guards(step, consts, hyper, hist)


# --------------------------------------------------------------------------------------------------------- dense table kernels
def _owners(n_rows):
    """-1, the first row, the last row and a few between, each row once."""
    rows = [0, n_rows - 1, n_rows // 2, n_rows - 2, n_rows - 5]
    out, seen = [-1], set()
    for r in rows:
        if 0 <= r < n_rows and r not in seen:
            seen.add(r)
            out += [r, -1] if len(seen) == 2 else [r]
    return np.array(out, dtype=np.int32)


def _padded(rg, ld):
    """(B, cols) gradient rows at row stride ld; the padding holds the sentinel (a NaN wherever it is read)."""
    full = np.full((rg.shape[0], ld), SENT, dtype=np.int32).view(np.float32)
    full[:, :rg.shape[1]] = rg
    return full


def _table_step(L, form, tab, n_rows, cols, owner, rg, ld, lr, wd, t, consts=None):
    """One dense step of one table: slot map filled from the owner list, the kernel, the map cleared again."""
    pb, mb, vb, slot = tab
    ob, rgb = Buf(owner), Buf(_padded(rg, ld))
    _check(L.mcl_row_slot_update(slot.ptr, ob.ptr, owner.size, 1, _st()), "mcl_row_slot_update fill")
    want = np.full(n_rows, -1, dtype=np.int32)
    want[owner[owner >= 0]] = np.flatnonzero(owner >= 0)
    assert np.array_equal(slot.get(), want), "slot map after the fill"
    if form == "host":
        _check(L.mcl_adam_table_step(pb.ptr, mb.ptr, vb.ptr, n_rows, cols, slot.ptr, rgb.ptr, ld, lr, B1, B2, EPS, wd,
                                     1 - B1 ** t, 1 - B2 ** t, _st()), "mcl_adam_table_step")
    else:
        _check(L.mcl_adam_table_step_dev(pb.ptr, mb.ptr, vb.ptr, n_rows, cols, slot.ptr, rgb.ptr, ld, consts.ptr, _st()),
               "mcl_adam_table_step_dev")
    _check(L.mcl_row_slot_update(slot.ptr, ob.ptr, owner.size, 0, _st()), "mcl_row_slot_update clear")
    assert np.all(slot.get() == -1), "slot map after the clearing call"
    assert _same_bits(rgb.get(), _padded(rg, ld)), "the gradient rows were written"
    _guards(pb, mb, vb, slot, ob, rgb)


def _dense_grad(n_rows, cols, owner, rg):
    G = np.zeros((n_rows, cols), dtype=np.float32)
    for b, r in enumerate(owner):
        if r >= 0:
            G[r] = rg[b]
    return G


@pytest.mark.parametrize("cols", [4, 172, 171, 1000])
@pytest.mark.parametrize("n_rows", [1, 2, 3, 5, 4097])
def test_dense_table_step(L, n_rows, cols):
    """adam_table_kernel, one step from non-zero moments, every row of p, m and v against float64: heights that leave 1 to 3
    rows of the last 4-row group missing, gradient rows at stride cols, cols + 4 (still the vector form where cols % 4 == 0)
    and cols + 1 (the non-vector form), an owner list with -1, the first and the last row; rows without a slot get a zero
    data gradient.  The three strides and the host-constant and device-constant forms agree bit for bit."""
    t = 3
    owner = _owners(n_rows)
    tail = GUARD + 4 * cols          # three whole rows past the end stay inside the guard
    worst = np.zeros(3)
    for lr, wd in HYPERS:
        p, g, m, v = (x.reshape(n_rows, cols) for x in ar.planted_inputs(n_rows * cols, wd, seed=n_rows + cols))
        rg = ar.planted_inputs(owner.size * cols, wd, seed=7)[1].reshape(owner.size, cols)
        for b, r in enumerate(owner):                # g + wd p cancels in every fifth column of a row with a gradient
            if r >= 0:
                rg[b, 1::5] = -(np.float32(wd) * p[r, 1::5])
        G = _dense_grad(n_rows, cols, owner, rg)
        _, consts, _ = _dev_consts(L, lr, wd, t)
        first = None
        for ld in (cols, cols + 4, cols + 1):
            for form in ("host", "dev"):
                tab = [Buf(p, tail=tail), Buf(m, tail=tail), Buf(v, tail=tail), Buf(np.full(n_rows, -1, dtype=np.int32))]
                _table_step(L, form, tab, n_rows, cols, owner, rg, ld, lr, wd, t, consts=consts)
                got_dev = [b.dev().clone() for b in tab[:3]]
                if first is None:
                    first = got_dev
                    got = (tab[0].get(), tab[1].get(), tab[2].get())
                    r = ar.ratios(p, G, m, v, *got, lr, B1, B2, EPS, wd, t)
                    print(f"table {n_rows}x{cols} lr={lr} wd={wd}: worst ratio p {r[0]:.3f} m {r[1]:.3f} v {r[2]:.3f}")
                    assert ar.within(r), f"table {n_rows}x{cols} lr={lr} wd={wd}: (p, m, v) use {r} of their bounds"
                    worst = np.maximum(worst, r)
                else:
                    assert all(torch.equal(a, b) for a, b in zip(got_dev, first)), \
                        f"table {n_rows}x{cols} ld_rg={ld} {form} form differs from ld_rg={cols} host form"
        _guards(consts)
    print(f"table {n_rows}x{cols} (3 strides x 2 forms, bit-identical): worst ratio p {worst[0]:.3f} m {worst[1]:.3f} "
          f"v {worst[2]:.3f}")


# ------------------------------------------------------------------------------------------------------- lazy table kernel
N_ROWS, HIST_LEN, T0, STEPS = 37, 16, 9, 20

# What each of the 20 steps does.  The counter starts at T0 = 9, so steps 10..29 use ring slots 10..15, 0..13: the index wraps
# after step 15 and steps 26..29 OVERWRITE the slots of steps 10..13, which rows that fell behind at step 23 then replay from.
#   pos:   forward catch-up BEFORE the step's constants exist (the counter still holds the previous step), rows (x, y) per spot
#   own:   owner lists (x, y) of the gradient rows of this step; None: no table receives a gradient
#   one:   call the one-table form (p1 == nullptr) once per table instead of the two-table form
#   ld1:   gradient rows at stride cols + 1 (the non-vector form also at cols = 172)
#   mat:   materialise after the step
# Gap rule: the ring holds the constants of the last 16 steps, and a row stamped s replays s + 1 .. t; the optimizer
# materialises before any row is 15 steps behind.  Here at step 8 (the first time, 8 behind at most), at 14 and at 20 (6 behind).
SCHEDULE = {
    1: dict(own=([5, -1, 3], [-1, 7, 0])),
    2: dict(pos=[[3.9, -3.0], [5.0, 0.5], [5.0, 7.0], [3.2, 7.0], [36.9, 20.0]]),   # duplicates; -3 -> 0, 3.9 -> 3, 36.9 -> 36
    3: dict(own=([36, 0, -1, 9], [1, -1, -1, 2])),                                  # rows that were never caught up
    4: dict(pos=[[1e9, 11.0], [10.0, 1e9], [10.0, 11.0]]),                          # 1e9 -> 36
    5: dict(pos=[[37.0, 2.0], [2.0, 37.0]], own=([36, 2], [2, 36])),                # 37.0 -> 36, alone on that row
    6: dict(lr=3e-5, own=([4, -1], [-1, -1])),                                      # new learning rate; y: every owner < 0
    7: dict(pos=[[3.9, 3.9], [12.0, 36.9]]),
    8: dict(mat=True),
    9: dict(own=([8, 30, -1, 1], [30, -1, 8, 0]), ld1=True),
    10: dict(pos=[[30.5, 8.2], [-0.9, 36.0], [30.0, 8.0]], one=True),
    11: dict(own=([30, -1, 0], [-1, 8, 36]), one=True),
    12: dict(pos=[[17.0, 17.0]]),
    13: dict(own=([17, 3, 36, -1, 0], [17, -1, 5, 20, 36])),
    14: dict(mat=True, one=True),
    15: dict(own=([2, -1, 36], [0, 19, -1])),
    16: dict(pos=[[19.0, 2.0], [36.9, 19.5]]),
    17: dict(lr=7e-5, own=([19, 6], [-1, 36])),                                     # steps 26..29 go into used slots
    18: dict(pos=[[6.0, 6.0], [-3.0, 1e9]], one=True),
    19: dict(own=([6, 11, -1], [11, -1, 0]), ld1=True),
    20: dict(mat=True),
}


class _Table:
    def __init__(self, p, m, v, cols, lazy):
        tail = GUARD + 4 * cols
        self.p, self.m, self.v = Buf(p, tail=tail), Buf(m, tail=tail), Buf(v, tail=tail)
        self.aux = Buf(np.full(p.shape[0], T0 if lazy else -1, dtype=np.int32))     # lazy: row stamps; dense: slot map
        self.bufs = [self.p, self.m, self.v, self.aux]

    def state(self):
        return self.p.get(), self.m.get(), self.v.get()


def _lazy_call(L, tabs, cols, step, hist, pos=None, owners=None, grads=None, ld=0, n_owner=N_ROWS, n_rows=N_ROWS,
               hist_len=HIST_LEN):
    def ptr(b):
        return b.ptr if b is not None else None
    t0 = tabs[0]
    t1 = tabs[1] if len(tabs) > 1 else None
    own = owners or [None, None]
    gr = grads or [None, None]
    return L.mcl_adam_table_lazy(t0.p.ptr, t0.m.ptr, t0.v.ptr, t0.aux.ptr, ptr(t1 and t1.p), ptr(t1 and t1.m), ptr(t1 and t1.v),
                                 ptr(t1 and t1.aux), n_rows, cols, ptr(pos), ptr(own[0]), ptr(own[1]) if t1 else None, n_owner,
                                 ptr(gr[0]), ptr(gr[1]) if t1 else None, ld, step.ptr, hist.ptr, hist_len, _st())


def _lazy_world(cols, seed):
    lazy, dense = [], []
    for k in range(2):
        p, _, m, v = (x.reshape(N_ROWS, cols) for x in ar.planted_inputs(N_ROWS * cols, 1e-3, seed=seed + k))
        lazy.append(_Table(p, m, v, cols, True))
        dense.append(_Table(p, m, v, cols, False))
    step = Buf(np.array([T0], dtype=np.int64))
    consts = Buf(np.zeros(8, dtype=np.float32))
    hyper = Buf(np.array([1e-4, B1, B2, EPS, 1e-3], dtype=np.float64))
    hist = Buf(np.full(8 * HIST_LEN, SENT, dtype=np.int32))      # a slot read before it is written poisons the row
    return lazy, dense, step, consts, hyper, hist


def _assert_rows_equal(lz, dn, rows, what):
    for name, a, b in zip("pmv", lz.state(), dn.state()):
        for r in rows:
            assert _same_bits(a[r], b[r]), f"{what}: row {r} of {name} differs from the dense run"


@pytest.mark.parametrize("cols", [172, 171])
def test_lazy_table_direct(L, cols):
    """mcl_adam_table_lazy against adam_table_kernel stepped on every step (pinned to float64 by test_dense_table_step), bit
    for bit: after every call the rows it had to bring up to date carry the counter as their stamp and equal the dense run,
    every other row is untouched; after the last materialisation the tables are equal and every stamp is the step count."""
    lazy, dense, step, consts, hyper, hist = _lazy_world(cols, seed=cols)
    rng = np.random.default_rng(cols)
    everything = [b for t in lazy + dense for b in t.bufs] + [step, consts, hyper, hist]

    def check_call(expect_rows, now, before, what):
        """expect_rows[k]: rows of table k the call had to bring to `now`; before: (stamps, state) per table before the call."""
        for k, (lz, dn) in enumerate(zip(lazy, dense)):
            stamps = lz.aux.get()
            old_stamps, old_state = before[k]
            exp = sorted(set(expect_rows[k]))
            assert np.all(stamps[exp] == now), f"{what}: table {k} rows {exp} carry stamps {stamps[exp]}, not {now}"
            rest = np.setdiff1d(np.arange(N_ROWS), exp)
            assert np.array_equal(stamps[rest], old_stamps[rest]), f"{what}: table {k}: a stamp of another row changed"
            for name, a, b in zip("pmv", lz.state(), old_state):
                assert _same_bits(a[rest], b[rest]), f"{what}: table {k}: another row of {name} changed"
            _assert_rows_equal(lz, dn, np.flatnonzero(stamps == now), f"{what}: table {k}")

    def snapshot():
        return [(lz.aux.get(), lz.state()) for lz in lazy]

    for k in range(1, STEPS + 1):
        s = SCHEDULE[k]
        t = T0 + k
        if "pos" in s:                               # the counter is t - 1 and the dense tables are as of t - 1
            pos = np.array(s["pos"], dtype=np.float32)
            rows = np.clip(np.trunc(pos.astype(np.float64)), 0, N_ROWS - 1).astype(np.int64)
            before = snapshot()
            if s.get("one"):
                for j in range(2):
                    pb = Buf(np.ascontiguousarray(pos[:, ::-1] if j else pos))
                    _check(_lazy_call(L, [lazy[j]], cols, step, hist, pos=pb, n_owner=pos.shape[0]), "lazy pos, one table")
                    _guards(pb)
            else:
                pb = Buf(pos)
                _check(_lazy_call(L, lazy, cols, step, hist, pos=pb, n_owner=pos.shape[0]), "lazy pos")
                _guards(pb)
            check_call([rows[:, 0], rows[:, 1]], t - 1, before, f"step {k} catch-up")
        if "lr" in s:
            hyper.set(np.array([s["lr"], B1, B2, EPS, 1e-3], dtype=np.float64))
        _check(L.mcl_adam_consts_update_hist(step.ptr, consts.ptr, hyper.ptr, hist.ptr, HIST_LEN, _st()), "consts")
        assert int(step.get()[0]) == t
        owners = s.get("own") or ([-1], [-1])
        owners = [np.array(o, dtype=np.int32) for o in owners]
        B = owners[0].size
        ld = cols + 1 if s.get("ld1") else cols
        rgs = [(rng.standard_normal((B, cols)) * 10.0 ** rng.uniform(-4, 0, (B, cols))).astype(np.float32) for _ in range(2)]
        for j in range(2):                           # the dense run: every row, every step
            _table_step(L, "dev", dense[j].bufs, N_ROWS, cols, owners[j], rgs[j], ld, None, None, t, consts=consts)
        if "own" in s:
            before = snapshot()
            obs, gbs = [Buf(o) for o in owners], [Buf(_padded(g, ld)) for g in rgs]
            if s.get("one"):
                for j in range(2):
                    _check(_lazy_call(L, [lazy[j]], cols, step, hist, owners=[obs[j], None], grads=[gbs[j], None], ld=ld,
                                      n_owner=B), "lazy gradient, one table")
            else:
                _check(_lazy_call(L, lazy, cols, step, hist, owners=obs, grads=gbs, ld=ld, n_owner=B), "lazy gradient")
            _guards(*obs, *gbs)
            check_call([o[o >= 0] for o in owners], t, before, f"step {k} gradient")
        if s.get("mat"):
            before = snapshot()
            if s.get("one"):
                for j in range(2):
                    _check(_lazy_call(L, [lazy[j]], cols, step, hist), "lazy materialise, one table")
            else:
                _check(_lazy_call(L, lazy, cols, step, hist), "lazy materialise")
            check_call([np.arange(N_ROWS)] * 2, t, before, f"step {k} materialise")
        for lz, dn in zip(lazy, dense):               # whatever is stamped current equals the dense run
            _assert_rows_equal(lz, dn, np.flatnonzero(lz.aux.get() == t), f"after step {k}")
        _guards(*everything)
    for lz, dn in zip(lazy, dense):
        assert np.all(lz.aux.get() == T0 + STEPS)
        assert all(_same_bits(a, b) for a, b in zip(lz.state(), dn.state())), "tables differ after the final materialisation"
    print(f"lazy {N_ROWS}x{cols}: both tables bit-identical to the dense run after {STEPS} steps")


def test_lazy_table_invalid_arguments(L):
    """The argument combinations the entry point refuses return MCL_EINVAL and change nothing."""
    cols = 172
    lazy, _, step, consts, hyper, hist = _lazy_world(cols, seed=1)
    _check(L.mcl_adam_consts_update_hist(step.ptr, consts.ptr, hyper.ptr, hist.ptr, HIST_LEN, _st()), "consts")
    owner = Buf(np.array([3, -1], dtype=np.int32))
    rg = Buf(np.ones((2, cols), dtype=np.float32))
    pos = Buf(np.array([[1.0, 2.0], [3.0, 4.0]], dtype=np.float32))
    bufs = [b for t in lazy for b in t.bufs] + [step, hist, owner, rg, pos]
    before = [b.base.clone() for b in bufs]
    calls = {
        "a gradient without an owner list": dict(grads=[rg, rg], n_owner=2, ld=cols),
        "pos together with a gradient": dict(pos=pos, owners=[owner, owner], grads=[rg, rg], n_owner=2, ld=cols),
        "materialise with n_owner != n_rows": dict(n_owner=N_ROWS - 1),
        "hist_len not a power of two": dict(hist_len=12),
    }
    for what, kw in calls.items():
        for tabs in (lazy, lazy[:1]):
            code = _lazy_call(L, tabs, cols, step, hist, **kw)
            assert code == MCL_EINVAL, f"{what} ({len(tabs)} tables) returned {code}"
    torch.cuda.synchronize()
    for b, old in zip(bufs, before):
        assert torch.equal(b.base, old), "a refused call changed a buffer"
