"""What the element-by-element GPU tests (test_dense_exact_gpu.py, test_stem_exact_gpu.py) share: device buffers between guard
words whose every element is a NaN sentinel until set, the check that nothing outside a kernel's output region changed, and the
assertions on the worst share of a derived bound and on the rounding bias.  A plain module: no tests, no fixtures."""
import numpy as np
import torch

import dense_reference as dr

DEV = "cuda"
EPS = 1e-5
GUARD = 256                      # guard bytes on either side of every buffer
SENT16 = 0x7FC1                  # a quiet NaN as bf16
SENT32 = 0x7FC0DEAD              # a quiet NaN as fp32
SENT8 = 0xEE                     # no window position (0..8) of the max pool


def _st():
    return torch.cuda.current_stream().cuda_stream


def _check(code, what):
    assert code == 0, f"{what} returned {code}"


_KINDS = {"bf16": (torch.int16, np.uint16, SENT16, 2), "f32": (torch.int32, np.uint32, SENT32, 4),
          "u8": (torch.uint8, np.uint8, SENT8, 1)}


class Mat:
    """A (rows, ld) device matrix of bf16 (bits in int16), fp32 (bits in int32) or bytes (u8: the arg-max positions of the max
    pool) between guards, every element the sentinel (a NaN for the two float kinds) until set().  freeze() remembers every
    bit; unchanged() then checks everything outside the columns a kernel may write."""

    def __init__(self, rows, ld, kind="bf16"):
        self.kind, self.rows, self.ld = kind, rows, ld
        self.tdt, self.ndt, self.sent, self.isz = _KINDS[kind]
        self.g = GUARD // self.isz
        self.base = torch.full((2 * self.g + rows * ld,), self.sent, dtype=self.tdt, device=DEV)
        self.before = None

    def ptr(self, col=0):
        return self.base.data_ptr() + self.isz * (self.g + col)

    def _body(self):
        return self.base[self.g:self.g + self.rows * self.ld].view(self.rows, self.ld)

    def set(self, c0, vals):
        if self.kind == "u8":
            return self.set_bits(c0, np.asarray(vals, dtype=np.uint8).reshape(self.rows, -1))
        vals = np.asarray(vals, dtype=np.float64).reshape(self.rows, -1)
        bits = dr.bf16_bits(vals) if self.kind == "bf16" else vals.astype(np.float32).view(np.uint32)
        assert self.kind != "bf16" or np.array_equal(dr.bits_to_f64(bits), vals), "operand is not a bf16 value"
        return self.set_bits(c0, bits)

    def set_bits(self, c0, bits):
        bits = np.ascontiguousarray(bits, dtype=self.ndt).reshape(self.rows, -1)
        view = {"bf16": np.int16, "f32": np.int32, "u8": np.uint8}[self.kind]
        self._body()[:, c0:c0 + bits.shape[1]] = torch.from_numpy(bits.view(view).copy()).to(DEV)
        return self

    def bits(self, c0=0, n=None):
        """The raw bits (uint16 / uint32 / uint8) of the columns [c0, c0 + n)."""
        n = self.ld - c0 if n is None else n
        return self._body()[:, c0:c0 + n].contiguous().cpu().numpy().view(self.ndt)

    def get(self, c0=0, n=None):
        bits = self.bits(c0, n)
        if self.kind == "u8":
            return bits
        return dr.bits_to_f64(bits) if self.kind == "bf16" else bits.view(np.float32).astype(np.float64)

    def freeze(self):
        """Remember every bit (guards included) for unchanged()."""
        self.before = self.base.cpu().numpy().copy()
        return self

    def unchanged(self, what, c0=None, n=None):
        """Guards and everything outside the columns [c0, c0 + n) are bit-unchanged since freeze()."""
        now = self.base.cpu().numpy()
        same = now == self.before
        if c0 is not None:
            body = same[self.g:self.g + self.rows * self.ld].reshape(self.rows, self.ld)
            body[:, c0:c0 + n] = True
        assert same.all(), f"{what}: {int((~same).sum())} elements outside the output region were written"


def vec(vals):
    v = np.asarray(vals, dtype=np.float64).reshape(1, -1)
    return Mat(1, v.shape[1], "f32").set(0, v)


def out_vec(n):
    return Mat(1, n, "f32")


def _within(name, out, ref, bound, report):
    assert np.isfinite(out).all(), f"{name}: non-finite output"
    w, at = dr.worst(out, ref, bound)
    report.append(f"{name} {w:.3f}")
    assert w <= 1.0, f"{name}: element {at} is {w:.3f} of its bound (out {out[at]!r}, ref {ref[at]!r}, bound {bound[at]!r})"
    return w


def _bits_equal(name, got, want, report):
    """got, want: integer bit patterns of the same shape."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{name}: shape {got.shape} against {want.shape}"
    bad = np.argwhere(got != want)
    report.append(f"{name} bits")
    assert bad.size == 0, (f"{name}: {len(bad)} of {got.size} elements differ in bits, the first at {tuple(bad[0])}: "
                           f"got {int(got[tuple(bad[0])]):#x}, expected {int(want[tuple(bad[0])]):#x}")


def _bias(name, out, ref, report):
    b, n, allowed = dr.bias(out, ref)
    report.append(f"bias({name}) {b:+.4f}/N={n}")
    assert abs(b) <= allowed, f"{name}: rounding bias {b:+.4f} half-ulps over {n} elements (allowed {allowed:.4f})"


def _bias_ok(name, out, ref):
    b, n, allowed = dr.bias(out, ref)
    assert abs(b) <= allowed, f"{name}: rounding bias {b:+.4f} half-ulps over {n} elements (allowed {allowed:.4f})"
    return abs(b)


def _stats(name, got, refs, bounds, report):
    for nm, o, r, b in zip(("mean", "var", "rstd"), got, refs, bounds):
        _within(f"{name}{nm}", o, r, b, report)
