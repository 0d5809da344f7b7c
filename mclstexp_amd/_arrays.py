"""The host array layer of the stages around the training step (retrieval, evaluate, cluster, preprocess, genes): argument
checks that need no device, and the few ways an array becomes a device tensor the C ABI can take.  Everything here is
plain copies -- no ``.contiguous()`` / ``.to(dtype)`` / ``torch.cat`` on a device tensor, which would launch a kernel of
another library -- and nothing falls back to the CPU."""
from __future__ import annotations

import json
from typing import Callable, Container, List, Optional, Sequence, Tuple, Type, Union

import numpy as np
import torch

Tensor = torch.Tensor
ArrayLike = Union[np.ndarray, Tensor]
FLOAT_CODE = {torch.float32: 0, torch.float64: 1}       # the C ABI's dtype argument of the fp32 / fp64 entry points


def device(who: str) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError(f"mclstexp_amd.{who}: no GPU available (HIP kernels, no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def upload(a: np.ndarray, dev: torch.device) -> Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def empty(dev: torch.device) -> Callable[..., Tensor]:
    """``(shape, dtype) ->`` an uninitialised tensor on ``dev``."""
    return lambda shape, dtype: torch.empty(shape, device=dev, dtype=dtype)


# ------------------------------------------------------------------------------------------------------ host checks
def check_int(v, name: str, lo: int, hi: Optional[int] = None) -> int:
    """``v`` as an int when it is an integer (no bool) in ``lo .. hi``, or ``>= lo`` where there is no ``hi``."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an integer {f'>= {lo}' if hi is None else f'in {lo} .. {hi}'}, got {v!r}")
    return int(v)


def check_flag(v, name: str) -> bool:
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} must be a bool, got {v!r}")
    return bool(v)


def cumulative_offsets(sizes) -> np.ndarray:
    """[0, sizes[0], sizes[0] + sizes[1], ...] as int64."""
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def validate_offsets(offsets: Optional[Sequence[int]], rows: int, min_rows: int, max_rows: Optional[int] = None,
                     max_segments: Optional[int] = None, none_is_one: bool = False, noun: str = "segment") -> np.ndarray:
    """The preconditions of device-resident segment offsets, checked on the host: offsets[0] = 0, offsets[-1] = rows,
    every segment holds min_rows .. max_rows rows, at most max_segments of them.  ``none_is_one``: None stands for one
    segment of all rows.  Returns them as int64."""
    if offsets is None and none_is_one:
        offsets = [0, rows]
    off = np.asarray(offsets)
    if off.ndim != 1 or off.size < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"offsets must be a 1-D integer array of S + 1 >= 2 entries, got {off!r}")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != rows:
        raise ValueError(f"offsets must run from 0 to the number of rows ({rows}), got {off[0]} .. {off[-1]}")
    seg = np.diff(off)
    if (seg < min_rows).any() or (max_rows is not None and (seg > max_rows).any()):
        span = f">= {min_rows}" if max_rows is None else f"{min_rows} .. {max_rows}"
        raise ValueError(f"every {noun} needs {span} rows; {noun} sizes {seg.tolist()}")
    if max_segments is not None and seg.size > max_segments:
        raise ValueError(f"at most {max_segments} {noun}s per call")
    return off


def paired_offsets(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], noun: str) -> np.ndarray:
    """The row offsets of per-``noun`` (spots, genes) predictions stacked, after checking that every prediction has a
    ground truth of its shape, all share one gene count and each holds >= 2 spots (Pearson r is undefined below 2)."""
    if len(preds) != len(trues) or not preds:
        raise ValueError(f"need one ground truth per prediction and >= 1 {noun}; got {len(preds)} and {len(trues)}")
    for i, (p, t) in enumerate(zip(preds, trues)):
        if tuple(p.shape) != tuple(t.shape):
            raise ValueError(f"{noun} {i}: pred {tuple(p.shape)} and true {tuple(t.shape)} differ in shape")
        if p.ndim != 2 or p.shape[1] != preds[0].shape[1]:
            raise ValueError(f"{noun} {i}: expected (spots, {preds[0].shape[1]}) arrays, got {tuple(p.shape)}")
    off = cumulative_offsets([int(p.shape[0]) for p in preds])
    return validate_offsets(off, int(off[-1]), min_rows=2, noun=noun)


def check_columns(x: ArrayLike, max_dim: int) -> Tuple[int, int]:
    """(rows, D) of the 2-D matrix ``x``, whose 1 .. ``max_dim`` columns one thread of a kernel keeps."""
    if not isinstance(x, Tensor) and np.asarray(x).ndim != 2:
        raise ValueError(f"x: expected a 2-D (rows, D) array, got shape {np.asarray(x).shape}")
    if len(x.shape) != 2:
        raise ValueError(f"x: expected a 2-D (rows, D) array, got shape {tuple(x.shape)}")
    rows, D = int(x.shape[0]), int(x.shape[1])
    if D < 1 or D > max_dim:
        raise ValueError(f"x has {D} columns; the kernel handles 1 .. {max_dim}")
    return rows, D


def nanmean(v) -> float:
    """The mean of the finite entries of ``v``; NaN when it has none."""
    v = np.asarray(v, dtype=np.float64)
    return float(v[np.isfinite(v)].mean()) if np.isfinite(v).any() else float("nan")


# -------------------------------------------------------------------------------------------------- device matrices
def _as_2d(x: ArrayLike, name: str, exc: Type[Exception] = ValueError) -> Tensor:
    t = x if isinstance(x, Tensor) else torch.as_tensor(np.asarray(x))
    if t.dim() != 2:
        raise exc(f"{name}: expected a 2-D array, got shape {tuple(t.shape)}")
    return t


def _copy_free(t: Tensor, dense: bool) -> bool:
    if dense:
        return t.is_cuda and t.is_contiguous()
    return t.is_cuda and (t.stride(1) == 1 or t.shape[1] == 1) and t.stride(0) >= t.shape[1]


def matrix(x: ArrayLike, name: str, dev: torch.device, accept: Container[torch.dtype],
           host_dtype: Union[torch.dtype, Callable[[Tensor], torch.dtype]], exc: Type[Exception] = ValueError,
           dense: bool = False) -> Tensor:
    """``x`` as a row-major device matrix of a dtype in ``accept``: unit column stride, rows that do not overlap
    (``dense``: no gap between them either).  No copy when it already is one; any other device layout costs one plain
    copy.  A host array of another dtype is converted on the host to ``host_dtype`` (a dtype, or a function of the host
    tensor that picks one); a device tensor of another dtype raises ``exc``, as a non-2-D ``x`` does."""
    t = _as_2d(x, name, exc)
    if t.dtype not in accept:
        if t.is_cuda:
            want = " or ".join(str(d).replace("torch.", "") for d in accept)
            raise exc(f"{name}: device tensors must be {want}, got {t.dtype}")
        t = t.to(host_dtype(t) if callable(host_dtype) else host_dtype)
    if _copy_free(t, dense):
        return t
    if t.is_cuda:
        out = torch.empty(tuple(t.shape), device=dev, dtype=t.dtype)
        out.copy_(t)
        return out
    return t.contiguous().to(dev)


def dense(a: ArrayLike, name: str, shape, dtype: torch.dtype, dev: torch.device, copy: bool = False,
          integer: Optional[bool] = None) -> Tensor:
    """``a`` as a dense device tensor of ``shape`` and ``dtype``: a host array is converted on the host, a device tensor
    of another dtype raises.  ``copy``: never the caller's own storage (the kernel writes it, or its outputs must alias
    nothing).  ``integer`` True / False: a host array must hold integers / floating-point values."""
    t = a if isinstance(a, Tensor) else torch.as_tensor(np.asarray(a))
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.is_cuda:
        if t.dtype != dtype:
            raise ValueError(f"{name}: device tensors must be {str(dtype).replace('torch.', '')}, got {t.dtype}")
    elif integer is not None and integer != (not t.dtype.is_floating_point and t.dtype != torch.bool):
        raise ValueError(f"{name}: expected {'integers' if integer else 'floating-point values'}, got {t.dtype}")
    if t.is_cuda and t.is_contiguous() and not copy:
        return t
    out = torch.empty(tuple(shape), device=dev, dtype=dtype)
    out.copy_(t if t.is_cuda else t.to(dtype))
    return out


def stack_rows(parts: Sequence[ArrayLike], name: str, dev: torch.device,
               convert_on_device: bool = False) -> Tuple[Tensor, np.ndarray]:
    """The (spots_i, genes) ``parts`` row-stacked into one row-major device matrix, and their int64 row offsets.  A single
    row-major device tensor is returned as it is; everything else is one ``copy_`` per part.  The stacked dtype is the
    parts' own when they share a float32 / float64 one, else float64; host parts are converted to it on the host.  The
    two callers differ on a DEVICE part of another dtype, and both behaviours are kept: ``convert_on_device=True``
    (``evaluate``) lets ``copy_`` convert it, False (``cluster``) raises ``ValueError``."""
    if not parts:
        raise ValueError(f"{name}: need at least one slide")
    ts = [_as_2d(p, f"{name}[{i}]") for i, p in enumerate(parts)]
    dtypes = {t.dtype for t in ts}
    dtype = dtypes.pop() if len(dtypes) == 1 and ts[0].dtype in FLOAT_CODE else torch.float64
    for i, t in enumerate(ts):
        if t.shape[1] != ts[0].shape[1]:
            raise ValueError(f"{name}[{i}]: expected (spots, {ts[0].shape[1]}), got {tuple(t.shape)}")
        if t.is_cuda and t.dtype != dtype and not convert_on_device:
            raise ValueError(f"{name}[{i}]: device slides must be float32 or float64 and share one dtype, got {t.dtype}")
    offsets = cumulative_offsets([int(t.shape[0]) for t in ts])
    if len(ts) == 1 and ts[0].dtype == dtype and _copy_free(ts[0], False):
        return ts[0], offsets
    out = torch.empty((int(offsets[-1]), ts[0].shape[1]), device=dev, dtype=dtype)
    for i, t in enumerate(ts):
        out[offsets[i]:offsets[i + 1]].copy_(t if t.is_cuda else t.to(dtype))
    return out, offsets


# ------------------------------------------------------------------------------------------------------------- files
def load_gene_major(paths: Sequence[str]) -> List[np.ndarray]:
    """(N_i, G) views of .npy files stored (G, N_i), the layout of the reference's ``preprocessed_matrix.npy``; every
    file must hold the first one's G."""
    mats = [np.load(p) for p in paths]
    for p, a in zip(paths, mats):
        if a.ndim != 2 or a.shape[0] != mats[0].shape[0]:
            raise ValueError(f"{p}: expected (G, N) with G = {mats[0].shape[0]}, got {a.shape}")
    return [a.T for a in mats]


def json_value(v):
    """``v`` as ``json`` can write it: a NaN float as None, an array as a list of Python numbers (NaN entries None)."""
    if isinstance(v, float) and v != v:
        return None
    if isinstance(v, np.ndarray):
        return [json_value(float(x)) if v.dtype.kind == "f" else int(x) for x in v]
    return v


def write_json(path: str, doc) -> None:
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
