"""The UMAP layout of the spot neighbourhood graph on the MI355X: what ``sc.tl.umap`` leaves in ``obsm["X_umap"]`` -- the
step of BLEEP's ``visualize_umap_clusters`` (baselines/Bleep/BLEEP_inference.ipynb: ``sc.pp.pca``, ``sc.pp.neighbors``,
``sc.tl.umap``, ``sc.tl.leiden``, ``sc.pl.umap``) that turns the graph of ``mclstexp_amd.neighbors`` into the coordinates
users look at -- for all slides of an evaluation per call.

What is computed is stated in DESIGN 6.12 and restated in numpy by ``tests/umap_reference.py``; it is that statement, not a
umap-learn release.  Things to know:

* One Jacobi step per epoch: every gradient of epoch n is taken at the positions at the start of epoch n (umap-learn
  updates in place, which is sequential, or a data race when run in parallel).  A vertex's new position is its old one
  plus alpha_n times the sum of its contributions in one fixed order.
* Negative samples are a pure function of (seed, epoch, vertex, entry rank, sample number): splitmix64, no generator state.
* fp64 (umap-learn holds float32).  A sample that coincides with the vertex contributes nothing.
* ``init``: ``"pca"`` (the first two columns of ``x``, the matrix the graph was built from, times 10 / their largest
  absolute value per slide; no noise, so duplicate rows start on top of each other), ``"random"`` (uniform in -10 .. 10
  from the seed) or a (rows, 2) array used as given.  umap-learn's spectral start is not built.
* ``a``, ``b`` come from ``find_ab_params(spread, min_dist)`` (umap-learn's curve fit through scipy, imported lazily)
  unless both are given.  ``n_epochs=None``: 500 for a slide of at most 10000 spots, 200 above, per slide.
* 2 <= n_s <= 16384 rows per segment, at most 65535 segments, 1 <= n_epochs <= 5000, 0 <= negative_sample_rate <= 64.
* One launch per epoch, enqueued back to back; the host reads nothing until the two counters per slide at the end.
* The Leiden clustering of the same graph is ``mclstexp_amd.leiden`` (``leiden.expression_clusters`` runs both).

Everything on the device is fp64, free of floating-point atomics and bit-reproducible run to run; a slide inside a batch
is bit-identical to the same slide alone.  No CPU fallback.

    python -m mclstexp_amd.umap --pred P1.npy ... [--raw] [--n_neighbors 150] [--n_pcs 50] [--n_epochs N] [--seed S] --out_dir D
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _arrays, neighbors
from ._arrays import FLOAT_CODE, ArrayLike, Tensor, cumulative_offsets, dense, device, empty, matrix, upload
from ._lib import call

MAX_ROWS = 16384         # csrc/umap.hip
MAX_SEGMENTS = 65535
MAX_EPOCHS = 5000
MAX_RATE = 64
INITS = ("pca", "random")
MIN_DIST, SPREAD = 0.5, 1.0          # scanpy's sc.tl.umap defaults
OUT_FILE = "X_umap.npy"
_MASK = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------- host rules
def find_ab_params(spread: float = SPREAD, min_dist: float = MIN_DIST) -> Tuple[float, float]:
    """umap-learn's ``find_ab_params``: the (a, b) whose curve 1 / (1 + a x^(2b)) fits 1 below ``min_dist`` and
    exp(-(x - min_dist) / spread) above it on 300 points of 0 .. 3 spread.  (1.0, 0.5) gives (0.5830300, 1.3341670)."""
    from scipy.optimize import curve_fit
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    params, _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    return float(params[0]), float(params[1])


def default_epochs(seg: np.ndarray) -> np.ndarray:
    """umap-learn's rule per segment: 500 epochs up to 10000 rows, 200 above."""
    return np.where(np.asarray(seg) <= 10000, 500, 200).astype(np.int32)


def validate_epochs(n_epochs: Optional[int], seg: np.ndarray) -> np.ndarray:
    if n_epochs is None:
        return default_epochs(seg)
    if isinstance(n_epochs, bool) or not isinstance(n_epochs, (int, np.integer)):
        raise ValueError(f"n_epochs must be an integer or None, got {n_epochs!r}")
    if not 1 <= n_epochs <= MAX_EPOCHS:
        raise ValueError(f"n_epochs must lie in 1 .. {MAX_EPOCHS}, got {n_epochs}")
    return np.full(np.asarray(seg).size, int(n_epochs), dtype=np.int32)


def _check_init(init) -> None:
    if isinstance(init, str) and init not in INITS:
        raise ValueError(f"init must be one of 'pca', 'random' or a (rows, 2) array, got {init!r}"
                         + (": the spectral start is not built" if init == "spectral" else ""))


def _check_params(a, b, gamma: float, alpha: float, negative_sample_rate: int, seed: int, stop_after) -> None:
    for name, v in (("a", a), ("b", b), ("gamma", gamma), ("alpha", alpha)):
        if v is not None and not math.isfinite(float(v)):
            raise ValueError(f"{name} must be finite, got {v!r}")
    if (a is None) != (b is None):
        raise ValueError("give both a and b, or neither (find_ab_params(spread, min_dist) then)")
    for name, v in (("a", a), ("b", b)):
        if v is not None and not float(v) > 0:
            raise ValueError(f"{name} must be positive, got {v!r}")
    _arrays.check_int(negative_sample_rate, "negative_sample_rate", 0, MAX_RATE)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"seed must be an integer (taken modulo 2^64), got {seed!r}")
    if stop_after is not None and (isinstance(stop_after, bool) or not isinstance(stop_after, (int, np.integer))
                                   or stop_after < 0):
        raise ValueError(f"stop_after must be None or an integer >= 0, got {stop_after!r}")


def check_keywords(init, kw: Dict[str, object]) -> None:
    """The checks of ``layout``'s keywords that need no graph, for the callers that build the graph first."""
    unknown = set(kw) - {"n_epochs", "a", "b", "min_dist", "spread", "alpha", "gamma", "negative_sample_rate", "seed",
                         "stop_after"}
    if unknown:
        raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
    _check_init(init)
    _check_params(kw.get("a"), kw.get("b"), kw.get("gamma", 1.0), kw.get("alpha", 1.0), kw.get("negative_sample_rate", 5),
                  kw.get("seed", 0), kw.get("stop_after"))
    validate_epochs(kw.get("n_epochs"), np.array([2]))


def check_graph(graph: Dict[str, object]) -> Tuple[np.ndarray, np.ndarray]:
    """(offsets, nnz_offsets) as int64 of a graph dict of ``neighbors``, after checking its keys and array lengths."""
    for key in ("indptr", "indices", "data", "offsets", "nnz_offsets"):
        if key not in graph:
            raise ValueError(f"graph: expected the dict of neighbors.neighbors() or connectivities(); it has no {key!r}")
    off = np.asarray(graph["offsets"])
    rows = int(off[-1]) if off.ndim == 1 and off.size else -1
    off = _arrays.validate_offsets(off, rows, 2, MAX_ROWS, max_segments=MAX_SEGMENTS)
    nnz_off = np.asarray(graph["nnz_offsets"])
    if (nnz_off.ndim != 1 or nnz_off.size != off.size or not np.issubdtype(nnz_off.dtype, np.integer) or nnz_off[0] != 0
            or (np.diff(nnz_off) < 0).any()):
        raise ValueError(f"graph: nnz_offsets must hold S + 1 = {off.size} ascending integers from 0, got {nnz_off!r}")
    nnz_off = nnz_off.astype(np.int64)
    S, total = off.size - 1, int(nnz_off[-1])
    for key, count in (("indptr", rows + S), ("indices", total), ("data", total)):
        shape = tuple(graph[key].shape)
        if shape != (count,):
            raise ValueError(f"graph: {key} must hold {count} entries, got shape {shape}")
    return off, nnz_off


def from_scipy(mats: Sequence) -> Dict[str, object]:
    """The graph dict ``layout`` takes, on the host, from one ``scipy.sparse`` matrix per slide.  A matrix must be square
    with 2 .. 16384 rows, exactly symmetric, without stored diagonal entries, its weights positive and finite."""
    from scipy import sparse
    if not len(mats):
        raise ValueError("from_scipy: need at least one matrix")
    indptr, indices, data, sizes, counts = [], [], [], [], []
    for s, m in enumerate(mats):
        if not sparse.issparse(m) or m.shape[0] != m.shape[1]:
            raise ValueError(f"matrix {s}: expected a square scipy.sparse matrix, got {type(m).__name__} "
                             f"{getattr(m, 'shape', '')}")
        c = sparse.csr_matrix(m, dtype=np.float64, copy=True)
        c.sum_duplicates()
        c.sort_indices()
        if c.diagonal().any() or (c.indices == np.repeat(np.arange(c.shape[0]), np.diff(c.indptr))).any():
            raise ValueError(f"matrix {s}: the diagonal must be empty")
        if not (np.isfinite(c.data).all() and (c.data > 0).all()):
            raise ValueError(f"matrix {s}: stored weights must be positive and finite")
        if (c != c.T).nnz:
            raise ValueError(f"matrix {s}: not symmetric")
        indptr.append(c.indptr.astype(np.int64))
        indices.append(c.indices.astype(np.int32))
        data.append(c.data)
        sizes.append(c.shape[0])
        counts.append(c.nnz)
    off = cumulative_offsets(sizes)
    _arrays.validate_offsets(off, int(off[-1]), 2, MAX_ROWS, max_segments=MAX_SEGMENTS)
    return {"indptr": np.concatenate(indptr), "indices": np.concatenate(indices), "data": np.concatenate(data),
            "offsets": off, "nnz_offsets": cumulative_offsets(counts)}


# ----------------------------------------------------------------------------------------------------------- device
def layout(graph: Dict[str, object], init: Union[str, ArrayLike] = "pca", x: Optional[ArrayLike] = None,
           n_epochs: Optional[int] = None, a: Optional[float] = None, b: Optional[float] = None,
           min_dist: float = MIN_DIST, spread: float = SPREAD, alpha: float = 1.0, gamma: float = 1.0,
           negative_sample_rate: int = 5, seed: int = 0, stop_after: Optional[int] = None) -> Dict[str, object]:
    """The layout of every segment of ``graph`` (the dict of ``neighbors.neighbors`` / ``connectivities`` / ``from_scipy``;
    see the module docstring).  ``x``: the (rows, D >= 2) matrix the graph was built from, read by ``init="pca"`` only.
    ``stop_after``: run only the first ``stop_after`` epochs of the ``n_epochs`` schedule.  Returns ``embedding`` (rows, 2)
    fp64 on the device, ``attractive_samples`` and ``negative_samples`` ((S,) int64: attractions taken, negative samples
    drawn), ``n_epochs`` ((S,) int32), ``a``, ``b`` and the host ``offsets``."""
    _check_init(init)
    _check_params(a, b, gamma, alpha, negative_sample_rate, seed, stop_after)
    off, nnz_off = check_graph(graph)
    seg = np.diff(off)
    S, rows, total = int(seg.size), int(off[-1]), int(nnz_off[-1])
    epochs = validate_epochs(n_epochs, seg)
    if isinstance(init, str) and init == "pca":
        if x is None:
            raise ValueError("init='pca' reads x, the matrix the graph was built from")
        if len(x.shape) != 2 or int(x.shape[0]) != rows or int(x.shape[1]) < 2:
            raise ValueError(f"x: expected a ({rows}, D >= 2) array, got shape {tuple(x.shape)}")
    elif not isinstance(init, str) and tuple(init.shape) != (rows, 2):
        raise ValueError(f"init: expected shape ({rows}, 2), got {tuple(init.shape)}")
    if a is None:
        a, b = find_ab_params(spread, min_dist)
    dev = device("umap")
    e = empty(dev)
    indptr = dense(graph["indptr"], "indptr", (rows + S,), torch.int64, dev)
    indices = dense(graph["indices"], "indices", (total,), torch.int32, dev) if total else e((1,), torch.int32)
    data = dense(graph["data"], "data", (total,), torch.float64, dev) if total else e((1,), torch.float64)
    off_d, nnz_off_d, epochs_d = upload(off, dev), upload(nnz_off, dev), upload(epochs, dev)
    work = e((max(int(call("mcl_umap_workspace_bytes", total, S)), 8) // 8 + 1,), torch.float64)
    counters = e((S, 2), torch.int64)
    Y = [e((rows, 2), torch.float64), e((rows, 2), torch.float64)]
    sizes = (S, rows, int(seg.min()), int(seg.max()))
    max_epochs, rate, seed64 = int(epochs.max()), int(negative_sample_rate), int(seed) & _MASK
    if isinstance(init, str):
        xd = matrix(x, "x", dev, FLOAT_CODE, torch.float64) if init == "pca" else None
        call("mcl_umap_init", INITS.index(init), xd, xd.stride(0) if xd is not None else 0,
             FLOAT_CODE[xd.dtype] if xd is not None else 1,
             int(xd.shape[1]) if xd is not None else 0, off_d, *sizes, seed64, Y[0])
    else:
        Y[0].copy_(dense(init, "init", (rows, 2), torch.float64, dev))
    call("mcl_umap_prepare", data, nnz_off_d, epochs_d, S, total, int(np.diff(nnz_off).max()), max_epochs, rate, work, counters)
    count = max_epochs if stop_after is None else min(int(stop_after), max_epochs)
    call("mcl_umap_epochs", 0, count, indptr, indices, off_d, nnz_off_d, epochs_d, *sizes, total, max_epochs,
         float(a), float(b), float(gamma), float(alpha), rate, seed64, work, Y[0], Y[1], counters)
    c = counters.cpu().numpy()                         # the one synchronisation
    return {"embedding": Y[count & 1], "attractive_samples": c[:, 0].copy(), "negative_samples": c[:, 1].copy(),
            "n_epochs": epochs, "a": float(a), "b": float(b), "offsets": off}


def umap(x: ArrayLike, offsets: Optional[Sequence[int]] = None, n_neighbors: int = 15, init: Union[str, ArrayLike] = "pca",
         **kw) -> Dict[str, object]:
    """``neighbors.neighbors(x, offsets, n_neighbors)`` then ``layout`` (its keywords): the layout's dict plus ``graph``."""
    check_keywords(init, kw)
    graph = neighbors.neighbors(x, offsets, n_neighbors)
    res = layout(graph, init, x=x, **kw)
    res["graph"] = graph
    return res


def expression_umap(expr: ArrayLike, batch_idx=None, preprocess: bool = True, normalize_and_log: bool = True,
                    n_top_genes: int = neighbors.N_TOP_GENES, n_pcs: int = neighbors.N_PCS,
                    n_neighbors: int = neighbors.N_NEIGHBORS, pca_solver: str = "host", **kw) -> Dict[str, object]:
    """``visualize_umap_clusters`` up to and including ``sc.tl.umap`` on one (spots, genes) matrix:
    ``neighbors.expression_graph`` (its arguments, ``pca_solver`` among them), then ``layout`` (its keywords) started from the PCA scores.  Needs
    ``n_pcs >= 2``.  Returns the layout's dict plus ``graph``, the dict of ``expression_graph``."""
    if n_pcs < 2:
        raise ValueError(f"n_pcs must be at least 2 for the PCA start, got {n_pcs}")
    init = kw.pop("init", "pca")
    check_keywords(init, kw)
    graph = neighbors.expression_graph(expr, batch_idx, preprocess, normalize_and_log, n_top_genes, n_pcs, n_neighbors,
                                       pca_solver)
    res = layout(graph, init, x=graph["scores"], **kw)
    res["graph"] = graph
    return res


# --------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.umap",
                                description="PCA, the exact neighbourhood graph and its UMAP layout, one per slide "
                                            "(BLEEP's visualize_umap_clusters: sc.pp.pca, sc.pp.neighbors, sc.tl.umap)")
    p.add_argument("--pred", required=True, nargs="+", help="one gene-major (genes, spots) .npy per slide")
    p.add_argument("--raw", action="store_true",
                   help="the files hold counts: select highly variable genes and log-normalise them first")
    p.add_argument("--n_top_genes", type=int, default=neighbors.N_TOP_GENES, help="with --raw")
    p.add_argument("--n_neighbors", type=int, default=neighbors.N_NEIGHBORS)
    p.add_argument("--n_pcs", type=int, default=neighbors.N_PCS)
    p.add_argument("--n_epochs", type=int, default=None, help="default: 500 up to 10000 spots, 200 above")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out_dir", required=True, help=f"writes OUT_DIR/<slide number from 1>/{OUT_FILE}")
    a = p.parse_args(argv)
    if not 2 <= a.n_neighbors <= neighbors.MAX_NEIGHBORS:
        p.error(f"--n_neighbors must lie in 2 .. {neighbors.MAX_NEIGHBORS}, got {a.n_neighbors}")
    if not 2 <= a.n_pcs <= neighbors.MAX_DIM:
        p.error(f"--n_pcs must lie in 2 .. {neighbors.MAX_DIM}, got {a.n_pcs}")
    if a.n_epochs is not None and not 1 <= a.n_epochs <= MAX_EPOCHS:
        p.error(f"--n_epochs must lie in 1 .. {MAX_EPOCHS}, got {a.n_epochs}")
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    for i, m in enumerate(_arrays.load_gene_major(a.pred)):
        res = expression_umap(np.ascontiguousarray(m), preprocess=a.raw, n_top_genes=a.n_top_genes, n_pcs=a.n_pcs,
                              n_neighbors=a.n_neighbors, n_epochs=a.n_epochs, seed=a.seed)
        Y = res["embedding"].cpu().numpy()
        path = os.path.join(a.out_dir, str(i + 1))
        os.makedirs(path, exist_ok=True)
        np.save(os.path.join(path, OUT_FILE), Y)
        print(f"slide {i + 1}: {m.shape[0]} spots, epochs {int(res['n_epochs'][0])}, attractions "
              f"{int(res['attractive_samples'][0])}, negative samples {int(res['negative_samples'][0])}, extent "
              f"{float(np.abs(Y).max()):.6g} -> {os.path.join(path, OUT_FILE)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
