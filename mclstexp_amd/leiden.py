"""Leiden clustering of the spot neighbourhood graph on the MI355X: what ``sc.tl.leiden`` leaves in ``obs["leiden"]`` -- the
last step of BLEEP's ``visualize_umap_clusters`` (baselines/Bleep/BLEEP_inference.ipynb: ``sc.pp.pca``, ``sc.pp.neighbors``,
``sc.tl.umap``, ``sc.tl.leiden``, then ``n_clusters`` is printed and the UMAP coloured by ``leiden``) and of THItoGene's
``utils`` -- for all slides of an evaluation per call.

What is computed is stated in DESIGN 6.13 and restated in numpy by ``tests/leiden_reference.py``; it is that statement, not
a leidenalg release (leidenalg is sequential and randomised).  Things to know:

* The quality is scanpy's default, ``RBConfigurationVertexPartition`` on the connectivities with ``resolution``.
* Weights are fixed point per slide, q = rint(w 2^e) with e = 61 - ex - ceil(log2(nnz)) and the largest weight below 2^ex:
  every sum of weights is an exact int64, so nothing depends on an order of summation.  An entry whose q is 0 is no edge.
* Local moving is one Jacobi sweep per launch: every vertex decides from the labels the sweep started with, moves only to
  a smaller community id on even sweeps and a larger one on odd sweeps, and the sweep is kept only if Q rose strictly.
  Refinement is Jacobi rounds inside each community (greedy, the theta -> 0 limit of Leiden's random choice), a round kept
  only if Q rose strictly.  Refined communities become the nodes of the next level, which starts from the partition of
  local moving.  Every returned community is connected.
* ``n_iterations=-1`` restarts from the partition found until an iteration accepts no sweep.
* Labels are renumbered by descending size per slide, ties to the smaller smallest member: cluster 0 is the largest.
* 2 <= n_s <= 16384 rows per slide, at most 65535 slides.  ``max_levels`` levels per iteration and ``max_sweeps`` sweeps
  (rounds) per phase are caps: reaching one raises.
* Acceptance happens on the device; the host reads one 128-byte record per slide after every ``BATCH`` sweeps or rounds and
  after every aggregation.

Bit-reproducible run to run, free of floating-point atomics; a slide inside a batch is bit-identical to the same slide
alone.  No CPU fallback.

    python -m mclstexp_amd.leiden --pred P1.npy ... [--raw] [--n_neighbors 150] [--n_pcs 50] [--resolution 1.0] [--umap] --out_dir D
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _arrays, neighbors, umap
from ._arrays import ArrayLike, Tensor, check_int, dense, device, empty, upload
from ._lib import call

MAX_ROWS = 16384         # csrc/leiden.hip
MAX_SEGMENTS = 65535
CUT = 512                # rows with more entries take the dense path (LD_CUT)
MAX_LEVELS, MAX_SWEEPS, MAX_ITERATIONS = 32, 512, 64
BATCH = 8                # sweeps (rounds) enqueued between two reads of the state records
OUT_FILE = "leiden.npy"
# the state record of csrc/leiden.hip (ld_state) and the slots of its f
STATE = np.dtype([("Q", "<f8"), ("QR", "<f8"), ("m2", "<i8"), ("scratch", "<i8"), ("f", "<i4", (24,))])
(F_N, F_SHIFT, F_CUR, F_RCUR, F_PARITY, F_FAILS, F_MOVE_DONE, F_REF_DONE, F_FINISHED, F_LEVEL_ACC, F_SWEEPS, F_ACCEPTED, F_ROUNDS,
 F_LEVELS, F_PHASE, F_ERROR, F_N_NEXT, F_MAX_ROW, F_N0) = range(19)
_KEYWORDS = ("resolution", "n_iterations", "partition", "max_levels", "max_sweeps")


# ------------------------------------------------------------------------------------------------------- host rules
def _check_params(resolution, n_iterations=-1, max_levels=MAX_LEVELS, max_sweeps=MAX_SWEEPS) -> None:
    if isinstance(resolution, bool) or not isinstance(resolution, (int, float, np.integer, np.floating)):
        raise ValueError(f"resolution must be a number, got {resolution!r}")
    if not math.isfinite(float(resolution)) or not float(resolution) > 0:
        raise ValueError(f"resolution must be finite and positive, got {resolution!r}")
    if isinstance(n_iterations, bool) or not isinstance(n_iterations, (int, np.integer)) or n_iterations == 0 or n_iterations < -1:
        raise ValueError(f"n_iterations must be -1 (until nothing changes) or a positive integer, got {n_iterations!r}")
    check_int(max_levels, "max_levels", 1)
    check_int(max_sweeps, "max_sweeps", 1)


def _check_keywords(kw: Dict[str, object]) -> None:
    unknown = set(kw) - set(_KEYWORDS)
    if unknown:
        raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
    _check_params(kw.get("resolution", 1.0), kw.get("n_iterations", -1), kw.get("max_levels", MAX_LEVELS),
                  kw.get("max_sweeps", MAX_SWEEPS))


def _check_labels(labels, rows: int, name: str) -> None:
    shape = tuple(labels.shape) if hasattr(labels, "shape") else None
    if shape != (rows,):
        raise ValueError(f"{name}: expected shape ({rows},), got {shape}")
    dt = labels.dtype
    integer = (dt in (torch.int32, torch.int64)) if isinstance(labels, Tensor) else np.issubdtype(dt, np.integer)
    if not integer or dt in (np.bool_, torch.bool):
        raise ValueError(f"{name}: expected integer community ids, got dtype {dt}")
    if not isinstance(labels, Tensor) and (np.asarray(labels) < 0).any():
        raise ValueError(f"{name}: community ids must not be negative")


def canonical(labels, offsets: np.ndarray) -> np.ndarray:
    """Per slide every id replaced by the smallest row (within the slide) that carries it: int32 on the host."""
    lab = labels.cpu().numpy() if isinstance(labels, Tensor) else np.asarray(labels)
    if (lab < 0).any():
        raise ValueError("community ids must not be negative")
    out = np.empty(lab.size, dtype=np.int32)
    for s in range(offsets.size - 1):
        _, idx, inv = np.unique(lab[offsets[s]:offsets[s + 1]], return_index=True, return_inverse=True)
        out[offsets[s]:offsets[s + 1]] = idx[inv.ravel()]
    return out


# ----------------------------------------------------------------------------------------------------------- device
class _Run:
    """The device side of one call: the graph's tensors, the workspace and the launches."""

    def __init__(self, graph: Dict[str, object], resolution: float, max_levels: int = MAX_LEVELS, max_sweeps: int = MAX_SWEEPS):
        off, nnz_off = umap.check_graph(graph)
        self.off, self.seg = off, np.diff(off)
        self.S, self.rows, self.total = int(self.seg.size), int(off[-1]), int(nnz_off[-1])
        self.max_n, self.gamma = int(self.seg.max()), float(resolution)
        self.max_levels, self.max_sweeps = int(max_levels), int(max_sweeps)
        dev = self.dev = device("leiden")
        e = empty(dev)
        S, rows, total = self.S, self.rows, self.total
        self.indptr = dense(graph["indptr"], "indptr", (rows + S,), torch.int64, dev)
        self.indices = dense(graph["indices"], "indices", (total,), torch.int32, dev) if total else e((1,), torch.int32)
        self.data = dense(graph["data"], "data", (total,), torch.float64, dev) if total else e((1,), torch.float64)
        self.off_d, self.nnz_off_d = upload(off, dev), upload(nnz_off, dev)
        nbytes = int(call("mcl_leiden_workspace_bytes", rows, total, S, self.max_n))
        self.work = e((nbytes // 8 + 1,), torch.int64)
        self.long0 = bool(total) and int((self.indptr[1:] - self.indptr[:-1]).max()) > CUT
        self.graph_args = (self.indptr, self.indices, self.off_d, self.nnz_off_d, S, rows, self.max_n, total)

    def state(self) -> np.ndarray:
        """The per-slide records: the synchronisation between batches of launches."""
        st = self.work[:self.S * 16].cpu().numpy().view(STATE)
        err = st["f"][:, F_ERROR]
        if (err == 2).any():
            raise RuntimeError(f"mclstexp_amd.leiden: the offsets of slide {int(np.flatnonzero(err == 2)[0])} do not fit the graph")
        if (err == 1).any():
            raise RuntimeError(f"mclstexp_amd.leiden: slide {int(np.flatnonzero(err == 1)[0])} reached a cap (max_levels = "
                               f"{self.max_levels} levels, max_sweeps = {self.max_sweeps} sweeps or rounds per phase)")
        return st

    def init(self, partition: Optional[Tensor], active: Optional[Tensor]) -> np.ndarray:
        call("mcl_leiden_init", self.indptr, self.indices, self.data, self.off_d, self.nnz_off_d, self.S, self.rows, self.max_n,
             self.total, self.gamma, partition, active, self.work)
        return self.state()

    def _sizes(self, st: np.ndarray, level: int):
        live = st["f"][:, F_FINISHED] == 0
        n_cur = int(st["f"][live, F_N].max())
        long_rows = self.long0 if level == 0 else bool((st["f"][live, F_MAX_ROW] > CUT).any())
        return n_cur, int(long_rows)

    def move(self, st: np.ndarray, level: int) -> np.ndarray:
        n_cur, long_rows = self._sizes(st, level)
        while True:
            call("mcl_leiden_move_sweeps", BATCH, level, n_cur, long_rows, self.max_sweeps, *self.graph_args, self.gamma,
                 self.work)
            st = self.state()
            if ((st["f"][:, F_MOVE_DONE] != 0) | (st["f"][:, F_FINISHED] != 0)).all():
                return st

    def refine(self, st: np.ndarray, level: int) -> np.ndarray:
        n_cur, long_rows = self._sizes(st, level)
        begin = 1
        while True:
            call("mcl_leiden_refine_rounds", begin, BATCH, level, n_cur, long_rows, self.max_sweeps, *self.graph_args,
                 self.gamma, self.work)
            begin = 0
            st = self.state()
            if ((st["f"][:, F_REF_DONE] != 0) | (st["f"][:, F_FINISHED] != 0)).all():
                return st

    def aggregate(self, st: np.ndarray, level: int) -> np.ndarray:
        n_cur, _ = self._sizes(st, level)
        call("mcl_leiden_aggregate", level, n_cur, self.max_levels, *self.graph_args, self.gamma, self.work)
        return self.state()

    def finish(self, source: int, final: int, active, canon: Tensor, labels=None, n_clusters=None) -> None:
        call("mcl_leiden_finish", source, final, active, *self.graph_args, self.work, canon, labels, n_clusters)

    def iteration(self, partition: Optional[Tensor], active: Tensor, canon: Tensor) -> np.ndarray:
        """One pass over the levels for the active slides from ``partition``; their canonical ids land in ``canon``."""
        st = self.init(partition, active)
        level = 0
        while not (st["f"][:, F_FINISHED] != 0).all():
            st = self.move(st, level)
            st = self.refine(st, level)
            st = self.aggregate(st, level)
            level += 1
        self.finish(0, 0, active, canon)
        return st


def leiden(graph: Dict[str, object], resolution: float = 1.0, n_iterations: int = -1, partition: Optional[ArrayLike] = None,
           max_levels: int = MAX_LEVELS, max_sweeps: int = MAX_SWEEPS) -> Dict[str, object]:
    """The clustering of every slide of ``graph`` (the dict of ``neighbors.neighbors`` / ``connectivities`` /
    ``umap.from_scipy``; see the module docstring).  ``partition``: (rows,) integer ids to start from (default: every vertex
    alone).  Returns ``labels`` (rows,) int32 on the device and, per slide on the host, ``n_clusters``, ``modularity``
    (fp64), ``levels``, ``sweeps``, ``accepted_sweeps``, ``rounds``, ``iterations`` and ``offsets``."""
    _check_params(resolution, n_iterations, max_levels, max_sweeps)
    off, _ = umap.check_graph(graph)
    rows = int(off[-1])
    start = None
    if partition is not None:
        _check_labels(partition, rows, "partition")
        start = canonical(partition, off)
    run = _Run(graph, resolution, max_levels, max_sweeps)
    S, dev = run.S, run.dev
    e = empty(dev)
    canon = e((rows,), torch.int32)
    totals = {k: np.zeros(S, dtype=np.int64) for k in ("levels", "sweeps", "accepted_sweeps", "rounds", "iterations")}
    active = np.ones(S, dtype=bool)
    P0 = upload(start, dev) if start is not None else None
    while active.any():
        if int(totals["iterations"].max()) >= MAX_ITERATIONS:
            raise RuntimeError(f"mclstexp_amd.leiden: the iterations did not end within {MAX_ITERATIONS}")
        st = run.iteration(P0, upload(active.astype(np.int32), dev), canon)
        ran = active & (st["m2"] > 0)
        f = st["f"]
        for key, slot in (("levels", F_LEVELS), ("sweeps", F_SWEEPS), ("accepted_sweeps", F_ACCEPTED), ("rounds", F_ROUNDS)):
            totals[key][ran] += f[ran, slot]
        totals["iterations"][ran] += 1
        active = ran & (f[:, F_ACCEPTED] > 0) & (totals["iterations"] != n_iterations)
        P0 = canon
    labels, n_clusters = e((rows,), torch.int32), e((S,), torch.int32)
    run.finish(0, 1, None, canon, labels, n_clusters)
    quality = run.init(canon, None)["Q"].copy()
    res = {"labels": labels, "n_clusters": n_clusters.cpu().numpy(), "modularity": quality, "offsets": off}
    res.update(totals)
    return res


def modularity(graph: Dict[str, object], labels: ArrayLike, resolution: float = 1.0) -> np.ndarray:
    """Q of ``labels`` ((rows,) integer ids, host or device) per slide, computed by the kernels of ``leiden``: (S,) fp64."""
    _check_params(resolution)
    off, _ = umap.check_graph(graph)
    _check_labels(labels, int(off[-1]), "labels")
    start = canonical(labels, off)
    run = _Run(graph, resolution)
    return run.init(upload(start, run.dev), None)["Q"].copy()


def refine(graph: Dict[str, object], partition: ArrayLike, resolution: float = 1.0) -> Tensor:
    """The refinement of ``partition`` at level 0: (rows,) int32 on the device, every vertex labelled by the smallest row (within
    its slide) of its refined community.  Each refined community lies inside one community of ``partition`` and is connected."""
    _check_params(resolution)
    off, _ = umap.check_graph(graph)
    _check_labels(partition, int(off[-1]), "partition")
    start = canonical(partition, off)
    run = _Run(graph, resolution)
    st = run.init(upload(start, run.dev), None)
    if not (st["f"][:, F_FINISHED] != 0).all():
        run.refine(st, 0)
    out = torch.empty((run.rows,), device=run.dev, dtype=torch.int32)
    run.finish(1, 0, None, out)
    return out


def cluster(x: ArrayLike, offsets: Optional[Sequence[int]] = None, n_neighbors: int = 15, **kw) -> Dict[str, object]:
    """``neighbors.neighbors(x, offsets, n_neighbors)`` then ``leiden`` (its keywords): the clustering's dict plus ``graph``."""
    _check_keywords(kw)
    graph = neighbors.neighbors(x, offsets, n_neighbors)
    res = leiden(graph, **kw)
    res["graph"] = graph
    return res


def expression_clusters(expr: ArrayLike, batch_idx=None, preprocess: bool = True, normalize_and_log: bool = True,
                        n_top_genes: int = neighbors.N_TOP_GENES, n_pcs: int = neighbors.N_PCS,
                        n_neighbors: int = neighbors.N_NEIGHBORS, layout: bool = True, umap_kw: Optional[Dict[str, object]] = None,
                        pca_solver: str = "host", **kw) -> Dict[str, object]:
    """``visualize_umap_clusters`` on one (spots, genes) matrix: ``neighbors.expression_graph`` (its arguments,
    ``pca_solver`` among them), with
    ``layout`` the UMAP layout started from the PCA scores (``umap_kw``: keywords of ``umap.layout``), and ``leiden`` (its
    keywords) on the same graph.  Returns the clustering's dict plus ``graph`` and ``embedding`` (None without ``layout``)."""
    _check_keywords(kw)
    umap_kw = dict(umap_kw or {})
    if layout:
        if n_pcs < 2:
            raise ValueError(f"n_pcs must be at least 2 for the PCA start of the layout, got {n_pcs}")
        umap.check_keywords(umap_kw.get("init", "pca"), {k: v for k, v in umap_kw.items() if k != "init"})
    graph = neighbors.expression_graph(expr, batch_idx, preprocess, normalize_and_log, n_top_genes, n_pcs, n_neighbors,
                                       pca_solver)
    embedding = None
    if layout:
        init = umap_kw.pop("init", "pca")
        embedding = umap.layout(graph, init, x=graph["scores"], **umap_kw)["embedding"]
    res = leiden(graph, **kw)
    res["graph"], res["embedding"] = graph, embedding
    return res


# --------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.leiden",
                                description="PCA, the exact neighbourhood graph and its Leiden clustering, one per slide "
                                            "(BLEEP's visualize_umap_clusters: sc.pp.pca, sc.pp.neighbors, sc.tl.leiden)")
    p.add_argument("--pred", required=True, nargs="+", help="one gene-major (genes, spots) .npy per slide")
    p.add_argument("--raw", action="store_true",
                   help="the files hold counts: select highly variable genes and log-normalise them first")
    p.add_argument("--n_top_genes", type=int, default=neighbors.N_TOP_GENES, help="with --raw")
    p.add_argument("--n_neighbors", type=int, default=neighbors.N_NEIGHBORS)
    p.add_argument("--n_pcs", type=int, default=neighbors.N_PCS)
    p.add_argument("--resolution", type=float, default=1.0)
    p.add_argument("--n_iterations", type=int, default=-1, help="-1: until an iteration changes nothing")
    p.add_argument("--umap", action="store_true", help=f"also lay the graph out and write {umap.OUT_FILE}")
    p.add_argument("--n_epochs", type=int, default=None, help="with --umap; default: 500 up to 10000 spots, 200 above")
    p.add_argument("--seed", type=int, default=0, help="with --umap")
    p.add_argument("--out_dir", required=True, help=f"writes OUT_DIR/<slide number from 1>/{OUT_FILE}")
    a = p.parse_args(argv)
    if not 2 <= a.n_neighbors <= neighbors.MAX_NEIGHBORS:
        p.error(f"--n_neighbors must lie in 2 .. {neighbors.MAX_NEIGHBORS}, got {a.n_neighbors}")
    if not 2 <= a.n_pcs <= neighbors.MAX_DIM:
        p.error(f"--n_pcs must lie in 2 .. {neighbors.MAX_DIM}, got {a.n_pcs}")
    if not (math.isfinite(a.resolution) and a.resolution > 0):
        p.error(f"--resolution must be finite and positive, got {a.resolution}")
    if a.n_iterations == 0 or a.n_iterations < -1:
        p.error(f"--n_iterations must be -1 or positive, got {a.n_iterations}")
    if a.n_epochs is not None and not 1 <= a.n_epochs <= umap.MAX_EPOCHS:
        p.error(f"--n_epochs must lie in 1 .. {umap.MAX_EPOCHS}, got {a.n_epochs}")
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    for i, m in enumerate(_arrays.load_gene_major(a.pred)):
        res = expression_clusters(np.ascontiguousarray(m), preprocess=a.raw, n_top_genes=a.n_top_genes, n_pcs=a.n_pcs,
                                  n_neighbors=a.n_neighbors, layout=a.umap, umap_kw={"n_epochs": a.n_epochs, "seed": a.seed},
                                  resolution=a.resolution, n_iterations=a.n_iterations)
        path = os.path.join(a.out_dir, str(i + 1))
        os.makedirs(path, exist_ok=True)
        np.save(os.path.join(path, OUT_FILE), res["labels"].cpu().numpy())
        if a.umap:
            np.save(os.path.join(path, umap.OUT_FILE), res["embedding"].cpu().numpy())
        print(f"slide {i + 1}: {m.shape[0]} spots")
        print(f"n_clusters:  {int(res['n_clusters'][0])}")
        print(f"modularity {float(res['modularity'][0]):.6f}, levels {int(res['levels'][0])}, sweeps "
              f"{int(res['sweeps'][0])} ({int(res['accepted_sweeps'][0])} accepted), rounds {int(res['rounds'][0])}, iterations "
              f"{int(res['iterations'][0])} -> {os.path.join(path, OUT_FILE)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
