"""Spatial-domain clustering of predicted expression on the MI355X: the score the reference's tutorial ends with,
``p, ari, nmi = cluster(adata_pred, label)`` (/root/reference/utils.py:67-79, tutorial.ipynb):

    drop the spots labelled 'undetermined' -> PCA to 9 components -> k-means (k = number of remaining labels) on the
    scores -> ARI and NMI of the clusters against the labels, rounded to 3 decimals

All slides of an evaluation run through ONE ``mcl_pca_gram`` / ``mcl_pca_project`` / ``mcl_kmeans`` /
``mcl_cluster_scores`` call each (csrc/cluster.hip: fp64, deterministic, a slide inside a batch is bit-identical to the same
slide alone).  Host side on purpose: the label strings -> integer codes and the row mask (bookkeeping), and
``numpy.linalg.eigh`` of the one small symmetric Gram matrix per slide -- by default: ``solver="device"`` (``--pca_solver
device``) hands the Gram matrices to ``mclstexp_amd.eig`` instead and they never leave the GPU.  t-SNE, which
the reference computes and never reads, is opt-in (``tsne=True`` / ``--tsne OUT.npz``: ``mclstexp_amd.tsne`` embeds the PCA
scores already at hand; the scores and clusters do not depend on it).  Seeding: the reference's k-means++ draws from NumPy's
``RandomState(0)``; that stream is NOT reproduced -- ``seed_rows`` replays given initial centres exactly, otherwise the
kernel's own k-means++ (counter-based generator) is used, best of ``n_init`` restarts.  No CPU fallback: without a GPU /
the HIP library these functions raise ``RuntimeError``.

    python -m mclstexp_amd.cluster --pred P1.npy ... --labels L1.npy ... [--n_init N] [--json OUT] [--tsne OUT.npz]
                                  [--pca_solver {host,device}] [--method {kmeans,gmm}]
"""
from __future__ import annotations

import argparse
import sys
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _arrays, eig
from ._arrays import FLOAT_CODE, ArrayLike, Tensor, cumulative_offsets, device, empty, matrix, stack_rows, upload, write_json
from ._lib import call

N_COMPS = 9          # sc.pp.pca(tmp, n_comps=9), utils.py:71
MAX_DIM = 64         # D <= 64 and K <= 64 (csrc/cluster.hip)
MAX_ROWS = 50000     # per segment: the pair counts of the ARI stay inside int64
MAX_LABEL = 1024     # label values in [0, 1024)
MAX_TABLE = 12288    # distinct(a) * distinct(b) per segment
SOLVERS = ("host", "device")   # of the PCA's symmetric eigenproblem: numpy.linalg.eigh / mclstexp_amd.eig
METHODS = ("kmeans", "gmm")    # of the clustering of the scores: Lloyd / mclstexp_amd.mixture (full covariance)


def validate_offsets(offsets: Optional[Sequence[int]], rows: int, min_rows: int = 1) -> np.ndarray:
    """offsets[0] = 0, offsets[-1] = rows, every segment holds min_rows .. 50 000 rows.  None: one segment.  int64."""
    return _arrays.validate_offsets(offsets, rows, min_rows, MAX_ROWS, max_segments=65535, none_is_one=True)


def _labels_i32(v: ArrayLike, name: str, dev: torch.device) -> Tensor:
    t = v if isinstance(v, Tensor) else torch.as_tensor(np.asarray(v))
    if t.dim() != 1:
        raise ValueError(f"{name}: expected a 1-D label vector, got shape {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{name}: expected integer labels, got {t.dtype}")
    if not t.is_cuda:
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= MAX_LABEL):
            raise ValueError(f"{name}: label values must lie in [0, {MAX_LABEL})")
        return t.to(torch.int32).contiguous().to(dev)
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError(f"{name}: device labels must be a contiguous int32 vector")
    return t


# ------------------------------------------------------------------------------------------------------------ PCA
def pca_device(x: ArrayLike, offsets: Optional[Sequence[int]] = None, n_comps: int = N_COMPS,
               solver: str = "host") -> Dict[str, object]:
    """PCA scores of every segment of the row-stacked (spots, genes) matrix ``x`` (fp32 / fp64), as sklearn's
    ``PCA(n_comps, svd_solver="arpack").fit_transform`` gives them (scanpy's ``pp.pca`` default): device ``scores``
    (rows, n_comps) fp64 and ``sign`` (S, n_comps); host ``explained_variance`` (S, n_comps) = eigenvalue / (n_s - 1).
    ``solver``: ``"host"`` copies the Gram matrices to the host for ``numpy.linalg.eigh``; ``"device"`` solves for the
    leading eigenpairs on the GPU (``mclstexp_amd.eig``, min(spots, genes) <= 4096 in every segment): the Gram matrices
    never cross to the host, only the certificate and the (S, n_comps) eigenvalues are read back."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if not isinstance(x, Tensor) and np.asarray(x).ndim != 2:
        raise ValueError(f"x: expected a 2-D (spots, genes) array, got shape {np.asarray(x).shape}")
    rows, G = int(x.shape[0]), int(x.shape[1])
    off = validate_offsets(offsets, rows, min_rows=2)
    n_comps = int(n_comps)
    seg = np.diff(off)
    m = np.minimum(seg, G)
    if n_comps < 1 or n_comps > MAX_DIM:
        raise ValueError(f"n_comps must lie in 1 .. {MAX_DIM}, got {n_comps}")
    if n_comps >= int(m.min()):
        raise ValueError(f"n_comps = {n_comps} needs more than {n_comps} spots and genes in every segment "
                         f"(smallest min(spots, genes) = {int(m.min())})")
    if solver == "device" and int(m.max()) > eig.MAX_M:
        raise ValueError(f"solver=\"device\" handles min(spots, genes) <= {eig.MAX_M} per segment, got {int(m.max())}; "
                         f"use solver=\"host\"")
    dev = device("cluster")
    xd = matrix(x, "x", dev, FLOAT_CODE, torch.float64)
    S = off.size - 1
    goff, eoff = cumulative_offsets(m * m), cumulative_offsets(m * n_comps)
    off_d, goff_d = upload(off, dev), upload(goff, dev)
    e = empty(dev)
    mean = e((S, G), torch.float64)
    gram = e((int(goff[-1]),), torch.float64)
    max_rows = int(seg.max())
    call("mcl_pca_gram", xd, xd.stride(0), FLOAT_CODE[xd.dtype], off_d, S, G, max_rows, goff_d, mean, gram)
    if solver == "device":
        res = eig.solve(gram, goff, m, n_comps, evec_offsets=eoff, a_offsets_d=goff_d)      # gram is overwritten
        evec_d, eval_d, eoff_d = res["vectors_flat"], res["values"], res["evec_offsets"]
    else:
        gram_h = gram.cpu().numpy()                      # the one synchronisation of the pipeline
        evec = np.empty((int(eoff[-1]),), dtype=np.float64)
        evals = np.empty((S, n_comps), dtype=np.float64)
        for s in range(S):
            ms = int(m[s])
            w, v = np.linalg.eigh(gram_h[goff[s]:goff[s + 1]].reshape(ms, ms))      # ascending
            evals[s] = w[::-1][:n_comps]
            evec[eoff[s]:eoff[s + 1]] = np.ascontiguousarray(v[:, ::-1][:, :n_comps]).reshape(-1)
        evec_d, eval_d, eoff_d = upload(evec, dev), upload(evals, dev), upload(eoff, dev)
    loadings = e((S * G * n_comps,), torch.float64)
    sign, z = e((S, n_comps), torch.float64), e((rows, n_comps), torch.float64)
    call("mcl_pca_project", xd, xd.stride(0), FLOAT_CODE[xd.dtype], off_d, S,
         G, max_rows, n_comps, mean, evec_d, eoff_d, eval_d, loadings, sign, z)
    if solver == "device":
        eig.check_certificate(res["certificate"].cpu().numpy(), res["sizes"])     # read back after everything is enqueued
        evals = eval_d.cpu().numpy()
    return {"scores": z, "sign": sign, "explained_variance": np.maximum(evals, 0.0) / (seg[:, None] - 1.0),
            "offsets": off}


def pca_scores(x: ArrayLike, offsets: Optional[Sequence[int]] = None, n_comps: int = N_COMPS,
               solver: str = "host") -> Tensor:
    """Device (rows, n_comps) fp64 PCA scores of every segment of ``x`` (see ``pca_device``)."""
    return pca_device(x, offsets, n_comps, solver)["scores"]


def pca_scores_slides(xs: Sequence[ArrayLike], n_comps: int = N_COMPS, solver: str = "host") -> List[Tensor]:
    """One (spots_i, n_comps) device score matrix per slide, all slides in one gram and one project call."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    x, off = stack_rows(xs, "xs", device("cluster"))
    z = pca_scores(x, off, n_comps, solver)
    return [z[off[i]:off[i + 1]] for i in range(len(xs))]


# -------------------------------------------------------------------------------------------------------- k-means
def k_per_segment(k: Union[int, Sequence[int]], seg: np.ndarray) -> np.ndarray:
    """``k`` as int32 per segment: an int stands for every segment; each 1 .. MAX_DIM and at most the segment's rows."""
    ks = np.asarray(k)
    if not np.issubdtype(ks.dtype, np.integer):
        raise ValueError(f"k must be an int or one int per segment, got {k!r}")
    ks = np.full(seg.size, int(ks), dtype=np.int32) if ks.ndim == 0 else ks.astype(np.int32)
    if ks.shape != seg.shape:
        raise ValueError(f"k: {ks.size} values for {seg.size} segments")
    if (ks < 1).any() or (ks > MAX_DIM).any():
        raise ValueError(f"k must lie in 1 .. {MAX_DIM}, got {ks.tolist()}")
    if (ks > seg).any():
        raise ValueError(f"k exceeds the number of rows of its segment: k = {ks.tolist()}, rows = {seg.tolist()}")
    return ks


def _seed_array(seed_rows, ks: np.ndarray, seg: np.ndarray) -> np.ndarray:
    """(S, R, k_max) int64 from (S, R, K) / (R, K) / (K,) arrays or a list of one (R, k_s) / (k_s,) array per segment."""
    S, k_max = ks.size, int(ks.max())
    if isinstance(seed_rows, (list, tuple)):
        nested = len(seed_rows) == S and all(np.ndim(a) >= 1 for a in seed_rows)
        per = [np.asarray(a) for a in seed_rows] if nested else [np.asarray(seed_rows)]
    else:
        arr = np.asarray(seed_rows)
        per = [arr[s] for s in range(arr.shape[0])] if arr.ndim == 3 else [arr]
    if len(per) != S:
        raise ValueError(f"seed_rows: {len(per)} segments given, {S} expected")
    per = [a[None, :] if a.ndim == 1 else a for a in per]
    R = per[0].shape[0]
    out = np.zeros((S, R, k_max), dtype=np.int64)
    for s, a in enumerate(per):
        if a.ndim != 2 or a.shape[0] != R or a.shape[1] < ks[s] or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"seed_rows[{s}]: expected an integer ({R}, {ks[s]}) array, got {a.dtype} {a.shape}")
        a = a[:, :ks[s]]
        if a.size and (a.min() < 0 or a.max() >= seg[s]):
            raise ValueError(f"seed_rows[{s}]: rows must lie inside the segment (0 .. {seg[s] - 1})")
        out[s, :, :ks[s]] = a
    return out


def kmeans(z: ArrayLike, k: Union[int, Sequence[int]], offsets: Optional[Sequence[int]] = None, seed_rows=None,
           n_init: int = 1, seed: int = 0, tol: float = 1e-4, max_iter: int = 300,
           segment_base: int = 0) -> Dict[str, Tensor]:
    """Lloyd k-means (sklearn's ``KMeans(algorithm="lloyd")`` iteration and stopping rule) of every segment of the
    row-stacked (rows, D <= 64) matrix ``z``; ``k`` an int or one int per segment.  ``seed_rows``: the rows (inside each
    segment) of the initial centres, (S, R, K) -- replayed exactly, R restarts; without it the kernel's own k-means++ draws
    ``n_init`` restarts from ``seed`` (generator keyed by (seed, segment_base + s, restart, draw)).  Device tensors:
    ``labels`` (rows,) int32, ``centers`` (S, k_max, D), ``inertia`` (S,), ``n_iter`` (S,), ``restart`` (S,) of the best
    restart per segment, and per restart ``inertia_all`` (S, R), ``n_iter_all`` (S, R), ``labels_all`` (R, rows),
    ``centers_all`` (S, R, k_max, D), ``seed_rows`` (S, R, k_max)."""
    if not isinstance(z, Tensor) and np.asarray(z).ndim != 2:
        raise ValueError(f"z: expected a 2-D (rows, D) array, got shape {np.asarray(z).shape}")
    rows, D = int(z.shape[0]), int(z.shape[1])
    if D < 1 or D > MAX_DIM:
        raise ValueError(f"z has {D} columns; the kernel handles 1 .. {MAX_DIM}")
    off = validate_offsets(offsets, rows)
    seg = np.diff(off)
    ks = k_per_segment(k, seg)
    S, k_max = ks.size, int(ks.max())
    if not (tol >= 0.0) or int(max_iter) < 1:
        raise ValueError(f"tol must be >= 0 and max_iter >= 1, got {tol}, {max_iter}")
    seeds_h = None
    if seed_rows is not None:
        seeds_h = _seed_array(seed_rows, ks, seg)
        R = seeds_h.shape[1]
    else:
        R = int(n_init)
    if R < 1 or R > 65535:
        raise ValueError(f"the number of restarts must lie in 1 .. 65535, got {R}")
    dev = device("cluster")
    zd = matrix(z, "z", dev, FLOAT_CODE, torch.float64)
    if zd.dtype != torch.float64:
        raise ValueError("z must be float64 (the PCA scores are)")
    off_d, ks_d = upload(off, dev), upload(ks, dev)
    seeds_d = upload(seeds_h, dev) if seeds_h is not None else None
    e = empty(dev)
    res = {"seed_rows": e((S, R, k_max), torch.int64), "labels_all": e((R, rows), torch.int32),
           "centers_all": e((S, R, k_max, D), torch.float64), "inertia_all": e((S, R), torch.float64),
           "n_iter_all": e((S, R), torch.int32), "labels": e((rows,), torch.int32),
           "centers": e((S, k_max, D), torch.float64), "inertia": e((S,), torch.float64),
           "n_iter": e((S,), torch.int32), "restart": e((S,), torch.int32)}
    work = e((R * rows,), torch.float64)
    call("mcl_kmeans", zd, zd.stride(0), off_d, S, rows, D, ks_d, k_max, R, seeds_d,
         int(seed) & 0xFFFFFFFFFFFFFFFF, int(segment_base), float(tol), int(max_iter), res["seed_rows"],
         res["labels_all"], res["centers_all"], res["inertia_all"], res["n_iter_all"], work,
         res["labels"], res["centers"], res["inertia"], res["n_iter"], res["restart"])
    return res


# ---------------------------------------------------------------------------------------------------------- scores
def cluster_scores(labels_a: ArrayLike, labels_b: ArrayLike,
                   offsets: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(ari, nmi), one unrounded fp64 value per segment: sklearn's ``adjusted_rand_score`` and
    ``normalized_mutual_info_score`` of two integer label vectors (values in [0, 1024))."""
    na, nb = int(labels_a.shape[0]) if hasattr(labels_a, "shape") else len(labels_a), \
        int(labels_b.shape[0]) if hasattr(labels_b, "shape") else len(labels_b)
    if na != nb:
        raise ValueError(f"label vectors differ in length: {na} and {nb}")
    off = validate_offsets(offsets, na)
    dev = device("cluster")
    a = _labels_i32(labels_a, "labels_a", dev)
    b = _labels_i32(labels_b, "labels_b", dev)
    S = off.size - 1
    off_d = upload(off, dev)
    out = torch.empty((S, 2), device=dev, dtype=torch.float64)
    call("mcl_cluster_scores", a, b, off_d, S, int(np.diff(off).max()), out)
    h = out.cpu().numpy()
    return h[:, 0].copy(), h[:, 1].copy()


# ------------------------------------------------------------------------------------------- the reference's cluster()
def encode_labels(label: Sequence, undetermined="undetermined") -> Tuple[np.ndarray, np.ndarray, int]:
    """Host bookkeeping of cluster(): the mask ``label != undetermined``, the integer codes of the kept labels (index
    into their sorted distinct values) and k = the number of distinct kept labels."""
    lab = np.asarray(label)
    if lab.ndim != 1:
        raise ValueError(f"label: expected a 1-D vector, got shape {lab.shape}")
    idx = lab != undetermined
    idx = np.broadcast_to(np.asarray(idx, dtype=bool), lab.shape).copy()
    kept = lab[idx]
    if kept.size == 0:
        raise ValueError("no spot is left after dropping the undetermined ones")
    uniq, codes = np.unique(kept, return_inverse=True)
    return idx, codes.astype(np.int32).reshape(-1), int(uniq.size)


def _take_rows(x: ArrayLike, idx: np.ndarray, dev: torch.device) -> ArrayLike:
    """The kept rows of a slide.  Host arrays are indexed on the host; a device tensor is copied run by run (plain
    copies: no gather kernel of another library)."""
    if idx.all():
        return x
    if not isinstance(x, Tensor):
        return np.asarray(x)[idx]
    if not x.is_cuda:
        return x[torch.from_numpy(idx)]
    keep = np.flatnonzero(idx)
    out = torch.empty((keep.size, x.shape[1]), device=x.device, dtype=x.dtype)
    cuts = np.flatnonzero(np.diff(keep) != 1) + 1
    pos = 0
    for run in np.split(keep, cuts):
        out[pos:pos + run.size].copy_(x[int(run[0]):int(run[-1]) + 1])
        pos += run.size
    return out


def cluster_slides(preds: Sequence[ArrayLike], labels: Sequence[Sequence], undetermined="undetermined",
                   n_comps: int = N_COMPS, seed_rows=None, n_init: int = 1, seed: int = 0, tol: float = 1e-4,
                   max_iter: int = 300, segment_base: int = 0, tsne: Union[bool, dict] = False,
                   solver: str = "host", method: str = "kmeans") -> Dict[str, object]:
    """cluster() for every slide of an evaluation in ONE gram / ONE project / ONE kmeans / ONE scores call.
    ``preds[i]``: (spots_i, genes) predicted expression, ``labels[i]``: (spots_i,) annotations.  Returns ``slides``: per
    slide ``p`` (cluster index per kept spot, int32), ``ari``, ``nmi`` (rounded to 3 decimals as the reference does),
    ``ari_raw``, ``nmi_raw``, ``k``, ``inertia``, ``n_iter``, ``restart``; and ``ari``, ``nmi``: the means over slides of
    the rounded values.  ``tsne`` (True, or a dict of ``mclstexp_amd.tsne.tsne`` arguments): every slide also gets ``tsne``,
    the (kept spots, 2) exact t-SNE embedding of its PCA scores (the reference's ``sc.tl.tsne``), as a numpy array;
    everything else is what ``tsne=False`` gives.  ``solver``: the PCA's eigensolver (see ``pca_device``).  ``method``:
    ``"gmm"`` hands the labels of every k-means restart to ``mclstexp_amd.mixture.gmm`` (full covariance, its default
    ``tol`` / ``max_iter``) as starts and scores the mixture's labels: ``restart`` is then the start of highest lower
    bound, ``n_iter`` EM's, ``inertia`` NaN, and every slide also gets ``lower_bound`` and ``bic``."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if len(preds) != len(labels) or not len(preds):
        raise ValueError(f"need one label vector per prediction and >= 1 slide; got {len(preds)} and {len(labels)}")
    enc = []
    for i, (p, l) in enumerate(zip(preds, labels)):
        if len(p.shape) != 2 or p.shape[0] != len(l):
            raise ValueError(f"slide {i}: prediction {tuple(p.shape)} and {len(l)} labels do not match")
        enc.append(encode_labels(l, undetermined))
    ks = np.array([e[2] for e in enc], dtype=np.int32)
    if (ks > MAX_DIM).any():
        raise ValueError(f"at most {MAX_DIM} distinct labels per slide, got {ks.tolist()}")
    dev = device("cluster")
    x, off = stack_rows([_take_rows(p, e[0], dev) for p, e in zip(preds, enc)], "preds", dev)
    k_per_segment(ks, np.diff(off))
    z = pca_scores(x, off, n_comps, solver)
    km = kmeans(z, ks, off, seed_rows=seed_rows, n_init=n_init, seed=seed, tol=tol, max_iter=max_iter,
                segment_base=segment_base)
    if method == "gmm":
        from . import mixture                         # mixture imports this module
        gm = mixture.gmm(z, ks, off, init_labels=km["labels_all"])
        km = {"labels": gm["labels"], "inertia": torch.full_like(gm["lower_bound"], float("nan")), "n_iter": gm["n_iter"],
              "restart": gm["restart"]}
    truth = upload(np.concatenate([e[1] for e in enc]), dev)
    ari, nmi = cluster_scores(truth, km["labels"], off)
    p_all = km["labels"].cpu().numpy()
    inertia, n_iter, restart = km["inertia"].cpu().numpy(), km["n_iter"].cpu().numpy(), km["restart"].cpu().numpy()
    slides = [{"p": p_all[off[i]:off[i + 1]].copy(), "ari": round(float(ari[i]), 3), "nmi": round(float(nmi[i]), 3),
               "ari_raw": float(ari[i]), "nmi_raw": float(nmi[i]), "k": int(ks[i]), "inertia": float(inertia[i]),
               "n_iter": int(n_iter[i]), "restart": int(restart[i])} for i in range(len(preds))]
    if method == "gmm":
        lower_bound, bic = gm["lower_bound"].cpu().numpy(), gm["bic"].cpu().numpy()
        for i, s in enumerate(slides):
            s["lower_bound"], s["bic"] = float(lower_bound[i]), float(bic[i])
    if tsne is not False and tsne is not None:
        from . import tsne as tsne_module             # tsne imports this module
        emb = tsne_module.tsne(z, off, **(tsne if isinstance(tsne, dict) else {}))["embedding"].cpu().numpy()
        for i, s in enumerate(slides):
            s["tsne"] = emb[off[i]:off[i + 1]].copy()
    return {"slides": slides, "ari": float(np.mean([s["ari"] for s in slides])),
            "nmi": float(np.mean([s["nmi"] for s in slides]))}


def cluster(pred: ArrayLike, label: Sequence, undetermined="undetermined", n_comps: int = N_COMPS, seed_rows=None,
            n_init: int = 1, seed: int = 0, tsne: Union[bool, dict] = False, solver: str = "host",
            method: str = "kmeans") -> tuple:
    """The reference's ``cluster(adata, label)`` -> ``(p, ari, nmi)``: ``p`` the cluster index of every kept spot,
    ``ari`` / ``nmi`` rounded to 3 decimals.  ``seed_rows`` (n_restarts, k) or (k,): initial centres as rows of the kept
    spots.  ``tsne`` (see ``cluster_slides``): ``(p, ari, nmi, embedding)``.  ``solver``: see ``pca_device``; ``method``: see
    ``cluster_slides``."""
    if seed_rows is not None:
        seed_rows = [np.asarray(seed_rows)]
    s = cluster_slides([pred], [label], undetermined, n_comps, seed_rows, n_init, seed, tsne=tsne,
                       solver=solver, method=method)["slides"][0]
    if "tsne" in s:
        return s["p"], s["ari"], s["nmi"], s["tsne"]
    return s["p"], s["ari"], s["nmi"]


# --------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.cluster",
                                description="PCA + k-means clustering of predicted expression, scored against "
                                            "annotations by ARI / NMI (the reference's utils.cluster)")
    p.add_argument("--pred", required=True, nargs="+", help="one (spots, genes) .npy per slide")
    p.add_argument("--labels", required=True, nargs="+", help="one (spots,) .npy of annotations per slide, same order")
    p.add_argument("--undetermined", default="undetermined", help="the annotation to drop (default: undetermined)")
    p.add_argument("--n_comps", type=int, default=N_COMPS)
    p.add_argument("--n_init", type=int, default=1, help="k-means restarts, the best inertia wins")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--json", default=None, help="also write per-slide and mean scores to this file")
    p.add_argument("--tsne", default=None, metavar="OUT.npz",
                   help="also embed every slide's PCA scores by exact t-SNE and write slide_<i> arrays (kept spots, 2)")
    p.add_argument("--pca_solver", choices=SOLVERS, default="host",
                   help="eigensolver of the PCA: numpy.linalg.eigh on the host (default) or mclstexp_amd.eig on the GPU")
    p.add_argument("--method", choices=METHODS, default="kmeans",
                   help="cluster the PCA scores by k-means (default) or by a Gaussian mixture started from it")
    a = p.parse_args(argv)
    if len(a.pred) != len(a.labels):
        p.error(f"{len(a.pred)} --pred files but {len(a.labels)} --labels files")
    return a


def format_report(res: Dict[str, object]) -> str:
    """One line per slide in the tutorial's format, then the mean."""
    lines = [f"ARI: {s['ari']}, NMI: {s['nmi']}" for s in res["slides"]]
    lines.append(f"mean ARI: {res['ari']:.3f}, mean NMI: {res['nmi']:.3f}")
    return "\n".join(lines)


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    preds = [np.load(f) for f in a.pred]
    labels = [np.load(f, allow_pickle=False) for f in a.labels]
    res = cluster_slides(preds, labels, a.undetermined, a.n_comps, None, a.n_init, a.seed, tsne=a.tsne is not None,
                         solver=a.pca_solver, method=a.method)
    print(format_report(res))
    if a.tsne:
        np.savez(a.tsne, **{f"slide_{i}": s.pop("tsne") for i, s in enumerate(res["slides"])})
    if a.json:
        doc = {"ari": res["ari"], "nmi": res["nmi"], "n_comps": a.n_comps, "n_init": a.n_init, "seed": a.seed,
               "slides": [{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
                          for s in res["slides"]]}
        write_json(a.json, doc)
    return 0


if __name__ == "__main__":
    sys.exit(main())
