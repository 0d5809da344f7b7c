"""Spatial domains on the MI355X: Gaussian mixtures of the PCA scores with a Potts prior on the labels over the spot lattice
(a hidden Markov random field), so that neighbouring spots tend to share a domain -- what BayesSpace, Giotto's HMRF and
SpaGCN's refinement exist for.  ``mixture.gmm`` is the same model at ``beta = 0``.

What is computed is stated in DESIGN 6.18 and restated in numpy by ``tests/hmrf_reference.py``: EM with the mean-field
approximation of Celeux, Forbes and Peyrard (2003) in synchronous sweeps -- during iteration t the neighbours' memberships
are the responsibilities of iteration t - 1.  Parity with BayesSpace, Giotto or SpaGCN is unpinned.  Things to know:

* ``hmrf``: every slide x start in ONE ``mcl_hmrf_fit`` call, one workgroup per problem.  ``graph`` is what
  ``spatial.lattice`` returns (its ``offsets`` are the slides); it is used as given: a kNN list is directed, so the model is
  defined by its conditionals (``prune="Grid"`` on grid coordinates gives symmetric lists).  With binary weights
  (``row_standardise=False``) ``beta`` is the bonus per agreeing neighbour; row-standardised weights need ``beta * deg``
  for the same fit.  ``lower_bound`` is the mean-field pseudo-log-likelihood, mean_i (lse_i - za_i); it is not monotone
  under synchronous sweeps, and ``converged = 0`` after ``max_iter`` is an ordinary result.  ``bic`` / ``aic`` are computed
  from that pseudo-likelihood.  D <= 64, k <= 64, k <= n_s <= 16 384, at most 64 neighbour slots.
* ``scan_beta``: every candidate beta of every slide in one ``hmrf`` call.  It chooses nothing: there is no agreed
  criterion for beta.
* ``refine_labels``: synchronous rounds of neighbourhood majority relabelling (shaped after SpaGCN's ``refine``) for labels
  from any caller; ``edge_agreement``: the weighted share of neighbour pairs that carry the same label.

Everything on the device is fp64, free of floating-point atomics and bit-reproducible; a slide inside a batch is
bit-identical to the same slide alone.  No CPU fallback: without a GPU / the HIP library these functions raise
``RuntimeError``.

    python -m mclstexp_amd.hmrf --pred P1.npy ... --coords C1.npy ... [--true T1.npy ...] [--k K | --k_range LO HI]
                                [--beta B] [--scan B1 B2 ...] [--refine N] [--out_dir D]
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import cluster, mixture
from ._arrays import ArrayLike, Tensor, device, empty, matrix, stack_rows, upload
from ._lib import call

MAX_DIM = cluster.MAX_DIM          # D <= 64 and K <= 64 (csrc/hmrf.hip)
MAX_ROWS = 16384                   # per slide: the lattice's
MAX_SLOTS = 64                     # neighbour slots per spot
BAD_INDEX = 4                      # status bit: a kept slot held an index outside the slide
_PER_SLIDE = mixture._PER_SLIDE


# ------------------------------------------------------------------------------------------------------ host checks
def _offsets(graph: Dict[str, object], rows: int, min_rows: int = 1) -> np.ndarray:
    if not isinstance(graph, dict) or any(name not in graph for name in ("nbr", "w", "offsets")):
        raise ValueError("graph: expected what spatial.lattice returns (nbr, w, offsets)")
    off = cluster.validate_offsets(graph["offsets"], rows, min_rows)
    if int(np.diff(off).max()) > MAX_ROWS:
        raise ValueError(f"a slide holds {int(np.diff(off).max())} spots; the lattice and the kernel handle <= {MAX_ROWS}")
    return off


def _check_scores(z) -> tuple:
    if not hasattr(z, "shape") or len(z.shape) != 2:
        raise ValueError(f"z: expected a 2-D (rows, D) array, got shape {tuple(np.shape(z))}")
    rows, D = int(z.shape[0]), int(z.shape[1])
    if D < 1 or D > MAX_DIM:
        raise ValueError(f"z has {D} columns; the kernel handles 1 .. {MAX_DIM}")
    if isinstance(z, Tensor) and z.dtype != torch.float64:
        raise ValueError("z must be float64 (the PCA scores are)")
    return rows, D


def _check_graph(graph: Dict[str, object], rows: int) -> int:
    """Shapes, dtypes and values of the neighbour list, on the host; returns its width."""
    nbr, w = graph["nbr"], graph["w"]
    if len(nbr.shape) != 2 or tuple(w.shape) != tuple(nbr.shape) or int(nbr.shape[0]) != rows:
        raise ValueError(f"graph: nbr and w must both be ({rows}, kw), got {tuple(nbr.shape)} and {tuple(w.shape)}")
    kw = int(nbr.shape[1])
    if kw < 1 or kw > MAX_SLOTS:
        raise ValueError(f"graph: {kw} neighbour slots per spot; the kernel handles 1 .. {MAX_SLOTS}")
    if isinstance(nbr, Tensor):
        if nbr.dtype != torch.int32:
            raise ValueError(f"graph: nbr must be int32, got {nbr.dtype}")
    elif not np.issubdtype(np.asarray(nbr).dtype, np.integer):
        raise ValueError(f"graph: nbr must hold integers, got {np.asarray(nbr).dtype}")
    if isinstance(w, Tensor):
        if w.dtype != torch.float64:
            raise ValueError(f"graph: w must be float64, got {w.dtype}")
    elif not np.isfinite(np.asarray(w, dtype=np.float64)).all():
        raise ValueError("graph: weights must be finite")
    return kw


def _graph(graph: Dict[str, object], dev: torch.device):
    """The device (rows, kw) int32 neighbour list and fp64 weights of a checked ``graph``."""
    nbr, w = graph["nbr"], graph["w"]
    nbr_d = nbr.to(dev).contiguous() if isinstance(nbr, Tensor) else upload(np.asarray(nbr).astype(np.int32), dev)
    w_d = w.to(dev).contiguous() if isinstance(w, Tensor) else upload(np.asarray(w, dtype=np.float64), dev)
    return nbr_d, w_d


def _betas(beta, S: int) -> np.ndarray:
    try:
        b = np.asarray(beta, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"beta must be a number or one per slide, got {beta!r}") from None
    b = np.full(S, float(b)) if b.ndim == 0 else b.copy()
    if b.shape != (S,):
        raise ValueError(f"beta: {b.size} values for {S} slides")
    if not np.isfinite(b).all() or (b < 0).any():
        raise ValueError(f"beta must be finite and >= 0, got {b.tolist()}")
    return b


def _check_labels(labels, rows: int) -> None:
    t = labels if isinstance(labels, Tensor) else torch.as_tensor(np.asarray(labels))
    if t.dim() != 1 or t.shape[0] != rows:
        raise ValueError(f"labels: expected a ({rows},) vector, got shape {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"labels: expected integer labels, got {t.dtype}")
    if not t.is_cuda:
        if t.numel() and (int(t.min()) < -1 or int(t.max()) > np.iinfo(np.int32).max):
            raise ValueError("labels: values must be int32 labels >= 0, or -1 for a spot without one")
    elif t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError("labels: device labels must be a contiguous int32 vector")


def _labels(labels, dev: torch.device) -> Tensor:
    t = labels if isinstance(labels, Tensor) else torch.as_tensor(np.asarray(labels))
    return t if t.is_cuda else t.to(torch.int32).contiguous().to(dev)


def _n_rows(labels) -> int:
    return int(labels.shape[0]) if hasattr(labels, "shape") and len(labels.shape) else len(labels)


def _edge_sums(lab: Tensor, nbr: Tensor, w: Tensor, kw: int, off_d: Tensor, S: int, rows: int) -> Tensor:
    sums = torch.empty((S, 2), device=lab.device, dtype=torch.float64)
    call("mcl_edge_agreement", off_d, S, rows, lab, nbr, w, kw, sums)
    return sums


def _ratio(sums: Tensor) -> np.ndarray:
    h = sums.cpu().numpy()
    with np.errstate(all="ignore"):
        return h[:, 0] / h[:, 1]


# ----------------------------------------------------------------------------------------------------------- device
def hmrf(z: ArrayLike, graph: Dict[str, object], k: Union[int, Sequence[int]], beta=1.0, covariance_type: str = "full",
         init_labels=None, n_init: int = 1, seed: int = 0, tol: float = 1e-3, max_iter: int = 100,
         reg_covar: float = 1e-6, check: bool = True) -> Dict[str, object]:
    """The Potts-HMRF mixture of every slide of the row-stacked (rows, D <= 64) fp64 scores ``z`` over ``graph`` from R
    given starts: ``init_labels`` (R, rows), or the ``labels_all`` of ``cluster.kmeans(z, k, offsets, n_init=R, seed=seed)``,
    exactly as ``mixture.gmm``.  ``k`` an int or one per slide; ``beta`` a float or one per slide, finite and >= 0.
    Returns ``mixture.gmm``'s keys -- ``lower_bound`` and ``score_all`` are the mean-field pseudo-log-likelihood, ``bic`` /
    ``aic`` are computed from it -- plus host ``beta`` (S,), device ``field`` (rows, k_max): the neighbourhood field of the
    winning start's final E-step, and host ``edge_agreement`` (S,): the weighted share of kept neighbour pairs with equal
    labels.  ``check=True`` raises ``ValueError`` naming the slide for an ill-defined empirical covariance (status 1) and
    for a neighbour index outside the slide (status bit 4); ``check=False`` returns ``status`` instead."""
    rows, D = _check_scores(z)
    code = mixture.check_type(covariance_type)
    off = _offsets(graph, rows)
    seg = np.diff(off)
    ks = cluster.k_per_segment(k, seg)
    S, k_max = ks.size, int(ks.max())
    bs = _betas(beta, S)
    if not (tol >= 0.0) or int(max_iter) < 1 or not (reg_covar >= 0.0):
        raise ValueError(f"tol and reg_covar must be >= 0 and max_iter >= 1, got {tol}, {reg_covar}, {max_iter}")
    if init_labels is None and int(n_init) < 1:
        raise ValueError(f"n_init must be >= 1, got {n_init}")
    kw = _check_graph(graph, rows)
    if init_labels is not None:
        shape = tuple(init_labels.shape) if hasattr(init_labels, "shape") else np.shape(init_labels)
        if len(shape) not in (1, 2) or shape[-1] != rows:
            raise ValueError(f"init_labels: expected (R, {rows}) or ({rows},) labels, got shape {shape}")
    dev = device("hmrf")
    zd = mixture.scores_matrix(z, dev)
    nbr, w = _graph(graph, dev)
    if init_labels is None:
        init = cluster.kmeans(zd, ks, off, n_init=int(n_init), seed=seed)["labels_all"]
    else:
        init = mixture.start_labels(init_labels, rows, ks, off, dev)
    R = int(init.shape[0])
    if R > 65535:
        raise ValueError(f"the number of starts must lie in 1 .. 65535, got {R}")
    off_d, ks_d, beta_d = upload(off, dev), upload(ks, dev), upload(bs, dev)
    e = empty(dev)
    cshape = mixture.cov_shape(covariance_type, k_max, D)
    wb = call("mcl_hmrf_workspace_bytes", rows, S, R, D, k_max)
    gb = call("mcl_gmm_workspace_bytes", rows, S, R, D, k_max)
    work = e((wb // 8,), torch.float64)
    field_all = work[gb // 8:].view(R, rows, k_max)
    field_all.zero_()                           # components past k[s] are never written by the kernel
    f64, i32 = torch.float64, torch.int32
    res = {"labels_all": e((R, rows), i32), "weights_all": e((S, R, k_max), f64), "means_all": e((S, R, k_max, D), f64),
           "covariances_all": e((S, R) + cshape, f64), "precisions_cholesky_all": e((S, R) + cshape, f64),
           "lower_bound_all": e((S, R), f64), "score_all": e((S, R), f64), "n_iter_all": e((S, R), i32),
           "converged_all": e((S, R), i32), "status_all": e((S, R), i32),
           "labels": e((rows,), i32), "resp": e((rows, k_max), f64), "weights": e((S, k_max), f64),
           "means": e((S, k_max, D), f64), "covariances": e((S,) + cshape, f64),
           "precisions_cholesky": e((S,) + cshape, f64), "lower_bound": e((S,), f64), "n_iter": e((S,), i32),
           "converged": e((S,), i32), "status": e((S,), i32), "bic": e((S,), f64), "aic": e((S,), f64),
           "restart": e((S,), i32)}
    for name in ("weights_all", "means_all", "covariances_all", "precisions_cholesky_all"):
        res[name].zero_()
    alls = [res[n] for n in ("labels_all", "weights_all", "means_all", "covariances_all", "precisions_cholesky_all",
                             "lower_bound_all", "score_all", "n_iter_all", "converged_all", "status_all")]
    call("mcl_hmrf_fit", zd, zd.stride(0), off_d, S, rows, D, ks_d, k_max, R, code, init, nbr, w, kw, beta_d, float(tol),
         int(max_iter), float(reg_covar), work, wb, *alls)
    call("mcl_gmm_select", off_d, S, rows, D, ks_d, k_max, R, code, work, wb, *alls, res["labels"], res["resp"],
         res["weights"], res["means"], res["covariances"], res["precisions_cholesky"], res["lower_bound"], res["n_iter"],
         res["converged"], res["status"], res["bic"], res["aic"], res["restart"])
    start = torch.repeat_interleave(res["restart"].long(), upload(seg, dev))          # the winning start of every row
    res["field"] = field_all[start, torch.arange(rows, device=dev)]
    res["edge_agreement"] = _ratio(_edge_sums(res["labels"], nbr, w, kw, off_d, S, rows))
    res.update(init_labels=init, k=ks, offsets=off, covariance_type=covariance_type, beta=bs)
    if check:
        st = res["status_all"].cpu().numpy()
        bad = np.flatnonzero(((st & BAD_INDEX) != 0).any(axis=1))
        if bad.size:
            raise ValueError(f"slide {', '.join(str(int(b)) for b in bad)}: the graph holds a neighbour index outside the "
                             f"slide (indices are local to the slide)")
        bad = np.flatnonzero((st != 0).any(axis=1))
        if bad.size:
            raise ValueError(f"slide {', '.join(str(int(b)) for b in bad)}: ill-defined empirical covariance (a component "
                             f"collapsed onto one point or fewer); fewer components or a larger reg_covar may help")
    return res


def estep(z: ArrayLike, model: Dict[str, object], graph: Dict[str, object], resp_prev: ArrayLike,
          beta=1.0) -> Dict[str, Tensor]:
    """One E-step of ``hmrf`` (the device function of the fit) on the rows of ``z`` under ``model`` (what ``hmrf`` /
    ``mixture.gmm`` return, or a dict with ``weights``, ``means``, ``precisions_cholesky``, ``k``, ``covariance_type``),
    with the neighbours' memberships held at ``resp_prev`` (rows, k_max): smoothing under a fixed model.  Device ``field``,
    ``log_resp``, ``resp`` (rows, k_max), ``labels`` (rows,) int32, ``log_prob_norm`` (rows,) = lse, ``log_prior_norm``
    (rows,) = za, ``score`` (S,) = the mean of lse - za per slide and ``status`` (S,)."""
    rows, D = _check_scores(z)
    ctype = model["covariance_type"]
    code = mixture.check_type(ctype)
    off = _offsets(graph, rows)
    ks = np.asarray(model["k"], dtype=np.int32).reshape(-1)
    S = off.size - 1
    bs = _betas(beta, S)
    wts, mu, pc = model["weights"], model["means"], model["precisions_cholesky"]
    if ks.size != S or wts.dim() != 2 or wts.shape[0] != S:
        raise ValueError(f"the model holds {ks.size} slides, the graph has {S}")
    k_max = int(wts.shape[1])
    if tuple(mu.shape) != (S, k_max, D) or tuple(pc.shape) != (S,) + mixture.cov_shape(ctype, k_max, D):
        raise ValueError(f"the model's parameters do not match z: means {tuple(mu.shape)}, precisions_cholesky "
                         f"{tuple(pc.shape)}, D = {D}")
    for name, t in (("weights", wts), ("means", mu), ("precisions_cholesky", pc)):
        if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"model[{name!r}] must be a contiguous float64 device tensor")
    if not hasattr(resp_prev, "shape") or tuple(resp_prev.shape) != (rows, k_max):
        raise ValueError(f"resp_prev: expected shape ({rows}, {k_max}), got {tuple(np.shape(resp_prev))}")
    kw = _check_graph(graph, rows)
    dev = device("hmrf")
    zd = mixture.scores_matrix(z, dev)
    q = matrix(resp_prev, "resp_prev", dev, (torch.float64,), torch.float64, dense=True)
    nbr, w = _graph(graph, dev)
    e = empty(dev)
    f64 = torch.float64
    res = {"field": torch.zeros((rows, k_max), device=dev, dtype=f64), "log_resp": e((rows, k_max), f64),
           "resp": torch.zeros((rows, k_max), device=dev, dtype=f64), "labels": e((rows,), torch.int32),
           "log_prob_norm": e((rows,), f64), "log_prior_norm": e((rows,), f64), "score": e((S,), f64),
           "status": e((S,), torch.int32)}
    res["log_resp"].fill_(float("-inf"))
    call("mcl_hmrf_estep", zd, zd.stride(0), upload(off, dev), S, rows, D, upload(ks, dev), k_max, code, wts, mu, pc, q, nbr,
         w, kw, upload(bs, dev), res["field"], res["log_resp"], res["resp"], res["labels"], res["log_prob_norm"],
         res["log_prior_norm"], res["score"], res["status"])
    return res


def refine_labels(labels: ArrayLike, graph: Dict[str, object], n_iter: int = 1) -> Dict[str, object]:
    """``n_iter`` synchronous rounds of neighbourhood majority relabelling of ``labels`` (rows,) from any caller (k-means,
    Leiden, an annotation; -1: no label, stays -1).  In a round a spot with label l looks at its kept neighbours that carry
    a label (m of them) and itself: it takes the most frequent label (ties: the smallest) iff fewer than half of the m carry
    l -- 2 count(l) < m, the spot counted -- and more than half carry that label.  Every decision of a round reads the
    labels the round began with.  Returns device ``labels`` (rows,) int32 and host ``changed`` (n_iter, S): the spots
    relabelled per round and slide; the rounds stop early when one changes nothing (its row and the later ones are 0)."""
    if int(n_iter) < 1:
        raise ValueError(f"n_iter must be >= 1, got {n_iter}")
    rows = _n_rows(labels)
    off = _offsets(graph, rows)
    _check_labels(labels, rows)
    kw = _check_graph(graph, rows)
    dev = device("hmrf")
    lab = _labels(labels, dev)
    nbr, w = _graph(graph, dev)
    S = off.size - 1
    off_d = upload(off, dev)
    changed = np.zeros((int(n_iter), S), dtype=np.int64)
    cnt = torch.empty((S,), device=dev, dtype=torch.int32)
    for it in range(int(n_iter)):
        out = torch.empty_like(lab)
        call("mcl_label_refine", off_d, S, rows, lab, nbr, w, kw, out, cnt)
        changed[it] = cnt.cpu().numpy()
        lab = out
        if not changed[it].any():
            break
    return {"labels": lab, "changed": changed}


def edge_agreement(labels: ArrayLike, graph: Dict[str, object]) -> np.ndarray:
    """Host (S,): per slide sum_i sum_c w_ic [l_i = l_nbr] / sum_i sum_c w_ic over the kept neighbour slots whose two spots
    carry a label (>= 0): the weighted share of neighbour pairs inside one domain (NaN for a slide without such a pair)."""
    rows = _n_rows(labels)
    off = _offsets(graph, rows)
    _check_labels(labels, rows)
    kw = _check_graph(graph, rows)
    dev = device("hmrf")
    lab = _labels(labels, dev)
    nbr, w = _graph(graph, dev)
    return _ratio(_edge_sums(lab, nbr, w, kw, upload(off, dev), off.size - 1, rows))


def scan_beta(z: ArrayLike, graph: Dict[str, object], k: Union[int, Sequence[int]], betas: Sequence[float],
              covariance_type: str = "full", init_labels=None, n_init: int = 1, seed: int = 0, tol: float = 1e-3,
              max_iter: int = 100, reg_covar: float = 1e-6) -> Dict[str, object]:
    """``hmrf`` at every candidate coupling of ``betas`` for every slide in ONE call: slides and graph rows are replicated
    once per candidate (as ``mixture.select_k`` replicates them per k), every replica from the same starts.  Host tables
    (S, B): ``lower_bound``, ``edge_agreement``, ``silhouette`` and ``changed``, the spots whose label differs from the first
    candidate's; ``betas``; ``fits``: per candidate the ``hmrf`` result of its replica (no ``*_all``).  It chooses nothing:
    the pseudo-likelihoods of different beta are not comparable and there is no agreed criterion for beta."""
    cand = [float(b) for b in betas]
    if not cand:
        raise ValueError("betas: expected at least one candidate")
    _betas(np.asarray(cand), len(cand))
    rows, _ = _check_scores(z)
    mixture.check_type(covariance_type)
    off = _offsets(graph, rows, min_rows=2)
    S, B = off.size - 1, len(cand)
    ks = cluster.k_per_segment(k, np.diff(off))
    if S * B > 65535:
        raise ValueError(f"{S} slides x {B} candidates exceed 65535 problems per call")
    _check_graph(graph, rows)
    if init_labels is None and int(n_init) < 1:
        raise ValueError(f"n_init must be >= 1, got {n_init}")
    dev = device("hmrf")
    zd = mixture.scores_matrix(z, dev)
    nbr, w = _graph(graph, dev)
    if init_labels is None:
        init = cluster.kmeans(zd, ks, off, n_init=int(n_init), seed=seed)["labels_all"]
    else:
        init = mixture.start_labels(init_labels, rows, ks, off, dev)
    big = {"nbr": nbr.repeat(B, 1), "w": w.repeat(B, 1),
           "offsets": np.concatenate([[0]] + [off[1:] + g * rows for g in range(B)]).astype(np.int64)}
    zz = zd.contiguous().repeat(B, 1)
    fit = hmrf(zz, big, np.tile(ks, B), np.repeat(np.asarray(cand), S), covariance_type, init.repeat(1, B).contiguous(),
               tol=tol, max_iter=max_iter, reg_covar=reg_covar, check=False)
    sil = mixture.validity(zz, fit["labels"], big["offsets"])["silhouette"]
    lab = fit["labels"].view(B, rows)
    diff = (lab != lab[0:1]).to(torch.int64)
    seg_id = torch.repeat_interleave(torch.arange(S, device=dev), upload(np.diff(off), dev))
    changed = torch.zeros((B, S), device=dev, dtype=torch.int64).index_add_(1, seg_id, diff).cpu().numpy().T
    fits = []
    for g in range(B):
        one = {"labels": lab[g], "resp": fit["resp"][g * rows:(g + 1) * rows], "field": fit["field"][g * rows:(g + 1) * rows],
               "edge_agreement": fit["edge_agreement"][g * S:(g + 1) * S], "beta": fit["beta"][g * S:(g + 1) * S], "k": ks,
               "offsets": off, "covariance_type": covariance_type}
        for name in _PER_SLIDE:
            one[name] = fit[name][g * S:(g + 1) * S]
        fits.append(one)
    return {"betas": cand, "lower_bound": fit["lower_bound"].cpu().numpy().reshape(B, S).T.copy(),
            "edge_agreement": fit["edge_agreement"].reshape(B, S).T.copy(), "silhouette": sil.reshape(B, S).T.copy(),
            "changed": np.ascontiguousarray(changed), "fits": fits}


# ------------------------------------------------------------------------------------------------- slides end to end
def _domains(xs, coords, k, k_range, beta, lattice_k, prune, n_comps, pca_solver, kw) -> Dict[str, object]:
    from . import spatial
    dev = device("hmrf")
    x, off = stack_rows(xs, "slides", dev)
    z = cluster.pca_scores(x, off, n_comps, pca_solver)
    if k is not None:
        base = mixture.gmm(z, k, off, **kw)
    else:
        lo, hi = int(k_range[0]), int(k_range[1])
        base = mixture.select_k(z, list(range(lo, hi + 1)), off, **kw)["model"]
    xy = np.concatenate([np.asarray(c.cpu() if isinstance(c, Tensor) else c, dtype=np.float64) for c in coords])
    graph = spatial.lattice(xy, off, lattice_k, prune, row_standardise=False)
    fit = hmrf(z, graph, base["k"], beta, kw["covariance_type"], init_labels=base["labels"][None, :].contiguous(),
               tol=kw["tol"], max_iter=kw["max_iter"], reg_covar=kw["reg_covar"])
    return {"model": fit, "gmm": base, "validity": mixture.validity(z, fit["labels"], off), "offsets": off, "scores": z,
            "graph": graph, "gmm_edge_agreement": edge_agreement(base["labels"], graph)}


def domains_slides(preds: Sequence[ArrayLike], coords: Sequence[ArrayLike], trues: Optional[Sequence[ArrayLike]] = None,
                   k: Union[None, int, Sequence[int]] = None, k_range: Sequence[int] = (2, 12), beta=1.0,
                   lattice_k: int = 8, prune: str = "NA", n_comps: int = cluster.N_COMPS, pca_solver: str = "host",
                   covariance_type: str = "full", n_init: int = 1, seed: int = 0, tol: float = 1e-3, max_iter: int = 100,
                   reg_covar: float = 1e-6) -> Dict[str, object]:
    """Spatial domains of slides nobody annotated, with the tissue in the model.  Per slide: PCA scores of the (spots, genes)
    prediction -> ``k`` given, or ``mixture.select_k`` by BIC over ``k_range`` = (lo, hi) inclusive -> the binary
    ``lattice_k``-neighbour lattice of ``coords`` (spots, 2) -> ``hmrf`` started from the mixture's own winning labels ->
    validity indices and edge agreement.  Returns ``slides``: per slide ``k``, ``beta``, ``labels`` (spots,) int32, ``proba``
    (spots, k), ``silhouette``, ``calinski_harabasz``, ``davies_bouldin``, ``edge_agreement``, ``n_iter``, ``converged``, and
    the non-spatial fit's ``gmm_labels`` and ``gmm_edge_agreement``: the effect of the prior is one subtraction away.  With
    ``trues`` the same runs on the measured matrices (``true_`` keys) and every slide gets ``ari`` / ``nmi`` between the two
    sets of domains.  Also ``scores``, ``graph`` and ``offsets`` of the predictions, for ``scan_beta`` / ``refine_labels``."""
    if not len(preds):
        raise ValueError("need at least one slide")
    if len(coords) != len(preds):
        raise ValueError(f"need one coordinate array per prediction; got {len(coords)} and {len(preds)}")
    for i, (p, c) in enumerate(zip(preds, coords)):
        if len(c.shape) != 2 or int(c.shape[1]) != 2 or int(c.shape[0]) != int(p.shape[0]):
            raise ValueError(f"slide {i}: coords must be ({int(p.shape[0])}, 2), got {tuple(c.shape)}")
    if trues is not None:
        if len(trues) != len(preds):
            raise ValueError(f"need one measured matrix per prediction; got {len(trues)} and {len(preds)}")
        for i, (p, t) in enumerate(zip(preds, trues)):
            if int(p.shape[0]) != int(t.shape[0]):
                raise ValueError(f"slide {i}: prediction and measurement differ in spots: {p.shape[0]} and {t.shape[0]}")
    _betas(beta, len(preds))
    kw = dict(covariance_type=covariance_type, n_init=n_init, seed=seed, tol=tol, max_iter=max_iter, reg_covar=reg_covar)
    args = (k, k_range, beta, lattice_k, prune, n_comps, pca_solver, kw)
    sides = [("", _domains(preds, coords, *args))]
    if trues is not None:
        sides.append(("true_", _domains(trues, coords, *args)))
    slides: List[Dict[str, object]] = [{} for _ in preds]
    for prefix, side in sides:
        m, v, off = side["model"], side["validity"], side["offsets"]
        lab, resp = m["labels"].cpu().numpy(), m["resp"].cpu().numpy()
        glab = side["gmm"]["labels"].cpu().numpy()
        n_iter, conv = m["n_iter"].cpu().numpy(), m["converged"].cpu().numpy()
        for i, sl in enumerate(slides):
            ki = int(np.asarray(m["k"]).reshape(-1)[i])
            sl.update({prefix + "k": ki, prefix + "beta": float(m["beta"][i]),
                       prefix + "silhouette": float(v["silhouette"][i]),
                       prefix + "calinski_harabasz": float(v["calinski_harabasz"][i]),
                       prefix + "davies_bouldin": float(v["davies_bouldin"][i]),
                       prefix + "edge_agreement": float(m["edge_agreement"][i]),
                       prefix + "n_iter": int(n_iter[i]), prefix + "converged": int(conv[i]),
                       prefix + "labels": lab[off[i]:off[i + 1]].copy(),
                       prefix + "proba": resp[off[i]:off[i + 1], :ki].copy(),
                       prefix + "gmm_labels": glab[off[i]:off[i + 1]].copy(),
                       prefix + "gmm_edge_agreement": float(side["gmm_edge_agreement"][i])})
    if trues is not None:
        ari, nmi = cluster.cluster_scores(sides[1][1]["model"]["labels"], sides[0][1]["model"]["labels"],
                                          sides[0][1]["offsets"])
        for i, sl in enumerate(slides):
            sl["ari"], sl["nmi"] = float(ari[i]), float(nmi[i])
    first = sides[0][1]
    return {"slides": slides, "scores": first["scores"], "graph": first["graph"], "offsets": first["offsets"]}


# --------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.hmrf",
                                description="Potts-HMRF spatial domains of predicted expression: PCA scores, the spot "
                                            "lattice, mean-field EM, validity indices and edge agreement")
    p.add_argument("--pred", required=True, nargs="+", help="one (spots, genes) .npy per slide")
    p.add_argument("--coords", required=True, nargs="+", help="one (spots, 2) .npy per slide, same order")
    p.add_argument("--true", nargs="+", default=None, help="one measured (spots, genes) .npy per slide, same order: "
                                                           "also ARI / NMI between the two sets of domains")
    p.add_argument("--k", type=int, default=None, help="the number of components (default: the mixture's BIC over --k_range)")
    p.add_argument("--k_range", type=int, nargs=2, default=(2, 12), metavar=("LO", "HI"))
    p.add_argument("--beta", type=float, default=1.0, help="the coupling: the bonus per agreeing neighbour")
    p.add_argument("--scan", type=float, nargs="+", default=None, metavar="B",
                   help="also fit every slide at these couplings and print one line per slide and coupling")
    p.add_argument("--refine", type=int, default=0, metavar="N", help="also N rounds of majority relabelling of the domains")
    p.add_argument("--lattice_k", type=int, default=8)
    p.add_argument("--prune", choices=("NA", "STD", "Grid"), default="NA")
    p.add_argument("--covariance_type", choices=sorted(mixture.COVARIANCE_TYPES), default="full")
    p.add_argument("--n_comps", type=int, default=cluster.N_COMPS)
    p.add_argument("--n_init", type=int, default=1, help="k-means starts per mixture, the best lower bound wins")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--pca_solver", choices=cluster.SOLVERS, default="host")
    p.add_argument("--out_dir", default=None, help="write <out_dir>/<i>/hmrf_labels.npy and hmrf_proba.npy per slide")
    a = p.parse_args(argv)
    if len(a.coords) != len(a.pred):
        p.error(f"{len(a.pred)} --pred files but {len(a.coords)} --coords files")
    if a.true is not None and len(a.true) != len(a.pred):
        p.error(f"{len(a.pred)} --pred files but {len(a.true)} --true files")
    for b in [a.beta] + list(a.scan or []):
        if not math.isfinite(b) or b < 0:
            p.error(f"a coupling must be finite and >= 0, got {b}")
    if a.refine < 0:
        p.error("--refine must be >= 0")
    return a


def format_report(res: Dict[str, object]) -> str:
    """One line per slide; ``repr`` of the floats: the printed numbers are the API's."""
    lines = []
    for i, s in enumerate(res["slides"]):
        line = (f"slide {i}: k: {s['k']}, beta: {s['beta']!r}, n_iter: {s['n_iter']}, converged: {s['converged']}, "
                f"edge_agreement: {s['edge_agreement']!r} (gmm: {s['gmm_edge_agreement']!r}), "
                f"silhouette: {s['silhouette']!r}, CH: {s['calinski_harabasz']!r}, DB: {s['davies_bouldin']!r}")
        if "ari" in s:
            line += f", ARI: {s['ari']!r}, NMI: {s['nmi']!r}"
        lines.append(line)
    return "\n".join(lines)


def format_scan(scan: Dict[str, object]) -> str:
    lines = []
    for i in range(scan["lower_bound"].shape[0]):
        for j, b in enumerate(scan["betas"]):
            lines.append(f"slide {i}: beta: {b!r}, lower_bound: {float(scan['lower_bound'][i, j])!r}, edge_agreement: "
                         f"{float(scan['edge_agreement'][i, j])!r}, silhouette: {float(scan['silhouette'][i, j])!r}, "
                         f"changed: {int(scan['changed'][i, j])}")
    return "\n".join(lines)


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    preds = [np.load(f) for f in a.pred]
    coords = [np.load(f) for f in a.coords]
    trues = [np.load(f) for f in a.true] if a.true is not None else None
    res = domains_slides(preds, coords, trues, a.k, a.k_range, a.beta, a.lattice_k, a.prune, a.n_comps, a.pca_solver,
                         a.covariance_type, a.n_init, a.seed)
    print(format_report(res))
    off = res["offsets"]
    ks = [s["k"] for s in res["slides"]]
    if a.scan:
        print(format_scan(scan_beta(res["scores"], res["graph"], ks, a.scan, a.covariance_type, n_init=a.n_init,
                                    seed=a.seed)))
    refined = None
    if a.refine:
        r = refine_labels(np.concatenate([s["labels"] for s in res["slides"]]), res["graph"], a.refine)
        refined = r["labels"].cpu().numpy()
        for i in range(len(preds)):
            print(f"slide {i}: refine: changed per round: {r['changed'][:, i].tolist()}")
    if a.out_dir:
        for i, s in enumerate(res["slides"]):
            d = os.path.join(a.out_dir, str(i))
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, "hmrf_labels.npy"), s["labels"])
            np.save(os.path.join(d, "hmrf_proba.npy"), s["proba"])
            if refined is not None:
                np.save(os.path.join(d, "hmrf_labels_refined.npy"), refined[off[i]:off[i + 1]])
    return 0


if __name__ == "__main__":
    sys.exit(main())
