"""Gaussian mixtures of PCA scores on the MI355X: soft spatial domains, a BIC that chooses their number, and internal
validity indices for slides nobody annotated (mclust is the domain caller of STAGATE / GraphST-style pipelines; what is
computed here is sklearn's ``GaussianMixture``, ``silhouette_samples``, ``calinski_harabasz_score`` and
``davies_bouldin_score``).

What is computed is stated in DESIGN 6.17 and restated in numpy by ``tests/mixture_reference.py``, which
``tests/test_mixture_host.py`` pins to sklearn itself.  Parity with mclust or an R release is unpinned.  Things to know:

* ``gmm``: EM for every slide (row segment) x ``n_init`` starts in ONE ``mcl_gmm_fit`` call, one workgroup per problem.
  The starts are label vectors (one-hot responsibilities, sklearn's ``_initialize``): ``init_labels`` (R, rows), or the
  ``labels_all`` of ``cluster.kmeans(z, k, offsets, n_init=R, seed=seed)``.  sklearn's own k-means stream is not reproduced.
  ``covariance_type``: full, tied, diag, spherical.  D <= 64, k <= 64, k <= n_s <= 50 000.  The start of highest lower bound
  wins (ties: the lowest).  A covariance that is not positive definite (sklearn: "ill-defined empirical covariance") sets
  the status of that (slide, start) and raises ``ValueError`` naming the slide; ``check=False`` returns ``status`` instead.
* ``select_k``: every candidate k of every slide goes into as few ``gmm`` calls as ``max_workspace_bytes`` allows (the
  slides are replicated once per candidate); the criterion table is (S, len(k_range)), lowest BIC / AIC wins (ties: lowest k).
* ``validity``: labels in [0, 1024), -1 drops the row; a slide with fewer than 2 or more than kept - 1 clusters scores NaN.

Everything on the device is fp64, free of floating-point atomics and bit-reproducible; a slide inside a batch is
bit-identical to the same slide alone.  No CPU fallback: without a GPU / the HIP library these functions raise
``RuntimeError``.

    python -m mclstexp_amd.mixture --pred P1.npy ... [--true T1.npy ...] [--k K | --k_range LO HI] [--covariance_type T]
                                   [--n_init N] [--seed S] [--out_dir D]
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import cluster
from ._arrays import FLOAT_CODE, ArrayLike, Tensor, device, empty, matrix, stack_rows, upload
from ._lib import call

MAX_DIM = cluster.MAX_DIM          # D <= 64 and K <= 64 (csrc/mixture.hip)
MAX_ROWS = cluster.MAX_ROWS
MAX_LABEL = cluster.MAX_LABEL
COVARIANCE_TYPES = {"full": 0, "tied": 1, "diag": 2, "spherical": 3}
CRITERIA = ("bic", "aic")
MAX_WORKSPACE_BYTES = 1 << 30      # select_k: the workspace of one gmm call
_PER_SLIDE = ("weights", "means", "covariances", "precisions_cholesky", "lower_bound", "n_iter", "converged", "status",
              "bic", "aic", "restart")


def cov_shape(ctype: str, k_max: int, D: int) -> tuple:
    """The shape of one slide's covariances (and precisions_cholesky) of type ``ctype``."""
    return {"full": (k_max, D, D), "tied": (D, D), "diag": (k_max, D), "spherical": (k_max,)}[ctype]


def scores_matrix(z: ArrayLike, dev: torch.device) -> Tensor:
    """``z`` as a float64 row-major device matrix of 1 .. MAX_DIM columns."""
    if not isinstance(z, Tensor) and np.asarray(z).ndim != 2:
        raise ValueError(f"z: expected a 2-D (rows, D) array, got shape {np.asarray(z).shape}")
    D = int(z.shape[1])
    if D < 1 or D > MAX_DIM:
        raise ValueError(f"z has {D} columns; the kernel handles 1 .. {MAX_DIM}")
    zd = matrix(z, "z", dev, FLOAT_CODE, torch.float64)
    if zd.dtype != torch.float64:
        raise ValueError("z must be float64 (the PCA scores are)")
    return zd


def check_type(covariance_type: str) -> int:
    """The C ABI's code of ``covariance_type``."""
    if covariance_type not in COVARIANCE_TYPES:
        raise ValueError(f"covariance_type must be one of {sorted(COVARIANCE_TYPES)}, got {covariance_type!r}")
    return COVARIANCE_TYPES[covariance_type]


def start_labels(init_labels, rows: int, ks: np.ndarray, off: np.ndarray, dev: torch.device) -> Tensor:
    """Start labels as an int32 (R, rows) device tensor; host labels are checked against 0 .. k - 1 of their slide."""
    t = init_labels if isinstance(init_labels, Tensor) else torch.as_tensor(np.asarray(init_labels))
    if t.dim() == 1:
        t = t[None, :]
    if t.dim() != 2 or t.shape[1] != rows or t.shape[0] < 1:
        raise ValueError(f"init_labels: expected (R, {rows}) or ({rows},) labels, got shape {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"init_labels: expected integer labels, got {t.dtype}")
    if not t.is_cuda:
        h = t.numpy()
        for s in range(ks.size):
            part = h[:, off[s]:off[s + 1]]
            if part.min() < 0 or part.max() >= ks[s]:
                raise ValueError(f"init_labels: slide {s} has labels outside 0 .. {int(ks[s]) - 1}")
        return t.to(torch.int32).contiguous().to(dev)
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError("init_labels: device labels must be a contiguous int32 (R, rows) tensor")
    return t


def gmm(z: ArrayLike, k: Union[int, Sequence[int]], offsets: Optional[Sequence[int]] = None,
        covariance_type: str = "full", init_labels=None, n_init: int = 1, seed: int = 0, tol: float = 1e-3,
        max_iter: int = 100, reg_covar: float = 1e-6, check: bool = True) -> Dict[str, object]:
    """sklearn's ``GaussianMixture(k, covariance_type, tol, reg_covar, max_iter).fit`` of every segment of the row-stacked
    (rows, D <= 64) fp64 matrix ``z`` from R given starts; ``k`` an int or one int per segment.  Device tensors of the
    winning start per segment: ``labels`` (rows,) int32, ``resp`` (rows, k_max), ``weights`` (S, k_max), ``means``
    (S, k_max, D), ``covariances`` / ``precisions_cholesky`` (S, k_max, D, D | D, D | k_max, D | k_max), ``lower_bound``,
    ``n_iter``, ``converged``, ``status``, ``bic``, ``aic``, ``restart`` (S,); per start ``labels_all`` (R, rows),
    ``weights_all`` ... ``status_all`` (S, R, ...), ``score_all`` (S, R): the mean log-likelihood under the final
    parameters; ``init_labels`` (R, rows) as used; host ``k`` (S,), ``offsets`` and ``covariance_type``."""
    dev = device("mixture")
    zd = scores_matrix(z, dev)
    rows, D = int(zd.shape[0]), int(zd.shape[1])
    code = check_type(covariance_type)
    off = cluster.validate_offsets(offsets, rows)
    seg = np.diff(off)
    ks = cluster.k_per_segment(k, seg)
    S, k_max = ks.size, int(ks.max())
    if not (tol >= 0.0) or int(max_iter) < 1 or not (reg_covar >= 0.0):
        raise ValueError(f"tol and reg_covar must be >= 0 and max_iter >= 1, got {tol}, {reg_covar}, {max_iter}")
    if init_labels is None:
        if int(n_init) < 1:
            raise ValueError(f"n_init must be >= 1, got {n_init}")
        init = cluster.kmeans(zd, ks, off, n_init=int(n_init), seed=seed)["labels_all"]
    else:
        init = start_labels(init_labels, rows, ks, off, dev)
    R = int(init.shape[0])
    if R > 65535:
        raise ValueError(f"the number of starts must lie in 1 .. 65535, got {R}")
    off_d, ks_d = upload(off, dev), upload(ks, dev)
    e = empty(dev)
    cshape = cov_shape(covariance_type, k_max, D)
    wb = call("mcl_gmm_workspace_bytes", rows, S, R, D, k_max)
    work = e((wb // 8,), torch.float64)
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
        res[name].zero_()                       # components past k[s] are never written by the kernel
    alls = [res[n] for n in ("labels_all", "weights_all", "means_all", "covariances_all", "precisions_cholesky_all",
                             "lower_bound_all", "score_all", "n_iter_all", "converged_all", "status_all")]
    call("mcl_gmm_fit", zd, zd.stride(0), off_d, S, rows, D, ks_d, k_max, R, code, init, float(tol), int(max_iter),
         float(reg_covar), work, wb, *alls)
    call("mcl_gmm_select", off_d, S, rows, D, ks_d, k_max, R, code, work, wb, *alls, res["labels"], res["resp"],
         res["weights"], res["means"], res["covariances"], res["precisions_cholesky"], res["lower_bound"], res["n_iter"],
         res["converged"], res["status"], res["bic"], res["aic"], res["restart"])
    res.update(init_labels=init, k=ks, offsets=off, covariance_type=covariance_type)
    if check:
        bad = np.flatnonzero((res["status_all"].cpu().numpy() != 0).any(axis=1))
        if bad.size:
            raise ValueError(f"slide {', '.join(str(int(b)) for b in bad)}: ill-defined empirical covariance (a component "
                             f"collapsed onto one point or fewer); fewer components or a larger reg_covar may help")
    return res


def predict(z: ArrayLike, model: Dict[str, object], offsets: Optional[Sequence[int]] = None) -> Dict[str, Tensor]:
    """The E-step of ``gmm`` on the rows of ``z`` under ``model`` (what ``gmm`` / ``select_k`` return, or a dict with
    ``weights``, ``means``, ``precisions_cholesky``, ``k``, ``covariance_type``): device ``labels`` (rows,) int32, ``resp`` and
    ``log_resp`` (rows, k_max), ``log_prob_norm`` (rows,) = sklearn's ``score_samples``, ``score`` (S,) its mean per slide.
    ``offsets``: the segments of ``z`` (one per slide of the model; None: one segment)."""
    dev = device("mixture")
    zd = scores_matrix(z, dev)
    rows, D = int(zd.shape[0]), int(zd.shape[1])
    ctype = model["covariance_type"]
    code = check_type(ctype)
    off = cluster.validate_offsets(offsets, rows)
    ks = np.asarray(model["k"], dtype=np.int32).reshape(-1)
    S = off.size - 1
    w, mu, pc = model["weights"], model["means"], model["precisions_cholesky"]
    if ks.size != S or w.dim() != 2 or w.shape[0] != S:
        raise ValueError(f"the model holds {ks.size} slides, z has {S} segments")
    k_max = int(w.shape[1])
    if tuple(mu.shape) != (S, k_max, D) or tuple(pc.shape) != (S,) + cov_shape(ctype, k_max, D):
        raise ValueError(f"the model's parameters do not match z: means {tuple(mu.shape)}, precisions_cholesky "
                         f"{tuple(pc.shape)}, D = {D}")
    for name, t in (("weights", w), ("means", mu), ("precisions_cholesky", pc)):
        if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"model[{name!r}] must be a contiguous float64 device tensor")
    e = empty(dev)
    res = {"log_prob_norm": e((rows,), torch.float64), "log_resp": e((rows, k_max), torch.float64),
           "resp": torch.zeros((rows, k_max), device=dev, dtype=torch.float64), "labels": e((rows,), torch.int32),
           "score": e((S,), torch.float64)}
    res["log_resp"].fill_(float("-inf"))
    call("mcl_gmm_predict", zd, zd.stride(0), upload(off, dev), S, rows, D, upload(ks, dev), k_max, code, w, mu, pc,
         res["log_prob_norm"], res["log_resp"], res["resp"], res["labels"], res["score"])
    return res


def m_step(z: ArrayLike, log_resp: ArrayLike, k: Union[int, Sequence[int]], offsets: Optional[Sequence[int]] = None,
           covariance_type: str = "full", reg_covar: float = 1e-6) -> Dict[str, object]:
    """The M-step of ``gmm`` alone (sklearn's ``_m_step``) from given log-responsibilities (rows, k_max): device ``weights``,
    ``means``, ``covariances``, ``precisions_cholesky`` (S, ...) and ``status`` (S,), plus ``k`` and ``covariance_type``, so
    that the result is a model ``predict`` takes.  Nothing is raised for an ill-defined covariance: read ``status``."""
    dev = device("mixture")
    zd = scores_matrix(z, dev)
    rows, D = int(zd.shape[0]), int(zd.shape[1])
    code = check_type(covariance_type)
    off = cluster.validate_offsets(offsets, rows)
    ks = cluster.k_per_segment(k, np.diff(off))
    S, k_max = ks.size, int(ks.max())
    lr = matrix(log_resp, "log_resp", dev, (torch.float64,), torch.float64, dense=True)
    if tuple(lr.shape) != (rows, k_max):
        raise ValueError(f"log_resp: expected shape ({rows}, {k_max}), got {tuple(lr.shape)}")
    cshape = cov_shape(covariance_type, k_max, D)
    z0 = lambda shape: torch.zeros(shape, device=dev, dtype=torch.float64)      # noqa: E731
    res = {"weights": z0((S, k_max)), "means": z0((S, k_max, D)), "covariances": z0((S,) + cshape),
           "precisions_cholesky": z0((S,) + cshape), "status": torch.empty((S,), device=dev, dtype=torch.int32)}
    wb = call("mcl_gmm_workspace_bytes", rows, S, 1, D, k_max)
    work = torch.empty((wb // 8,), device=dev, dtype=torch.float64)
    call("mcl_gmm_mstep", zd, zd.stride(0), upload(off, dev), S, rows, D, upload(ks, dev), k_max, code, lr, float(reg_covar),
         work, wb, res["weights"], res["means"], res["covariances"], res["precisions_cholesky"], res["status"])
    res.update(k=ks, offsets=off, covariance_type=covariance_type)
    return res


def score_samples(z: ArrayLike, model: Dict[str, object], offsets: Optional[Sequence[int]] = None) -> Tensor:
    """Device (rows,) log-likelihood of every row under its slide's mixture (sklearn's ``score_samples``)."""
    return predict(z, model, offsets)["log_prob_norm"]


def select_k(z: ArrayLike, k_range: Sequence[int], offsets: Optional[Sequence[int]] = None, criterion: str = "bic",
             covariance_type: str = "full", init_labels: Optional[Dict[int, ArrayLike]] = None, n_init: int = 1,
             seed: int = 0, tol: float = 1e-3, max_iter: int = 100, reg_covar: float = 1e-6,
             max_workspace_bytes: int = MAX_WORKSPACE_BYTES) -> Dict[str, object]:
    """The number of components of every slide by the lowest ``criterion`` ("bic" / "aic") over ``k_range`` (ties: the
    first candidate).  ``init_labels``: {k: (R, rows) labels} for every candidate, else k-means as in ``gmm``.  Returns host
    ``table`` (S, len(k_range)), ``k`` (S,) and ``k_range``; ``model``: what ``gmm`` returns for the chosen k of every
    slide (arrays padded to the largest candidate, no ``*_all``); ``fits``: the ``gmm`` result of every call made and
    ``calls``: per call the candidates it held."""
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be one of {list(CRITERIA)}, got {criterion!r}")
    cand = [int(c) for c in k_range]
    if not cand or len(set(cand)) != len(cand):
        raise ValueError(f"k_range: expected distinct candidates, got {list(k_range)}")
    dev = device("mixture")
    zd = scores_matrix(z, dev)
    rows, D = int(zd.shape[0]), int(zd.shape[1])
    off = cluster.validate_offsets(offsets, rows)
    S = off.size - 1
    seg = np.diff(off)
    for c in cand:
        cluster.k_per_segment(c, seg)
    if init_labels is not None and set(init_labels) != set(cand):
        raise ValueError(f"init_labels: expected one entry per candidate {cand}, got {sorted(init_labels)}")
    R = int(n_init) if init_labels is None else int(np.atleast_2d(np.asarray(
        init_labels[cand[0]].cpu() if isinstance(init_labels[cand[0]], Tensor) else init_labels[cand[0]])).shape[0])
    k_top = max(cand)
    per = int(call("mcl_gmm_workspace_bytes", rows, S, R, D, k_top))
    width = max(1, min(len(cand), int(max_workspace_bytes) // max(per, 1), 65535 // S))
    table = np.empty((S, len(cand)), dtype=np.float64)
    fits, calls = [], []
    for c0 in range(0, len(cand), width):
        group = cand[c0:c0 + width]
        zz = zd if len(group) == 1 else zd.contiguous().repeat(len(group), 1)       # the slides once per candidate
        oo = np.concatenate([[0]] + [off[1:] + g * rows for g in range(len(group))]).astype(np.int64)
        kk = np.repeat(np.asarray(group, dtype=np.int32), S)
        init = None
        if init_labels is not None:
            init = np.concatenate([np.atleast_2d(np.asarray(init_labels[c].cpu() if isinstance(init_labels[c], Tensor)
                                                            else init_labels[c])) for c in group], axis=1)
        fit = gmm(zz, kk, oo, covariance_type, init, n_init, seed, tol, max_iter, reg_covar)
        table[:, c0:c0 + len(group)] = fit[criterion].cpu().numpy().reshape(len(group), S).T
        fits.append(fit)
        calls.append(group)
    best = np.argmin(table, axis=1)             # the first lowest
    chosen = np.asarray(cand, dtype=np.int32)[best]
    ctype = covariance_type
    model: Dict[str, object] = {"labels": torch.empty((rows,), device=dev, dtype=torch.int32),
                                "resp": torch.zeros((rows, k_top), device=dev, dtype=torch.float64)}
    for name in _PER_SLIDE:
        src = fits[0][name]
        shape = list(src.shape[1:])
        if name in ("weights", "means") or (name in ("covariances", "precisions_cholesky") and ctype != "tied"):
            shape[0] = k_top
        model[name] = torch.zeros([S] + shape, device=dev, dtype=src.dtype)
    for s in range(S):
        ci, g = divmod(int(best[s]), width)
        fit = fits[ci]
        seg_id = g * S + s
        r0, r1 = int(fit["offsets"][seg_id]), int(fit["offsets"][seg_id + 1])
        km = int(fit["resp"].shape[1])
        model["labels"][off[s]:off[s + 1]].copy_(fit["labels"][r0:r1])
        model["resp"][off[s]:off[s + 1], :km].copy_(fit["resp"][r0:r1])
        for name in _PER_SLIDE:
            src = fit[name][seg_id]
            dst = model[name][s]
            if src.dim() == 0:
                model[name][s] = src
            elif src.shape == dst.shape:
                dst.copy_(src)
            else:
                dst[:src.shape[0]].copy_(src)
    model.update(k=chosen, offsets=off, covariance_type=ctype)
    return {"table": table, "k": chosen, "k_range": cand, "criterion": criterion, "model": model, "fits": fits,
            "calls": calls}


def validity(z: ArrayLike, labels: ArrayLike, offsets: Optional[Sequence[int]] = None) -> Dict[str, object]:
    """Internal validity of a labelling of the rows of ``z`` (rows, D <= 64) fp64: device ``silhouette_samples`` (rows,)
    (sklearn's, Euclidean; NaN for a row labelled -1) and host ``silhouette``, ``calinski_harabasz``, ``davies_bouldin``
    (S,).  Labels are integers in [0, 1024); -1 drops the row.  2 .. 50 000 rows per segment."""
    dev = device("mixture")
    zd = scores_matrix(z, dev)
    rows, D = int(zd.shape[0]), int(zd.shape[1])
    off = cluster.validate_offsets(offsets, rows, min_rows=2)
    t = labels if isinstance(labels, Tensor) else torch.as_tensor(np.asarray(labels))
    if t.dim() != 1 or t.shape[0] != rows:
        raise ValueError(f"labels: expected a ({rows},) vector, got shape {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"labels: expected integer labels, got {t.dtype}")
    if not t.is_cuda:
        if t.numel() and (int(t.min()) < -1 or int(t.max()) >= MAX_LABEL):
            raise ValueError(f"labels: values must lie in [0, {MAX_LABEL}), or be -1 for a dropped row")
        t = t.to(torch.int32).contiguous().to(dev)
    elif t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError("labels: device labels must be a contiguous int32 vector")
    S = off.size - 1
    wb = call("mcl_cluster_validity_workspace_bytes", rows, S, D)
    work = torch.empty((wb // 8,), device=dev, dtype=torch.float64)
    sil = torch.empty((rows,), device=dev, dtype=torch.float64)
    scores = torch.empty((S, 3), device=dev, dtype=torch.float64)
    call("mcl_cluster_validity", zd, zd.stride(0), upload(off, dev), S, rows, D, t, work, wb, sil, scores)
    h = scores.cpu().numpy()
    return {"silhouette_samples": sil, "silhouette": h[:, 0].copy(), "calinski_harabasz": h[:, 1].copy(),
            "davies_bouldin": h[:, 2].copy()}


# ------------------------------------------------------------------------------------------------- slides end to end
def _domains(xs: Sequence[ArrayLike], k, k_range, n_comps, pca_solver, kw) -> Dict[str, object]:
    dev = device("mixture")
    x, off = stack_rows(xs, "slides", dev)
    z = cluster.pca_scores(x, off, n_comps, pca_solver)
    if k is not None:
        model = gmm(z, k, off, **kw)
    else:
        lo, hi = int(k_range[0]), int(k_range[1])
        model = select_k(z, list(range(lo, hi + 1)), off, **kw)["model"]
    val = validity(z, model["labels"], off)
    return {"model": model, "validity": val, "offsets": off, "scores": z}


def domains_slides(preds: Sequence[ArrayLike], trues: Optional[Sequence[ArrayLike]] = None,
                   k: Union[None, int, Sequence[int]] = None, k_range: Sequence[int] = (2, 12),
                   n_comps: int = cluster.N_COMPS, pca_solver: str = "host", covariance_type: str = "full",
                   n_init: int = 1, seed: int = 0, tol: float = 1e-3, max_iter: int = 100,
                   reg_covar: float = 1e-6) -> Dict[str, object]:
    """Spatial domains of slides nobody annotated.  Per slide: PCA scores of the (spots, genes) prediction -> a Gaussian
    mixture with ``k`` components, or the k of lowest BIC over ``k_range`` = (lo, hi) inclusive -> validity indices.  With
    ``trues`` the same runs on the measured matrices and every slide also gets ``ari`` / ``nmi`` between the two sets of
    domains (``cluster.cluster_scores``; unrounded).  Returns ``slides``: per slide ``k``, ``bic``, ``silhouette``,
    ``calinski_harabasz``, ``davies_bouldin``, ``labels`` (spots,) int32 and ``proba`` (spots, k) as numpy arrays, and with
    ``trues`` the same keys with the prefix ``true_``."""
    if not len(preds):
        raise ValueError("need at least one slide")
    if trues is not None and len(trues) != len(preds):
        raise ValueError(f"need one measured matrix per prediction; got {len(trues)} and {len(preds)}")
    kw = dict(covariance_type=covariance_type, n_init=n_init, seed=seed, tol=tol, max_iter=max_iter, reg_covar=reg_covar)
    sides = [("", _domains(preds, k, k_range, n_comps, pca_solver, kw))]
    if trues is not None:
        for i, (p, t) in enumerate(zip(preds, trues)):
            if int(p.shape[0]) != int(t.shape[0]):
                raise ValueError(f"slide {i}: prediction and measurement differ in spots: {p.shape[0]} and {t.shape[0]}")
        sides.append(("true_", _domains(trues, k, k_range, n_comps, pca_solver, kw)))
    slides: List[Dict[str, object]] = [{} for _ in preds]
    for prefix, side in sides:
        m, v, off = side["model"], side["validity"], side["offsets"]
        lab, resp = m["labels"].cpu().numpy(), m["resp"].cpu().numpy()
        bic = m["bic"].cpu().numpy()
        for i, sl in enumerate(slides):
            ki = int(np.asarray(m["k"]).reshape(-1)[i])
            sl.update({prefix + "k": ki, prefix + "bic": float(bic[i]), prefix + "silhouette": float(v["silhouette"][i]),
                       prefix + "calinski_harabasz": float(v["calinski_harabasz"][i]),
                       prefix + "davies_bouldin": float(v["davies_bouldin"][i]),
                       prefix + "labels": lab[off[i]:off[i + 1]].copy(),
                       prefix + "proba": resp[off[i]:off[i + 1], :ki].copy()})
    if trues is not None:
        ari, nmi = cluster.cluster_scores(sides[1][1]["model"]["labels"], sides[0][1]["model"]["labels"],
                                          sides[0][1]["offsets"])
        for i, sl in enumerate(slides):
            sl["ari"], sl["nmi"] = float(ari[i]), float(nmi[i])
    return {"slides": slides}


# --------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.mixture",
                                description="Gaussian-mixture spatial domains of predicted expression: PCA scores, EM, "
                                            "BIC over k, silhouette / Calinski-Harabasz / Davies-Bouldin")
    p.add_argument("--pred", required=True, nargs="+", help="one (spots, genes) .npy per slide")
    p.add_argument("--true", nargs="+", default=None, help="one measured (spots, genes) .npy per slide, same order: "
                                                           "also ARI / NMI between the two sets of domains")
    p.add_argument("--k", type=int, default=None, help="the number of components (default: chosen by BIC over --k_range)")
    p.add_argument("--k_range", type=int, nargs=2, default=(2, 12), metavar=("LO", "HI"))
    p.add_argument("--covariance_type", choices=sorted(COVARIANCE_TYPES), default="full")
    p.add_argument("--n_comps", type=int, default=cluster.N_COMPS)
    p.add_argument("--n_init", type=int, default=1, help="k-means starts per mixture, the best lower bound wins")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--pca_solver", choices=cluster.SOLVERS, default="host")
    p.add_argument("--out_dir", default=None, help="write <out_dir>/<i>/gmm_labels.npy and gmm_proba.npy per slide")
    a = p.parse_args(argv)
    if a.true is not None and len(a.true) != len(a.pred):
        p.error(f"{len(a.pred)} --pred files but {len(a.true)} --true files")
    return a


def format_report(res: Dict[str, object]) -> str:
    """One line per slide: k, bic, silhouette, CH, DB, and ARI / NMI where there is a measurement.  ``repr`` of the
    floats: the printed numbers are the API's."""
    lines = []
    for i, s in enumerate(res["slides"]):
        line = (f"slide {i}: k: {s['k']}, bic: {s['bic']!r}, silhouette: {s['silhouette']!r}, "
                f"CH: {s['calinski_harabasz']!r}, DB: {s['davies_bouldin']!r}")
        if "ari" in s:
            line += f", ARI: {s['ari']!r}, NMI: {s['nmi']!r}"
        lines.append(line)
    return "\n".join(lines)


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    preds = [np.load(f) for f in a.pred]
    trues = [np.load(f) for f in a.true] if a.true is not None else None
    res = domains_slides(preds, trues, a.k, a.k_range, a.n_comps, a.pca_solver, a.covariance_type, a.n_init, a.seed)
    print(format_report(res))
    if a.out_dir:
        for i, s in enumerate(res["slides"]):
            d = os.path.join(a.out_dir, str(i))
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, "gmm_labels.npy"), s["labels"])
            np.save(os.path.join(d, "gmm_proba.npy"), s["proba"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
