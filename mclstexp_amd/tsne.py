"""Exact t-SNE of spots in two dimensions on the MI355X: the embedding the reference's ``cluster(adata, label)`` computes
with ``sc.tl.tsne(tmp)`` (utils.py:67-79) and its users look at, all slides of an evaluation per call.

What is reproduced is sklearn's exact path (``sklearn.manifold.TSNE(method="exact", n_components=2)``; DESIGN 6.10 states
the arithmetic and ``tests/tsne_reference.py`` restates it in numpy): per-row precision search to the perplexity, joint
probabilities, 250 iterations at ``early_exaggeration`` with momentum 0.5, then momentum 0.8 up to ``n_iter``, sklearn's
gains and its two stopping tests every 50 iterations.  Every segment (slide) of the row-stacked input is embedded on its
own.  Things to know:

* O(n^2) memory and time: one (n_s, n_s) fp64 matrix per slide.  2 <= n_s <= 16384, the sum of n_s^2 at most 2^31
  (BLEEP's 9269 spots as one segment: 0.7 GB), D <= 64.  No Barnes-Hut, no other metric, two components only.
* Squared distances are direct sums of squared differences in fp64.  ``float32_distances=True`` rounds them to float32 as
  sklearn does before its search; the default keeps fp64.
* ``learning_rate="auto"`` is sklearn's ``max(n_s / early_exaggeration / 4, 50)`` per slide (scanpy's habitual 1000 makes
  small slides blow up).
* ``init``: ``"pca"`` (the first two ``cluster.pca_device`` scores, scaled so that the first has population standard
  deviation 1e-4; needs D >= 3), ``"random"`` (sklearn's draw: 1e-4 x ``RandomState(random_state).standard_normal``
  rounded through float32, one draw per slide in order) or a (rows, 2) array, replayed exactly.
* The host reads two doubles per slide every 50 iterations to apply the stopping tests; nothing else leaves the device.
  A slide that meets a stop in the first phase moves on to the second, one that meets it there is frozen, as in sklearn.
  ``n_iter`` reports the iterations a slide performed.

Everything on the device is fp64, atomics-free and bit-reproducible run to run; a slide inside a batch is bit-identical to
the same slide alone.  No CPU fallback.

    python -m mclstexp_amd.tsne --pred P1.npy ... [--labels L1.npy ...] [--n_pcs 9] [--perplexity 30] [--out_dir D]
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _arrays, cluster
from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, check_columns, cumulative_offsets, dense, device, empty, matrix,
                      stack_rows, upload)
from ._lib import call

MAX_DIM = 64             # csrc/tsne.hip
MAX_ROWS = 16384         # per segment: one row of distances lives in LDS
MAX_PAIRS = 2 ** 31      # the sum of n_s^2
MAX_SEGMENTS = 65535
EXPLORATION_ITERS = 250  # sklearn's _EXPLORATION_MAX_ITER: the exaggerated phase
CHECK_EVERY = 50         # sklearn's _N_ITER_CHECK
PATIENCE = (250, 300)    # iterations without progress: the first phase, then TSNE's n_iter_without_progress default
MIN_GRAD_NORM = 1e-7
MOMENTUM = (0.5, 0.8)
OUT_FILE = "X_tsne.npy"


# ------------------------------------------------------------------------------------------------------- host rules
def validate_offsets(offsets: Optional[Sequence[int]], rows: int) -> np.ndarray:
    """offsets[0] = 0, offsets[-1] = rows, every segment holds 2 .. 16384 rows, the n_s^2 sum to at most 2^31."""
    off = _arrays.validate_offsets(offsets, rows, 2, MAX_ROWS, max_segments=MAX_SEGMENTS, none_is_one=True)
    pairs = int((np.diff(off) ** 2).sum())
    if pairs > MAX_PAIRS:
        raise ValueError(f"the segments hold {pairs} pairs (sum of n_s^2); the kernels handle at most 2^31")
    return off


def learning_rates(learning_rate: Union[str, float], seg: np.ndarray, early_exaggeration: float) -> np.ndarray:
    """One learning rate per segment: sklearn's "auto" (max(n_s / early_exaggeration / 4, 50)) or the given number."""
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError(f"learning_rate must be 'auto' or a positive number, got {learning_rate!r}")
        return np.maximum(seg / float(early_exaggeration) / 4.0, 50.0)
    lr = float(learning_rate)
    if not lr > 0:
        raise ValueError(f"learning_rate must be 'auto' or a positive number, got {learning_rate!r}")
    return np.full(seg.size, lr)


def random_init(seg: np.ndarray, random_state: int) -> np.ndarray:
    """sklearn's random initialisation, one draw per segment in order from one ``RandomState(random_state)``."""
    rng = np.random.RandomState(random_state)
    return np.concatenate([(1e-4 * rng.standard_normal(size=(int(n), 2)).astype(np.float32)).astype(np.float64)
                           for n in seg])


def scale_pca_init(scores: np.ndarray, off: np.ndarray) -> np.ndarray:
    """sklearn's scaling of a PCA initialisation: per segment, column 0 gets population standard deviation 1e-4."""
    out = np.array(scores[:, :2], dtype=np.float64)
    for s in range(off.size - 1):
        part = out[off[s]:off[s + 1]]
        part /= np.std(part[:, 0]) / 1e-4
    return out


class Schedule:
    """sklearn's two ``_gradient_descent`` calls per segment: which parameters an iteration runs with and what the
    checks every 50 iterations decide.  Pure host bookkeeping."""

    def __init__(self, seg: np.ndarray, n_iter: int, early_exaggeration: float, lr: np.ndarray):
        S = seg.size
        self.n_total = int(n_iter)
        self.switch = min(EXPLORATION_ITERS, self.n_total)
        self.exaggeration = float(early_exaggeration)
        self.lr = np.asarray(lr, dtype=np.float64)
        self.phase = np.zeros(S, dtype=np.int64)
        self.active = np.ones(S, dtype=bool)
        self.reset = np.zeros(S, dtype=bool)
        self.best_error = np.full(S, np.finfo(float).max)
        self.best_iter = np.zeros(S, dtype=np.int64)
        self.n_iter = np.full(S, self.n_total, dtype=np.int64)
        self.kl = np.full(S, np.nan)

    def params(self) -> np.ndarray:
        """(S, 5): exaggeration, momentum, learning rate, active, reset -- the kernels' per-segment table."""
        first = self.phase == 0
        return np.stack([np.where(first, self.exaggeration, 1.0), np.where(first, MOMENTUM[0], MOMENTUM[1]), self.lr,
                         self.active.astype(np.float64), self.reset.astype(np.float64)], axis=1)

    def _second_phase(self, s: int, it: int) -> None:
        self.phase[s], self.reset[s] = 1, True
        self.best_error[s], self.best_iter[s] = np.finfo(float).max, it

    def begin(self, it: int) -> bool:
        """Before iteration ``it``: at the end of the exaggerated phase every segment still in it moves on.  True when
        the table changed."""
        changed = False
        if it == self.switch:
            for s in np.flatnonzero(self.active & (self.phase == 0)):
                self._second_phase(int(s), it)
                changed = True
        return changed

    def after_update(self) -> bool:
        """After an iteration: a reset holds for one update only.  True when the table changed."""
        if not self.reset.any():
            return False
        self.reset[:] = False
        return True

    def wants_error(self, it: int) -> bool:
        return (it + 1) % CHECK_EVERY == 0 or it == self.n_total - 1

    def check(self, it: int, kl: np.ndarray, grad_norm2: np.ndarray) -> bool:
        """After iteration ``it`` on which the error was computed.  True when the table changed."""
        changed = False
        for s in np.flatnonzero(self.active):
            self.kl[s] = kl[s]
            if (it + 1) % CHECK_EVERY != 0:
                continue
            stop = False
            if kl[s] < self.best_error[s]:
                self.best_error[s], self.best_iter[s] = kl[s], it
            elif it - self.best_iter[s] > PATIENCE[self.phase[s]]:
                stop = True
            if not stop and np.sqrt(grad_norm2[s]) <= MIN_GRAD_NORM:
                stop = True
            if stop:
                changed = True
                if self.phase[s] == 0 and it + 1 < self.n_total:
                    self._second_phase(int(s), it + 1)
                else:
                    self.active[s], self.n_iter[s] = False, it + 1
        return changed


# ----------------------------------------------------------------------------------------------------------- device
class _Plan:
    """The offsets of one call on the device, the scalars the entry points are sized by, and the workspace."""

    def __init__(self, off: np.ndarray, dev: torch.device):
        seg = np.diff(off)
        self.off, self.seg, self.dev = off, seg, dev
        self.poff = cumulative_offsets(seg * seg)
        self.S, self.rows = int(seg.size), int(off[-1])
        self.min_n, self.max_n, self.pairs = int(seg.min()), int(seg.max()), int(self.poff[-1])
        self.off_d, self.poff_d = upload(off, dev), upload(self.poff, dev)
        self.work = empty(dev)((max(int(call("mcl_tsne_workspace_doubles", self.rows, self.S)), 8),), torch.float64)

    def affinities(self, xd: Tensor, perplexity: float, f32: bool, P: Tensor, beta: Tensor) -> None:
        call("mcl_tsne_affinities", xd, xd.stride(0), FLOAT_CODE[xd.dtype], int(xd.shape[1]), self.off_d, self.poff_d,
             self.S, self.rows, self.min_n, self.max_n, self.pairs, float(perplexity), bool(f32), self.work, P, beta)

    def gradient(self, P: Tensor, Y: Tensor, params: Tensor, want_kl: bool, grad: Tensor, kl: Tensor) -> None:
        call("mcl_tsne_gradient", P, self.poff_d, Y, self.off_d, self.S, self.rows,
             self.min_n, self.max_n, self.pairs, params, want_kl, self.work, grad, kl)

    def update(self, grad: Tensor, params: Tensor, Y: Tensor, upd: Tensor, gains: Tensor, norm2: Tensor) -> None:
        call("mcl_tsne_update", grad, self.off_d, self.S, self.rows, self.min_n, self.max_n, params, Y, upd, gains, norm2)


def _check_x(x: ArrayLike, offsets, perplexity: float):
    rows, D = check_columns(x, MAX_DIM)
    off = validate_offsets(offsets, rows)
    seg = np.diff(off)
    if not perplexity > 0 or perplexity >= seg.min():
        raise ValueError(f"perplexity must be positive and less than the rows of every segment; got {perplexity}, "
                         f"segment sizes {seg.tolist()}")
    return off, seg, D


def _segment_table(v: Union[float, Sequence[float]], S: int, name: str) -> np.ndarray:
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(S, float(a))
    if a.shape != (S,):
        raise ValueError(f"{name}: a number or one value per segment ({S}), got shape {a.shape}")
    return a


def joint_probabilities(x: ArrayLike, offsets: Optional[Sequence[int]] = None, perplexity: float = 30.0,
                        float32_distances: bool = False) -> Dict[str, object]:
    """The joint probabilities of every segment of the row-stacked (rows, D <= 64) matrix ``x`` (fp32 / fp64, host or
    device, a row stride allowed): device ``P`` (the (n_s, n_s) matrices one after the other, flat, fp64; ``P_s`` is
    ``P[pair_offsets[s]:pair_offsets[s + 1]].view(n_s, n_s)``), ``beta`` (rows,), host ``offsets`` and ``pair_offsets``."""
    off, seg, _ = _check_x(x, offsets, perplexity)
    dev = device("tsne")
    plan = _Plan(off, dev)
    xd = matrix(x, "x", dev, FLOAT_CODE, torch.float64)
    e = empty(dev)
    P, beta = e((plan.pairs,), torch.float64), e((plan.rows,), torch.float64)
    plan.affinities(xd, perplexity, float32_distances, P, beta)
    return {"P": P, "beta": beta, "offsets": off, "pair_offsets": plan.poff, "_plan": plan}


def gradient(P: ArrayLike, Y: ArrayLike, offsets: Optional[Sequence[int]] = None,
             exaggeration: Union[float, Sequence[float]] = 1.0, kl: bool = True):
    """``(grad, kl)`` at the embedding ``Y`` (rows, 2): device (rows, 2) and (S,) fp64 (``kl=False``: ``None``).  ``P``
    as ``joint_probabilities`` returns it (one (n, n) matrix is accepted for a single segment); the sums run over
    ``exaggeration * P`` (a number or one per segment)."""
    rows = int(Y.shape[0])
    off = validate_offsets(offsets, rows)
    seg = np.diff(off)
    pairs = int((seg * seg).sum())
    n_p = int(np.prod(tuple(P.shape)))
    if n_p != pairs:
        raise ValueError(f"P holds {n_p} entries; the segments {seg.tolist()} need {pairs}")
    ex = _segment_table(exaggeration, seg.size, "exaggeration")
    dev = device("tsne")
    plan = _Plan(off, dev)
    Pd = dense(P, "P", tuple(P.shape), torch.float64, dev)
    Yd = dense(Y, "Y", (rows, 2), torch.float64, dev)
    params = np.stack([ex, np.zeros_like(ex), np.zeros_like(ex), np.ones_like(ex), np.zeros_like(ex)], axis=1)
    e = empty(dev)
    grad, kl_d = e((rows, 2), torch.float64), e((plan.S,), torch.float64)
    plan.gradient(Pd, Yd, upload(params, dev), kl, grad, kl_d)
    return grad, (kl_d if kl else None)


def update(Y: ArrayLike, grad: ArrayLike, upd: ArrayLike, gains: ArrayLike, offsets: Optional[Sequence[int]] = None,
           momentum: Union[float, Sequence[float]] = 0.8, learning_rate: Union[float, Sequence[float]] = 200.0):
    """One step of sklearn's ``_gradient_descent`` from a given state: new device ``(Y, update, gains)`` (rows, 2) and the
    squared norm of the gain-scaled gradient per segment (S,).  The arguments are left as they are."""
    rows = int(Y.shape[0])
    off = validate_offsets(offsets, rows)
    S = off.size - 1
    m, lr = _segment_table(momentum, S, "momentum"), _segment_table(learning_rate, S, "learning_rate")
    dev = device("tsne")
    plan = _Plan(off, dev)
    Yd, ud, gd = (dense(a, n, (rows, 2), torch.float64, dev, copy=True)
                  for a, n in ((Y, "Y"), (upd, "update"), (gains, "gains")))
    g = dense(grad, "grad", (rows, 2), torch.float64, dev)
    params = np.stack([np.ones(S), m, lr, np.ones(S), np.zeros(S)], axis=1)
    norm2 = empty(dev)((S,), torch.float64)
    plan.update(g, upload(params, dev), Yd, ud, gd, norm2)
    return Yd, ud, gd, norm2


def tsne(x: ArrayLike, offsets: Optional[Sequence[int]] = None, perplexity: float = 30.0,
         early_exaggeration: float = 12.0, learning_rate: Union[str, float] = "auto", n_iter: int = 1000,
         init: Union[str, ArrayLike] = "pca", random_state: int = 0,
         float32_distances: bool = False, pca_solver: str = "host") -> Dict[str, object]:
    """Exact t-SNE of every segment of the row-stacked (rows, D <= 64) matrix ``x`` (see the module docstring).  Returns
    device ``embedding`` (rows, 2) fp64 and ``beta`` (rows,), host ``kl_divergence`` (S,), ``n_iter`` (S,) and
    ``offsets``.  ``pca_solver``: the eigensolver of the ``"pca"`` start (``cluster.pca_device``'s ``solver``)."""
    if pca_solver not in cluster.SOLVERS:
        raise ValueError(f"pca_solver must be one of {cluster.SOLVERS}, got {pca_solver!r}")
    off, seg, D = _check_x(x, offsets, perplexity)
    rows, S = int(off[-1]), seg.size
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError(f"n_iter must be >= 1, got {n_iter}")
    if not early_exaggeration >= 1.0:
        raise ValueError(f"early_exaggeration must be >= 1, got {early_exaggeration}")
    lr = learning_rates(learning_rate, seg, early_exaggeration)
    y0 = None
    if isinstance(init, str):
        if init not in ("pca", "random"):
            raise ValueError(f"init must be 'pca', 'random' or a (rows, 2) array, got {init!r}")
        if init == "pca" and (D < 3 or seg.min() < 3):
            raise ValueError(f"init='pca' needs D >= 3 and >= 3 rows per segment (two components); got D = {D}, "
                             f"smallest segment {int(seg.min())}")
        if init == "random":
            y0 = random_init(seg, random_state)
    else:
        if tuple(init.shape) != (rows, 2):
            raise ValueError(f"init: expected a ({rows}, 2) array, got shape {tuple(init.shape)}")
        y0 = init
    dev = device("tsne")
    if y0 is None:
        y0 = scale_pca_init(cluster.pca_device(x, off, 2, pca_solver)["scores"].cpu().numpy(), off)
    aff = joint_probabilities(x, off, perplexity, float32_distances)
    plan, P = aff["_plan"], aff["P"]
    e = empty(dev)
    Y = dense(y0, "init", (rows, 2), torch.float64, dev, copy=True)
    grad, upd, gains = (e((rows, 2), torch.float64) for _ in range(3))
    stats = e((2, S), torch.float64)                  # kl, squared gradient norm: the one read per check
    sched = Schedule(seg, n_iter, early_exaggeration, lr)
    sched.reset[:] = True                             # update = 0, gains = 1 without a fill
    params = upload(sched.params(), dev)
    for it in range(n_iter):
        if sched.begin(it):
            params.copy_(torch.from_numpy(sched.params()))
        want = sched.wants_error(it)
        plan.gradient(P, Y, params, want, grad, stats[0])
        plan.update(grad, params, Y, upd, gains, stats[1])
        if sched.after_update():
            params.copy_(torch.from_numpy(sched.params()))
        if want:
            h = stats.cpu().numpy()
            if sched.check(it, h[0], h[1]):
                params.copy_(torch.from_numpy(sched.params()))
            if not sched.active.any():
                break
    return {"embedding": Y, "kl_divergence": sched.kl.copy(), "n_iter": sched.n_iter.copy(), "beta": aff["beta"],
            "offsets": off}


def embed_slides(matrices: Sequence[ArrayLike], n_pcs: int = cluster.N_COMPS, pca_solver: str = "host",
                 **kw) -> Dict[str, object]:
    """The reference's sequence for every slide in one call each: ``cluster.pca_scores_slides`` (``n_pcs`` components,
    eigensolver ``pca_solver``), then ``tsne`` of the scores (whose ``"pca"`` start uses the same solver).  Returns
    ``tsne``'s dict plus ``slides``: the (spots_i, 2) device views per slide."""
    parts = cluster.pca_scores_slides(matrices, n_pcs, pca_solver)
    z, off = stack_rows(parts, "scores", device("tsne"))
    res = tsne(z, off, pca_solver=pca_solver, **kw)
    res["slides"] = [res["embedding"][off[i]:off[i + 1]] for i in range(len(parts))]
    return res


# --------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.tsne",
                                description="PCA + exact t-SNE of predicted expression, one 2-D embedding per slide "
                                            "(the reference's utils.cluster: sc.pp.pca, sc.tl.tsne)")
    p.add_argument("--pred", required=True, nargs="+", help="one (spots, genes) .npy per slide")
    p.add_argument("--labels", nargs="+", default=None,
                   help="one (spots,) .npy of annotations per slide: undetermined spots are dropped as in cluster")
    p.add_argument("--undetermined", default="undetermined")
    p.add_argument("--n_pcs", type=int, default=cluster.N_COMPS)
    p.add_argument("--perplexity", type=float, default=30.0)
    p.add_argument("--early_exaggeration", type=float, default=12.0)
    p.add_argument("--learning_rate", default="auto", help="'auto' (sklearn's rule) or a number")
    p.add_argument("--n_iter", type=int, default=1000)
    p.add_argument("--init", default="pca", choices=("pca", "random"))
    p.add_argument("--random_state", type=int, default=0)
    p.add_argument("--out_dir", default=".", help=f"writes OUT_DIR/<slide number from 1>/{OUT_FILE}")
    a = p.parse_args(argv)
    if a.labels is not None and len(a.labels) != len(a.pred):
        p.error(f"{len(a.pred)} --pred files but {len(a.labels)} --labels files")
    if a.learning_rate != "auto":
        try:
            a.learning_rate = float(a.learning_rate)
        except ValueError:
            p.error(f"--learning_rate must be 'auto' or a number, got {a.learning_rate!r}")
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    preds: List[np.ndarray] = [np.load(f) for f in a.pred]
    if a.labels is not None:
        for i, f in enumerate(a.labels):
            lab = np.load(f, allow_pickle=False)
            if preds[i].ndim != 2 or preds[i].shape[0] != len(lab):
                raise ValueError(f"slide {i}: prediction {preds[i].shape} and {len(lab)} labels do not match")
            preds[i] = preds[i][cluster.encode_labels(lab, a.undetermined)[0]]
    res = embed_slides(preds, a.n_pcs, perplexity=a.perplexity, early_exaggeration=a.early_exaggeration,
                       learning_rate=a.learning_rate, n_iter=a.n_iter, init=a.init, random_state=a.random_state)
    for i, y in enumerate(res["slides"]):
        path = os.path.join(a.out_dir, str(i + 1))
        os.makedirs(path, exist_ok=True)
        np.save(os.path.join(path, OUT_FILE), y.cpu().numpy())
        print(f"slide {i + 1}: {tuple(preds[i].shape)} -> {os.path.join(path, OUT_FILE)} {tuple(y.shape)}, "
              f"KL {res['kl_divergence'][i]:.6g} after {int(res['n_iter'][i])} iterations")
    return 0


if __name__ == "__main__":
    sys.exit(main())
