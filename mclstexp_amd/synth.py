"""Procedural (formula-generated) weights and inputs.

Every value is a pure function of (tensor name, flat index, seed) through a splitmix64
hash, so the 2 x (65536, G) position tables never have to be stored or shipped: tests on
the GPU box, the golden generator in the build container and ``bench.py`` all regenerate
bit-identical fp32 data from the same formula, independent of any torch/numpy RNG.

Shapes/keys follow the reference's ``state_dict``.
"""
from __future__ import annotations

import math
import zlib
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        x = x ^ (x >> np.uint64(31))
    return x


def name_seed(name: str, seed: int = 0) -> int:
    return (zlib.crc32(name.encode()) + 0x1000003 * seed) & 0xFFFFFFFF


def uniform01(name: str, idx: np.ndarray, seed: int = 0) -> np.ndarray:
    """u in [0,1) with 24 random bits (exactly representable in fp32)."""
    with np.errstate(over="ignore"):
        key = (idx.astype(np.uint64) + (np.uint64(name_seed(name, seed)) << np.uint64(32))) & _M64
    h = _splitmix64(key)
    return ((h >> np.uint64(40)).astype(np.float32)) * np.float32(1.0 / (1 << 24))


def uniform_tensor(name: str, shape: Sequence[int], lo: float, hi: float, seed: int = 0,
                   rows: Optional[np.ndarray] = None) -> torch.Tensor:
    """fp32 tensor of ``shape`` uniform in [lo, hi).  With ``rows`` (for 2-D shapes) only the
    listed rows are generated -> shape (len(rows), shape[1]) -- the same values the full
    tensor holds at those rows."""
    if rows is None:
        n = int(np.prod(shape)) if len(shape) else 1
        idx = np.arange(n, dtype=np.uint64)
        out_shape = tuple(shape)
    else:
        cols = int(shape[1])
        idx = (np.asarray(rows, dtype=np.uint64)[:, None] * np.uint64(cols)
               + np.arange(cols, dtype=np.uint64)[None, :]).reshape(-1)
        out_shape = (len(rows), cols)
    u = uniform01(name, idx, seed)
    v = (np.float32(lo) + u * np.float32(hi - lo)).astype(np.float32)
    return torch.from_numpy(v.reshape(out_shape))


SQRT3 = math.sqrt(3.0)


def param_spec(spot_dim: int, image_dim: int, projection_dim: int = 256, heads: int = 8,
               dim_head: int = 64, layers: int = 2, with_tables: bool = True,
               table_rows: int = 65536) -> Dict[str, Tuple[Tuple[int, ...], float, float]]:
    """name -> (shape, lo, hi) for every non-backbone parameter of mclSTExp_Attention
    (/root/reference/model.py:201-223).  Ranges mimic the module defaults' magnitudes:
    Linear U(-1/sqrt(in), 1/sqrt(in)); LayerNorm weight 1 +- 0.05, bias +- 0.05 (perturbed
    so that their gradients are exercised); Embedding unit variance."""
    G, D, P, inner = spot_dim, image_dim, projection_dim, heads * dim_head
    spec: Dict[str, Tuple[Tuple[int, ...], float, float]] = {}
    if with_tables:
        spec["x_embed.weight"] = ((table_rows, G), -SQRT3, SQRT3)
        spec["y_embed.weight"] = ((table_rows, G), -SQRT3, SQRT3)
    for l in range(layers):
        q = f"spot_encoder.{l}."
        kG, kI = 1.0 / math.sqrt(G), 1.0 / math.sqrt(inner)
        spec[q + "attn.norm.weight"] = ((G,), 0.95, 1.05)
        spec[q + "attn.norm.bias"] = ((G,), -0.05, 0.05)
        spec[q + "attn.fn.to_qkv.weight"] = ((3 * inner, G), -kG, kG)
        spec[q + "attn.fn.to_out.0.weight"] = ((G, inner), -kI, kI)
        spec[q + "attn.fn.to_out.0.bias"] = ((G,), -kI, kI)
        spec[q + "ff.norm.weight"] = ((G,), 0.95, 1.05)
        spec[q + "ff.norm.bias"] = ((G,), -0.05, 0.05)
        spec[q + "ff.fn.net.0.weight"] = ((G, G), -kG, kG)
        spec[q + "ff.fn.net.0.bias"] = ((G,), -kG, kG)
        spec[q + "ff.fn.net.3.weight"] = ((G, G), -kG, kG)
        spec[q + "ff.fn.net.3.bias"] = ((G,), -kG, kG)
    for head, d_in in (("image_projection.", D), ("spot_projection.", G)):
        k1, k2 = 1.0 / math.sqrt(d_in), 1.0 / math.sqrt(P)
        spec[head + "projection.weight"] = ((P, d_in), -k1, k1)
        spec[head + "projection.bias"] = ((P,), -k1, k1)
        spec[head + "fc.weight"] = ((P, P), -k2, k2)
        spec[head + "fc.bias"] = ((P,), -k2, k2)
        spec[head + "layer_norm.weight"] = ((P,), 0.95, 1.05)
        spec[head + "layer_norm.bias"] = ((P,), -0.05, 0.05)
    return spec


def make_params(spot_dim: int, image_dim: int, projection_dim: int = 256, heads: int = 8,
                dim_head: int = 64, layers: int = 2, seed: int = 0, with_tables: bool = True,
                table_rows: int = 65536) -> Dict[str, torch.Tensor]:
    spec = param_spec(spot_dim, image_dim, projection_dim, heads, dim_head, layers, with_tables, table_rows)
    return {k: uniform_tensor(k, shp, lo, hi, seed) for k, (shp, lo, hi) in spec.items()}


def make_batch(batch: int, spot_dim: int, image_dim: Optional[int] = None, image_hw: Optional[int] = None,
               seed: int = 0, grid: int = 64, rank: int = 0) -> Dict[str, torch.Tensor]:
    """Synthetic batch in the reference's batch contract (dataset.py:188-195,226-231):
    ``expression`` ~70 % zeros, else log10(1+x)-like values in (0, 4); ``position`` integer-valued
    floats in [0, grid)^2; ``image`` either (B, D) precomputed features (image_dim) or
    (B, 3, H, W) uniform[0,1) pixels (image_hw)."""
    tag = f"@r{rank}"
    u = uniform_tensor("expression" + tag, (batch, spot_dim), 0.0, 1.0, seed)
    expr = torch.where(u < 0.7, torch.zeros_like(u), (u - 0.7) * (4.0 / 0.3))
    pos = torch.floor(uniform_tensor("position" + tag, (batch, 2), 0.0, float(grid), seed))
    out = {"expression": expr.contiguous(), "position": pos.contiguous()}
    if image_dim is not None:
        out["image"] = uniform_tensor("image_features" + tag, (batch, image_dim), -1.0, 1.0, seed)
    elif image_hw is not None:
        out["image"] = uniform_tensor("image" + tag, (batch, 3, image_hw, image_hw), 0.0, 1.0, seed)
    return out


def make_retrieval_case(n_keys: int, n_query: int, dim: int = 256, genes: int = 785, clusters: int = 24,
                        seed: int = 0, duplicates: int = 0) -> Dict[str, np.ndarray]:
    """Synthetic inference-time retrieval problem in the layout the reference's eval scripts hold after their
    transposes (evel_her2st.py:158-172): ``spot_key`` (N, dim) and ``image_query`` (Q, dim) un-normalised
    projection-head outputs (cluster centre + noise, so the cosine top-k is structured like real embeddings),
    ``expression_key`` (N, genes) log-normalised expression (~60 % zeros).  ``duplicates`` > 0 makes the last
    ``duplicates`` keys exact copies of key 0 (ties in the similarity)."""
    cen = uniform_tensor("retr.centres", (clusters, dim), -1.0, 1.0, seed).numpy()
    kc = np.floor(uniform_tensor("retr.key_cluster", (n_keys,), 0.0, float(clusters), seed).numpy()).astype(np.int64)
    qc = np.floor(uniform_tensor("retr.query_cluster", (n_query,), 0.0, float(clusters), seed).numpy()).astype(np.int64)
    key = cen[kc] + 0.8 * uniform_tensor("retr.key_noise", (n_keys, dim), -1.0, 1.0, seed).numpy()
    qry = cen[qc] + 0.8 * uniform_tensor("retr.query_noise", (n_query, dim), -1.0, 1.0, seed).numpy()
    u = uniform_tensor("retr.expression", (n_keys, genes), 0.0, 1.0, seed).numpy()
    expr = np.where(u < 0.6, np.float32(0.0), (u - np.float32(0.6)) * np.float32(10.0)).astype(np.float32)
    key = key.astype(np.float32)
    if duplicates:
        key[n_keys - duplicates:] = key[0]
    return {"spot_key": np.ascontiguousarray(key), "image_query": np.ascontiguousarray(qry.astype(np.float32)),
            "expression_key": np.ascontiguousarray(expr)}


def make_eval_case(segments: Sequence[int], genes: int, seed: int = 0, const_true: Sequence[int] = (),
                   const_pred: Sequence[int] = (), heg_const: bool = False) -> Dict[str, np.ndarray]:
    """Synthetic scoring problem for ``mclstexp_amd.evaluate``: folds of ``segments[i]`` spots stacked row-wise.
    ``true`` (rows, genes) is log-normalised expression (~60 % zeros, a per-gene scale so the gene means spread out);
    ``pred`` (rows, genes) is 0.5 * true + uniform noise, like a k-NN average of expression rows.  Both float64 (the
    reference's prediction buffers are ``np.zeros`` float64).  Columns in ``const_true`` / ``const_pred`` are constant
    (Pearson r undefined -> NaN); ``heg_const`` makes the last gene a constant column with the largest true mean (so
    it is one of the highest-expressed genes).  ``offsets`` (len(segments) + 1,) int64 are the fold boundaries."""
    rows = int(sum(segments))
    u = uniform_tensor("eval.true", (rows, genes), 0.0, 1.0, seed).numpy().astype(np.float64)
    scale = 0.2 + 3.0 * uniform_tensor("eval.gene_scale", (genes,), 0.0, 1.0, seed).numpy().astype(np.float64)
    true = np.where(u < 0.6, 0.0, (u - 0.6) * 10.0) * scale[None, :]
    noise = uniform_tensor("eval.pred_noise", (rows, genes), 0.0, 2.0, seed).numpy().astype(np.float64)
    pred = 0.5 * true + noise
    for g in const_true:
        true[:, g] = 1.5
    for g in const_pred:
        pred[:, g] = 0.75
    if heg_const:
        true[:, genes - 1] = 2.0 * float(true.mean(axis=0).max()) + 1.0
    offsets = np.concatenate([[0], np.cumsum(np.asarray(segments, dtype=np.int64))]).astype(np.int64)
    return {"pred": np.ascontiguousarray(pred), "true": np.ascontiguousarray(true), "offsets": offsets}


def make_cluster_case(n: int, genes: int, k: int, seed: int = 0, sep: float = 0.1,
                      undetermined_frac: float = 0.1) -> Dict[str, np.ndarray]:
    """Synthetic spatial-domain clustering problem for ``mclstexp_amd.cluster``: ``k`` latent cluster programmes (12
    factors, scale ``sep``) times random gene loadings plus unit noise on a per-gene baseline, ``log1p`` of the positive
    part -- ``pred`` (n, genes) float64, shaped like a predicted log-expression matrix.  ``label`` (n,) holds the
    cluster of every spot as a string ('0' .. str(k - 1)) with a fraction ``undetermined_frac`` replaced by
    'undetermined' (the annotation the reference's cluster() drops); ``truth`` (n,) int64 is the cluster of every spot.
    Drawn from ``numpy.random.default_rng(seed)`` (unlike the hash-generated tensors above: the draws are normal)."""
    r = np.random.default_rng(seed)
    truth = r.integers(0, k, n)
    prog = r.standard_normal((k, 12)) * sep
    load = r.standard_normal((12, genes))
    base = np.abs(r.standard_normal(genes)) * 2
    x = base + prog[truth] @ load * 0.5 + r.standard_normal((n, genes)) * 1.0
    x = np.log1p(np.maximum(x, 0))
    und = r.random(n) < undetermined_frac
    label = truth.astype(str).astype(object)
    label[und] = "undetermined"
    return {"pred": np.ascontiguousarray(x), "label": label.astype(str), "truth": truth.astype(np.int64)}


def make_counts_case(spots: int, genes: int, seed: int = 0, zero_genes: int = 0, zero_spot: bool = False,
                     top_gene: bool = False, duplicate: Optional[Tuple[int, int]] = None,
                     dtype=np.int32) -> Dict[str, np.ndarray]:
    """Synthetic raw count table for ``mclstexp_amd.preprocess``: ``counts`` (spots, genes), negative-binomial with mean
    ``depth_i * mean_g`` and dispersion ``disp_g`` (variance = mu + disp * mu^2).  ``mean`` (log-uniform over
    exp(-4) .. exp(2.5)), ``disp`` (0.1 .. 2) and ``depth`` (0.5 .. 2) come from the counter-based generator above, and so
    does the uniform draw behind every count (inverse CDF by the pmf recursion in fp64): no NumPy random stream.
    ``zero_genes``: that many evenly spread all-zero columns; ``zero_spot``: spot 1 holds no count; ``top_gene``: the last
    gene gets 40 x the largest mean, alone in the top mean bin; ``duplicate`` = (a, b): column b is a copy of column a."""
    tag = f"counts.{spots}x{genes}"
    mean = np.exp(uniform_tensor(tag + ".mean", (genes,), -4.0, 2.5, seed).numpy().astype(np.float64))
    disp = uniform_tensor(tag + ".disp", (genes,), 0.1, 2.0, seed).numpy().astype(np.float64)
    depth = uniform_tensor(tag + ".depth", (spots,), 0.5, 2.0, seed).numpy().astype(np.float64)
    if top_gene:
        mean[genes - 1] = 40.0 * mean[:genes - 1].max()
        disp[genes - 1] = 0.5
    u = uniform_tensor(tag + ".u", (spots, genes), 0.0, 1.0, seed).numpy().astype(np.float64).reshape(-1)
    mu = (depth[:, None] * mean[None, :]).reshape(-1)
    r = np.broadcast_to(1.0 / disp[None, :], (spots, genes)).reshape(-1)
    q = mu / (r + mu)
    pmf = np.exp(r * np.log1p(-q))                       # P(0) = (r / (r + mu))^r
    cdf = pmf.copy()
    k = np.zeros(u.shape, dtype=np.int64)
    live = np.flatnonzero(u >= cdf)
    step = 0
    while live.size and step < 100000:                   # P(k + 1) = P(k) (k + r) / (k + 1) q
        pmf[live] *= (step + r[live]) / (step + 1.0) * q[live]
        cdf[live] += pmf[live]
        k[live] += 1
        step += 1
        live = live[(u[live] >= cdf[live]) & (pmf[live] > 0.0)]
    counts = k.reshape(spots, genes)
    if zero_genes:
        counts[:, (np.arange(zero_genes) * genes) // zero_genes + genes // (2 * zero_genes)] = 0
    if duplicate is not None:
        counts[:, duplicate[1]] = counts[:, duplicate[0]]
    if zero_spot:
        counts[1, :] = 0
    return {"counts": np.ascontiguousarray(counts.astype(dtype)), "mean": mean, "disp": disp, "depth": depth}
