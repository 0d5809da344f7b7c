#!/usr/bin/env python3
"""Micro-benchmark of BLEEP's evaluation protocol (mclstexp_amd.bleep, retrieval.combine_device) on one MI355X, at
BLEEP's own fold size (Q = 2265 queries, N = 7004 keys, P = 256, G = 3467 genes, k = 50) and at a her2st fold's
(Q = 400, N = 12000, G = 785).  Per shape:

  * ``mcl_knn_combine`` for the three methods on device-resident matrices and given matches (HIP events), with the gathered
    bytes per second (Q k (G + P) 4 bytes);  ``average`` and ``weighted_average`` both on the dense expression matrix (its
    leading dimension G is no multiple of 4: rows are read element by element) and on a copy padded to a multiple of 4
    (16-byte row loads) -- the two load variants of the kernel on the same problem;
  * ``predict_expression`` end to end per method (retrieval + combination + results to the host; host clock);
  * the scoring sequence ``mcl_expr_metrics`` + ``mcl_cell_pearson`` + ``mcl_bleep_summary`` (``bleep.summary_device``);
  * for context, the notebook's numpy loops on the host, run once (tests/bleep_reference.py).

One JSON line; ``--out FILE`` also writes it there.  No threshold: this is a record, not a check.

    python tools/bench_bleep.py [--out profiles/bleep_eval.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bleep_reference as ref  # noqa: E402
from bench_eval import device_ms, host_ms  # noqa: E402
from mclstexp_amd import bleep, retrieval, synth  # noqa: E402

SHAPES = [  # name, Q, N, P, G, k
    ("bleep fold: Q 2265, N 7004, G 3467", 2265, 7004, 256, 3467, 50),
    ("her2st fold: Q 400, N 12000, G 785", 400, 12000, 256, 785, 50),
]


def padded(a: torch.Tensor, multiple: int = 4) -> torch.Tensor:
    """The same matrix with its leading dimension rounded up to ``multiple`` elements (a view of a wider buffer)."""
    ld = -(-a.shape[1] // multiple) * multiple
    buf = torch.zeros((a.shape[0], ld), device=a.device, dtype=a.dtype)
    buf[:, :a.shape[1]] = a
    return buf[:, :a.shape[1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    shapes = []
    for name, Q, N, P, G, k in SHAPES:
        c = synth.make_retrieval_case(N, Q, P, G, seed=1)
        key, qry, expr = (torch.from_numpy(c[n]).to(dev) for n in ("spot_key", "image_query", "expression_key"))
        expr_pad = padded(expr)
        _, idx = retrieval.find_matches_device(key, qry, k)
        gathered = Q * k * (G + P) * 4
        row = {"shape": name, "Q": Q, "N": N, "P": P, "G": G, "k": k, "gathered_bytes": gathered,
               "lde_dense": int(expr.stride(0)), "lde_padded": int(expr_pad.stride(0))}
        for method in ("simple", "average", "weighted_average"):
            for tag, e in (("dense_elementwise", expr), ("padded_16byte", expr_pad)):
                ms = device_ms(lambda: retrieval.combine_device(key, e, qry, idx, method))
                row[f"knn_combine_{method}_{tag}_ms"] = round(ms, 4)
                if method != "simple":
                    row[f"knn_combine_{method}_{tag}_GBps"] = round(gathered / ms / 1e6, 1)
            top_k = 1 if method == "simple" else k
            row[f"predict_expression_{method}_ms"] = round(host_ms(
                lambda: retrieval.predict_expression(key, expr, qry, top_k=top_k, method=method), iters=5, warm=1), 3)
        pred = retrieval.combine_device(key, expr, qry, idx, "average")[1]
        true = expr[:Q].clone()
        off = np.array([0, Q], dtype=np.int64)
        row["scoring_sequence_ms"] = round(device_ms(lambda: bleep.summary_device(pred, true, off, [3, 50, 96])), 4)
        row["score_ms"] = round(host_ms(lambda: bleep.score(pred, true, markers=[3, 50, 96]), iters=5, warm=1), 3)
        idx_h, pred_h, true_h = idx.cpu().numpy(), pred.cpu().numpy().astype(np.float64), true.cpu().numpy()
        t0 = time.perf_counter()
        ref.average(c["spot_key"], c["expression_key"], idx_h)
        row["host_numpy_average_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        ref.weighted_average(c["spot_key"], c["expression_key"], c["image_query"], idx_h)
        row["host_numpy_weighted_average_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        ref.score(pred_h, true_h, [3, 50, 96])
        row["host_numpy_scoring_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        shapes.append(row)
    line = json.dumps({"bench": "bleep_eval", "device": torch.cuda.get_device_name(0), "shapes": shapes})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
