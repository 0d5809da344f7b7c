#!/usr/bin/env python3
"""Micro-benchmark of the scoring of expression predictions (mclstexp_amd.evaluate) on one MI355X.  Per shape: the one
``mcl_expr_metrics`` call on device-resident matrices (HIP events; both launches), ``score_folds`` end to end on
device-resident per-fold tensors (stacking copy, offsets upload, the call, results to the host; host clock around a
device synchronise) and the fp64 numpy restatement of the reference's scoring block on the host (tests/eval_reference.py)
for scale.  One JSON line per shape.

    python tools/bench_eval.py
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mclstexp_amd import evaluate, synth  # noqa: E402
from eval_reference import score_segments  # noqa: E402

SHAPES = [  # name, fold sizes, genes
    ("her2st: 32 folds x 785 genes", [300 + 13 * (i % 7) for i in range(32)], 785),
    ("configs[4]: 9 folds x 3467 genes", [600 + 41 * (i % 5) for i in range(9)], 3467),
]


def device_ms(fn, iters=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def host_ms(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    dev = torch.device("cuda")
    for name, sizes, G in SHAPES:
        d = synth.make_eval_case(sizes, G, seed=1)
        off = d["offsets"]
        pred32 = torch.from_numpy(d["pred"]).float().to(dev)
        true32 = torch.from_numpy(d["true"]).float().to(dev)
        preds = [pred32[off[s]:off[s + 1]].contiguous() for s in range(len(sizes))]
        trues = [true32[off[s]:off[s + 1]].contiguous() for s in range(len(sizes))]
        t_call = device_ms(lambda: evaluate.metrics_device(pred32, true32, off))
        t_score = host_ms(lambda: evaluate.score_folds(preds, trues))
        p_np, t_np = pred32.cpu().double().numpy(), true32.cpu().double().numpy()
        t0 = time.perf_counter()
        score_segments(p_np, t_np, off)
        t_host = (time.perf_counter() - t0) * 1e3
        bytes_read = 2 * 2 * pred32.numel() * 4      # pred + true, fp32, two passes
        print(json.dumps({"shape": name, "rows": int(off[-1]), "genes": G, "folds": len(sizes),
                          "metrics_call_ms": round(t_call, 4), "score_folds_ms": round(t_score, 4),
                          "host_numpy_fp64_ms": round(t_host, 2),
                          "metrics_call_GBps": round(bytes_read / (t_call * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
