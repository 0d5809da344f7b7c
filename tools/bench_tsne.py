"""The pair pass of exact t-SNE (mclstexp_amd.tsne, mcl_tsne_gradient) at three sizes: n = 9269 (BLEEP's four slides as one
segment), 32 segments of 300 .. 700 rows (HER2ST), n = 257.  P and Y are synthetic (the pass does the same work on any
values).  Prints one JSON line and, with --out, writes it (profiles/tsne.json): per size the time of one
mcl_tsne_gradient and one mcl_tsne_update call (HIP events on the launch stream, after a warm-up), the bytes of P the pass
streams (8 n_s^2 summed) and the share of the measured HBM copy rate (6.29 TB/s) that stream reaches; for n = 9269 also
the affinities' one-off time.

    python tools/bench_tsne.py [--out profiles/tsne.json] [--calls 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12


def shapes():
    her2st = np.random.RandomState(0).randint(300, 701, size=32)
    return {"bleep_9269": np.array([9269]), "her2st_32x300_700": her2st, "n257": np.array([257])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=30)
    a = ap.parse_args()
    from mclstexp_amd import _lib, tsne
    from mclstexp_amd._arrays import cumulative_offsets, device, upload
    dev = device("bench_tsne")
    doc = {}
    for name, seg in shapes().items():
        off = cumulative_offsets(seg)
        plan = tsne._Plan(off, dev)
        rows, S = plan.rows, plan.S
        gen = torch.Generator(device=dev).manual_seed(0)
        P = torch.rand((plan.pairs,), device=dev, dtype=torch.float64, generator=gen) / float(plan.pairs)
        Y = torch.randn((rows, 2), device=dev, dtype=torch.float64, generator=gen) * 10.0
        grad, upd, gains = (torch.zeros((rows, 2), device=dev, dtype=torch.float64) for _ in range(3))
        stats = torch.zeros((2, S), device=dev, dtype=torch.float64)
        params = upload(np.tile([1.0, 0.8, 1e-9, 1.0, 0.0], (S, 1)), dev)        # a step too small to move Y
        for _ in range(3):
            plan.gradient(P, Y, params, False, grad, stats[0])
            plan.update(grad, params, Y, upd, gains, stats[1])
        with _lib.AbiTimer(["mcl_tsne_gradient", "mcl_tsne_update"]) as t:
            for i in range(a.calls):
                plan.gradient(P, Y, params, False, grad, stats[0])
                plan.update(grad, params, Y, upd, gains, stats[1])
            for i in range(max(a.calls // 10, 1)):
                plan.gradient(P, Y, params, True, grad, stats[0])
        s = t.summary()
        ms = sorted(s["mcl_tsne_gradient"]["ms"][:a.calls])
        ms_kl = sorted(s["mcl_tsne_gradient"]["ms"][a.calls:])
        med = ms[len(ms) // 2]
        doc[name] = {"segments": int(S), "rows": int(rows), "pairs": int(plan.pairs),
                     "gradient_ms_median": med, "gradient_ms_min": ms[0], "gradient_ms_max": ms[-1],
                     "gradient_with_kl_ms_median": ms_kl[len(ms_kl) // 2],
                     "update_ms_median": sorted(s["mcl_tsne_update"]["ms"])[a.calls // 2],
                     "p_stream_bytes": 8 * int(plan.pairs), "p_stream_bound_ms": 8e3 * plan.pairs / HBM_BYTES_PER_S,
                     "share_of_p_stream_bound": 8e3 * plan.pairs / HBM_BYTES_PER_S / med}
        del P
    x = np.random.RandomState(1).standard_normal((9269, 9))
    tsne.joint_probabilities(x[:500], None, 30.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    tsne.joint_probabilities(x, None, 30.0)
    e1.record()
    torch.cuda.synchronize()
    doc["bleep_9269"]["affinities_ms"] = e0.elapsed_time(e1)
    line = json.dumps(doc)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
