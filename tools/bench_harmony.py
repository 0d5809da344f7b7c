"""Harmony (mclstexp_amd.harmony) at BLEEP's own shape, once: N = 9269 cells in batches of 2378 / 2349 / 2277 / 2265,
d = 3467 genes, K = 100, synthetic log1p-like data with a per-batch shift.  Prints one JSON line and, with --out, writes it
(profiles/harmony.json): total time, time per k-means iteration and per correction (HIP events around the entry points),
the achieved fp64 rate of the two products, the bytes/s of the centroid product, and the time of the numpy restatement
(tests/harmony_reference.py) on the same host at the threads it is granted.

    python tools/bench_harmony.py [--out profiles/harmony.json] [--skip_numpy]
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

SIZES = (2378, 2349, 2277, 2265)
D, K = 3467, 100
KMEANS = ("mcl_harmony_centroids", "mcl_harmony_dist", "mcl_harmony_softmax", "mcl_harmony_update_block",
          "mcl_harmony_objective")
CORRECTION = ("mcl_harmony_ridge", "mcl_harmony_apply")


def make_data(seed=0):
    rng = np.random.RandomState(seed)
    N, B = sum(SIZES), len(SIZES)
    batch = np.repeat(np.arange(B), SIZES).astype(np.int32)
    profile = rng.gamma(2.0, 1.0, size=(8, D))
    cell_type = rng.randint(0, 8, size=N)
    counts = rng.poisson(profile[cell_type] * rng.uniform(0.5, 2.0, size=(N, 1)) * 3.0)
    shift = np.abs(rng.normal(0.0, 0.4, size=(B, D)))
    return np.log1p(counts.astype(np.float64)) + shift[batch] + 0.05, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_numpy", action="store_true")
    a = ap.parse_args()
    from mclstexp_amd import _lib, harmony
    import harmony_reference as hr
    Z, batch = make_data()
    N = len(Z)
    rows = np.random.RandomState(1).choice(N, K, replace=False)
    harmony.run_harmony(Z[:600], batch[:600] % 2, nclust=20, max_iter_harmony=1)      # warm: library, allocator
    torch.cuda.synchronize()
    with _lib.AbiTimer(KMEANS + CORRECTION + ("mcl_harmony_lloyd", "mcl_harmony_normalize")) as t:
        t0 = time.perf_counter()
        res = harmony.run_harmony(Z, batch, nclust=K, seed_rows=rows)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    s = t.summary()
    iters = sum(r + 1 for r in res.kmeans_rounds)
    n_corr = len(res.kmeans_rounds)
    # mcl_harmony_centroids is called once per k-means iteration (B = 0) and once per correction (B > 0: argument 6)
    cen = [(ms, args[6]) for ms, args in zip(s["mcl_harmony_centroids"]["ms"], s["mcl_harmony_centroids"]["args"])]
    cen_iter = [ms for ms, b in cen if b == 0]
    cen_corr = [ms for ms, b in cen if b > 0]
    ms = lambda n: s[n]["total_ms"]
    kmeans_ms = sum(ms(n) for n in KMEANS) - sum(cen_corr)
    corr_ms = sum(ms(n) for n in CORRECTION) + sum(cen_corr)
    flops = 2.0 * N * K * D
    cen_bytes = 8.0 * (N * D + N * K + K * D)
    doc = {
        "shape": {"N": N, "batches": list(SIZES), "d": D, "K": K},
        "kmeans_rounds": res.kmeans_rounds, "kmeans_iterations": iters, "corrections": n_corr, "converged": res.converged,
        "objective_harmony": res.objective_harmony,
        "total_s": total,
        "device_ms_per_kmeans_iteration": kmeans_ms / iters,
        "device_ms_per_correction": corr_ms / n_corr,
        "lloyd_init_ms": ms("mcl_harmony_lloyd"),
        "per_entry_point_avg_ms": {n: s[n]["avg_ms"] for n in s},
        "centroid_product_ms": float(np.mean(cen_iter)),
        "centroid_product_fp64_tflops": flops / (np.mean(cen_iter) * 1e-3) / 1e12,
        "centroid_product_tb_per_s": cen_bytes / (np.mean(cen_iter) * 1e-3) / 1e12,
        "dist_product_ms": s["mcl_harmony_dist"]["avg_ms"],
        "dist_product_fp64_tflops": flops / (s["mcl_harmony_dist"]["avg_ms"] * 1e-3) / 1e12,
        "correction_sums_ms": float(np.mean(cen_corr)),
        "correction_sums_fp64_tflops": flops * (len(SIZES) + 1) / (np.mean(cen_corr) * 1e-3) / 1e12,
        "device": torch.cuda.get_device_name(0),
    }
    if not a.skip_numpy:
        t0 = time.perf_counter()
        Y0 = hr.lloyd(hr.normalize_rows(Z, True), rows)
        ref = hr.harmony(Z, batch, K, Y0, hr.draw_orders(0, N, 200))
        doc["numpy_restatement_s"] = time.perf_counter() - t0
        doc["numpy_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
        doc["numpy_kmeans_rounds"] = ref["kmeans_rounds"].tolist()
        zc = res.Z_corr.cpu().numpy()
        doc["z_corr_max_dev_vs_numpy"] = float(np.max(np.abs(zc - ref["Z_corr"])) / np.max(np.abs(ref["Z_corr"])))
        doc["speedup_vs_numpy"] = doc["numpy_restatement_s"] / total
    line = json.dumps(doc)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
