#!/usr/bin/env python3
"""Micro-benchmark of the Gaussian mixtures and the cluster-validity pass (mclstexp_amd.mixture) on one MI355X:

  evaluation   32 HER2ST-sized slides (300 - 700 spots, 15 500 in all) x 9 PCA scores, ``select_k`` over k = 2 .. 12, full
               covariance, 4 k-means starts per mixture: 1408 EM problems in one ``mcl_gmm_fit`` launch
  slide        one 4000-spot slide at D = 50, K = 8, full covariance, one start
  single CU    one 16 384 x 50 slide, K = 20, full covariance, ``max_iter`` fixed: one workgroup (one CU) does all of it --
               the cost the design accepts for never leaving the launch; reported per EM iteration next to the
               ~0.85 G multiply-adds an iteration needs (n K D^2 / 2 for the triangular product and for the triangle of
               the scatter matrix each, plus 2 n K D for the moments and the squares): ~1.7 GFLOP
  validity     silhouette / Calinski-Harabasz / Davies-Bouldin at 16 384 rows x 9, 7 clusters

Per workload, after warm-up, medians of repeated runs: end to end (host clock around a device synchronise; it includes the
k-means starts, allocations, uploads and the status read-back) and the entry points alone by HIP events on the launch
stream.  The yardstick is sklearn on the host of the same machine, on at most 16 threads: ``GaussianMixture`` with its own
k-means initialisation (one (slide, k) fit per task) and ``silhouette_samples`` + the two scores.  The evaluation's host
figure is timed on ``--host_slides`` slides and scaled to 32, and is labelled as an extrapolation.  The two sides start
from different k-means draws, so their iteration counts differ: both are recorded.  Nothing gates on these numbers.

    python tools/bench_mixture.py [--out FILE] [--no_host] [--runs N]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mixture_reference as mr  # noqa: E402
from mclstexp_amd import _lib, mixture  # noqa: E402

ENTRY_POINTS = ["mcl_kmeans", "mcl_gmm_fit", "mcl_gmm_select", "mcl_cluster_validity"]
THREADS = 16


def timed(run, runs):
    """(median end-to-end ms, {entry point: median total ms}, the last result) of ``run`` after two warm-up calls."""
    for _ in range(2):
        out = run()
    torch.cuda.synchronize()
    wall = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    per = {n: [] for n in ENTRY_POINTS}
    for _ in range(runs):
        with _lib.AbiTimer(ENTRY_POINTS) as t:
            run()
        for n, rec in t.summary().items():
            per[n].append(rec["total_ms"])
    return statistics.median(wall), {n: statistics.median(v) for n, v in per.items() if v}, out


def host_gmm(tasks, **kw):
    """Wall ms of sklearn fits, one (x, k) task per thread-pool job; also the mean n_iter."""
    from sklearn.mixture import GaussianMixture

    def one(task):
        x, k = task
        return GaussianMixture(n_components=k, random_state=0, **kw).fit(x).n_iter_
    one(tasks[0])
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=THREADS) as ex:
        iters = list(ex.map(one, tasks))
    return (time.perf_counter() - t0) * 1e3, float(np.mean(iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host_slides", type=int, default=8)
    args = ap.parse_args()
    results = []

    def note(r):
        results.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)

    # ---- the evaluation
    sizes = [300 + 50 * (i % 9) for i in range(32)]
    xs = [mr.make_case(n, 9, 5 + i % 4, 2.0, seed=100 + i)[0] for i, n in enumerate(sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    zd = torch.from_numpy(np.concatenate(xs)).cuda()
    cand = list(range(2, 13))
    wall, per, out = timed(lambda: mixture.select_k(zd, cand, off, n_init=4, seed=0), args.runs)
    n_iter = np.concatenate([f["n_iter_all"].cpu().numpy().ravel() for f in out["fits"]])
    r = {"workload": "evaluation: 32 slides x 9 scores, k = 2 .. 12, full, 4 starts", "rows": int(off[-1]), "D": 9,
         "em_problems": int(n_iter.size), "calls": len(out["fits"]), "end_to_end_ms": wall, "kmeans_ms": per["mcl_kmeans"],
         "gmm_fit_ms": per["mcl_gmm_fit"], "gmm_select_ms": per["mcl_gmm_select"], "mean_n_iter": float(n_iter.mean()),
         "max_n_iter": int(n_iter.max()), "chosen_k": out["k"].tolist()}
    if not args.no_host:
        hs = min(args.host_slides, len(xs))
        ms, it = host_gmm([(x, k) for x in xs[:hs] for k in cand], n_init=4, covariance_type="full")
        r.update(host_threads=THREADS, host_slides_timed=hs, host_ms_timed=ms, host_mean_n_iter=it,
                 host_ms_extrapolated_to_32_slides=ms * float(off[-1]) / float(off[hs]),
                 end_to_end_speedup_over_host_extrapolated=ms * float(off[-1]) / float(off[hs]) / wall)
    note(r)

    # ---- one slide
    x = mr.make_case(4000, 50, 8, 1.5, seed=7)[0]
    xd = torch.from_numpy(x).cuda()
    wall, per, out = timed(lambda: mixture.gmm(xd, 8, n_init=1, seed=0), args.runs)
    r = {"workload": "one 4000 x 50 slide, K = 8, full, 1 start", "rows": 4000, "D": 50, "K": 8, "end_to_end_ms": wall,
         "kmeans_ms": per["mcl_kmeans"], "gmm_fit_ms": per["mcl_gmm_fit"], "n_iter": int(out["n_iter"].cpu()[0])}
    r["gmm_fit_ms_per_iteration"] = r["gmm_fit_ms"] / (r["n_iter"] + 1)
    if not args.no_host:
        ms, it = host_gmm([(x, 8)], n_init=1, covariance_type="full")
        r.update(host_threads=THREADS, host_ms=ms, host_n_iter=it, host_ms_per_iteration=ms / (it + 1),
                 per_iteration_speedup_over_host=(ms / (it + 1)) / r["gmm_fit_ms_per_iteration"])
    note(r)

    # ---- the single-CU worst case
    n, D, K, iters = 16384, 50, 20, 5
    x, init, _ = mr.make_case(n, D, K, 1.5, seed=9)
    xd, init_d = torch.from_numpy(x).cuda(), torch.from_numpy(init[None]).cuda()
    wall, per, out = timed(lambda: mixture.gmm(xd, K, init_labels=init_d, tol=0.0, max_iter=iters), max(3, args.runs // 2))
    macs = float(n) * K * D * D + 2.0 * n * K * D      # E-step triangle + scatter triangle (n K D^2 / 2 each) + moments
    flop = 2.0 * macs
    r = {"workload": "single CU: one 16384 x 50 slide, K = 20, full, given start", "rows": n, "D": D, "K": K,
         "iterations": iters, "gmm_fit_ms": per["mcl_gmm_fit"],
         "gmm_fit_ms_per_iteration": per["mcl_gmm_fit"] / (iters + 1), "multiply_adds_per_iteration": macs,
         "flop_per_iteration": flop,
         "gflops_on_one_cu": flop / (per["mcl_gmm_fit"] / (iters + 1) * 1e-3) / 1e9}
    if not args.no_host:
        ms, it = host_gmm([(x, K)], n_init=1, covariance_type="full", tol=0.0, max_iter=iters, init_params="random")
        r.update(host_threads=THREADS, host_ms=ms, host_ms_per_iteration=ms / (iters + 1),
                 per_iteration_speedup_over_host=(ms / (iters + 1)) / r["gmm_fit_ms_per_iteration"])
    note(r)

    # ---- validity
    x, _, truth = mr.make_case(16384, 9, 7, 2.0, seed=5)
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(truth).cuda()
    wall, per, out = timed(lambda: mixture.validity(xd, ld), args.runs)
    pairs = float(x.shape[0]) ** 2
    r = {"workload": "validity: 16384 x 9, 7 clusters", "rows": 16384, "D": 9, "end_to_end_ms": wall,
         "cluster_validity_ms": per["mcl_cluster_validity"], "pair_distances": pairs,
         "pair_distances_per_s": pairs / (per["mcl_cluster_validity"] * 1e-3)}
    if not args.no_host:
        from sklearn.metrics import calinski_harabasz_score, davies_bouldin_score, silhouette_samples
        t0 = time.perf_counter()
        silhouette_samples(x, truth, n_jobs=THREADS)
        calinski_harabasz_score(x, truth)
        davies_bouldin_score(x, truth)
        ms = (time.perf_counter() - t0) * 1e3
        r.update(host_threads=THREADS, host_ms=ms, speedup_over_host=ms / per["mcl_cluster_validity"])
    note(r)

    doc = {"bench": "mixture", "device": torch.cuda.get_device_name(0), "runs": args.runs, "results": results}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
