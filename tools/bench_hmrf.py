#!/usr/bin/env python3
"""Micro-benchmark of the Potts-HMRF mixtures (mclstexp_amd.hmrf) on one MI355X, each workload against ``mixture.gmm`` from
the same starts in the same process -- the nearest capability without the spatial prior, so the ratio is the price of the
field pass -- and against the numpy restatement (tests/hmrf_reference.py) on at most 16 host threads of the same machine:

  evaluation   32 HER2ST-sized slides (300 - 700 spots, 15 500 in all) x 9 scores, k per slide from the mixture's BIC over
               2 .. 12 (chosen once, outside the timed region), 4 k-means starts, beta = 1, binary k = 8 lattice: 128 problems
               in one ``mcl_hmrf_fit`` launch
  slide        one 4000-spot slide at D = 50, K = 8, full covariance, one start, ``tol = 0`` and ``max_iter`` fixed so that
               both sides run the same number of iterations; reported per EM iteration, next to the n kw K responsibilities
               (8 bytes each) the field pass reads per iteration
  scan         ``scan_beta`` over 6 candidates on the evaluation's slides: 768 problems in one launch

Per workload, after warm-up, medians of repeated runs, the two sides alternating: end to end (host clock around a device
synchronise) and the entry points alone by HIP events on the launch stream.  The host figure of the evaluation is timed on
``--host_slides`` slides and scaled, and is labelled as an extrapolation; the slide's host figure is timed over
``--host_iters`` iterations.  Nothing gates on these numbers.

    python tools/bench_hmrf.py [--out FILE] [--no_host] [--runs N]
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
import hmrf_reference as hr  # noqa: E402
from mclstexp_amd import _lib, cluster, hmrf, mixture, spatial  # noqa: E402

ENTRY_POINTS = ["mcl_hmrf_fit", "mcl_gmm_fit", "mcl_gmm_select", "mcl_edge_agreement"]
THREADS = 16
LATTICE_K = 8


def timed_pair(run_a, run_b, runs):
    """Medians of two alternating workloads after two warm-up calls each: (wall ms a, wall ms b, entry-point ms a, b, out a)."""
    for _ in range(2):
        out = run_a()
        run_b()
    torch.cuda.synchronize()
    wall = ([], [])
    for _ in range(runs):
        for side, run in enumerate((run_a, run_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            wall[side].append((time.perf_counter() - t0) * 1e3)
    per = ({n: [] for n in ENTRY_POINTS}, {n: [] for n in ENTRY_POINTS})
    for _ in range(runs):
        for side, run in enumerate((run_a, run_b)):
            with _lib.AbiTimer(ENTRY_POINTS) as t:
                run()
            for n, rec in t.summary().items():
                per[side][n].append(rec["total_ms"])
    med = [{n: statistics.median(v) for n, v in p.items() if v} for p in per]
    return statistics.median(wall[0]), statistics.median(wall[1]), med[0], med[1], out


def make_slide(n, D, K, seed, noise=1.5):
    """n spots of a jittered grid, K planted vertical stripes, D scores."""
    gc = int(np.ceil(np.sqrt(n * 1.3)))
    gr = -(-n // gc)
    coords, _ = hr.grid_coords(gr, gc, jitter=0.1, seed=seed)
    coords = coords[:n]
    truth = np.minimum((coords[:, 0] / (gc / K)).astype(np.int64), K - 1)
    return hr.blobs(truth, D, K, 1.5, noise, seed), coords


def host_fits(tasks, **kw):
    """Wall ms of the restatement's fits, one (x, K, init, nbr, w, beta) task per thread-pool job; also the mean n_iter."""
    def one(t):
        return hr.fit(*t, **kw)["n_iter"]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=THREADS) as ex:
        iters = list(ex.map(one, tasks))
    return (time.perf_counter() - t0) * 1e3, float(np.mean(iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host_slides", type=int, default=4)
    ap.add_argument("--host_iters", type=int, default=2)
    args = ap.parse_args()
    results = []

    def note(r):
        results.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)

    # ---- the evaluation
    sizes = [300 + 50 * (i % 9) for i in range(32)]
    slides = [make_slide(n, 9, 4 + i % 4, 100 + i) for i, n in enumerate(sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    zd = torch.from_numpy(np.concatenate([s[0] for s in slides])).cuda()
    graph = spatial.lattice(np.concatenate([s[1] for s in slides]), off, LATTICE_K, "NA", row_standardise=False)
    ks = mixture.select_k(zd, list(range(2, 13)), off, n_init=4, seed=0)["k"]
    init = cluster.kmeans(zd, ks, off, n_init=4, seed=0)["labels_all"]
    wa, wb, pa, pb, out = timed_pair(lambda: hmrf.hmrf(zd, graph, ks, 1.0, init_labels=init),
                                     lambda: mixture.gmm(zd, ks, off, init_labels=init), args.runs)
    n_iter = out["n_iter_all"].cpu().numpy().ravel()
    g_iter = mixture.gmm(zd, ks, off, init_labels=init)["n_iter_all"].cpu().numpy().ravel()
    r = {"workload": "evaluation: 32 slides x 9 scores, k by BIC, full, 4 starts, beta = 1, k = 8 lattice", "rows": int(off[-1]),
         "D": 9, "problems": int(n_iter.size), "k": [int(v) for v in ks], "hmrf_end_to_end_ms": wa, "gmm_end_to_end_ms": wb,
         "hmrf_fit_ms": pa["mcl_hmrf_fit"], "gmm_fit_ms": pb["mcl_gmm_fit"], "edge_agreement_ms": pa["mcl_edge_agreement"],
         "fit_ratio_hmrf_over_gmm": pa["mcl_hmrf_fit"] / pb["mcl_gmm_fit"], "hmrf_mean_n_iter": float(n_iter.mean()),
         "hmrf_max_n_iter": int(n_iter.max()), "gmm_mean_n_iter": float(g_iter.mean()), "gmm_max_n_iter": int(g_iter.max()),
         "converged_share": float(out["converged_all"].double().mean().cpu()),
         "mean_edge_agreement": float(np.mean(out["edge_agreement"]))}
    if not args.no_host:
        hs = min(args.host_slides, len(slides))
        nbr, w, init_h = graph["nbr"].cpu().numpy(), graph["w"].cpu().numpy(), init.cpu().numpy()
        tasks = [(slides[s][0], int(ks[s]), init_h[rr, off[s]:off[s + 1]], nbr[off[s]:off[s + 1]], w[off[s]:off[s + 1]], 1.0)
                 for s in range(hs) for rr in range(4)]
        ms, it = host_fits(tasks)
        scale = float(off[-1]) / float(off[hs])
        r.update(host_threads=THREADS, host_slides_timed=hs, host_ms_timed=ms, host_mean_n_iter=it,
                 host_ms_extrapolated_to_32_slides=ms * scale, end_to_end_speedup_over_host_extrapolated=ms * scale / wa)
    note(r)

    # ---- scan_beta on the evaluation's slides
    betas = [0.0, 0.25, 0.5, 1.0, 2.0, 4.0]
    ws, wo, ps, po, sc = timed_pair(lambda: hmrf.scan_beta(zd, graph, ks, betas, init_labels=init),
                                    lambda: hmrf.hmrf(zd, graph, ks, 1.0, init_labels=init), max(3, args.runs // 2))
    note({"workload": "scan_beta: 6 candidates x 32 slides, 4 starts", "betas": betas, "problems": 6 * 32 * 4,
          "scan_end_to_end_ms": ws, "scan_hmrf_fit_ms": ps["mcl_hmrf_fit"], "one_beta_end_to_end_ms": wo,
          "one_beta_hmrf_fit_ms": po["mcl_hmrf_fit"], "fit_ratio_scan_over_one_beta": ps["mcl_hmrf_fit"] / po["mcl_hmrf_fit"],
          "mean_edge_agreement_per_beta": [float(v) for v in sc["edge_agreement"].mean(axis=0)],
          "mean_changed_per_beta": [float(v) for v in sc["changed"].mean(axis=0)]})

    # ---- one slide, per iteration
    n, D, K, iters = 4000, 50, 8, 10
    x, coords = make_slide(n, D, K, 7)
    xd = torch.from_numpy(x).cuda()
    g1 = spatial.lattice(coords, None, LATTICE_K, "NA", row_standardise=False)
    init1 = cluster.kmeans(xd, K, None, n_init=1, seed=0)["labels_all"]
    wa, wb, pa, pb, out = timed_pair(lambda: hmrf.hmrf(xd, g1, K, 1.0, init_labels=init1, tol=0.0, max_iter=iters),
                                     lambda: mixture.gmm(xd, K, None, init_labels=init1, tol=0.0, max_iter=iters), args.runs)
    field_bytes = 8.0 * n * LATTICE_K * K
    r = {"workload": "one 4000 x 50 slide, K = 8, full, 1 start, 10 iterations", "rows": n, "D": D, "K": K, "iterations": iters,
         "hmrf_fit_ms": pa["mcl_hmrf_fit"], "gmm_fit_ms": pb["mcl_gmm_fit"],
         "hmrf_fit_ms_per_iteration": pa["mcl_hmrf_fit"] / (iters + 1), "gmm_fit_ms_per_iteration": pb["mcl_gmm_fit"] / (iters + 1),
         "fit_ratio_hmrf_over_gmm": pa["mcl_hmrf_fit"] / pb["mcl_gmm_fit"],
         "field_pass_ms_per_iteration": (pa["mcl_hmrf_fit"] - pb["mcl_gmm_fit"]) / (iters + 1),
         "field_pass_responsibility_bytes_per_iteration": field_bytes, "hmrf_end_to_end_ms": wa, "gmm_end_to_end_ms": wb}
    if not args.no_host:
        hi = max(1, args.host_iters)
        ms, _ = host_fits([(x, K, init1.cpu().numpy()[0], g1["nbr"].cpu().numpy(), g1["w"].cpu().numpy(), 1.0)], tol=0.0,
                          max_iter=hi)
        r.update(host_threads=THREADS, host_iterations_timed=hi, host_ms_per_iteration=ms / (hi + 1),
                 per_iteration_speedup_over_host=(ms / (hi + 1)) / r["hmrf_fit_ms_per_iteration"])
    note(r)

    doc = {"bench": "hmrf", "device": torch.cuda.get_device_name(0), "runs": args.runs, "results": results}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
