#!/usr/bin/env python3
"""Micro-benchmark of the batched NMF (mclstexp_amd.nmf) on one MI355X, on the workloads the other evaluation modules
report: the 32-slide HER2ST-sized evaluation (15500 spots x 785 genes), pooled into one problem and with every slide a
problem of its own, and one 4000 x 3467 slide; k = 8, 16, 64; n_init = 1 and 4; both losses.  fp32 spots resident on the
device, ``log1p(poisson(W_t H_t))`` with a sparse ``H_t``.

Per configuration, after warm-up, medians (and the extremes) of repeated runs with ``tol = 0`` and ``--iters`` iterations:
``nmf_device`` end to end (host clock around a device synchronise: the input check, the host draw of the random start and
its upload, the allocations and the final error included), ``mcl_nmf_steps`` by HIP events on the launch stream (time per
iteration), and the row pass alone -- the W update, timed as ``mcl_nmf_steps`` with ``update_h = 0``, whose iterations
are that one kernel (for KL the ratio is formed inside it) plus ``nm_hht_kernel`` / ``nm_axis_sum_kernel`` once per call of 10
iterations, which the figure includes.  Derived, from bytes and flops, no counter read: the row
pass against reading ``x`` once per iteration at the HBM rate (6.29 TB/s, the measured float4-copy rate) and its
2 rows G k + 2 rows k^2 flops per start against the fp64 MFMA rate (78.6 TFLOP/s, the MI355X's specification), and the cost
of ``n_init = 4`` over ``n_init = 1``.

The yardstick is scikit-learn's ``NMF(solver="mu", init="random", tol=0)`` with the same iteration count on the host of the
same machine (BLAS on the threads the environment allows, 16), one start, timed before this process touches the GPU; per
slide it is one fit per slide in a loop.

    python tools/bench_nmf.py [--workload 0|1|2] [--out FILE] [--no_host] [--runs 20] [--iters 20] [--ks 8,64] [--starts 1]
                                 [--losses frobenius] [--merge] [--variant NAME] [--merge_files A B ... --out FILE]

A library built with other flags (tools/build_variant.sh, e.g. ``nmf_walk nmf.hip -DNM_RUN_ROWS=16384``: the column pass as
one workgroup walking all row tiles of a segment; ``nmf_fused nmf.hip -DNM_FUSED -DNM_RUN_ROWS=128``: the X-shared fused
pass) is measured by pointing MCL_LIB_PATH at it and recorded with ``--variant NAME --merge --out profiles/nmf.json``.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12
MFMA_F64_FLOPS = 78.6e12
KS = (8, 16, 64)
STARTS = (1, 4)
LOSSES = ("frobenius", "kullback-leibler")
WORKLOADS = [  # name, spots, genes, slides (segments; 1 = pooled)
    ("her2st: 32 slides pooled, 15500 x 785", 15500, 785, 1),
    ("her2st: 32 slides, each a problem, 15500 x 785", 15500, 785, 32),
    ("one 4000 x 3467 slide", 4000, 3467, 1),
]


def make_matrix(rows, G, seed):
    rng = np.random.RandomState(seed)
    Wt = rng.gamma(1.0, 1.0, size=(rows, 12)).astype(np.float32)
    Ht = (rng.gamma(1.0, 2.0, size=(12, G)) * (rng.uniform(size=(12, G)) < 0.3)).astype(np.float32)
    return np.log1p(rng.poisson(Wt @ Ht)).astype(np.float32)


def offsets_of(rows, slides):
    return np.linspace(0, rows, slides + 1).astype(np.int64)


def host_ms(x, off, k, loss, iters):
    from sklearn.decomposition import NMF
    x = x.astype(np.float64)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for j in range(off.size - 1):
            NMF(n_components=k, init="random", solver="mu", beta_loss=loss, tol=0, max_iter=iters,
                random_state=0).fit(x[off[j]:off[j + 1]])
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ks", default=None, help="comma-separated k (default 8,16,64)")
    ap.add_argument("--starts", default=None, help="comma-separated n_init, 1 first (default 1,4)")
    ap.add_argument("--losses", default=None, help="comma-separated losses (default both)")
    ap.add_argument("--merge", action="store_true", help="append to the results already in --out instead of replacing the file")
    ap.add_argument("--variant", default=None, help="record the results under variants[NAME] (an MCL_LIB_PATH library)")
    ap.add_argument("--merge_files", nargs="+", default=None, help="no measurement: merge files this tool wrote into --out")
    args = ap.parse_args()
    if args.merge_files:
        for f in args.merge_files:
            with open(f) as fh:
                write_doc(args.out, json.load(fh), True, args.variant)
        return
    global KS, STARTS, LOSSES
    if args.losses:
        LOSSES = tuple(args.losses.split(","))
    if args.ks:
        KS = tuple(int(v) for v in args.ks.split(","))
    if args.starts:
        STARTS = tuple(int(v) for v in args.starts.split(","))
    picked = [w for i, w in enumerate(WORKLOADS) if args.workload in (None, i)]
    mats = [make_matrix(n, G, n + G) for _, n, G, _ in picked]
    host = {}
    if not args.no_host:
        for (name, n, G, S), x in zip(picked, mats):
            for k in KS:
                for loss in LOSSES:
                    host[(name, k, loss)] = host_ms(x, offsets_of(n, S), k, loss, args.iters)
                    print(f"host {name} k = {k} {loss}: {host[(name, k, loss)]:.1f} ms", file=sys.stderr, flush=True)
    import torch
    from mclstexp_amd import _lib, nmf
    results = []
    for (name, n, G, S), x in zip(picked, mats):
        xd = torch.from_numpy(x).cuda()
        off = None if S == 1 else offsets_of(n, S)
        for k in KS:
            for loss in LOSSES:
                base = {}
                for n_init in STARTS:
                    def run():
                        return nmf.nmf_device(xd, k, off, beta_loss=loss, n_init=n_init, seed=0, max_iter=args.iters, tol=0.0)

                    H = run()["H"]
                    torch.cuda.synchronize()
                    wall, steps = [], []
                    for _ in range(args.runs):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        run()
                        torch.cuda.synchronize()
                        wall.append((time.perf_counter() - t0) * 1e3)
                    for _ in range(args.runs):
                        with _lib.AbiTimer(["mcl_nmf_steps"]) as t:
                            run()
                        steps.append(t.summary()["mcl_nmf_steps"]["total_ms"] / args.iters)
                    r = {"workload": name, "rows": n, "genes": G, "segments": S, "k": k, "beta_loss": loss, "n_init": n_init,
                         "iterations": args.iters, "input": "float32, device-resident", "end_to_end_ms": spread(wall),
                         "ms_per_iteration": spread(steps), "counters_read": None}
                    if n_init == 1:
                        rowp = []
                        for _ in range(args.runs):
                            with _lib.AbiTimer(["mcl_nmf_steps"]) as t:
                                nmf.transform_device(xd, H, off, beta_loss=loss, max_iter=args.iters, tol=0.0)
                            rowp.append(t.summary()["mcl_nmf_steps"]["total_ms"] / args.iters)
                        ms = statistics.median(rowp)
                        flops = 2.0 * n * G * k + 2.0 * n * k * k + (2.0 * n * G * k if loss != "frobenius" else 0.0)
                        r.update(row_pass_ms=spread(rowp), x_bytes=n * G * 4,
                                 row_pass_share_of_hbm_rate=n * G * 4 / HBM_BYTES_PER_S * 1e3 / ms,
                                 row_pass_share_of_mfma_f64_rate=flops / MFMA_F64_FLOPS * 1e3 / ms)
                        base = {"it": statistics.median(steps), "wall": statistics.median(wall)}
                        if (name, k, loss) in host:
                            r.update(host_ms=host[(name, k, loss)], host_threads=int(os.environ.get("OMP_NUM_THREADS", 0)) or None,
                                     end_to_end_speedup_over_host=host[(name, k, loss)] / statistics.median(wall))
                    else:
                        r.update(per_iteration_cost_over_one_start=statistics.median(steps) / base["it"],
                                 end_to_end_cost_over_one_start=statistics.median(wall) / base["wall"])
                    results.append(r)
                    print(f"{name} k = {k} {loss} n_init = {n_init}: {statistics.median(steps):.3f} ms / iteration, end to end "
                          f"{statistics.median(wall):.2f} ms", file=sys.stderr, flush=True)
    doc = {"bench": "nmf", "library": os.path.basename(os.environ.get("MCL_LIB_PATH") or "default"),
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "results": results}
    print(json.dumps(doc))
    if args.out:
        write_doc(args.out, doc, args.merge, args.variant)


def write_doc(path, doc, merge, variant):
    """Writes ``doc``; with ``merge`` into the file already there: its results are appended to the file's, or, with
    ``variant``, to ``variants[variant]`` (a library built with other flags), so that a profile of several runs is the
    tool's own output."""
    if merge and os.path.exists(path):
        with open(path) as fh:
            old = json.load(fh)
        if variant:
            slot = old.setdefault("variants", {}).setdefault(variant, {"library": doc["library"], "results": []})
            slot["results"] += doc["results"]
        else:
            old["results"] += doc["results"]
        doc = old
    elif variant:
        doc = {"bench": "nmf", "device": doc["device"], "runs": doc["runs"], "results": [],
               "variants": {variant: {"library": doc["library"], "results": doc["results"]}}}
    with open(path, "w") as fh:
        fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
