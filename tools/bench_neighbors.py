"""The three stages of the neighbourhood graph (mclstexp_amd.neighbors: mcl_knn_exact, mcl_knn_smooth,
mcl_knn_connectivities) at two shapes on synthetic Gaussian blobs: the fixture's case b (257 + 151 + 300 rows, D = 50,
k = 150) and BLEEP's (9269 rows as one segment, D = 50, k = 150).  Prints one JSON line and, with --out, writes it
(profiles/neighbors.json): per shape the median, smallest and largest time of each entry point over --calls calls after a
warm-up (HIP events on the launch stream; mcl_knn_connectivities is timed per phase, the host's read of S integers
between them is not in either), and the whole of neighbors() by the wall clock.

    python tools/bench_neighbors.py [--out profiles/neighbors.json] [--calls 10]

--cpu instead times, on the host, sklearn's brute-force kneighbors plus tests/neighbors_reference.py's smoothing and fuzzy
union at the same shapes (context for the figures above; needs no GPU) and prints that JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"case_b_257_151_300": (np.array([257, 151, 300]), 50, 150), "bleep_9269": (np.array([9269]), 50, 150)}


def blobs(seg, D, seed=0):
    rng = np.random.RandomState(seed)
    xs = []
    for n in seg:
        centres = 4.0 * rng.standard_normal((3, D))
        xs.append(centres[np.arange(n) % 3] + rng.standard_normal((n, D)))
    return np.concatenate(xs)


def cpu():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import neighbors_reference as nr
    from sklearn.neighbors import NearestNeighbors
    doc = {"threads": len(os.sched_getaffinity(0))}
    for name, (seg, D, k) in SHAPES.items():
        x = blobs(seg, D)
        off = np.concatenate([[0], np.cumsum(seg)])
        t_knn = t_rest = 0.0
        for s in range(seg.size):
            xs = x[off[s]:off[s + 1]]
            t0 = time.perf_counter()
            dist, idx = NearestNeighbors(n_neighbors=k, algorithm="brute").fit(xs).kneighbors(xs)
            t1 = time.perf_counter()
            rho, sigma, _ = nr.smooth(dist)
            nr.connectivities(idx, dist, rho, sigma)
            t_knn, t_rest = t_knn + t1 - t0, t_rest + time.perf_counter() - t1
        doc[name] = {"sklearn_brute_kneighbors_ms": 1e3 * t_knn, "restatement_smooth_and_union_ms": 1e3 * t_rest}
    return doc


def gpu(calls):
    import torch
    from mclstexp_amd import _lib, neighbors
    names = ["mcl_knn_exact", "mcl_knn_smooth", "mcl_knn_connectivities"]
    doc = {}
    for name, (seg, D, k) in SHAPES.items():
        x = torch.from_numpy(blobs(seg, D)).cuda()
        off = np.concatenate([[0], np.cumsum(seg)]).astype(np.int64)
        for _ in range(2):
            res = neighbors.neighbors(x, off, k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with _lib.AbiTimer(names) as t:
            for _ in range(calls):
                neighbors.neighbors(x, off, k)
        s = t.summary()
        wall = (time.perf_counter() - t0) / calls
        entry = {"segments": int(seg.size), "rows": int(off[-1]), "D": D, "k": k, "nnz": int(res["nnz_offsets"][-1]),
                 "neighbors_wall_ms": 1e3 * wall}
        conn = s["mcl_knn_connectivities"]["ms"]
        for key, ms in (("knn_exact", s["mcl_knn_exact"]["ms"]), ("knn_smooth", s["mcl_knn_smooth"]["ms"]),
                        ("connectivities_count", conn[0::2]), ("connectivities_fill", conn[1::2])):
            ms = sorted(ms)
            entry[f"{key}_ms_median"], entry[f"{key}_ms_min"], entry[f"{key}_ms_max"] = ms[len(ms) // 2], ms[0], ms[-1]
        doc[name] = entry
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    line = json.dumps(cpu() if a.cpu else gpu(a.calls))
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
