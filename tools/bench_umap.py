"""The UMAP layout (mclstexp_amd.umap: mcl_umap_prepare and the epoch loop mcl_umap_epochs) at two shapes on synthetic
Gaussian blobs: the fixture's case b (257 + 151 + 300 rows, D = 50, k = 150, 40 epochs) and BLEEP's (9269 rows as one
segment, D = 50, k = 150, 500 epochs).  Prints one JSON line and, with --out, writes it (profiles/umap.json): per shape the
median, smallest and largest time of the two entry points over --calls calls after a warm-up (HIP events on the launch
stream; the epoch loop is one entry-point call, n_epochs launches back to back), the time per epoch, and the whole of
layout() by the wall clock.  The graph is built once by neighbors.neighbors and is not in any figure.

    python tools/bench_umap.py [--out profiles/umap.json] [--calls 5]

--cpu instead times, on the host, tests/umap_reference.py's Jacobi restatement on tests/neighbors_reference.py's graph at the
same shapes (context for the figures above; needs no GPU; minutes at the larger shape) and prints that JSON line.  --merge
FILE puts the "cpu_context" of an earlier profile into the one written.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"case_b_257_151_300": (np.array([257, 151, 300]), 50, 150, 40), "bleep_9269": (np.array([9269]), 50, 150, 500)}
A, B = 0.5830300, 1.3341670


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
    import umap_reference as ur
    doc = {"threads": len(os.sched_getaffinity(0))}
    for name, (seg, D, k, n_epochs) in SHAPES.items():
        x = blobs(seg, D)
        off = np.concatenate([[0], np.cumsum(seg)])
        total = 0.0
        for s in range(seg.size):
            xs = x[off[s]:off[s + 1]]
            g = nr.graph(xs, k)
            m = nr.connectivities(g["knn_indices"], g["knn_distances"], g["rho"], g["sigma"])
            t0 = time.perf_counter()
            ur.run(m, ur.pca_init(xs), n_epochs, A, B, 0)
            total += time.perf_counter() - t0
        doc[name] = {"restatement_jacobi_ms": 1e3 * total, "n_epochs": n_epochs}
    return doc


def gpu(calls):
    import torch
    from mclstexp_amd import _lib, neighbors, umap
    names = ["mcl_umap_prepare", "mcl_umap_epochs"]
    doc = {}
    for name, (seg, D, k, n_epochs) in SHAPES.items():
        x = torch.from_numpy(blobs(seg, D)).cuda()
        off = np.concatenate([[0], np.cumsum(seg)]).astype(np.int64)
        graph = neighbors.neighbors(x, off, k)
        kw = dict(init="pca", x=x, n_epochs=n_epochs, a=A, b=B, seed=0)
        for _ in range(2):
            res = umap.layout(graph, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with _lib.AbiTimer(names) as t:
            for _ in range(calls):
                umap.layout(graph, **kw)
        s = t.summary()
        wall = (time.perf_counter() - t0) / calls
        entry = {"segments": int(seg.size), "rows": int(off[-1]), "k": k, "nnz": int(graph["nnz_offsets"][-1]),
                 "n_epochs": n_epochs, "attractive_samples": int(res["attractive_samples"].sum()),
                 "negative_samples": int(res["negative_samples"].sum()), "layout_wall_ms": 1e3 * wall,
                 "extent": float(res["embedding"].abs().max())}
        for key, ms in (("prepare", s["mcl_umap_prepare"]["ms"]), ("epochs", s["mcl_umap_epochs"]["ms"])):
            ms = sorted(ms)
            entry[f"{key}_ms_median"], entry[f"{key}_ms_min"], entry[f"{key}_ms_max"] = ms[len(ms) // 2], ms[0], ms[-1]
        entry["per_epoch_us_median"] = 1e3 * entry["epochs_ms_median"] / n_epochs
        doc[name] = entry
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--merge", default=None)
    a = ap.parse_args()
    if a.cpu:
        doc = {"gpu": "not measured: no timing run on an MI355X was made", "cpu_context": cpu()}
    else:
        doc = {"gpu": gpu(a.calls), "gpu_note": "HIP-event times on one MI355X"}
    if a.merge:
        with open(a.merge) as fh:
            doc["cpu_context"] = json.load(fh).get("cpu_context")
    line = json.dumps(doc)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
