#!/usr/bin/env python3
"""Generate ``hvg.npz``: tests/hvg_reference.py (numpy + pandas' own cut / groupby) run over
``mclstexp_amd.synth.make_counts_case`` tables.  Inputs are regenerated from their seeds by the tests, never stored.

Per case ``c`` and slide ``i`` (key prefix ``c.i.``): ``means``, ``dispersions``, ``dispersions_norm``, ``cutoff``,
``target_sum`` of the fp64 mode (numpy sums), the same with suffix ``32`` of the fp32 mode (what scanpy does to an integer
matrix), ``mean_bin``, ``highly_variable``, ``edges``.  Per case: ``c.n_top``, ``c.order_gap`` = the largest gap between the
fp64 mode with numpy sums and with exactly rounded sums (math.fsum) over all continuous outputs of all slides -- the
yardstick of the GPU tolerance -- and ``c.gap32`` = the largest fp32-mode vs fp64-mode gap.

The generator asserts the room that makes EXACT equality of bins and flags a fair demand (tests/test_preprocess_host.py
asserts the same on the stored arrays): no ``means`` within 1000 x order_gap of a bin edge, no ``dispersions_norm`` within
10 x gap32 of the cut-off (the gene at the cut-off and the planted tie excepted), the two modes agree on every bin and
flag.  A case that fails is re-seeded in tests/hvg_reference.py, not excused.

    python tests/golden/gen_hvg_goldens.py        # writes tests/golden/hvg.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import hvg_reference as hr  # noqa: E402


def tie_n_top(counts, pair):
    """n_top_genes that puts the cut-off exactly on the duplicated pair: both pass, one more gene than asked for."""
    r = hr.highly_variable_genes(counts, counts.shape[1])
    v = r["dispersions_norm"]
    assert v[pair[0]] == v[pair[1]] and not np.isnan(v[pair[0]])
    rank = int((v[~np.isnan(v)] > v[pair[0]]).sum())          # genes strictly above the pair
    assert hr.TIE_RANK_WINDOW[0] <= rank < hr.TIE_RANK_WINDOW[1], f"re-seed the tie case: the pair ranks {rank}"
    return rank + 1


def build():
    out = {}
    for name, (n_top, slide_kw) in hr.HVG_CASES.items():
        slides = hr.case_slides(name)
        if n_top is None:
            n_top = tie_n_top(slides[0], slide_kw[0]["duplicate"])
        order_gap = gap32 = 0.0
        for i, c in enumerate(slides):
            r64 = hr.highly_variable_genes(c, n_top, np.float64, "numpy")
            rfs = hr.highly_variable_genes(c, n_top, np.float64, "fsum")
            r32 = hr.highly_variable_genes(c, n_top, np.float32)
            order_gap = max(order_gap, hr.max_gap(r64, rfs))
            gap32 = max(gap32, hr.max_gap(r64, r32))
            for k in hr.CONTINUOUS:
                out[f"{name}.{i}.{k}"] = np.asarray(r64[k], dtype=np.float64)
                out[f"{name}.{i}.{k}32"] = np.asarray(r32[k], dtype=np.float64)
            out[f"{name}.{i}.mean_bin"] = r64["mean_bin"]
            out[f"{name}.{i}.highly_variable"] = r64["highly_variable"]
            out[f"{name}.{i}.edges"] = r64["edges"]
            for other in (rfs, r32):
                assert np.array_equal(other["mean_bin"], r64["mean_bin"]), (name, i)
                assert np.array_equal(other["highly_variable"], r64["highly_variable"]), (name, i)
            assert r64["mean_bin"].min() >= 0
        out[f"{name}.n_top"] = np.int64(n_top)
        out[f"{name}.order_gap"] = np.float64(order_gap)
        out[f"{name}.gap32"] = np.float64(gap32)
        assert order_gap >= 1e-15, (name, order_gap, "a zero yardstick measures nothing: enlarge the case")
        for i in range(len(slides)):
            em = hr.edge_margin(out[f"{name}.{i}.means"], out[f"{name}.{i}.edges"])
            cm = hr.cutoff_margin(out[f"{name}.{i}.dispersions_norm"], out[f"{name}.{i}.cutoff"])
            cm32 = hr.cutoff_margin(out[f"{name}.{i}.dispersions_norm32"], out[f"{name}.{i}.cutoff32"])
            assert em > 1000 * order_gap, (name, i, em, order_gap)
            assert min(cm, cm32) > 10 * gap32, (name, i, cm, cm32, gap32)
            hv = out[f"{name}.{i}.highly_variable"]
            print(f"{name}.{i}: {slides[i].shape} n_top {n_top} flagged {int(hv.sum())} NaN "
                  f"{int(np.isnan(out[f'{name}.{i}.dispersions_norm']).sum())} cutoff {float(out[f'{name}.{i}.cutoff']):.4f} "
                  f"edge margin {em:.1e} cutoff margin {min(cm, cm32):.1e}")
        print(f"{name}: order_gap {order_gap:.2e} gap32 {gap32:.2e}")
    # what each case is there for
    assert int(np.isnan(out["zero_genes.0.dispersions_norm"]).sum()) >= 9
    assert np.bincount(out["single_bin.0.mean_bin"], minlength=hr.N_BINS)[-1] == 1
    assert out["single_bin.0.dispersions_norm"][-1] == 1.0
    assert int(out["n_top_large.n_top"]) > int((~np.isnan(out["n_top_large.0.dispersions_norm"])).sum())
    assert out["n_top_large.0.highly_variable"].all()
    assert float(out["neg_cutoff.0.cutoff"]) <= 0 and out["neg_cutoff.0.highly_variable"][
        np.isnan(out["neg_cutoff.0.dispersions_norm"])].all()
    assert int(out["tie.0.highly_variable"].sum()) == int(out["tie.n_top"]) + 1
    return out


def main():
    out = build()
    path = os.path.join(HERE, "hvg.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
