"""Generates tests/golden/deconv.npz: what ``scipy.optimize.nnls(S^T, x_i)`` gives, spot by spot, for the cases of
tests/deconv_reference.py (``CASES`` and ``SLIDES_CASE``): ``<case>.coef`` (n, T) and ``<case>.rnorm`` (n,).

    python tests/golden/gen_deconv_goldens.py

The inputs are not stored: ``deconv_reference.make_case`` regenerates them from ``case_seed``.  Before writing, the numpy
restatement of the device's four calls is checked against scipy within a quarter of the perturbation bound
(``deconv_reference.coef_bound``), spot by spot, none left out."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deconv_reference as dr  # noqa: E402


def build(check=True):
    out = {}
    for G, T, n, collinear in dr.CASES + [dr.SLIDES_CASE]:
        S, x = dr.make_case(G, T, n, dr.case_seed(G, T, n), collinear)
        coef, rnorm = dr.scipy_nnls(x, S)
        if check:
            got = dr.nnls(x, S)
            assert (np.abs(got["coef"] - coef).max(axis=1) <= 0.25 * dr.coef_bound(x, S)).all(), (G, T, n)
            assert got["converged"].all()
        name = dr.case_name(G, T, n, collinear)
        out[f"{name}.coef"], out[f"{name}.rnorm"] = coef, rnorm
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "deconv.npz")
    np.savez_compressed(path, **build())
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
