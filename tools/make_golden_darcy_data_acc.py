"""Writes tests/golden/g28_darcy_data_acc.npz from the reference data generator (src/darcy_data_generation.py of the reference
checkout given by --reference) at finite-difference orders 4 and 6: for P = 16, two samples per order, the seed, K, p and the mean
residual, all from the reference's own generate_sample.  CPU only.

findiff is not installed: the FinDiff / Coef the reference module sees are tools/findiff_standin_acc, whose coefficients are this
project's restatement of findiff's rule (grad_utils.fd_coefficients; parity with the real findiff unpinned, as oracle/shims/findiff
says of itself).  The system assembly, the row order and the lstsq solve are the reference's.

    python tools/make_golden_darcy_data_acc.py --reference /path/to/PhysicsInformedDiffusionModels
"""
import argparse
import importlib.util
import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
P = 16
SEEDS = {4: (1234567, 2718281828), 6: (31415926, 4000000007)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "g28_darcy_data_acc.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "findiff_standin_acc"))
    spec = importlib.util.spec_from_file_location("ref_darcy_gen", os.path.join(a.reference, "src", "darcy_data_generation.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    pab, L, l, q, rev = True, 1., 0.1, 64, True
    shape = (P, P)
    pts = R.uniform_points_pixelwise(P, L, pab)
    d0 = L / (P - 1)
    d1 = -d0
    lam, phi = R.compute_eigenpairs(R.complete_covariance_matrix(pts, l), q)
    f_s = R.create_f_s(pts[:, 0], pts[:, 1])
    bd = R.create_boundary_idcs(shape)
    int_cond = R.create_int_cond(True, shape, d0)
    out = {}
    for acc, seeds in SEEDS.items():
        for k, seed in enumerate(seeds):
            args = (k, lam, phi, q, P, shape, acc, d0, d1, f_s, int_cond, *bd, rev)
            # the reference derives the seed from pid and wall clock: pin both so that it is `seed`
            with mock.patch.object(R.os, "getpid", return_value=1), mock.patch.object(R.time, "time", return_value=seed / 1000.):
                K, p, res, s = R.generate_sample(args)
            assert s == seed, (s, seed)
            out[f"P{P}_acc{acc}_s{k}_seed"] = np.int64(seed)
            out[f"P{P}_acc{acc}_s{k}_K"] = K
            out[f"P{P}_acc{acc}_s{k}_p"] = p
            out[f"P{P}_acc{acc}_s{k}_res"] = np.float64(res)
            print(f"P={P} acc={acc} seed={seed}: K {K.min():.3g}..{K.max():.3g}, res {res:.4e}")
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
