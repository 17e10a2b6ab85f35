"""Throughput of the Darcy data generator (csrc/k_darcy_gen.hip) on the MI355X: samples/s and CGLS iterations per sample
(min / median / max) at P = 64 for batches of 256 and 1024, and at P = 32.  The KLE basis (host eigh) is computed once per P
and not timed.  Results go to stdout; DESIGN.md / profiles/ keep the recorded numbers.

    python tools/bench_darcy_gen.py [--cases 64:256,64:1024,32:256]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicsinformeddiffusionmodels_amd import darcy_data_generation as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64:256,64:1024,32:256")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    bases = {}
    for case in a.cases.split(","):
        P, B = (int(v) for v in case.split(":"))
        if P not in bases:
            bases[P] = D.kle_basis(P, 0.1, 64, True)
        seeds = list(range(1000, 1000 + B))
        D.generate_darcy_batch(seeds[:8], P, basis=bases[P], device=dev)          # warm-up (module load, LDS attribute)
        torch.cuda.synchronize()
        t = time.perf_counter()
        K, p, res, iters = D.generate_darcy_batch(seeds, P, basis=bases[P], device=dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        it = iters.cpu().numpy()
        print(f"P={P} B={B}: {dt:.3f} s, {B / dt:.1f} samples/s, iterations min {it.min()} median {int(np.median(it))} "
              f"max {it.max()}, {dt / B * 1e3:.2f} ms/sample, {dt / it.max() * 1e6:.2f} us per iteration of the batch, "
              f"res {float(res.mean()):.3e}", flush=True)


if __name__ == "__main__":
    main()
