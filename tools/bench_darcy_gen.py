"""Throughput of the Darcy data generator (csrc/k_darcy_gen_cgls.h) on the MI355X: samples/s and CGLS iterations per sample
(min / median / max) at P = 64 for batches of 256 and 1024, and at P = 32, with the number of launches and the longest single
launch (launch + read-back of the done flags).  The KLE basis (host eigh) is computed once per P and not timed.  --acc 2 / 4 / 6
selects the classed operators (csrc/k_darcy_gen_acc.hip); --bcs periodic (csrc/k_darcy_gen_per.hip) solves the periodic system on
fields of the periodic KLE basis (both files instantiate the one solver body).  Results go to stdout; DESIGN.md / profiles/ keep
the recorded numbers.

    python tools/bench_darcy_gen.py [--cases 64:256,64:1024,32:256] [--acc 4] [--iters-per-launch N] [--bcs periodic]
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
    ap.add_argument("--acc", type=int, default=2, choices=D.ACCS)
    ap.add_argument("--iters-per-launch", type=int, default=None)
    ap.add_argument("--max-iter", type=int, default=None)
    ap.add_argument("--bcs", default="none", choices=D.BCS)
    a = ap.parse_args()
    kw = dict(acc=a.acc, iters_per_launch=a.iters_per_launch, max_iter=a.max_iter, bcs=a.bcs)
    dev = torch.device("cuda:0")
    bases = {}
    for case in a.cases.split(","):
        P, B = (int(v) for v in case.split(":"))
        if P not in bases:
            bases[P] = D.kle_basis(P, 0.1, 64, True, bcs=a.bcs)
        seeds = list(range(1000, 1000 + B))
        D.generate_darcy_batch(seeds[:8], P, basis=bases[P], device=dev, **dict(kw, max_iter=10), rtol=1.)   # warm-up (module
        #                                                                    load, LDS attribute); rtol 1: converged at once
        torch.cuda.synchronize()
        t = time.perf_counter()
        st = {}
        K, p, res, iters = D.generate_darcy_batch(seeds, P, basis=bases[P], device=dev, stats=st, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        it = iters.cpu().numpy()
        entry = (f"{'pidm_darcy_gen_periodic' if a.bcs == 'periodic' else 'pidm_darcy_gen_acc'}, {st['launches']} launches of <= "
                 f"{st['iters_per_launch']} iterations, longest {st['longest_launch_s']:.3f} s")
        print(f"P={P} B={B} acc={a.acc} bcs={a.bcs} ({entry}): {dt:.3f} s, {B / dt:.1f} samples/s, iterations min {it.min()} median {int(np.median(it))} "
              f"max {it.max()}, {dt / B * 1e3:.2f} ms/sample, {dt / it.max() * 1e6:.2f} us per iteration of the batch, "
              f"res {float(res.mean()):.3e}", flush=True)


if __name__ == "__main__":
    main()
