"""Throughput of the mechanics data generator (csrc/k_mech_gen.hip) on the MI355X: samples/s for a batch of 256 at nel = 64,
SIMP iterations per sample and CG iterations per SIMP iteration (min / median / max), plus the time of one `pidm_simp_step`
launch.  `--filter` takes a comma-separated list (sensitivity, density, heaviside): every case runs once per listed filter, in
that order, in one process.  Results go to stdout; DESIGN.md / profiles/mech_gen_bench.txt / profiles/mech_gen_bench_filtered.txt
keep the recorded numbers.

    python tools/bench_mech_gen.py [--cases 64:256] [--max-iter 100] [--filter sensitivity,heaviside]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicsinformeddiffusionmodels_amd import mechanics_data_generation as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64:256")
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--n-loads", type=int, default=1)
    ap.add_argument("--filter", default="sensitivity", help="comma-separated: sensitivity, density, heaviside")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = [(case, filt) for case in a.cases.split(",") for filt in a.filter.split(",")]
    for case, filt in cases:
        nel, B = (int(v) for v in case.split(":"))
        tag = "" if filt == "sensitivity" else f" filter={filt}"
        seeds = list(range(1000, 1000 + B))
        M.generate_mechanics_batch(seeds[:4], nel, n_loads=a.n_loads, max_iter=2, filter=filt, device=dev)      # warm-up (module load, mesh tables)
        torch.cuda.synchronize()
        t = time.perf_counter()
        data, info = M.generate_mechanics_batch(seeds, nel, n_loads=a.n_loads, max_iter=a.max_iter, filter=filt, return_info=True,
                                                device=dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        ns = info["iters"]["simp"].cpu().numpy()
        pcg = info["iters"]["pcg"].cpu().numpy()                    # [steps, B]; 0 where a sample was already done
        steps = pcg.shape[0]
        live = pcg[np.arange(steps)[:, None] < ns[None, :]]
        comp = info["compliance"].cpu().numpy()
        print(f"nel={nel} B={B}{tag}: {dt:.3f} s, {B / dt:.1f} samples/s, {dt / B * 1e3:.2f} ms/sample; SIMP iterations per sample min "
              f"{ns.min()} median {int(np.median(ns))} max {ns.max()} ({steps} launches, {(ns < a.max_iter).sum()} of {B} samples "
              f"below tol); CG iterations per SIMP iteration min {live.min()} median {int(np.median(live))} max {live.max()}, first "
              f"step median {int(np.median(pcg[0]))}; compliance first -> last step median {np.median(comp[0]):.2f} -> "
              f"{np.median(comp[ns - 1, np.arange(B)]):.2f}; "
              f"solid fraction of E_field {float((data[:, 5, :nel, :nel] == 1).float().mean()):.3f}", flush=True)
        # time per SIMP iteration of the batch: the optimisation loop alone, max_iter launches with nothing switched off (tol = 0)
        bcs, vf = data[:, 6:10].contiguous(), data[:, 0, 0, 0].contiguous()
        torch.cuda.synchronize()
        t = time.perf_counter()
        _, _, _, it_info = M.simp_optimize(bcs, vf, nel, max_iter=a.max_iter, tol=0., filter=filt, device=dev)
        torch.cuda.synchronize()
        dts = time.perf_counter() - t
        cg = it_info["pcg"].cpu().numpy()
        print(f"nel={nel} B={B}{tag}: simp_optimize with tol 0: {a.max_iter} launches in {dts:.3f} s = {dts / a.max_iter * 1e3:.2f} ms per "
              f"SIMP iteration of the batch; CG iterations per launch (max over the batch) median {int(np.median(cg.max(1)))}, "
              f"sum {int(cg.max(1).sum())}: {dts / cg.max(1).sum() * 1e6:.1f} us per CG iteration of the batch, everything else included",
              flush=True)
        # one launch in isolation: the step after the first, warm-started, every sample active
        x = vf.double().view(B, 1).repeat(1, nel * nel).contiguous()
        u = torch.zeros(B, 2 * (nel + 1) ** 2, dtype=torch.float64, device=dev)
        o = M.simp_step(x, u, bcs, vf, nel, filter=filt)
        torch.cuda.synchronize()
        t = time.perf_counter()
        o2 = M.simp_step(o["x"], o["u"], bcs, vf, nel, filter=filt)
        torch.cuda.synchronize()
        dt1 = time.perf_counter() - t
        it2 = o2["pcg_iters"].cpu().numpy()
        print(f"nel={nel} B={B}{tag}: second pidm_simp_step launch {dt1 * 1e3:.1f} ms, CG iterations max {it2.max()}: "
              f"{dt1 / it2.max() * 1e6:.1f} us per CG iteration of the batch", flush=True)


if __name__ == "__main__":
    main()
