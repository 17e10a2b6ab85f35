"""Wall time of a whole Darcy sampling chain against the number of visited time levels, in ONE process on one GPU:
p_sample_loop at dim 32, 64 x 64, batch 1024, n_steps = 1000, keep_history=False, for sampling_steps in (None, 100, 50, 20) -
None is the full ancestral walk, the others strided DDIM steps (eta = 0) through the same kernels.  One line per chain: the wall
time (host clock around the loop, device synchronised before and after), the time per visited level and the mean |r| of the final
state.  The expectation to CHECK (nothing is asserted): time proportional to the number of visited levels.

The weights are the oracle's deterministic fill, not a trained checkpoint: the residual column shows that the chain ran and stayed
finite, it says NOTHING about sample quality.

A chain of 1000 levels at batch 1024 takes about half a minute; run the tool under a time limit of its own, e.g.
    timeout -k 10 600 python tools/bench_sampler_steps.py --out profiles/sampler_steps.txt
Usage: bench_sampler_steps.py [--out FILE] [--batch B] [--n-steps T] [--steps none,100,50,20]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pidm_oracle as O  # noqa: E402
from physicsinformeddiffusionmodels_amd._lib import get_lib  # noqa: E402
from physicsinformeddiffusionmodels_amd.denoising_utils import DenoisingDiffusion  # noqa: E402
from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy  # noqa: E402
from physicsinformeddiffusionmodels_amd.unet_model import Unet3D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n-steps", type=int, default=1000)
    ap.add_argument("--steps", default="none,100,50,20", help="comma-separated sampling_steps values; 'none' = the full walk")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sampler_steps.py measures on an MI355X"
    assert get_lib().backend == "hip"
    dev, dim, P, B, T = torch.device("cuda:0"), 32, 64, args.batch, args.n_steps
    prop = torch.cuda.get_device_properties(0)
    lines = [f"whole Darcy sampling chain, dim {dim}, {P} x {P}, batch {B}, n_steps {T}, eta 0, keep_history=False; device: {prop.name}, "
             f"{prop.multi_processor_count} CUs; wall time of p_sample_loop, device synchronised before and after",
             "weights: deterministic fill, NOT a trained model - the mean |r| column says nothing about sample quality"]
    m = Unet3D(dim=dim, channels=2)
    m.load_state_dict(O.fill_state_dict(m.state_dict()))
    m = m.to(dev).eval()
    res = ResidualsDarcy(model=m, fd_acc=2, pixels_per_dim=P, pixels_at_boundary=True, reverse_d1=True, device=dev)
    diff = DenoisingDiffusion(T, dev)
    shape = (B, 2, P, P)

    def chain(sampling_steps):
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        (x_seq, _), aux = diff.p_sample_loop(None, shape, residual_func=res, eval_residuals=True, keep_history=False,
                                             sampling_steps=sampling_steps)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        x = x_seq[0]
        return wall, res.residual_of(x).abs().mean().item(), bool(torch.isfinite(x).all())

    chain(3)            # warm-up: engine set-up, graph capture and first replays
    chain(3)
    base = None
    for s in args.steps.split(","):
        S = None if s.strip().lower() == "none" else int(s)
        wall, r, finite = chain(S)
        n = T if S is None else S
        base = base or (wall, n)
        lines.append(f"  sampling_steps {str(S):>5s}: {n:5d} levels  {wall:9.3f} s  {1e3 * wall / n:8.3f} ms / level  "
                     f"time x{wall / base[0]:.4f} for levels x{n / base[1]:.4f}  mean |r| of the final state {r:.4e}  finite {finite}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
