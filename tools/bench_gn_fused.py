"""What finishing GroupNorm inside the 3x3 convolution workgroup (16x16 / 8x8 levels; PIDM_NO_GN_FUSED=1: off) is worth: the Darcy
training step (dim 32, 64 x 64; the step of DESIGN section 5 - model_estimation_loss, zero_grad, backward, fused clip + Adam - on
synthetic data resident in HBM) on one MI355X, three legs:

  new       this tree's libpidm_hip.so, default knobs
  knob_off  this tree's library with PIDM_NO_GN_FUSED=1 (the launches of the parent commit, from the new binary)
  parent    the library named by --parent (the parent commit's build, e.g. tools/build_old_lib.sh: ab_old/libpidm_hip.so); left out
            without --parent

Two libraries cannot share a process, so every block is a child process of its own (PIDM_LIBRARY selects the library): set-up,
--warmup untimed steps (they include the hipGraph capture), then --steps timed steps.  The legs alternate block by block, one process
at a time, so that clock drift and neighbours hit all legs alike; a leg's figure is the median of its blocks, the spread is
max - min.  The change counts as a gain if median(parent) - median(new) exceeds the parent's spread.  Times are host clock around
work that ends in a device synchronise.  Needs the GPU: there is no CPU fall-back.

    python tools/bench_gn_fused.py [--parent ab_old/libpidm_hip.so] [--batch 64 16] [--steps 30] [--rounds 5] [--warmup 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(batch, steps, warmup):
    import torch
    from physicsinformeddiffusionmodels_amd._lib import get_lib
    from physicsinformeddiffusionmodels_amd.data_utils import synthetic_darcy_batch
    from physicsinformeddiffusionmodels_amd.denoising_utils import DenoisingDiffusion
    from physicsinformeddiffusionmodels_amd.optim import FusedClipAdam
    from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
    from physicsinformeddiffusionmodels_amd.unet_model import Unet3D
    assert torch.cuda.is_available() and get_lib().backend == "hip", "bench_gn_fused needs an MI355X and libpidm_hip.so"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Unet3D(dim=32, channels=2).to(dev)
    diffusion = DenoisingDiffusion(100, dev)
    residuals = ResidualsDarcy(model=model, fd_acc=2, pixels_per_dim=64, pixels_at_boundary=True, reverse_d1=True, device=dev,
                               bcs='none', domain_length=1.)
    data = synthetic_darcy_batch(batch, 64, seed=100, device=dev)
    opt = FusedClipAdam(model, lr=1e-4, max_norm=1., image_size=64)

    def step():
        loss, *_ = diffusion.model_estimation_loss(data, residual_func=residuals, c_data=1., c_residual=1e-3, c_ineq=0., lambda_opt=0.)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    assert torch.isfinite(loss).all()
    print(json.dumps({"ms": ms, "loss": float(loss.detach())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parent", default=None, help="the parent commit's libpidm_hip.so")
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 16])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block-timeout", type=int, default=120, help="seconds a block's process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.batch[0], args.steps, args.warmup)
    legs = [("new", {}), ("knob_off", {"PIDM_NO_GN_FUSED": "1"})]
    if args.parent:
        legs.append(("parent", {"PIDM_LIBRARY": os.path.abspath(args.parent)}))
    lines = []
    for batch in args.batch:
        ms = {name: [] for name, _ in legs}
        loss = {}
        for _ in range(args.rounds):
            for name, env in legs:
                e = {k: v for k, v in os.environ.items() if k not in ("PIDM_NO_GN_FUSED", "PIDM_LIBRARY")}
                e.update(env)
                # a block that fails or hangs ends the measurement: nothing more is started on the GPU behind it
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--batch", str(batch), "--steps", str(args.steps),
                                    "--warmup", str(args.warmup)], env=e, stdout=subprocess.PIPE, timeout=args.block_timeout, check=True)
                r = json.loads(p.stdout.decode().strip().splitlines()[-1])
                ms[name].append(r["ms"])
                loss[name] = r["loss"]
        med = {n: statistics.median(v) for n, v in ms.items()}
        lines.append(f"# tools/bench_gn_fused.py: Darcy step, dim 32, 64x64, batch {batch}; {args.rounds} alternating blocks (one process each) of "
                     f"{args.steps} steps per leg, {args.warmup} untimed steps before each")
        lines.append("# leg        median ms/step   min .. max      max-min   last loss")
        for name, _ in legs:
            v = ms[name]
            lines.append(f"{name:<10} {med[name]:10.3f}      {min(v):7.3f} .. {max(v):7.3f}  {max(v) - min(v):7.3f}   {loss[name]:.9e}")
        rec = {"batch": batch, "ms_per_step": med, "blocks_ms": ms}
        if args.parent:
            spread = max(ms["parent"]) - min(ms["parent"])
            rec.update({"parent_minus_new_ms": med["parent"] - med["new"], "parent_spread_ms": spread,
                        "gain_exceeds_parent_spread": med["parent"] - med["new"] > spread})
            lines.append(f"# parent - new = {med['parent'] - med['new']:.3f} ms ({(med['parent'] - med['new']) / med['parent'] * 100:.2f} %), "
                         f"parent's spread {spread:.3f} ms")
        lines.append(json.dumps(rec))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
