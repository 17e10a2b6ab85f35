"""What circular padding costs: the Darcy batch-64 training step (dim 32, 64 x 64; the step of DESIGN section 5 - model_estimation_loss,
zero_grad, backward, fused clip + Adam - on synthetic data resident in HBM) in three legs of ONE process on one MI355X:

  zeros        Unet3D(padding_mode='zeros'), default knobs (the bench.py headline configuration)
  circular     Unet3D(padding_mode='circular'), default knobs
  zeros_fp32   the zeros model with PIDM_CONV_SPLIT=0 PIDM_WGRAD_SPLIT=0 PIDM_LAP_SPLIT=0: every convolution, weight gradient and the
               attention products on the fp32-MFMA kernels

The legs alternate (--rounds blocks of --steps steps each, every block after --warmup untimed steps under its own knobs) so that clock
drift and neighbours hit all three alike; a leg's figure is the median of its blocks, the spread is min .. max.  Times are host clock
around work that ends in a device synchronise.  Needs the GPU: there is no CPU fall-back.

    python tools/bench_padding.py [--batch 64] [--steps 30] [--rounds 5] [--warmup 5] [--out profiles/circular_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicsinformeddiffusionmodels_amd._lib import get_lib, reload_knobs  # noqa: E402
from physicsinformeddiffusionmodels_amd.data_utils import synthetic_darcy_batch  # noqa: E402
from physicsinformeddiffusionmodels_amd.denoising_utils import DenoisingDiffusion  # noqa: E402
from physicsinformeddiffusionmodels_amd.optim import FusedClipAdam  # noqa: E402
from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy  # noqa: E402
from physicsinformeddiffusionmodels_amd.unet_model import Unet3D  # noqa: E402

FP32_KNOBS = {"PIDM_CONV_SPLIT": "0", "PIDM_WGRAD_SPLIT": "0", "PIDM_LAP_SPLIT": "0"}
LEGS = (("zeros", "zeros", {}), ("circular", "circular", {}), ("zeros_fp32", "zeros", FP32_KNOBS))


class Leg:
    def __init__(self, name, padding_mode, knobs, batch, dev):
        self.name, self.knobs = name, knobs
        torch.manual_seed(0)
        self.model = Unet3D(dim=32, channels=2, padding_mode=padding_mode).to(dev)
        self.diffusion = DenoisingDiffusion(100, dev)
        self.residuals = ResidualsDarcy(model=self.model, fd_acc=2, pixels_per_dim=64, pixels_at_boundary=True, reverse_d1=True,
                                        device=dev, bcs='none', domain_length=1.)
        self.batch = synthetic_darcy_batch(batch, 64, seed=100, device=dev)
        self.opt = FusedClipAdam(self.model, lr=1e-4, max_norm=1., image_size=64)
        self.ms = []

    def enter(self):
        for k in FP32_KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.knobs)
        reload_knobs()

    def step(self):
        loss, *_ = self.diffusion.model_estimation_loss(self.batch, residual_func=self.residuals, c_data=1., c_residual=1e-3,
                                                       c_ineq=0., lambda_opt=0.)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss

    def block(self, steps, warmup):
        self.enter()
        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = self.step()
        torch.cuda.synchronize()
        self.ms.append((time.perf_counter() - t0) / steps * 1e3)
        assert torch.isfinite(loss).all(), self.name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and get_lib().backend == "hip", "bench_padding needs an MI355X and libpidm_hip.so"
    dev = torch.device("cuda:0")
    legs = [Leg(n, pm, kn, args.batch, dev) for n, pm, kn in LEGS]
    for _ in range(args.rounds):
        for leg in legs:
            leg.block(args.steps, args.warmup)
    for k in FP32_KNOBS:
        os.environ.pop(k, None)
    reload_knobs()
    med = {leg.name: statistics.median(leg.ms) for leg in legs}
    lines = [f"# tools/bench_padding.py: Darcy step, dim 32, 64x64, batch {args.batch}; {args.rounds} alternating blocks of {args.steps} steps "
             f"per leg ({args.warmup} untimed steps before each); {torch.cuda.get_device_name(0)}",
             "# leg          median ms/step   min .. max        samples/s   vs zeros"]
    for leg in legs:
        m = med[leg.name]
        lines.append(f"{leg.name:<12} {m:10.3f}      {min(leg.ms):7.3f} .. {max(leg.ms):7.3f}   {args.batch / m * 1e3:9.0f}   {m / med['zeros']:6.3f}")
    lines.append(json.dumps({"batch": args.batch, "ms_per_step": med, "blocks_ms": {leg.name: leg.ms for leg in legs},
                             "circular_over_zeros": med["circular"] / med["zeros"],
                             "circular_not_slower_than_zeros_fp32": med["circular"] <= med["zeros_fp32"]}))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
