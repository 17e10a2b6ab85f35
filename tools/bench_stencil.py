"""Stencil engine alone (csrc/k_stencil.hip) on one MI355X: us per launch and the fraction of the byte floor.

  * StencilGradients(fd_acc = 2 / 4 / 6) mode='all' and its adjoint on [64, 2, 64, 64] and [4096, 2, 64, 64].  Byte floor: six fp32
    fields (x and five derivatives forward, five cotangents and gx backward) over the HBM peak bench.py uses for its residual_only
    leg (PEAK_HBM_GBS, copied here).  Next to it the same operators as a user would write them without this library: the
    nine-convolution algorithm (one full interior convolution, eight edge strips, slice assignment) in plain torch on the same GPU.
  * The Darcy residual through the general entries with second-order tables against the specialised kernel, forward and backward.

    python tools/bench_stencil.py [batch ...]
"""
import itertools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pidm_oracle as O  # noqa: E402
from physicsinformeddiffusionmodels_amd._lib import get_lib, ptr, stream_ptr  # noqa: E402
from physicsinformeddiffusionmodels_amd.grad_utils import StencilGradients, _ops_array  # noqa: E402

PEAK_HBM_GBS = 8000.0       # bench.py's figure
WARMUP = 300                # launches before a timed window (what three cost)
P = 64
D0, D1 = 1.0 / 63, -1.0 / 63


def timed(call, min_seconds=0.3):
    """us per call: WARMUP calls, a short calibration window, then one window of at least min_seconds between two events."""
    for _ in range(WARMUP):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        call()
    e1.record()
    torch.cuda.synchronize()
    per = max(e0.elapsed_time(e1) / 20 * 1e-3, 1e-6)
    n = max(100, min(20000, int(min_seconds / per)))
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


class TorchNineConv:
    """One classed stencil operator in plain torch: the interior by one convolution over the whole image, each of the eight edge
    classes by a convolution over the strip it owns, written into place."""

    def __init__(self, comp, dev):
        self.mio, R = comp.max_inner_offset, max(comp.max_inner_offset, comp.max_offset)
        self.R = R
        self.k = {}
        for key, st in comp.stencils.items():
            k = torch.zeros(1, 1, 2 * R + 1, 2 * R + 1)
            for (di, dj), v in st.items():
                k[0, 0, R + di, R + dj] = v
            self.k[key] = k.to(dev)

    def __call__(self, x):      # [N, H, W]
        N, H, W = x.shape
        R, m = self.R, self.mio
        xp = F.pad(x[:, None], (R, R, R, R))
        y = F.conv2d(xp, self.k[("C", "C")])
        span = {"L": (0, m), "C": (m, H - m), "H": (H - m, H)}
        spanw = {"L": (0, m), "C": (m, W - m), "H": (W - m, W)}
        for rc, cc in itertools.product("LCH", repeat=2):
            if (rc, cc) == ("C", "C"):
                continue
            (r0, r1), (c0, c1) = span[rc], spanw[cc]
            y[:, :, r0:r1, c0:c1] = F.conv2d(xp[:, :, r0:r1 + 2 * R, c0:c1 + 2 * R], self.k[(rc, cc)])
        return y[:, 0]


def bench_operators(B, dev):
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 2, P, P, generator=g).to(dev)
    cots = [torch.randn(B, 2, P, P, generator=g).to(dev) for _ in range(5)]
    nbytes = 6 * x.numel() * 4
    floor_us = nbytes / (PEAK_HBM_GBS * 1e3)
    for acc in (2, 4, 6):
        sg = StencilGradients(d0=D0, d1=D1, fd_acc=acc, device=dev)
        with torch.no_grad():
            fwd = timed(lambda: sg(x, "all"))
        xr = x.clone().requires_grad_(True)
        ys = sg(xr, "all")
        adj = timed(lambda: torch.autograd.grad(ys, xr, cots, retain_graph=True))
        ref_ops = [TorchNineConv(getattr(sg, m), dev) for m in sg.MODES]
        xf = x.reshape(-1, P, P)
        with torch.no_grad():
            worst = max(float((r(xf) - y.reshape(-1, P, P)).abs().max() / y.abs().max()) for r, y in zip(ref_ops, ys))
            ref = timed(lambda: [r(xf) for r in ref_ops], min_seconds=0.2)
        print(f"stencil all  fd_acc={acc} B={B:5d}: fwd {fwd:9.2f} us ({floor_us / fwd:5.3f} of the {floor_us:.1f} us byte floor)  "
              f"adjoint {adj:9.2f} us ({floor_us / adj:5.3f})  plain-torch nine-conv fwd {ref:10.2f} us = {ref / fwd:6.1f} x "
              f"(max-norm difference {worst:.1e})", flush=True)


def bench_darcy(B, dev):
    L = get_lib()
    st = stream_ptr(dev)
    g = torch.Generator().manual_seed(B + 1)
    x0 = torch.randn(B, 2, P, P, generator=g)
    x0[:, 1] = torch.exp(0.5 * x0[:, 1])
    x0 = x0.to(dev)
    gr = torch.randn(B, P * P, 3, generator=g).to(dev)
    fs = O.darcy_source_field(P).reshape(-1).contiguous().to(dev)
    inv_h = float(P - 1)
    res, gx = torch.empty(B, P * P, 3, device=dev), torch.empty_like(x0)
    sg = StencilGradients(d0=1.0 / inv_h, d1=-1.0 / inv_h, fd_acc=2, device=dev)
    ops, keep = _ops_array((sg.d_d0, sg.d_d1, sg.d_d00, sg.d_d11), dev)
    ws = torch.empty(L.pidm_darcy_general_ws(B, P), dtype=torch.uint8, device=dev)
    t = {
        "spec_fwd": timed(lambda: L.check(L.pidm_darcy_residual_fwd(ptr(x0), ptr(fs), inv_h, -inv_h, ptr(res), B, P, st))),
        "gen_fwd": timed(lambda: L.check(L.pidm_darcy_residual_general_fwd(ptr(x0), ptr(fs), ops, 0, 1.0, ptr(res), ptr(ws), B, P, st))),
        "spec_bwd": timed(lambda: L.check(L.pidm_darcy_residual_bwd(ptr(x0), ptr(gr), inv_h, -inv_h, ptr(gx), B, P, st))),
        "gen_bwd": timed(lambda: L.check(L.pidm_darcy_residual_general_bwd(ptr(x0), ptr(gr), ops, 0, 1.0, ptr(gx), ptr(ws), B, P, st))),
    }
    print(f"darcy residual fd_acc=2 B={B:5d}: fwd specialised {t['spec_fwd']:8.2f} us, general {t['gen_fwd']:8.2f} us = "
          f"{t['gen_fwd'] / t['spec_fwd']:5.2f} x;  bwd specialised {t['spec_bwd']:8.2f} us, general {t['gen_bwd']:8.2f} us = "
          f"{t['gen_bwd'] / t['spec_bwd']:5.2f} x", flush=True)


def main():
    assert torch.cuda.is_available() and get_lib().backend == "hip", "bench_stencil.py measures on an MI355X"
    dev = torch.device("cuda:0")
    batches = [int(a) for a in sys.argv[1:]] or [64, 4096]
    print(f"{torch.cuda.get_device_name(0)}; warm-up {WARMUP} launches per timed window; byte floor at {PEAK_HBM_GBS:.0f} GB/s", flush=True)
    for B in batches:
        bench_operators(B, dev)
    for B in batches:
        bench_darcy(B, dev)


if __name__ == "__main__":
    main()
