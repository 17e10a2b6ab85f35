"""One guided sampler step at dim 32, 64 x 64, three ways in ONE process on one GPU (ms per step, device events):
  (a) inference forward only (an unguided step's UNet cost),
  (b) training-mode forward + pidm_unet_backward with an input gradient - how an input gradient was obtained before
      pidm_unet_backward_input existed (weight gradients computed and thrown away),
  (c) input_gradient_pass + cotangent kernel + pull + guided update kernel - the step of p_sample_loop_guided;
      (c-unet) is its UNet part alone (input_gradient_pass + pull), the like-for-like counterpart of (b),
  (c-flux) the same step with flux readings (flux_obs / flux_mask / zeta_flux): the one-launch flux cotangent kernel in place of
      the two-term one; its yardstick is (c) of the same run.
The legs alternate inside every round; the median over the rounds is reported, with the kernels per step from
pidm_debug_launch_counts (enqueued launch by launch + inside replayed graphs).  Usage: bench_guided.py [--out FILE] [BATCH ...]

--workload mechanics: the topology-optimisation sampler at dim 128, nel 64 (65 x 65 state), batch 32 by default:
  (plain) one unguided sampler step: input resize + inference forward + pidm_mech_residual_fwd + pidm_psample_update,
  (b) training-mode forward + full backward with an input gradient,
  (c) one guided step of p_sample_loop_guided_mechanics: input resize + input_gradient_pass + the one-launch cotangent kernel +
      pull + pidm_psample_update_guided_resized; (c-unet) is its resize + UNet part alone,
  (c-comp-e / c-comp-s) the same step with the compliance term (zeta_comp, compliance_form 'energy' / 'sensitivity'): the
      instantiations of the cotangent kernel with the fourth sum; their yardstick is (c) of the same run,
  (cot / cot-comp-e / cot-comp-s) the cotangent launch alone, without and with the compliance term; (cot-last) repeats (cot) at
      the end of the round: what the place in the round is worth for legs this short."""
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pidm_oracle as O  # noqa: E402
from physicsinformeddiffusionmodels_amd._engine import frozen_weights  # noqa: E402
from physicsinformeddiffusionmodels_amd._lib import get_lib, ptr, stream_ptr  # noqa: E402
from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy  # noqa: E402
from physicsinformeddiffusionmodels_amd.unet_model import Unet3D, input_gradient_pass  # noqa: E402


def kernels(L):
    a = (C.c_longlong * 4)()
    L.check(L.pidm_debug_launch_counts(a))
    return a[0] + a[2]


def engine_clock(L, dev, B):
    """the shader clock under load, as bench.py's roofline leg measures it (stamps inside a convolution kernel)"""
    try:
        from bench import rs_clock_probe
        probe = rs_clock_probe(L, dev, B) or {}
        ghz = probe.get("shader_clock_ghz")
        return f"{ghz:.2f} GHz" if ghz else "not measured"
    except Exception:
        return "not measured"


def measure(L, m, legs, lines, B, rounds=7, inner=5, warm=4):
    """alternate the legs inside every round; append one line per leg; returns the per-round times"""
    times = {k: [] for k, _ in legs}
    count = {}
    with frozen_weights(m):
        for k, fn in legs:
            for _ in range(warm):       # eager, capture, replay, replay
                fn()
            torch.cuda.synchronize()
            k0 = kernels(L)
            fn()
            count[k] = kernels(L) - k0
        for _ in range(rounds):
            for k, fn in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / inner)
    lines.append(f"batch {B}:")
    for k, _ in legs:
        v = times[k]
        lines.append(f"  ({k:42s}) {statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})  {count[k]:4d} kernels / step")
    return times


def finish(lines, out_path):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def main_mechanics(out_path, batches):
    from physicsinformeddiffusionmodels_amd.residuals_mechanics_K import ResidualsMechanics, _MechResidualFn, resize_image
    L, dev, dim, nel = get_lib(), torch.device("cuda:0"), 128, 64
    nn = nel + 1
    prop = torch.cuda.get_device_properties(0)
    lines = [f"guided mechanics step, dim {dim}, nel {nel} ({nn} x {nn} state); device: {prop.name}, {prop.multi_processor_count} CUs, "
             f"shader clock under load {engine_clock(L, dev, 64)}; ms per step = median of rounds (min .. max)"]
    m = Unet3D(dim=dim, channels=10, out_dim=3, sigmoid_last_channel=True)
    m.load_state_dict(O.fill_state_dict(m.state_dict()))
    m = m.to(dev)
    res = ResidualsMechanics(model=m, pixels_per_dim=nel, pixels_at_boundary=True, no_BC_folder="/nonexistent/", device=dev)
    for B in batches or [32]:
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, 3, nn, nn, generator=g).to(dev)
        z = torch.randn(B, 3, nn, nn, generator=g).to(dev)
        w = torch.randn(B, 3, nel, nel, generator=g).to(dev)
        obs = torch.rand(B, 3, nn, nn, generator=g).to(dev)
        mask = (torch.rand(B, 3, nn, nn, generator=g) < 0.1).float().to(dev)
        bcs = torch.zeros(B, 4, nn, nn)
        bcs[:, 0:2, :, 0] = 1.0
        bcs[:, 3, nn // 2, nn - 1] = -1.0
        bcs = bcs.to(dev)
        vf = (0.3 + 0.2 * torch.rand(B, generator=g)).to(dev)
        fixed_r = torch.randn(B, 7, nel, nel, generator=g).to(dev)          # conditioning and bcs, resized once before the loop
        t = torch.full((B,), 50, dtype=torch.long, device=dev)
        out = torch.empty_like(x)

        def net_input():
            return torch.cat((resize_image(x, nel, L), fixed_r), dim=1)

        def leg_plain():
            with torch.no_grad():
                x0p = m(net_input(), t)
                _, mo, _, _ = _MechResidualFn.apply(x0p, bcs, vf, res.stiffs, L)
                L.check(L.pidm_psample_update(ptr(mo), ptr(x), ptr(z), 0.3, 0.7, 0.05, ptr(out), x.numel(), stream_ptr(dev)))

        def leg_b():
            xr = net_input().requires_grad_(True)
            m(xr, t).backward(w)
            for p in m.parameters():
                p.grad = None

        def leg_c(**comp):
            with torch.no_grad():
                x0p, pull = input_gradient_pass(m, net_input(), t)
                v, mo, _ = res.guidance_cotangent(x0p, bcs, vf, obs, mask, 1.0, 1.0, 1.0, **comp)
                gr = pull(v)
                L.check(L.pidm_psample_update_guided_resized(ptr(mo), ptr(x), ptr(z), ptr(gr), 0.3, 0.7, 0.05, ptr(out), B, 3, 10, nel,
                                                             nn, stream_ptr(dev)))

        def leg_c_unet():
            with torch.no_grad():
                x0p, pull = input_gradient_pass(m, net_input(), t)
                pull(w)

        x0_fixed = torch.randn(B, 3, nel, nel, generator=g).to(dev)
        x0_fixed[:, 2] = torch.sigmoid(x0_fixed[:, 2])
        energy, sens = dict(zeta_comp=1.0, compliance_form='energy'), dict(zeta_comp=1.0, compliance_form='sensitivity')

        def leg_cot(**comp):
            res.guidance_cotangent(x0_fixed, bcs, vf, obs, mask, 1.0, 1.0, 1.0, **comp)

        legs = [("plain  unguided sampler step", leg_plain), ("b  training forward + full backward", leg_b),
                ("c-unet  resize + input_gradient_pass + pull", leg_c_unet), ("c  guided step", leg_c),
                ("c-comp-e  guided step, compliance (energy)", lambda: leg_c(**energy)),
                ("c-comp-s  guided step, compliance (sens.)", lambda: leg_c(**sens)),
                ("cot  cotangent call alone", leg_cot), ("cot-comp-e  cotangent call, energy", lambda: leg_cot(**energy)),
                ("cot-comp-s  cotangent call, sensitivity", lambda: leg_cot(**sens)),
                ("cot-last  the cot leg again (leg order)", lambda: leg_cot())]
        times = measure(L, m, legs, lines, B)
        p_, b_, u_, c_, ce_, cs_, k_, ke_, ks_, kl_ = (statistics.median(times[k]) for k, _ in legs)
        lines.append(f"  c / plain = {c_ / p_:.3f}   c / b = {c_ / b_:.3f}   c - c-unet = {1e3 * (c_ - u_):+.1f} us (the two guidance kernels)")
        lines.append(f"  c-comp-e - c = {1e3 * (ce_ - c_):+.1f} us   c-comp-s - c = {1e3 * (cs_ - c_):+.1f} us   "
                     f"cot-comp-e - cot = {1e3 * (ke_ - k_):+.1f} us   cot-comp-s - cot = {1e3 * (ks_ - k_):+.1f} us   cot-last - cot = {1e3 * (kl_ - k_):+.1f} us")
    finish(lines, out_path)


def main():
    args = sys.argv[1:]
    out_path = None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    workload = "darcy"
    if "--workload" in args:
        i = args.index("--workload")
        workload = args[i + 1]
        del args[i:i + 2]
    assert workload in ("darcy", "mechanics"), workload
    assert torch.cuda.is_available(), "bench_guided.py measures on an MI355X"
    if workload == "mechanics":
        return main_mechanics(out_path, [int(a) for a in args])
    batches = [int(a) for a in args] or [64, 1024]
    L, dev, dim, P = get_lib(), torch.device("cuda:0"), 32, 64
    prop = torch.cuda.get_device_properties(0)
    lines = [f"guided step, dim {dim}, {P} x {P}; device: {prop.name}, {prop.multi_processor_count} CUs, "
             f"shader clock under load {engine_clock(L, dev, 64)}; ms per step = median of rounds (min .. max)"]
    m = Unet3D(dim=dim, channels=2)
    m.load_state_dict(O.fill_state_dict(m.state_dict()))
    m = m.to(dev)
    res = ResidualsDarcy(model=m, fd_acc=2, pixels_per_dim=P, pixels_at_boundary=True, reverse_d1=True, device=dev)
    for B in batches:
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, 2, P, P, generator=g).to(dev)
        z = torch.randn(B, 2, P, P, generator=g).to(dev)
        w = torch.randn(B, 2, P, P, generator=g).to(dev)
        obs = torch.randn(B, 2, P, P, generator=g).to(dev)
        obs[:, 1] = torch.exp(0.5 * obs[:, 1])
        mask = (torch.rand(B, 2, P, P, generator=g) < 0.1).float().to(dev)
        yq = torch.randn(B, 2, P, P, generator=g).to(dev)
        mq = (torch.rand(B, 2, P, P, generator=g) < 0.1).float().to(dev)
        t = torch.full((B,), 50, dtype=torch.long, device=dev)
        x_nhwc = x.permute(0, 2, 3, 1).reshape(B, P * P, 2).contiguous()
        out = torch.empty_like(x)

        def leg_a():
            with torch.no_grad():
                m(x_nhwc, t)

        def leg_b():
            xr = x_nhwc.detach().requires_grad_(True)
            m(xr, t).backward(w)
            for p in m.parameters():
                p.grad = None

        def leg_c_unet():
            with torch.no_grad():
                x0p, pull = input_gradient_pass(m, x_nhwc, t)
                pull(w)

        def leg_c():
            with torch.no_grad():
                x0p, pull = input_gradient_pass(m, x_nhwc, t)
                v, _ = res.guidance_cotangent(x0p, obs, mask, 1.0, 1e-3)
                gr = pull(v)
                L.check(L.pidm_psample_update_guided(ptr(x0p), ptr(x), ptr(z), ptr(gr), 0.3, 0.7, 0.05, ptr(out), B, 2, P * P, stream_ptr(dev)))

        def leg_c_flux():
            with torch.no_grad():
                x0p, pull = input_gradient_pass(m, x_nhwc, t)
                v, _ = res.guidance_cotangent(x0p, obs, mask, 1.0, 1e-3, flux_obs=yq, flux_mask=mq, zeta_flux=0.01)
                gr = pull(v)
                L.check(L.pidm_psample_update_guided(ptr(x0p), ptr(x), ptr(z), ptr(gr), 0.3, 0.7, 0.05, ptr(out), B, 2, P * P, stream_ptr(dev)))

        legs = [("a  inference forward", leg_a), ("b  training forward + full backward", leg_b),
                ("c-unet  input_gradient_pass + pull", leg_c_unet), ("c  guided step (4 native calls)", leg_c),
                ("c-flux  guided step with flux readings", leg_c_flux)]
        times = measure(L, m, legs, lines, B)
        b_, c_ = statistics.median(times[legs[1][0]]), statistics.median(times[legs[2][0]])
        lines.append(f"  c-unet / b = {c_ / b_:.3f}")
        g_, f_ = statistics.median(times[legs[3][0]]), statistics.median(times[legs[4][0]])
        lines.append(f"  c-flux / c = {f_ / g_:.4f}  (c-flux - c = {1e3 * (f_ - g_):+.1f} us)")
    finish(lines, out_path)


if __name__ == "__main__":
    main()
