"""Circular padding: `Unet3D(padding_mode='circular')` and `pidm_conv_desc::pad_mode = 1` (reference: src/unet_model.py:161-199,
224-229, 424, 452-455, 480-511).  `backend` = host-emulated build of the unmodified .hip sources on CPU, the real gfx950 library
with -m gpu.

Yardsticks: tests/golden/g28_unet_circular.npz holds the genuine reference's results (tools/make_golden_unet_circular.py);
tests/unet_circ_ref.py restates circular padding on top of the oracle's functional UNet and is held to g28 here before it is used
for the shapes the golden does not cover.  Shift equivariance needs neither: a circular UNet commutes with shifts by multiples of
2^(levels - 1) up to rounding (the reference shows <= 6e-7 of max |y| there and >= 0.17 for any other shift or a zero-padding
model), which a zero-padding engine cannot pass.

Tolerances are those of tests/test_unet_config_sweep.py (forward 3e-5 max-norm relative; gradients 1e-3 |g_ref| + 2e-6 g_max) and
of tests/test_kernels_conv.py for the same entry points (forward 2e-6, dgrad / wgrad 5e-6); two engine evaluations are compared
at twice the forward bound."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pidm_oracle as O
from physicsinformeddiffusionmodels_amd._engine import frozen_weights, get_engine
from physicsinformeddiffusionmodels_amd._lib import ConvDesc, PidmError, ptr, stream_ptr
from physicsinformeddiffusionmodels_amd.denoising_utils import DenoisingDiffusion
from physicsinformeddiffusionmodels_amd.optim import FusedClipAdam
from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
from physicsinformeddiffusionmodels_amd.unet_model import Unet3D
from tests.test_training_step import patched_rng
from tests.unet_circ_ref import circular_conv2d, circular_conv_transpose2d, unet_forward_circular

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G28 = os.path.join(REPO, "tests", "golden", "g28_unet_circular.npz")
FWD_TOL = 3e-5

# tag -> (constructor arguments, image size, batch, conditioned): the cases of tools/make_golden_unet_circular.py
GOLDEN_CASES = {
    "d8_p16": (dict(dim=8), 16, 3, False),
    "d8_p8_l2": (dict(dim=8, dim_mults=(1, 2)), 8, 2, False),
    "d32_p32_l3": (dict(dim=32, dim_mults=(1, 2, 4)), 32, 1, False),
    "d8_p16_cond": (dict(dim=8), 16, 3, True),
}
PROBES = ("init_conv.weight", "downs.0.0.block1.proj.weight", "downs.0.3.weight", "ups.0.3.conv_transpose.weight",
          "downs.0.2.fn.fn.to_qkv.weight")
# the shapes of tests/test_unet_config_sweep.py the issue names, in circular mode
SWEEP_CASES = {
    "channels_3": (16, 2, dict(dim=8, channels=3)),
    "three_levels": (16, 2, dict(dim=8, dim_mults=(1, 2, 4))),
    "init_kernel_3": (16, 2, dict(dim=8, init_kernel_size=3)),
    "init_kernel_5": (16, 2, dict(dim=8, init_kernel_size=5)),
    "sigmoid_last_channel": (16, 2, dict(dim=8, sigmoid_last_channel=True)),
    "heads_4_projected_attention": (32, 1, dict(dim=32, dim_mults=(1, 2, 4), attn_heads=4)),
    "row_streaming_groups_4": (32, 1, dict(dim=32, dim_mults=(1, 2, 4), resnet_groups=4)),
}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _lib_of(backend):
    L, dev = backend
    return (L if dev.type == "cpu" else None), dev


def _model(backend, padding_mode="circular", **kw):
    lib, dev = _lib_of(backend)
    m = Unet3D(padding_mode=padding_mode, **kw)
    m.load_state_dict(O.fill_state_dict(m.state_dict()))
    m = m.to(dev)
    m._pidm_lib = lib
    return m


def _oracle_cfg(kw):
    ch = kw.get("channels", 2)
    return O.UnetCfg(kw["dim"], channels=ch, out_dim=kw.get("out_dim"), dim_mults=kw.get("dim_mults", (1, 2, 4, 8)),
                     heads=kw.get("attn_heads", 8), groups=kw.get("resnet_groups", 8),
                     sigmoid_last_channel=kw.get("sigmoid_last_channel", False))


def _restated(m, x, t, w, kw, cond=None):
    """forward and all parameter gradients of sum(w * out) from the restatement, on CPU copies of m's parameters"""
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    ref = unet_forward_circular(p, x, t, _oracle_cfg(kw), cond=cond)
    (ref * w).sum().backward()
    return ref.detach(), p


def _assert_gradients(m, p):
    gmax = max(float(v.grad.norm()) for v in p.values() if v.grad is not None)
    n = 0
    for k, prm in m.named_parameters():
        rg = p[k].grad
        if prm.grad is None:
            assert rg is None or float(rg.abs().max()) == 0.0, k      # exactly the parameters the forward uses
            continue
        rg = torch.zeros_like(p[k]) if rg is None else rg
        err = float((prm.grad.double().cpu() - rg.double()).norm())
        assert err <= 1e-3 * float(rg.double().norm()) + 2e-6 * gmax, (k, err)
        n += 1
    return n, gmax


# ------------------------------------------------------------------------------------------------------------------------------
# golden and restatement parity
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(GOLDEN_CASES))
def test_restatement_and_engine_reproduce_the_reference(backend, tag):
    """g28: the restatement first (it is the yardstick of the next test), then the engine: forward, the gradient norm of every
    parameter, the full gradient of the probe tensors, and the same set of parameters without a gradient."""
    g = np.load(G28)
    kw, P, B, conditioned = GOLDEN_CASES[tag]
    m = _model(backend, **kw)
    dev = next(m.parameters()).device
    x, t, w = torch.from_numpy(g[tag + "/x"]), torch.from_numpy(g[tag + "/t"]), torch.from_numpy(g[tag + "/w"])
    cond = torch.from_numpy(g[tag + "/cond"]) if conditioned else None
    gold = torch.from_numpy(g[tag + "/out"])
    names = [str(k) for k in g[tag + "/grad_names"]]
    norms = dict(zip(names, g[tag + "/grad_norms"]))
    gmax = float(max(norms.values()))

    ref, p = _restated(m, x, t, w, kw, cond)
    assert rel(ref, gold) < FWD_TOL
    assert sorted(k for k, v in p.items() if v.grad is not None and float(v.grad.abs().max()) > 0) == sorted(names)
    for k in names:
        assert abs(float(p[k].grad.double().norm()) - norms[k]) <= 1e-3 * norms[k] + 2e-6 * gmax, k
    for k in PROBES:
        gk = torch.from_numpy(g[tag + "/grad/" + k]).double()
        assert float((p[k].grad.double() - gk).norm()) <= 1e-3 * float(gk.norm()) + 2e-6 * gmax, k

    xb = x.permute(0, 2, 3, 1).reshape(B, P * P, 2).to(dev)
    out = m(xb, t.to(dev), cond=cond.to(dev)) if conditioned else m(xb, t.to(dev))
    (out * w.to(dev)).sum().backward()
    assert rel(out, gold) < FWD_TOL
    got = {k: prm.grad for k, prm in m.named_parameters() if prm.grad is not None}
    assert sorted(got) == sorted(names)
    for k in names:
        assert abs(float(got[k].double().norm()) - norms[k]) <= 1e-3 * norms[k] + 2e-6 * gmax, k
    for k in PROBES:
        gk = torch.from_numpy(g[tag + "/grad/" + k]).double()
        assert float((got[k].double().cpu() - gk).norm()) <= 1e-3 * float(gk.norm()) + 2e-6 * gmax, k
    _assert_gradients(m, p)


@pytest.mark.parametrize("name", sorted(SWEEP_CASES))
def test_circular_configuration_matches_the_restatement(backend, monkeypatch, name):
    if name.startswith("row_streaming"):
        monkeypatch.setenv("PIDM_CONV_RS_WAVES", "4")
        monkeypatch.setenv("PIDM_CONV_RS_MINR", "4")
    P, B, kw = SWEEP_CASES[name]
    torch.manual_seed(7)
    m = _model(backend, **kw)
    dev = next(m.parameters()).device
    ch = kw.get("channels", 2)
    x = torch.randn(B, P * P, ch)
    t = torch.randint(0, 100, (B,))
    pz = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    ref = unet_forward_circular(pz, x, t, _oracle_cfg(kw))
    w = torch.randn_like(ref)
    (ref * w).sum().backward()
    out = m(x.to(dev), t.to(dev))
    assert tuple(out.shape) == tuple(ref.shape)
    (out * w.to(dev)).sum().backward()
    assert rel(out, ref) < FWD_TOL
    _assert_gradients(m, pz)


def test_parameters_without_gradient_are_those_of_zero_mode(backend):
    """after one step, `grad is None` for the same parameters as in the zero-padding model (names differ only in the upsamplers'
    sub-module)"""
    none = {}
    for mode in ("zeros", "circular"):
        m = _model(backend, padding_mode=mode, dim=8)
        dev = next(m.parameters()).device
        gen = torch.Generator().manual_seed(9)
        out = m(torch.randn(2, 256, 2, generator=gen).to(dev), torch.tensor([4, 40]).to(dev))
        out.sum().backward()
        none[mode] = {k.replace(".3.conv_transpose.", ".3.") for k, v in m.named_parameters() if v.grad is None}
    assert none["circular"] == none["zeros"] and len(none["zeros"]) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# shift equivariance
# ------------------------------------------------------------------------------------------------------------------------------
EQUIVARIANCE = {   # name -> (image, constructor arguments, shifts): multiples of 2^(levels - 1)
    "p16_l4": (16, dict(dim=8), (8,)),
    "p8_l2": (8, dict(dim=8, dim_mults=(1, 2)), (2, 4)),
    "p16_l3": (16, dict(dim=8, dim_mults=(1, 2, 4)), (4, 12)),
}
_base = {}


def _evaluate(m, x_img, t, w_img):
    """x_img [B, C, P, P] -> (out, d sum(w out) / dx as an image, parameter gradients)"""
    B, C, P, _ = x_img.shape
    for prm in m.parameters():
        prm.grad = None
    xb = x_img.permute(0, 2, 3, 1).reshape(B, P * P, C).contiguous().requires_grad_(True)
    out = m(xb, t)
    (out * w_img).sum().backward()
    gx = xb.grad.reshape(B, P, P, C).permute(0, 3, 1, 2)
    return out.detach().clone(), gx.clone(), {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}


def _equivariance_base(backend, name):
    """the unshifted evaluation, computed once per configuration and backend and left unchanged"""
    lib, dev = _lib_of(backend)
    key = (name, dev.type)
    if key not in _base:
        P, kw, _ = EQUIVARIANCE[name]
        m = _model(backend, **kw)
        gen = torch.Generator().manual_seed(31)
        x = torch.randn(2, 2, P, P, generator=gen).to(dev)
        w = torch.randn(2, 2, P, P, generator=gen).to(dev)
        t = torch.tensor([11, 83]).to(dev)
        _base[key] = (m, x, t, w) + _evaluate(m, x, t, w)
    return _base[key]


@pytest.mark.parametrize("dims", [(2, 3), (2,)], ids=["rows_and_columns", "rows_only"])
@pytest.mark.parametrize("name,shift", [(n, s) for n in sorted(EQUIVARIANCE) for s in EQUIVARIANCE[n][2]])
def test_shift_equivariance(backend, name, shift, dims):
    m, x, t, w, out, gx, grads = _equivariance_base(backend, name)
    sh = (shift,) * len(dims)
    out_s, gx_s, grads_s = _evaluate(m, torch.roll(x, sh, dims), t, torch.roll(w, sh, dims))
    assert rel(out_s, torch.roll(out, sh, dims)) < 2 * FWD_TOL
    gmax = max(float(v.norm()) for v in grads.values())
    err = float((gx_s.double() - torch.roll(gx, sh, dims).double()).norm())
    assert err <= 1e-3 * float(gx.double().norm()) + 2e-6 * gmax, err
    assert sorted(grads_s) == sorted(grads)
    for k, gk in grads.items():
        err = float((grads_s[k].double() - gk.double()).norm())
        assert err <= 1e-3 * float(gk.double().norm()) + 2e-6 * gmax, (k, err)


def test_zero_padding_model_is_not_shift_equivariant(backend):
    """the property above is one of the padding: the same shapes with zero padding miss it by the size of the output"""
    P, kw, shifts = EQUIVARIANCE["p8_l2"]
    m = _model(backend, padding_mode="zeros", **kw)
    dev = next(m.parameters()).device
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(2, 2, P, P, generator=gen).to(dev)
    t = torch.tensor([11, 83]).to(dev)
    with torch.no_grad():
        f = lambda z: m(z.permute(0, 2, 3, 1).reshape(2, P * P, 2).contiguous(), t)  # noqa: E731
        assert rel(f(torch.roll(x, (4, 4), (2, 3))), torch.roll(f(x), (4, 4), (2, 3))) > 0.1


# ------------------------------------------------------------------------------------------------------------------------------
# unit level: pidm_conv_* with pad_mode = 1
# ------------------------------------------------------------------------------------------------------------------------------
UNIT_CASES = [
    # B, H, C0, C1, Cout, K, stride, pad, transposed
    (3, 2, 16, 0, 32, 3, 1, 1, 0),       # 2x2: both horizontal (and vertical) neighbours of a pixel are the same pixel; 32 images per tile
    (3, 4, 32, 0, 32, 3, 1, 1, 0),       # 4x4: 8 images per tile, the wrap stays inside its image
    (3, 8, 32, 0, 64, 3, 1, 1, 0),       # 8x8: two images per tile, ragged batch; the streaming kernel's re-written halo columns
    (1, 32, 32, 0, 32, 3, 1, 1, 0),      # 32-wide rows: tiles of 4 rows, the halo rows of the first / last tile are rows 31 / 0
    (3, 4, 16, 0, 16, 4, 2, 1, 0),       # downsample 4x4 -> 2x2 (phased); its input gradient is the parity form at 2x2
    (3, 2, 16, 0, 16, 4, 2, 1, 1),       # upsample 2x2 -> 4x4 (parity form); its input gradient is the phased form
    (2, 8, 2, 0, 8, 7, 1, 3, 0),         # init convolution: 3 wrapped taps on either side of an 8-wide row
    (3, 8, 16, 16, 40, 3, 1, 1, 0),      # two sources, Cout not a multiple of 32
    (2, 8, 12, 0, 8, 4, 2, 1, 0),        # 4x4 / stride 2 with ragged channels: the un-phased generic kernels
    (2, 16, 32, 32, 32, 3, 1, 1, 0),     # 16-wide rows, two 32-channel sources: two 8-pixel strips per row in the row-streaming weight gradient
]


def _unit(backend, B, H, C0, C1, Cout, K, stride, pad, transposed):
    L, dev = backend
    st = stream_ptr(dev)
    g = torch.Generator().manual_seed(4321 + B + H + C0 + Cout)
    Cin = C0 + C1
    nhwc = lambda z: z.permute(0, 2, 3, 1).contiguous()  # noqa: E731
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(*((Cin, Cout) if transposed else (Cout, Cin)), K, K, generator=g) / (Cin * (4 if transposed else K * K)) ** 0.5
    bias = torch.randn(Cout, generator=g)
    xr, wr, br = (z.clone().requires_grad_(True) for z in (x, w, bias))
    ref = circular_conv_transpose2d(xr, wr, br) if transposed else circular_conv2d(xr, wr, br, stride, pad)
    Ho = ref.shape[-1]
    res = torch.randn(B, Cout, Ho, Ho, generator=g)
    dy = torch.randn(B, Cout, Ho, Ho, generator=g)
    (ref + res).backward(dy)
    zero = F.conv_transpose2d(x, w, bias, stride=2, padding=1) if transposed else F.conv2d(x, w, bias, stride=stride, padding=pad)
    assert rel(zero, ref) > 1e-2                          # the case tells the two padding modes apart

    x0 = nhwc(x[:, :C0]).to(dev)
    x1 = nhwc(x[:, C0:]).to(dev) if C1 else None
    w, bias = w.to(dev), bias.to(dev)
    d = ConvDesc(B=B, Hi=H, Wi=H, C0=C0, C1=C1, ld0=C0, ld1=C1, Cout=Cout, KH=K, KW=K, stride=stride, pad=pad,
                 transposed=transposed, out_nchw=0, ldo=Cout, pad_mode=1)
    wp = torch.empty(L.pidm_conv_packed_weight_floats(d), device=dev)
    L.check(L.pidm_conv_pack_weights(d, ptr(w), ptr(wp), 0, st))
    out = torch.full((B, Ho, Ho, Cout), float("nan"), device=dev)
    resn = nhwc(res).to(dev)
    L.check(L.pidm_conv_forward(d, ptr(x0), ptr(x1), ptr(wp), ptr(bias), ptr(resn), ptr(out), st))
    assert rel(out, nhwc((ref + res).detach())) < 2e-6
    wd = torch.empty(L.pidm_conv_dgrad_packed_weight_floats(d), device=dev)
    L.check(L.pidm_conv_pack_weights(d, ptr(w), ptr(wd), 1, st))
    dx = torch.full((B, H, H, Cin), float("nan"), device=dev)
    extra = torch.randn(B, H, H, Cin, generator=g).to(dev)
    dyn = nhwc(dy).to(dev)
    L.check(L.pidm_conv_dgrad(d, ptr(dyn), Cout, ptr(wd), ptr(extra), ptr(dx), Cin, st))
    assert rel(dx - extra, nhwc(xr.grad)) < 5e-6
    ws = torch.empty(L.pidm_conv_wgrad_ws(d), dtype=torch.uint8, device=dev)
    dw = torch.full_like(w, float("nan"))
    db = torch.full((Cout,), float("nan"), device=dev)
    L.check(L.pidm_conv_wgrad(d, ptr(x0), ptr(x1), ptr(dyn), Cout, ptr(dw), ptr(db), ptr(ws), st))
    assert rel(dw, wr.grad) < 5e-6
    assert rel(db, br.grad) < 5e-6


@pytest.mark.parametrize("B,H,C0,C1,Cout,K,stride,pad,transposed", UNIT_CASES)
def test_circular_conv_forward_dgrad_wgrad(backend, B, H, C0, C1, Cout, K, stride, pad, transposed):
    _unit(backend, B, H, C0, C1, Cout, K, stride, pad, transposed)


@pytest.mark.parametrize("B,H,C0,C1,Cout,K,stride,pad,transposed", [UNIT_CASES[2], UNIT_CASES[3], UNIT_CASES[4]])
def test_circular_conv_with_the_split_forms_off(backend, monkeypatch, B, H, C0, C1, Cout, K, stride, pad, transposed):
    monkeypatch.setenv("PIDM_CONV_SPLIT", "0")
    monkeypatch.setenv("PIDM_WGRAD_SPLIT", "0")
    _unit(backend, B, H, C0, C1, Cout, K, stride, pad, transposed)


@pytest.mark.parametrize("B,H,C0,C1,Cout,K,stride,pad,transposed", [UNIT_CASES[2], UNIT_CASES[3]])
def test_circular_conv_on_the_plain_tile_kernels(backend, monkeypatch, B, H, C0, C1, Cout, K, stride, pad, transposed):
    """the streaming forward kernel and the row-staged weight gradient off: the pipelined tile kernels' wrap at the same shapes"""
    monkeypatch.setenv("PIDM_CONV_STREAM", "0")
    monkeypatch.setenv("PIDM_WGRAD_ROWST", "0")
    _unit(backend, B, H, C0, C1, Cout, K, stride, pad, transposed)


@pytest.mark.parametrize("B,H,C0,C1,Cout,K,stride,pad,transposed", [
    (1, 32, 32, 0, 32, 3, 1, 1, 0),      # one strip per row, strips of 4 rows: every strip's first / last input row is another strip's or the wrapped one
    (2, 64, 32, 32, 64, 3, 1, 1, 0),     # 64-wide rows (two strips per row: only the outer columns wrap), two sources, two n-tiles per wave
    (1, 32, 64, 0, 32, 3, 1, 1, 0),      # four 16-channel chunks
])
def test_circular_conv_row_streaming(backend, monkeypatch, capfd, B, H, C0, C1, Cout, K, stride, pad, transposed):
    """conv3x3_rs_kernel<..., WRAP> (the occupancy gate lowered as in tests/test_unet_config_sweep.py, so that one image is enough
    work for it) and the row-streaming weight gradient's wrapping family"""
    monkeypatch.setenv("PIDM_CONV_RS_WAVES", "4")
    monkeypatch.setenv("PIDM_CONV_RS_MINR", "4")
    monkeypatch.setenv("PIDM_TRACE_CONV", "1")
    _unit(backend, B, H, C0, C1, Cout, K, stride, pad, transposed)
    err = capfd.readouterr().err
    assert err.count("conv3x3_rs_kernel") == 2 and "conv_wgrad_rs_kernel" in err, err      # forward and input gradient; weight gradient


def test_circular_conv_groupnorm_partials(backend):
    """pidm_conv_forward_gn_partials with pad_mode = 1: the output is the circular convolution, and where the kernel that took it
    has the statistics epilogue the partial sums are those of that output"""
    L, dev = backend
    st = stream_ptr(dev)
    B, H, C, Cout, groups = 2, 16, 32, 64, 8
    g = torch.Generator().manual_seed(78)
    x = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(Cout, C, 3, 3, generator=g) * 0.1
    bias = torch.randn(Cout, generator=g)
    ref = circular_conv2d(x, w, bias, 1, 1)
    d = ConvDesc(B=B, Hi=H, Wi=H, C0=C, C1=0, ld0=C, ld1=0, Cout=Cout, KH=3, KW=3, stride=1, pad=1, transposed=0, out_nchw=0, ldo=Cout,
                 pad_mode=1)
    wp = torch.zeros(L.pidm_conv_packed_weight_floats(d), device=dev)
    wdev = w.to(dev)
    L.check(L.pidm_conv_pack_weights(d, ptr(wdev), ptr(wp), 0, st))
    out = torch.empty(B, H, H, Cout, device=dev)
    chunks_max = H * H // 32
    part = torch.full((B, chunks_max, groups, 2), float("nan"), dtype=torch.float64, device=dev)
    x0, bd = x.permute(0, 2, 3, 1).contiguous().to(dev), bias.to(dev)
    nch = L.lib.pidm_conv_forward_gn_partials(d, ptr(x0), None, ptr(wp), ptr(bd), ptr(out), groups, ptr(part), st)
    assert 0 <= nch <= chunks_max, L.lib.pidm_last_error().decode()
    assert rel(out.permute(0, 3, 1, 2), ref) < 5e-6
    if nch:
        cpg = Cout // groups
        rg = ref.double().reshape(B, groups, cpg, H * H)
        s1, s2 = rg.sum(dim=(2, 3)), (rg * rg).sum(dim=(2, 3))
        pc = part.cpu().reshape(-1)[:B * nch * groups * 2].reshape(B, nch, groups, 2)
        assert torch.isfinite(pc).all()
        assert (pc[..., 0].sum(dim=1) - s1).abs().max().item() < 1e-5 * s2.sqrt().max().item() * (H * H * cpg) ** 0.5
        assert rel(pc[..., 1].sum(dim=1), s2) < 2e-6


def test_conv_desc_refusals(backend):
    L, dev = backend
    d = ConvDesc(B=1, Hi=8, Wi=8, C0=8, C1=0, ld0=8, ld1=0, Cout=8, KH=3, KW=3, stride=1, pad=1, transposed=0, out_nchw=0, ldo=8, pad_mode=2)
    assert L.pidm_conv_packed_weight_floats(d) == 0
    assert "padding mode" in L.lib.pidm_last_error().decode()
    d = ConvDesc(B=1, Hi=2, Wi=2, C0=8, C1=0, ld0=8, ld1=0, Cout=8, KH=7, KW=7, stride=1, pad=3, transposed=0, out_nchw=0, ldo=8, pad_mode=1)
    assert L.pidm_conv_packed_weight_floats(d) == 0      # 3 wrapped taps on a 2-wide row: the reference's F.pad refuses it too
    assert "more than once" in L.lib.pidm_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------------------
# modes and contract
# ------------------------------------------------------------------------------------------------------------------------------
def test_inference_and_replay_equal_the_training_forward(backend):
    m = _model(backend, dim=8)
    dev = next(m.parameters()).device
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3, 256, 2, generator=gen).to(dev)
    t = torch.tensor([0, 50, 99]).to(dev)
    w = torch.randn(3, 2, 16, 16, generator=gen).to(dev)
    outs, grads = [], []
    for _ in range(3):                                    # the third call with the same key is a graph replay
        for prm in m.parameters():
            prm.grad = None
        out = m(x, t)
        (out * w).sum().backward()
        outs.append(out.detach().clone())
        grads.append(get_engine(m, 16, m._pidm_lib).flat_grad.clone())
    assert torch.equal(outs[2], outs[0]) and torch.equal(outs[1], outs[0])
    assert torch.equal(grads[2], grads[0]) and torch.equal(grads[1], grads[0])
    with torch.no_grad(), frozen_weights(m):
        inf = [m(x, t).clone() for _ in range(3)]
    for o in inf:
        assert rel(o, outs[0]) < 2 * FWD_TOL              # in-place inference GroupNorm: same arithmetic, other kernels
    assert torch.equal(inf[1], inf[0]) and torch.equal(inf[2], inf[0])


def test_state_dict_and_parameter_names(backend):
    g = np.load(G28)
    m = _model(backend, dim=8)
    assert list(m.state_dict().keys()) == [str(k) for k in g["keys"]]
    assert len(m.state_dict()) == 317
    z = Unet3D(dim=8)
    assert [k.replace(".3.conv_transpose.", ".3.") for k in m.state_dict()] == list(z.state_dict())
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(z.state_dict()[k.replace(".3.conv_transpose.", ".3.")].shape), k
    names = get_engine(m, 16, m._pidm_lib).names
    assert len(names) == 265 and sum(".3.conv_transpose." in k for k in names) == 6
    assert not any(k.startswith("ups.") and k.endswith((".3.weight", ".3.bias")) for k in names)


def test_unknown_padding_mode_raises():
    with pytest.raises(ValueError, match="Unknown padding mode: reflect"):
        Unet3D(dim=8, padding_mode="reflect")


def test_level_of_extent_one_raises(backend):
    m = _model(backend, dim=8)                            # four levels at 8x8: the bottom level is 1x1
    dev = next(m.parameters()).device
    with pytest.raises(PidmError, match="level 3"):
        m(torch.randn(2, 64, 2, device=dev), torch.tensor([1, 2], device=dev))


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from oracle import pidm_oracle as O
from physicsinformeddiffusionmodels_amd.unet_model import Unet3D
dev = torch.device(sys.argv[2])
lib = None
if dev.type == "cpu":
    from tests.emu_util import emu_lib
    lib = emu_lib()
def run(mode):
    m = Unet3D(dim=8, dim_mults=(1, 2), padding_mode=mode)
    m.load_state_dict(O.fill_state_dict(m.state_dict()))
    m = m.to(dev)
    m._pidm_lib = lib
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 256, 2, generator=g).to(dev)
    w = torch.randn(2, 2, 16, 16, generator=g).to(dev)
    out = m(x, torch.tensor([7, 70]).to(dev))
    (out * w).sum().backward()
    return out.detach().cpu(), torch.cat([p.grad.reshape(-1).cpu() for p in m.parameters() if p.grad is not None])
before = run("zeros")            # no circular model has existed in this process
circ = run("circular")
after = run("zeros")
assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]), "zero-padding results changed"
assert not torch.equal(before[0], circ[0])
print("zero-mode bit-identical")
"""


def test_zero_mode_is_untouched_by_a_circular_model_in_the_process(backend):
    """a fresh process (this is what the test is about): zero-mode output and gradients before any circular model existed in the
    process, and after one was built and run, are bit-identical"""
    _, dev = backend
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO, "cpu" if dev.type == "cpu" else "cuda:0"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "zero-mode bit-identical" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------------------------
# periodic training step
# ------------------------------------------------------------------------------------------------------------------------------
def test_periodic_training_step(backend):
    """One step of the circular dim-8 UNet on the periodic Darcy residual, after tests/test_darcy_general.py::
    test_training_step_through_the_general_residual: the loss equals the loss algebra (reference src/denoising_utils.py:677-684)
    restated in float64 from the step's own model_out and residual (1e-5 relative), the 259 used parameters get finite, non-zero
    gradients, and one fused clip + Adam step runs on the circular parameter layout."""
    lib, dev = _lib_of(backend)
    P, B = 16, 3
    m = _model(backend, dim=8)
    diff = DenoisingDiffusion(100, dev, lib=lib)
    res = ResidualsDarcy(model=m, fd_acc=2, pixels_per_dim=P, pixels_at_boundary=False, reverse_d1=True, device=dev, bcs="periodic",
                         domain_length=1., lib=lib)
    gen = torch.Generator().manual_seed(4)
    x0 = torch.randn(B, 2, P, P, generator=gen).to(dev)
    eps = torch.randn(B, 2, P, P, generator=gen).to(dev)
    t = torch.tensor([3, 50, 97]).to(dev)
    seen = {}
    inner = res.compute_residual

    def recording(*a, **k):
        out = inner(*a, **k)
        seen.update(out)
        return out
    res.compute_residual = recording
    opt = FusedClipAdam(m, lr=2e-3, max_norm=1.0, image_size=P, lib=lib)
    with patched_rng(randint=lambda *a, **k: t.clone(), randn_like=lambda *a, **k: eps.clone()):
        loss, data_l, res_l, ineq_l, opt_l = diff.model_estimation_loss(x0, residual_func=res, c_data=1., c_residual=1e-3,
                                                                        c_ineq=0., lambda_opt=0.)
    out, r = seen["model_out"].detach().double().cpu(), seen["residual"].detach().double().cpu()
    if out.dim() == 3:
        out = out.reshape(B, P, P, 2).permute(0, 3, 1, 2)
    tc = t.cpu()
    p2w, var = diff.diff_dict["p2_loss_weight"].double().cpu()[tc], diff.diff_dict["posterior_variance_clipped"].double().cpu()[tc]
    data64 = (((x0.double().cpu() - out) ** 2).reshape(B, -1).mean(dim=1) * p2w).mean()
    want = 1. * data64 + (1e-3 * 0.5 * r ** 2 / var.view(B, 1, 1)).mean()
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item()), (loss.item(), want.item())
    assert abs(data_l - data64.item()) <= 1e-5 * abs(data64.item())
    assert abs(res_l - r.abs().mean().item()) <= 1e-5 * r.abs().mean().item()
    loss.backward()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) == 259 and all(torch.isfinite(gr).all() for gr in grads)
    assert all(float(gr.abs().sum()) > 0. for gr in grads)
    before = torch.cat([p.detach().reshape(-1).cpu() for p in m.parameters()]).clone()
    norm = opt.step()
    assert torch.isfinite(norm).all() and float(norm) > 0.
    after = torch.cat([p.detach().reshape(-1).cpu() for p in m.parameters()])
    assert torch.isfinite(after).all() and not torch.equal(before, after)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU only: the Darcy model's shape
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_darcy_shape_on_the_gpu():
    """dim 32 at 64x64 with the default four levels, batch 2: parity with the restatement, equivariance at shift 8, one p_sample"""
    from physicsinformeddiffusionmodels_amd._lib import get_lib
    assert torch.cuda.is_available() and get_lib().backend == "hip"
    dev = torch.device("cuda:0")
    kw, P, B = dict(dim=32), 64, 2
    m = _model((get_lib(), dev), **kw)
    gen = torch.Generator().manual_seed(64)
    x = torch.randn(B, 2, P, P, generator=gen)
    w = torch.randn(B, 2, P, P, generator=gen)
    t = torch.tensor([5, 77])
    ref, p = _restated(m, x, t, w, kw)
    out, gx, grads = _evaluate(m, x.to(dev), t.to(dev), w.to(dev))
    assert rel(out, ref) < FWD_TOL
    _, gmax = _assert_gradients(m, p)
    out_s, gx_s, grads_s = _evaluate(m, torch.roll(x, (8, 8), (2, 3)).to(dev), t.to(dev), torch.roll(w, (8, 8), (2, 3)).to(dev))
    assert rel(out_s, torch.roll(out, (8, 8), (2, 3))) < 2 * FWD_TOL
    assert float((gx_s.double() - torch.roll(gx, (8, 8), (2, 3)).double()).norm()) <= 1e-3 * float(gx.double().norm()) + 2e-6 * gmax
    for k, gk in grads.items():
        assert float((grads_s[k].double() - gk.double()).norm()) <= 1e-3 * float(gk.double().norm()) + 2e-6 * gmax, k
    diff = DenoisingDiffusion(100, dev)
    res = ResidualsDarcy(model=m, fd_acc=2, pixels_per_dim=P, pixels_at_boundary=False, reverse_d1=True, device=dev, bcs="periodic",
                         domain_length=1.)
    with torch.no_grad():
        (nx, _), _ = diff.p_sample(x.to(dev), None, 57, save_output=False, surpress_noise=True, residual_func=res)
    assert tuple(nx.shape) == (B, 2, P, P) and torch.isfinite(nx).all()
