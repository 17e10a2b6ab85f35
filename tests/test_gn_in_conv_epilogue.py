"""GroupNorm finished inside the 3x3 convolution workgroup (csrc/k_conv.hip: conv3x3_split_kernel / conv3x3_split_ws_kernel with FZ = 1 / 2,
csrc/k_conv_epilogue.h: pidm_fz_*; PIDM_NO_GN_FUSED=1 restores the separate gn_apply / gn_bwd_apply launches).

The smallest model that reaches it is Unet3D(dim=32, dim_mults=(1, 2, 4)) at 32 x 32: an 8 x 8 level with 128 channels (16 per group,
two images per 128-pixel tile) and a 16 x 16 level with 64 channels (8 per group) whose images fill the 256-pixel tile - taken at these
batch sizes only with PIDM_SPLIT_NW=8; the default 128-pixel tile holds half an image there and must stay as it was.  Batch 1 leaves
the second image of the 8 x 8 tile empty, an odd batch the second image of the last tile.

The fused epilogues repeat the additions of gn_finalize_stats / gn_bwd_apply_kernel term by term (float sums per wave, doubles
across waves, the same interleaved runs) and spell out the multiply-add pairs the compiler fuses in the separate kernels, so every
output is BIT-identical to the unfused pass - on the host emulator (built without FMA contraction) and on the GPU.  The float64
criterion of the half block (err_fused <= 1.5 err_unfused + 1e-7 max|ref| per output tensor) and the oracle tolerances of
tests/test_unet_engine.py are checked as well.
`backend` = host emulator or the gfx950 library (-m gpu)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import pidm_oracle as O
from physicsinformeddiffusionmodels_amd._engine import get_engine
from physicsinformeddiffusionmodels_amd._lib import reload_knobs
from physicsinformeddiffusionmodels_amd.unet_model import Unet3D, input_gradient_pass

MULTS = (1, 2, 4)
KNOBS = ("PIDM_NO_GN_FUSED", "PIDM_SPLIT_NW")


def _counts(L):
    a = (C.c_longlong * 4)()
    L.check(L.pidm_debug_launch_counts(a))
    return a[0] + a[2]          # kernels enqueued one by one + kernels inside replayed graphs


def _model(L, dev, dim=32, dim_mults=MULTS, **kw):
    m = Unet3D(dim=dim, dim_mults=dim_mults, channels=2, **kw)
    sd = O.fill_state_dict(m.state_dict())
    m.load_state_dict(sd)
    m = m.to(dev)
    m._pidm_lib = L if dev.type == "cpu" else None
    return m, sd


def _inputs(dev, B, P, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, P * P, 2, generator=g)
    t = torch.randint(0, 100, (B,), generator=g)
    w = torch.randn(B, 2, P, P, generator=g)
    return x.to(dev), t.to(dev), w.to(dev)


def _set(monkeypatch, fused, nw=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if not fused:
        monkeypatch.setenv("PIDM_NO_GN_FUSED", "1")
    if nw:
        monkeypatch.setenv("PIDM_SPLIT_NW", nw)


def _step(m, x, t, w):
    """training forward + backward through autograd: output, input gradient, every parameter gradient, kernels enqueued"""
    L = get_engine(m, int(round(x.shape[1] ** 0.5)), m._pidm_lib).lib
    for p in m.parameters():
        p.grad = None
    xr = x.clone().requires_grad_(True)
    c0 = _counts(L)
    out = m(xr, t)
    (out * w).sum().backward()
    n = _counts(L) - c0
    return {"out": out.detach().clone(), "gx": xr.grad.clone(), "n": n,
            "grads": {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}}


_PASSES = {}       # (backend, batch, tile, fused) -> _step result of a fresh model: computed once, shared, never modified
_ORACLE = {}       # (batch, dtype) -> oracle autograd on the CPU


def _pass(backend, monkeypatch, B, nw, fused, P=32):
    L, dev = backend
    key = (dev.type, B, nw, fused, P)
    if key not in _PASSES:
        _set(monkeypatch, fused, nw)
        m, _ = _model(L, dev) if P == 32 else _model(L, dev, 32, (1, 2, 4, 8))
        _PASSES[key] = _step(m, *_inputs(dev, B, P))
    return _PASSES[key]


def _time_embedding64(p, t, dim):
    """O.time_embedding in the dtype of the parameters (the oracle's builds its sinusoids in float32 whatever they are)"""
    dt = p["time_mlp.1.weight"].dtype
    half = dim // 2
    freqs = torch.exp(torch.arange(half, dtype=dt) * -(math.log(10000) / (half - 1)))
    emb = t.to(dt)[:, None] * freqs[None, :]
    emb = torch.cat((emb.sin(), emb.cos()), dim=-1)
    h = F.gelu(F.linear(emb, p["time_mlp.1.weight"], p["time_mlp.1.bias"]))
    return F.linear(h, p["time_mlp.3.weight"], p["time_mlp.3.bias"])


def _oracle(B, dtype, P=32):
    """the oracle's UNet (conv -> GroupNorm -> FiLM -> SiLU ... in torch) and its autograd, in float32 or restated in float64"""
    key = (B, dtype, P)
    if key not in _ORACLE:
        mults = MULTS if P == 32 else (1, 2, 4, 8)
        m = Unet3D(dim=32, dim_mults=mults, channels=2)
        sd = O.fill_state_dict(m.state_dict())
        p = {k: v.clone().to(dtype).requires_grad_(True) if v.dtype.is_floating_point else v.clone() for k, v in sd.items()}
        x, t, w = _inputs(torch.device("cpu"), B, P)
        xr = x.to(dtype).requires_grad_(True)
        keep = O.time_embedding
        try:
            if dtype == torch.float64:
                O.time_embedding = _time_embedding64
            out = O.unet_forward(p, xr, t, O.UnetCfg(dim=32, channels=2, dim_mults=mults))
        finally:
            O.time_embedding = keep
        (out * w.to(dtype)).sum().backward()
        _ORACLE[key] = {"out": out.detach(), "gx": xr.grad, "grads": {k: v.grad for k, v in p.items() if getattr(v, "grad", None) is not None}}
    return _ORACLE[key]


def _tensors(r):
    yield "out", r["out"]
    yield "gx", r["gx"]
    for k in sorted(r["grads"]):
        yield "grad " + k, r["grads"][k]


def _all_equal(a, b, what):
    assert a["grads"].keys() == b["grads"].keys(), what
    bad = [k for (k, u), (_, v) in zip(_tensors(a), _tensors(b)) if not torch.equal(u, v)]
    assert not bad, (what, bad[:8])


def _float64_bound(fused, unfused, ref, what):
    """err_fused <= 1.5 err_unfused + 1e-7 max|ref| for the output, the input gradient and every parameter gradient"""
    assert fused["grads"].keys() == unfused["grads"].keys() == ref["grads"].keys(), what
    worst, bad, ratios = (0.0, None), [], []
    for (k, f), (_, u), (_, r) in zip(_tensors(fused), _tensors(unfused), _tensors(ref)):
        r = r.reshape(f.shape)
        ef = (f.double().cpu() - r).abs().max().item()
        eu = (u.double().cpu() - r).abs().max().item()
        mx = r.abs().max().item()
        ratios.append(ef / max(eu, 1e-300))
        if ef / max(mx, 1e-300) > worst[0]:
            worst = (ef / max(mx, 1e-300), f"{k}: err_fused {ef:.3e} err_unfused {eu:.3e} max|ref| {mx:.3e}")
        if not ef <= 1.5 * eu + 1e-7 * mx:
            bad.append(f"{k}: err_fused {ef:.3e} > 1.5 x err_unfused {eu:.3e} + 1e-7 x max|ref| {mx:.3e}")
    print(f"[gn_in_conv_epilogue] {what}: largest err_fused / max|ref| = {worst[0]:.3e} ({worst[1]}); "
          f"{len(bad)} of {len(ratios)} tensors beyond the bound, err_fused > err_unfused in {sum(q > 1 for q in ratios)}, "
          f"< in {sum(q < 1 for q in ratios)}, ratio min / median / max {min(ratios):.2f} / {sorted(ratios)[len(ratios) // 2]:.2f} / {max(ratios):.2f}")
    assert not bad, (what, bad[:8])


def _fused_groupnorms(levels):
    """launches a fused pass saves: per ResnetBlock of an eligible level GroupNorm 1 forward and backward, and GroupNorm 2 forward of the
    blocks not followed by an attention block (one of every pair; the other's gn_apply carries the LayerNorm).  levels: (blocks, ...)"""
    return sum(2 * nb + nb // 2 for nb in levels)


LOWEST = 6     # ResnetBlocks of the lowest level: two down, two mid, two up
MIDDLE = 4     # of a level in between: two down, two up


@pytest.mark.parametrize("nw", [None, "8"])
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_fused_against_unfused(backend, monkeypatch, B, nw):
    """Training forward output, input gradient and every parameter gradient, fused against PIDM_NO_GN_FUSED=1: the same bits
    on both backends.  The fused pass enqueues exactly one kernel less per eligible
    GroupNorm: the 8 x 8 level always, the 16 x 16 level only on the whole-image 256-pixel tile."""
    fused, unfused = _pass(backend, monkeypatch, B, nw, True), _pass(backend, monkeypatch, B, nw, False)
    assert torch.isfinite(fused["out"]).all() and fused["gx"].abs().max().item() > 0 and len(fused["grads"]) > 100
    _all_equal(fused, unfused, (B, nw))
    assert unfused["n"] - fused["n"] == _fused_groupnorms((LOWEST, MIDDLE) if nw else (LOWEST,)), (fused["n"], unfused["n"])


@pytest.mark.parametrize("nw", [None, "8"])
@pytest.mark.parametrize("B", [2, 5])
def test_fused_against_oracle_autograd(backend, monkeypatch, B, nw):
    """The fused pass against the oracle's float32 autograd with the tolerances of tests/test_unet_engine.py (output 3e-5 of its
    maximum, gradient norms 5e-4 + 2e-6 of the largest, gradients 1e-3 of their maximum)."""
    _against_oracle(_pass(backend, monkeypatch, B, nw, True), _oracle(B, torch.float32))


def _against_oracle(got, ref):
    rel = lambda a, b: (a.double().cpu() - b.double().reshape(a.shape)).abs().max().item() / max(b.abs().max().item(), 1e-30)  # noqa: E731
    assert rel(got["out"], ref["out"]) < 3e-5
    assert rel(got["gx"], ref["gx"]) < 1e-3
    assert got["grads"].keys() == ref["grads"].keys()
    gmax = max(v.double().norm().item() for v in ref["grads"].values())
    bad = []
    for k, r in ref["grads"].items():
        a, b = got["grads"][k].double().norm().item(), r.double().norm().item()
        if not abs(a - b) <= 5e-4 * b + 2e-6 * gmax or not rel(got["grads"][k], r) < 1e-3:
            bad.append((k, a, b, rel(got["grads"][k], r)))
    assert not bad, bad[:8]


def test_launch_accounting_replay_and_determinism(backend, monkeypatch):
    """Three passes of one engine (launch by launch, captured on the second sighting, replayed) give the same bits and every one
    enqueues the same number of kernels; a second model repeats every gradient bit for bit; the knob flipped on the LIVE handle (it is
    part of the hipGraph key and of the workspace-plan signature) switches to the unfused launches and back."""
    L, dev = backend
    B, P = 2, 32
    first = _pass(backend, monkeypatch, B, "8", True)          # (another model's pass: run to run)
    _set(monkeypatch, True, "8")
    m, _ = _model(L, dev)
    x, t, w = _inputs(dev, B, P)
    steps = [_step(m, x, t, w) for rep in range(3)]
    for rep, s in enumerate(steps):
        _all_equal(first, s, f"pass {rep} of a second model")
        assert s["n"] == first["n"], [s["n"] for s in steps]
    # the knob on the live handle: unfused launches (more kernels, the same bits), then fused again
    monkeypatch.setenv("PIDM_NO_GN_FUSED", "1")
    off = _step(m, x, t, w)
    assert off["n"] - first["n"] == _fused_groupnorms((LOWEST, MIDDLE)), (first["n"], off["n"])
    _all_equal(off, _pass(backend, monkeypatch, B, "8", False), "knob off on a live handle")
    _set(monkeypatch, True, "8")
    _all_equal(first, _step(m, x, t, w), "knob back on")


@pytest.mark.parametrize("case", ["half_image_tile", "dim8", "circular"])
def test_ineligible_shapes_keep_their_launches(backend, monkeypatch, case):
    """Where the split kernels' tile holds no whole image (dim 8 with the default four levels at 16 x 16: its only 32-channel split
    convolutions run on 4 x 4 images, 16 pixels) and with circular padding (those levels never reach the LDS-staged kernels) the
    knob changes nothing: the same kernels, the same bits.  The 128-pixel tile at 16 x 16 (half an image) sits in a model whose 8 x 8
    level IS fused (the engine takes no model that ends at 16 x 16): there every GroupNorm of the 16 x 16 level is still a launch
    of its own - the launches saved are the lowest level's alone - and an unfused launch is the kernel and the arguments of the
    knob-off pass; the bits of the whole pass are compared too."""
    L, dev = backend
    if case == "half_image_tile":
        fused, unfused = _pass(backend, monkeypatch, 2, None, True), _pass(backend, monkeypatch, 2, None, False)
        assert unfused["n"] - fused["n"] == _fused_groupnorms((LOWEST,))
        _all_equal(fused, unfused, case)
        return
    kw, P = {"dim8": (dict(dim=8, dim_mults=(1, 2, 4, 8)), 16), "circular": (dict(dim=32, dim_mults=MULTS, padding_mode="circular"), 32)}[case]
    x, t, w = _inputs(dev, 2, P)
    r = {}
    for fused in (True, False):
        _set(monkeypatch, fused)
        m, _ = _model(L, dev, **kw)
        r[fused] = _step(m, x, t, w)
    assert r[True]["n"] == r[False]["n"]
    _all_equal(r[True], r[False], case)


def test_input_only_and_inference_passes_are_eligible(backend, monkeypatch):
    """Run::input_only (guided sampling) takes the fused backward epilogue like the full pass - its input gradient is bit-identical to
    the full backward's and it saves the GroupNorm-1 backward launches - and an inference forward (GroupNorm in place) takes the fused
    forward epilogues: the same bits as unfused."""
    L, dev = backend
    B, P = 2, 32
    x, t, w = _inputs(dev, B, P)
    r = {}
    for fused in (True, False):
        _set(monkeypatch, fused)
        m, _ = _model(L, dev)
        eng = get_engine(m, P, m._pidm_lib)
        eng.forward(x, t, training=True)
        gx_full = eng.backward(w, True, 2).clone()
        eng.forward(x, t, training=True)
        c0 = _counts(eng.lib)
        gx_in = eng.backward_input(w).clone()
        n_in = _counts(eng.lib) - c0
        assert torch.equal(gx_in, gx_full), fused
        with torch.no_grad():
            c0 = _counts(eng.lib)
            y = eng.forward(x, t, training=False).clone()
            n_inf = _counts(eng.lib) - c0
            x0p, pull = input_gradient_pass(m, x, t)
            assert torch.equal(pull(w), gx_full), fused
        r[fused] = (gx_in, n_in, y, n_inf)
    assert r[False][1] - r[True][1] == LOWEST                           # GroupNorm 1 backward of every block of the 8 x 8 level
    assert r[False][3] - r[True][3] == LOWEST + LOWEST // 2             # GroupNorm 1 forward, GroupNorm 2 where no LayerNorm rides
    assert torch.equal(r[True][0], r[False][0]) and torch.equal(r[True][2], r[False][2])


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [None, "8"])
def test_flagship_small_levels_dim32_p64_gpu(monkeypatch, nw):
    """The flagship's own 16 x 16 (128 channels) and 8 x 8 (256 channels, 32 per group) levels, batch 2: fused against unfused within the
    float64 criterion, and against the oracle's autograd.  (At batch 2 the 16 x 16 level takes the whole-image tile only when forced.)
"""
    from physicsinformeddiffusionmodels_amd._lib import get_lib
    backend = (get_lib(), torch.device("cuda:0"))
    fused, unfused = _pass(backend, monkeypatch, 2, nw, True, P=64), _pass(backend, monkeypatch, 2, nw, False, P=64)
    assert unfused["n"] - fused["n"] == _fused_groupnorms((LOWEST, MIDDLE) if nw else (LOWEST,)), (fused["n"], unfused["n"])
    _against_oracle(fused, _oracle(2, torch.float32, P=64))
    _float64_bound(fused, unfused, _oracle(2, torch.float64, P=64), f"dim 32, 64 x 64, batch 2, tile {nw or 'default'}")


# ---- one ResnetBlock half on its own: conv -> GroupNorm -> FiLM -> SiLU and its backward against float64 -------------------------
def _block(backend, monkeypatch, H, Cc, B, nw, fused, film):
    """pidm_conv_gn_forward / pidm_conv_dgrad_gn_backward (the launches of resblock_fwd / resblock_bwd for one GroupNorm) on random
    data: (what the launches returned, their outputs on the CPU, the inputs)"""
    from physicsinformeddiffusionmodels_amd._lib import ConvDesc, ptr, stream_ptr
    L, dev = backend
    _set(monkeypatch, fused, nw)
    st, G = stream_ptr(dev), 8
    g = torch.Generator().manual_seed(100 * H + B)
    rn = lambda *sh, k=1.0: (torch.randn(*sh, generator=g) * k)  # noqa: E731
    i = {"x": rn(B, H, H, Cc), "w1": rn(Cc, Cc, 3, 3, k=0.05), "b1": rn(Cc), "gamma": 1 + rn(Cc, k=0.2), "beta": rn(Cc, k=0.2),
         "ss": rn(B, 2 * Cc, k=0.3), "ssb": rn(2 * Cc, k=0.1), "w2": rn(Cc, Cc, 3, 3, k=0.05), "g_c": rn(B, H, H, Cc), "res": rn(B, H, H, Cc)}
    t = {k: v.to(dev) for k, v in i.items()}
    d = ConvDesc(B=B, Hi=H, Wi=H, C0=Cc, C1=0, ld0=Cc, ld1=0, Cout=Cc, KH=3, KW=3, stride=1, pad=1, transposed=0, out_nchw=0, ldo=Cc)
    wp = torch.zeros(L.pidm_conv_packed_weight_floats(d), device=dev)
    L.check(L.pidm_conv_pack_weights(d, ptr(t["w1"]), ptr(wp), 0, st))
    wd = torch.zeros(L.pidm_conv_dgrad_packed_weight_floats(d), device=dev)
    L.check(L.pidm_conv_pack_weights(d, ptr(t["w2"]), ptr(wd), 1, st))
    ws = torch.zeros(B * (H * H // 32) * Cc * 4 + B * 2 * Cc + 64, device=dev)
    o = {"a": torch.zeros(B, H, H, Cc, device=dev), "y": torch.zeros(B, H, H, Cc, device=dev), "stats": torch.zeros(B, G, 2, device=dev),
         "dx": torch.zeros(B, H, H, Cc, device=dev), "dss": torch.zeros(B, 2 * Cc, device=dev), "dgb": torch.zeros(B, 2, Cc, device=dev)}
    dy = torch.zeros(B, H, H, Cc, device=dev)
    ss, ssb, res = (ptr(t["ss"]), ptr(t["ssb"]), None) if film else (None, None, ptr(t["res"]))
    rf = L.lib.pidm_conv_gn_forward(C.byref(d), ptr(t["x"]), None, ptr(wp), ptr(t["b1"]), G, ptr(t["gamma"]), ptr(t["beta"]), ss, ssb, 2 * Cc,
                                    res, ptr(o["a"]), ptr(o["y"]), ptr(o["stats"]), ptr(ws), st)
    rb = L.lib.pidm_conv_dgrad_gn_backward(C.byref(d), ptr(t["g_c"]), ptr(wd), ptr(o["a"]), ptr(o["stats"]), G, ptr(t["gamma"]), ptr(t["beta"]),
                                           ss, ssb, 2 * Cc, ptr(o["dss"]) if film else None, ptr(o["dgb"]), ptr(dy), ptr(o["dx"]), ptr(ws), st)
    assert rf >= 0 and rb >= 0, L.lib.pidm_last_error().decode()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return (rf, rb), {k: v.cpu() for k, v in o.items()}, i


def _block_float64(i, a, film, G=8):
    """the same half block in float64 with torch; its backward starts from the float32 convolution output `a` both paths share"""
    D = {k: v.double() for k, v in i.items()}
    nchw = lambda v: v.permute(0, 3, 1, 2)  # noqa: E731
    B, Cc = D["x"].shape[0], D["x"].shape[3]

    def act(a64, gamma_b, beta_b, scale, shift):
        h = F.group_norm(a64, G, eps=1e-5) * gamma_b[:, :, None, None] + beta_b[:, :, None, None]
        return F.silu(h * (1 + scale[:, :, None, None]) + shift[:, :, None, None])
    zero = torch.zeros(B, Cc, dtype=torch.float64)
    scale = (D["ss"][:, :Cc] + D["ssb"][:Cc]) if film else zero
    shift = (D["ss"][:, Cc:] + D["ssb"][Cc:]) if film else zero
    a64 = F.conv2d(nchw(D["x"]), D["w1"], D["b1"], padding=1)
    y = act(a64, D["gamma"].expand(B, Cc), D["beta"].expand(B, Cc), scale, shift) + (0 if film else nchw(D["res"]))
    ag = a64.reshape(B, G, -1)
    mean, var = ag.mean(dim=2), ag.var(dim=2, unbiased=False)
    ref = {"y": y.permute(0, 2, 3, 1), "stats": torch.stack((mean, 1 / torch.sqrt(var + 1e-5)), dim=2)}
    leaves = [nchw(a.double()).clone(), D["gamma"].expand(B, Cc).clone(), D["beta"].expand(B, Cc).clone(), scale.clone(), shift.clone()]
    for v in leaves:
        v.requires_grad_(True)
    (F.conv2d(act(*leaves), D["w2"], padding=1) * nchw(D["g_c"])).sum().backward()
    ref["dx"] = leaves[0].grad.permute(0, 2, 3, 1)
    ref["dgb"] = torch.stack((leaves[1].grad, leaves[2].grad), dim=1)
    if film:
        ref["dss"] = torch.cat((leaves[3].grad, leaves[4].grad), dim=1)
    return ref


BLOCKS = {"8x8": (8, 128, None, True), "16x16_whole_image_tile": (16, 64, "8", True), "16x16_half_image_tile": (16, 64, None, False),
          "flagship_8x8": (8, 256, None, True), "flagship_16x16": (16, 128, "8", True)}


@pytest.mark.parametrize("film", [True, False], ids=["film", "residual"])
@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("shape", sorted(BLOCKS))
def test_block_against_float64(backend, monkeypatch, shape, B, film):
    """conv -> GroupNorm -> FiLM -> SiLU (or GroupNorm -> SiLU -> + residual, the form of GroupNorm 2) and the GroupNorm's backward behind
    the next convolution's input gradient, fused against unfused against float64: err_fused <= 1.5 err_unfused + 1e-7 max|ref| for y,
    the statistics, dx and the per-image dgamma / dbeta / FiLM rows; the same bits on both backends.  An eligible launch reports that it
    finished the GroupNorm; the half-image tile at 16 x 16 does not and leaves the bits of the knob-off pass on both backends."""
    H, Cc, nw, eligible = BLOCKS[shape]
    rcf, fused, i = _block(backend, monkeypatch, H, Cc, B, nw, True, film)
    rcu, unfused, _ = _block(backend, monkeypatch, H, Cc, B, nw, False, film)
    assert rcf == ((1, 1) if eligible else (0, 0)) and rcu == (0, 0), (rcf, rcu)
    assert torch.equal(fused["a"], unfused["a"])
    ref = _block_float64(i, fused["a"], film)
    # (both backends: the fused epilogues spell out the fused multiply-adds of the separate kernels)
    assert all(torch.equal(fused[k], unfused[k]) for k in fused), [k for k in fused if not torch.equal(fused[k], unfused[k])]
    bad, line = [], []
    for k in sorted(ref):
        ef, eu = (fused[k].double() - ref[k]).abs().max().item(), (unfused[k].double() - ref[k]).abs().max().item()
        mx = ref[k].abs().max().item()
        line.append(f"{k} {ef:.2e} / {eu:.2e} / {mx:.2e}")
        assert eu <= 2e-4 * mx, (k, eu, mx)                         # (the unfused path itself is sound on this shape)
        if not ef <= 1.5 * eu + 1e-7 * mx:
            bad.append(line[-1])
    print(f"[gn_in_conv_epilogue] block {shape} batch {B} {'film' if film else 'residual'} ({backend[1].type}): "
          f"err_fused / err_unfused / max|ref|: " + "; ".join(line))
    assert not bad, bad
