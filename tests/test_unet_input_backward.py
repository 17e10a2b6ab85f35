"""pidm_unet_backward_input / UnetEngine.backward_input / input_gradient_pass: the input-gradient chain of the UNet backward alone.
Its grad_x is bit-identical to pidm_unet_backward's (same kernels, same arguments, same arena layout), it computes no weight
gradient, and it leaves no trace in the model's gradient state.  `backend` = host emulator or the gfx950 library (-m gpu)."""
import ctypes as C

import pytest
import torch

from oracle import pidm_oracle as O
from physicsinformeddiffusionmodels_amd._engine import GUIDE_SLOT, get_engine
from physicsinformeddiffusionmodels_amd._lib import PidmError
from physicsinformeddiffusionmodels_amd.unet_model import Unet3D, input_gradient_pass


def _counts(L):
    a = (C.c_longlong * 4)()
    L.check(L.pidm_debug_launch_counts(a))
    return {"eager": a[0], "graph_launches": a[1], "graph_kernels": a[2], "captures": a[3]}


def _model(L, dev, dim=8, **kw):
    m = Unet3D(dim=dim, channels=2, **kw)
    m.load_state_dict(O.fill_state_dict(m.state_dict()))
    m = m.to(dev)
    m._pidm_lib = L if dev.type == "cpu" else None
    return m


def _inputs(dev, B, P, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, P * P, 2, generator=g).to(dev)
    t = torch.randint(0, 100, (B,), generator=g).to(dev)
    w = torch.randn(B, 2, P, P, generator=g).to(dev)
    return x, t, w


def _input_only_equals_full(L, dev, dim, P, B, **kw):
    m = _model(L, dev, dim, **kw)
    x, t, w = _inputs(dev, B, P)
    eng = get_engine(m, P, m._pidm_lib)
    out = eng.forward(x, t, training=True)
    gx_full = eng.backward(w, True, 2).clone()
    assert torch.isfinite(gx_full).all() and gx_full.abs().max().item() > 0
    # the same tape, the full pass behind it: the tape is read-only for both
    assert torch.equal(eng.backward_input(w), gx_full)
    # three passes with a forward each: launch by launch, captured on the second sighting, replayed
    c0 = _counts(eng.lib)
    for rep in range(3):
        out2 = eng.forward(x, t, training=True)
        gx = eng.backward_input(w)
        assert torch.equal(out2, out), rep
        assert torch.equal(gx, gx_full), rep
    c1 = _counts(eng.lib)
    assert c1["captures"] - c0["captures"] >= 1 and c1["graph_launches"] - c0["graph_launches"] >= 2
    # ... and the full pass still finds its own graph entries and results afterwards
    eng.forward(x, t, training=True)
    assert torch.equal(eng.backward(w, True, 2), gx_full)


@pytest.mark.parametrize("padding_mode", ["zeros", "circular"])
def test_input_only_grad_x_is_bit_identical_to_full_backward(backend, padding_mode):
    L, dev = backend
    _input_only_equals_full(L, dev, 8, 16, 3, padding_mode=padding_mode)


@pytest.mark.gpu
def test_input_only_grad_x_is_bit_identical_dim32_p64_gpu():
    """The flagship shape: the row-streaming and split convolution kernels run with their GroupNorm-sum epilogues, so an input-only
    pass that changed an epilogue decision (or the arena the sums go through) would differ here."""
    from physicsinformeddiffusionmodels_amd._lib import get_lib
    _input_only_equals_full(get_lib(), torch.device("cuda:0"), 32, 64, 2)


def _train_step(m, x, t, w, between=None):
    for p in m.parameters():
        p.grad = None
    xr = x.clone().requires_grad_(True)
    out = m(xr, t)
    if between is not None:
        between()
    (out * w).sum().backward()
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, xr.grad.clone()


def test_input_only_pass_leaves_no_trace(backend):
    L, dev = backend
    P, B = 16, 3
    m = _model(L, dev)
    x, t, w = _inputs(dev, B, P)
    x2, t2, w2 = _inputs(dev, B, P, seed=6)
    A, gxA = _train_step(m, x, t, w)
    assert len(A) > 100
    eng = get_engine(m, P, m._pidm_lib)
    flat_A = eng.flat_grad.clone()
    with torch.no_grad():
        x0p, pull = input_gradient_pass(m, x2, t2)
        g = pull(w2)
    assert g.shape == (B, P * P, 2) and x0p.shape == (B, 2, P, P) and not g.requires_grad
    assert torch.equal(eng.flat_grad, flat_A)
    for k, p in m.named_parameters():
        if k in A:
            assert torch.equal(p.grad, A[k]), k
        else:
            assert p.grad is None, k
    geng = get_engine(m, P, m._pidm_lib, GUIDE_SLOT)
    assert geng is not eng and geng.flat_grad is None          # runs without any gradient buffer bound
    # the pass agrees with autograd through the ordinary engine path
    _, gx2 = _train_step(m, x2, t2, w2)
    assert torch.equal(g, gx2)
    # a second identical training step, this time with an input-only pass BETWEEN its forward and its backward (pending tape)
    def between():
        with torch.no_grad():
            _, pl = input_gradient_pass(m, x2, t2)
            assert torch.equal(pl(w2), g)
    A2, gxA2 = _train_step(m, x, t, w, between)
    assert A2.keys() == A.keys() and torch.equal(gxA2, gxA)
    for k in A:
        assert torch.equal(A2[k], A[k]), k


def test_input_only_pass_on_a_fresh_model_creates_no_gradients(backend):
    L, dev = backend
    m = _model(L, dev)
    x, t, w = _inputs(dev, 2, 16)
    x0p, pull = input_gradient_pass(m, x.reshape(2, 16, 16, 2).permute(0, 3, 1, 2), t)      # NCHW input form
    g = pull(w)
    assert torch.isfinite(g).all() and g.abs().max().item() > 0
    assert all(p.grad is None for p in m.parameters())
    assert all(e.flat_grad is None for e in m._engines.values())
    _, pull_b = input_gradient_pass(m, x, t)
    with pytest.raises(PidmError, match="earlier pass"):
        pull(w)
    assert torch.equal(pull_b(w), g)


def test_input_only_pass_enqueues_fewer_kernels(backend):
    L, dev = backend
    m = _model(L, dev)
    x, t, w = _inputs(dev, 3, 16)
    eng = get_engine(m, 16, m._pidm_lib)
    n = {}
    for kind in ("full", "input"):
        eng.forward(x, t, training=True)
        c0 = _counts(eng.lib)
        eng.backward(w, True, 2) if kind == "full" else eng.backward_input(w)
        c1 = _counts(eng.lib)
        n[kind] = (c1["eager"] - c0["eager"]) + (c1["graph_kernels"] - c0["graph_kernels"])
    assert 0 < n["input"] < n["full"], n


def test_input_only_errors(backend):
    L, dev = backend
    m = _model(L, dev)
    x, t, w = _inputs(dev, 2, 16)
    with pytest.raises(PidmError, match="cond"):
        input_gradient_pass(m, x, t, cond=torch.zeros_like(x))
    with pytest.raises(PidmError, match="multi-frame"):
        input_gradient_pass(m, torch.zeros(2, 2, 1, 16, 16, device=dev), t)
    msc = _model(L, dev, self_condition=True)
    with pytest.raises(PidmError, match="self-conditioning"):
        input_gradient_pass(msc, x, t)
    eng = get_engine(m, 16, m._pidm_lib)
    lib = eng.lib
    eng.forward(x, t, training=True)
    ws = eng.workspace
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    gx = torch.empty(2, 256, 2, device=dev)
    vp = C.c_void_p
    args = lambda **k: [k.get("h", eng.handle), vp(k.get("go", w.data_ptr())), vp(k.get("gx", gx.data_ptr())), k.get("B", 2), vp(base),
                        ws.numel() - 256, vp(0)]
    for bad, msg in ((dict(h=None), b"null"), (dict(go=0), b"null"), (dict(gx=0), b"null"), (dict(B=0), b"positive"),
                     (dict(B=-1), b"positive"), (dict(B=3), b"no matching forward")):
        assert lib.pidm_unet_backward_input(*args(**bad)) != 0
        assert msg in lib.pidm_last_error(), (bad, lib.pidm_last_error())
