"""Float64 parity of the Darcy kernels (csrc/k_darcy.hip) across band plans, sizes, geometries and kernel variants: residual
forward, adjoint, fused loss, Jacobian maximum, the PIDM_DARCY_ROWS knob and the argument guards.  The reference is
tests/darcy_ref.py (plain torch), evaluated in float64 on the fp32 inputs the kernels see.

Tolerance rule (that of test_kernels_mech_f64.py).  For a compared tensor q:  err(q) = max|q - q64| / max|q64|.  A kernel passes when
    err(kernel) <= 4 * err(ref32) + 4 * 2^-23,
where ref32 is the SAME reference evaluated in float32 by torch on the CPU inside the test: the bound is what fp32 arithmetic costs
the reference, never what the code under test returns.  The factor 4 covers another summation order and fma contraction, the four
ulp cover quantities the fp32 reference happens to hit exactly.  Scalars (the loss figures, the Jacobian maximum of one sample)
use the same rule on their relative error.

Every plan case asserts the number of row bands the launch planner gives it (pidm_darcy_loss_ws == B * nb * 32 bytes), so a change
of the planner cannot turn these cases into repeats of one plan.  Where k_darcy.hip promises the same taps in the same order - one
sample alone against the same sample in a batch, two runs, every kernel variant at P = 64, the one-pixel kernel an unaligned
buffer falls back to, every PIDM_DARCY_ROWS - residual, adjoint and loss gradient are compared with torch.equal.  The loss SCALARS
of two different kernels group the same doubles differently (per band, per sample), so between kernels they follow the float64
rule; two runs of one plan give the same scalars bit for bit.

Worst err(kernel) / err(ref32) per quantity over the cases of this module - the pair that uses the largest share of its bound, the
share in brackets (every test prints its figures before it asserts):

    quantity                  emulator                      MI355X
    residual                  1.6e-07 / 6.9e-08 (0.21)      1.6e-07 / 6.9e-08 (0.21)      P = 5, one band
    adjoint                   1.8e-07 / 1.1e-07 (0.19)      1.8e-07 / 1.1e-07 (0.19)      (21, 256), bands of 6 rows
    fused loss: loss          1.1e-07 / 1.2e-08 (0.20)      9.1e-08 / 1.9e-08 (0.17)      (12, 2) / (5, 1)
    fused loss: c_data * data 7.8e-08 / 1.3e-08 (0.15)      7.7e-08 / 1.3e-08 (0.15)      (21, 256)
    fused loss: mean |r|      4.9e-08 / 4.4e-08 (0.07)      4.9e-08 / 4.4e-08 (0.07)      (8, 2)
    fused loss: grad          2.7e-07 / 1.5e-07 (0.25)      2.1e-07 / 1.1e-07 (0.23)      P = 10, inv_h = (15, -7) / (15, 22)
    jacobian max              5.4e-08 / 5.4e-08 (0.08)      5.4e-08 / 5.4e-08 (0.08)      P = 5, sample 0

No quantity uses more than a quarter of its bound on either back end: neither the factor 4 nor the four ulp is tight anywhere,
and every torch.equal of this module holds on the gfx950 build (fma contraction on) as on the emulator (contraction off).
"""
import functools

import numpy as np
import pytest
import torch

from physicsinformeddiffusionmodels_amd._lib import ptr, stream_ptr
from tests import darcy_ref as R

ULP = 2.0 ** -23
C_DATA, C_RES = 1.3, 0.02
F64, F32 = torch.float64, torch.float32
NAN = float("nan")


def is_quad(P):
    """The sizes the four-pixels-per-thread kernel takes (P / 4 a power of two, at most 256 quads per row)."""
    q = P // 4
    return P % 4 == 0 and P >= 8 and q <= 256 and q & (q - 1) == 0


# (kernel, P, B, nb)
PLAN_CASES = [
    # one-pixel kernel, small: one band; P % 4 == 0 but P / 4 no power of two
    ("pixel", 5, 1, 1), ("pixel", 6, 1, 1), ("pixel", 7, 2, 1), ("pixel", 12, 2, 3), ("pixel", 20, 2, 5),
    # one-pixel kernel, thick bands: R = 6 (last band 3 rows), R = 8 (last 6), R = 12, one band of 13 rows
    ("pixel", 21, 256, 4), ("pixel", 22, 342, 3), ("pixel", 24, 512, 2), ("pixel", 13, 1024, 1),
    # quad kernel, thick bands; (64, 342): R = 22, last band 20 rows - no multiple of four
    ("quad", 8, 2, 2), ("quad", 16, 512, 2), ("quad", 16, 1024, 1), ("quad", 32, 256, 4), ("quad", 32, 512, 2),
    ("quad", 32, 1024, 1), ("quad", 64, 128, 8), ("quad", 64, 256, 4), ("quad", 64, 342, 3),
    # quad kernel, large P: (128, 40) R = 5 with a last band of 3 rows; 256: more (quad, row) items than the 256-thread cap
    ("quad", 128, 1, 32), ("quad", 128, 40, 26), ("quad", 256, 1, 64),
    # one-pixel kernel at the LDS limit: 8 fields of R + 7 = 11 rows of 464 floats
    ("pixel", 464, 1, 116),
]
PLAN_IDS = [f"{k}-P{P}-B{B}-nb{nb}" for k, P, B, nb in PLAN_CASES]
# forward only: the adjoint and the loss do not fit LDS (1024: P / 4 = 256, the quad kernel's limit)
FWD_ONLY_CASES = [(512, 1, 128), (1024, 1, 256)]


def err(q, q64):
    q = np.asarray(q.detach().cpu() if torch.is_tensor(q) else q, dtype=np.float64)
    q64 = np.asarray(q64.detach().cpu() if torch.is_tensor(q64) else q64, dtype=np.float64)
    assert q.shape == q64.shape, (q.shape, q64.shape)
    return float(np.abs(q - q64).max() / max(np.abs(q64).max(), 1e-300))


def check(case, name, got, e32, q64):
    ek = err(got, q64)
    print(f"DARCY_F64 {case} | {name}: err(kernel) {ek:.3e} err(ref32) {e32:.3e}")
    assert ek <= 4 * e32 + 4 * ULP, (case, name, ek, e32)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs and reference
# ------------------------------------------------------------------------------------------------------------------------------
def make_inputs(P, B, seed=0):
    """Target x0 and prediction (p ~ N(0,1), K = exp(N(0,1) / 2)), a RANDOM source field, a random residual cotangent, per-sample
    loss weights in [0.5, 1.5] and inverse variances in [0.1, 10]."""
    g = torch.Generator().manual_seed(1000 * P + B + seed)
    x0 = torch.randn(B, 2, P, P, generator=g)
    pred = x0 + 0.3 * torch.randn(B, 2, P, P, generator=g)
    x0[:, 1] = torch.exp(0.5 * x0[:, 1])
    pred[:, 1] = torch.exp(0.5 * pred[:, 1])
    return {"x0": x0, "pred": pred, "fs": torch.randn(P * P, generator=g), "gr": torch.randn(B, P * P, 3, generator=g),
            "p2w": 0.5 + torch.rand(B, generator=g), "iv": 0.1 + 9.9 * torch.rand(B, generator=g)}


def reference_of(inp, ih0, ih1, fwd_only=False):
    """(float64 results, err(ref32) of each) of the reference on `inp` with spacings 1 / ih0, 1 / ih1."""
    h0, h1 = 1.0 / ih0, 1.0 / ih1
    s = R.bc1_sign_of(h1)
    ref = {}
    for dt in (F64, F32):
        pr = inp["pred"].to(dt).requires_grad_(not fwd_only)
        if fwd_only:
            ref[dt] = {"residual": R.residual(pr, inp["fs"].to(dt), h0, h1, s)}
            continue
        lo, data, rabs, res = R.loss(inp["x0"].to(dt), pr, inp["fs"].to(dt), inp["p2w"], inp["iv"], C_DATA, C_RES, h0, h1, s)
        (gl,) = torch.autograd.grad(lo, pr, retain_graph=True)
        (ga,) = torch.autograd.grad(res, pr, inp["gr"].to(dt))
        ref[dt] = {"residual": res.detach(), "adjoint": ga, "loss": lo.detach(), "data": data.detach(), "rabs": rabs.detach(),
                   "grad": gl}
    return ref[F64], {k: err(ref[F32][k], v) for k, v in ref[F64].items()}


@functools.lru_cache(maxsize=2)
def reference(P, B, ih0, ih1, fwd_only=False):
    inp = make_inputs(P, B)
    return (inp,) + reference_of(inp, ih0, ih1, fwd_only)


def test_reference_agrees_with_the_oracle_on_its_geometry():
    """tests/darcy_ref.py restates the oracle's residual for any spacings and source field; on the oracle's own (h0 = 1 / (P - 1),
    h1 = -h0, the two-corner source) the two are the same function."""
    from oracle import pidm_oracle as O
    P = 10
    x = make_inputs(P, 2)["pred"].double()
    ours = R.residual(x, O.darcy_source_field(P).reshape(-1).double(), 1.0 / (P - 1), -1.0 / (P - 1), 1.0)
    assert err(ours, O.darcy_residual(x)) < 1e-13


# ------------------------------------------------------------------------------------------------------------------------------
# the kernels through the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def put(t, dev, shift=0):
    """t on the device; shift > 0: placed `shift` elements into a larger allocation (4-byte instead of 16-byte alignment)."""
    if not shift:
        return t.to(dev).contiguous()
    v = torch.empty(t.numel() + shift, dtype=t.dtype, device=dev)[shift:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def blank(shape, dev, shift=0, fill=NAN):
    """An output buffer pre-filled with NaN (a pixel the kernel leaves out fails every comparison)."""
    return put(torch.full(shape, fill), dev, shift)


def run_fwd(backend, inp, ih0, ih1, shift=0):
    L, dev = backend
    B, _, P, _ = inp["pred"].shape
    pred, fs, res = put(inp["pred"], dev, shift), put(inp["fs"], dev, shift), blank((B, P * P, 3), dev, shift)
    L.check(L.pidm_darcy_residual_fwd(ptr(pred), ptr(fs), ih0, ih1, ptr(res), B, P, stream_ptr(dev)), "pidm_darcy_residual_fwd")
    return res.cpu()


def run_bwd(backend, inp, ih0, ih1, shift=0):
    L, dev = backend
    B, _, P, _ = inp["pred"].shape
    pred, gr, gx = put(inp["pred"], dev, shift), put(inp["gr"], dev, shift), blank((B, 2, P, P), dev, shift)
    L.check(L.pidm_darcy_residual_bwd(ptr(pred), ptr(gr), ih0, ih1, ptr(gx), B, P, stream_ptr(dev)), "pidm_darcy_residual_bwd")
    return gx.cpu()


def run_loss(backend, inp, ih0, ih1, shift=0):
    """(residual by-product, d loss / d pred, out[4]).  The workspace holds doubles and stays aligned in every case."""
    L, dev = backend
    B, _, P, _ = inp["pred"].shape
    x0, pred, fs, p2w, iv = (put(inp[k], dev, shift) for k in ("x0", "pred", "fs", "p2w", "iv"))
    res, gpred, out = blank((B, P * P, 3), dev, shift), blank((B, 2, P, P), dev, shift), blank((4,), dev, shift)
    ws = torch.empty(L.pidm_darcy_loss_ws(B, P), dtype=torch.uint8, device=dev)
    L.check(L.pidm_darcy_loss_fwd_bwd(ptr(x0), ptr(pred), ptr(fs), ptr(p2w), ptr(iv), C_DATA, C_RES, ih0, ih1, ptr(res), ptr(gpred),
                                      ptr(out), ptr(ws), B, P, stream_ptr(dev)), "pidm_darcy_loss_fwd_bwd")
    return res.cpu(), gpred.cpu(), out.cpu()


def run_all(backend, inp, ih0, ih1, shift=0):
    res_l, grad, out = run_loss(backend, inp, ih0, ih1, shift)
    return {"residual": run_fwd(backend, inp, ih0, ih1, shift), "adjoint": run_bwd(backend, inp, ih0, ih1, shift),
            "loss_residual": res_l, "grad": grad, "out": out}


def check_all(case, got, r64, e32):
    """Forward residual, adjoint and the fused loss of one run against float64."""
    check(case, "residual", got["residual"], e32["residual"], r64["residual"])
    check(case, "adjoint", got["adjoint"], e32["adjoint"], r64["adjoint"])
    assert torch.equal(got["loss_residual"], got["residual"])           # the by-product is the forward kernel's residual
    for i, (key, name) in enumerate((("loss", "loss"), ("data", "c_data * data"), ("rabs", "mean |r|"))):
        check(case, f"fused loss: {name}", got["out"][i], e32[key], r64[key])
    assert got["out"][3].item() == 0.0
    check(case, "fused loss: grad", got["grad"], e32["grad"], r64["grad"])


def same(a, b, keys=("residual", "adjoint", "loss_residual", "grad")):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


def nbands(L, B, P):
    ws = L.pidm_darcy_loss_ws(B, P)
    assert ws % (B * 32) == 0
    return ws // (B * 32)


# ------------------------------------------------------------------------------------------------------------------------------
# band plans
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,P,B,nb", PLAN_CASES, ids=PLAN_IDS)
def test_plan_case_vs_float64(backend, kernel, P, B, nb):
    L, _ = backend
    assert nbands(L, B, P) == nb and is_quad(P) == (kernel == "quad")
    ih = float(P - 1)
    inp, r64, e32 = reference(P, B, ih, -ih)
    check_all(f"plan {kernel} P={P} B={B} nb={nb}", run_all(backend, inp, ih, -ih), r64, e32)


@pytest.mark.parametrize("P,B,nb", FWD_ONLY_CASES, ids=[f"P{P}" for P, _, _ in FWD_ONLY_CASES])
def test_forward_beyond_the_adjoint_sizes_vs_float64(backend, P, B, nb):
    L, _ = backend
    assert nbands(L, B, P) == nb and is_quad(P)
    ih = float(P - 1)
    inp, r64, e32 = reference(P, B, ih, -ih, True)
    check(f"plan quad P={P} B={B} nb={nb} forward only", "residual", run_fwd(backend, inp, ih, -ih), e32["residual"],
          r64["residual"])


@pytest.mark.parametrize("P,B", [(16, 1024), (32, 512), (64, 128), (21, 256), (64, 342)])
def test_one_sample_is_the_same_alone_and_in_the_batch(backend, P, B):
    """Same taps in the same order in every plan: sample B // 2 + 1 alone (B = 1: the thinnest bands) gives the bits it gives
    inside the batch (thick bands), and two runs of the batch agree bit for bit, the loss scalars included."""
    L, _ = backend
    ih = float(P - 1)
    inp = make_inputs(P, B)
    a, b = run_all(backend, inp, ih, -ih), run_all(backend, inp, ih, -ih)
    same(a, b)
    assert torch.equal(a["out"], b["out"]) and not torch.isnan(a["out"]).any()
    i = B // 2 + 1
    assert nbands(L, 1, P) == P // 4 and nbands(L, B, P) < P // 4
    one = {k: (v[i:i + 1] if v.shape[0] == B else v) for k, v in inp.items() if k != "fs"}
    one["fs"] = inp["fs"]
    assert torch.equal(run_fwd(backend, one, ih, -ih), a["residual"][i:i + 1])
    assert torch.equal(run_bwd(backend, one, ih, -ih), a["adjoint"][i:i + 1])


# ------------------------------------------------------------------------------------------------------------------------------
# geometry: independent spacings, both signs of inv_h1
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["uniform-positive", (15.0, -7.0), (3.0, -9.0), (15.0, 22.0)], ids=str)
@pytest.mark.parametrize("P", [10, 16, 64])
def test_geometry_vs_float64(backend, P, geom):
    ih0, ih1 = (float(P - 1), float(P - 1)) if geom == "uniform-positive" else geom
    inp, r64, e32 = reference(P, 3, ih0, ih1)
    check_all(f"geometry P={P} inv_h=({ih0:g}, {ih1:g})", run_all(backend, inp, ih0, ih1), r64, e32)


# ------------------------------------------------------------------------------------------------------------------------------
# kernel variants at P = 64
# ------------------------------------------------------------------------------------------------------------------------------
VARIANTS = {"one_pixel": {"PIDM_DARCY_QUAD": "0"},
            "stream": {"PIDM_DARCY_FULL": "1"},
            "stream_1wg": {"PIDM_DARCY_FULL": "1", "PIDM_DARCY_STREAM_WGS": "1"},
            "full": {"PIDM_DARCY_FULL": "1", "PIDM_DARCY_STREAM": "0"}}


@pytest.mark.parametrize("variant,B", [("one_pixel", 3)] + [(v, B) for v in ("stream", "stream_1wg", "full") for B in (1, 3)])
def test_variants_at_64_vs_float64_and_bit_identical_to_the_band_kernel(backend, monkeypatch, variant, B):
    L, _ = backend
    P, ih = 64, 63.0
    inp, r64, e32 = reference(P, B, ih, -ih)
    monkeypatch.setenv("PIDM_DARCY_FULL", "0")
    assert nbands(L, B, P) == 16
    base = run_all(backend, inp, ih, -ih)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    assert nbands(L, B, P) == (16 if variant == "one_pixel" else 1)
    got = run_all(backend, inp, ih, -ih)
    check_all(f"variant {variant} P=64 B={B}", got, r64, e32)
    same(got, base)


# ------------------------------------------------------------------------------------------------------------------------------
# buffers that are not 16-byte aligned: the quad kernel's launch falls back to the one-pixel kernel
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,B,full", [(16, 2, False), (64, 2, False), (64, 3, True)], ids=["P16-B2", "P64-B2", "P64-B3-full"])
def test_unaligned_buffers(backend, monkeypatch, P, B, full):
    """Every tensor argument one float into a larger allocation.  With PIDM_DARCY_FULL=1 the fall-back is the one-pixel kernel with
    a single 64-row band."""
    L, _ = backend
    ih = float(P - 1)
    if full:
        monkeypatch.setenv("PIDM_DARCY_FULL", "1")
    assert nbands(L, B, P) == (1 if full else P // 4)
    inp, r64, e32 = reference(P, B, ih, -ih)
    aligned, got = run_all(backend, inp, ih, -ih), run_all(backend, inp, ih, -ih, shift=1)
    check_all(f"unaligned P={P} B={B} full={int(full)}", got, r64, e32)
    same(got, aligned)


# ------------------------------------------------------------------------------------------------------------------------------
# Jacobian maximum
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [-1.0, 1.0], ids=["h1neg", "h1pos"])
@pytest.mark.parametrize("P", [5, 7, 8, 12])
def test_jacobian_max_vs_dense_float64(backend, P, sign):
    L, dev = backend
    B, ih0, ih1 = 3, float(P - 1), sign * float(P - 1)
    x = make_inputs(P, B, seed=7)["pred"]
    x[1, 1] = 1.0                                                        # K == 1
    x[2, 1] = 1e-3                                                       # the boundary rows hold the maximum
    j64, j32 = (R.jacobian_max(x.to(dt), 1.0 / ih0, 1.0 / ih1, R.bc1_sign_of(ih1)) for dt in (F64, F32))
    assert abs(j64[2].item() - 1.5 * ih0) < 1e-9 * ih0                   # |-1.5 / h| of the one-sided first derivative
    xd = x.to(dev)
    out = torch.full((B,), NAN, device=dev)
    L.check(L.pidm_darcy_jacobian_max(ptr(xd), ih0, ih1, ptr(out), B, P, stream_ptr(dev)), "pidm_darcy_jacobian_max")
    out = out.cpu()
    for b in range(B):
        check(f"jacobian max P={P} inv_h1={ih1:g} sample {b}", "jacobian max", out[b], err(j32[b], j64[b]), j64[b])


# ------------------------------------------------------------------------------------------------------------------------------
# PIDM_DARCY_ROWS follows knob reloads
# ------------------------------------------------------------------------------------------------------------------------------
def test_darcy_rows_knob_changes_the_plan_not_the_bits(backend, monkeypatch):
    L, _ = backend
    P, B, ih = 32, 1024, 31.0
    inp = make_inputs(P, B)
    runs = []
    for rows, nb in ((None, 1), ("8", 4), ("4", 8), ("1", 8)):           # a value below 4 is raised to 4
        if rows is None:
            monkeypatch.delenv("PIDM_DARCY_ROWS", raising=False)
        else:
            monkeypatch.setenv("PIDM_DARCY_ROWS", rows)
        assert nbands(L, B, P) == nb, (rows, nb)
        runs.append(run_all(backend, inp, ih, -ih))
        assert not torch.isnan(runs[-1]["out"]).any()
    for r in runs[1:]:
        same(r, runs[0])


# ------------------------------------------------------------------------------------------------------------------------------
# argument guards: nothing is launched, nothing is written
# ------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 7.5


class Args:
    """Full-size, sentinel-filled buffers of the four entry points at (B, P)."""

    def __init__(self, backend, B, P):
        self.L, self.dev = backend
        self.B, self.P = B, P
        f = lambda *s: torch.full(s, SENTINEL, device=self.dev)   # noqa: E731
        self.t = {"x0": f(B, 2, P, P), "pred": f(B, 2, P, P), "fs": f(P * P), "gr": f(B, P * P, 3), "p2w": f(B), "iv": f(B),
                  "res": f(B, P * P, 3), "gx": f(B, 2, P, P), "out": f(4), "tab_w": f(10), "tab_v": f(10),
                  "t": torch.zeros(B, dtype=torch.int64, device=self.dev),
                  "ws": torch.full((max(B * (P // 4 + 1) * 32, 32),), 0x5A, dtype=torch.uint8, device=self.dev)}

    def call(self, entry, null=None, B=None, P=None):
        L, st = self.L, stream_ptr(self.dev)
        B, P = self.B if B is None else B, self.P if P is None else P
        a = {k: (None if k == null else ptr(v)) for k, v in self.t.items()}
        ih = float(self.P - 1)
        if entry == "fwd":
            return L.pidm_darcy_residual_fwd(a["pred"], a["fs"], ih, -ih, a["res"], B, P, st)
        if entry == "bwd":
            return L.pidm_darcy_residual_bwd(a["pred"], a["gr"], ih, -ih, a["gx"], B, P, st)
        if entry == "loss":
            return L.pidm_darcy_loss_fwd_bwd(a["x0"], a["pred"], a["fs"], a["p2w"], a["iv"], C_DATA, C_RES, ih, -ih, a["res"], a["gx"],
                                             a["out"], a["ws"], B, P, st)
        return L.pidm_darcy_loss_fwd_bwd_t(a["x0"], a["pred"], a["fs"], a["t"], a["tab_w"], a["tab_v"], C_DATA, C_RES, ih, -ih,
                                           a["res"], a["gx"], a["out"], a["ws"], B, P, st)

    def refused(self, rc, what):
        msg = self.L.pidm_last_error().decode()
        assert rc != 0 and what in msg, (rc, msg)
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        for k in ("res", "gx", "out"):
            assert (self.t[k] == SENTINEL).all(), k
        assert (self.t["ws"] == 0x5A).all()


REQUIRED = {"fwd": ("pred", "fs", "res"),
            "bwd": ("pred", "gr", "gx"),
            "loss": ("x0", "pred", "fs", "p2w", "iv", "res", "gx", "out", "ws"),
            "loss_t": ("x0", "pred", "fs", "t", "tab_w", "tab_v", "res", "gx", "out", "ws")}


@pytest.mark.parametrize("entry", list(REQUIRED))
def test_null_pointers_are_refused(backend, entry):
    a = Args(backend, 2, 8)
    for name in REQUIRED[entry]:
        what = "null time steps / tables" if name in ("t", "tab_w", "tab_v") else "darcy: null buffer"
        a.refused(a.call(entry, null=name), what)


@pytest.mark.parametrize("entry", list(REQUIRED))
def test_empty_batch_and_too_small_an_image_are_refused(backend, entry):
    a = Args(backend, 2, 8)
    for B, P in ((0, 8), (-1, 8), (2, 4)):
        assert a.L.pidm_darcy_loss_ws(B, P) == 0
        a.refused(a.call(entry, B=B, P=P), "need B>0 and P>=5")


@pytest.mark.parametrize("entry,P", [("bwd", 468), ("loss", 512)])
def test_sizes_beyond_lds_are_refused(backend, entry, P):
    """8 fields of R + 7 = 11 rows: 464 floats per row are the last that fit 160 KiB."""
    a = Args(backend, 1, P)
    a.refused(a.call(entry), "does not fit the 160 KiB LDS")
