"""Float64 parity of the stencil engine (csrc/k_stencil.hip) across the branches of its launch planner: pidm_stencil_apply,
pidm_stencil_apply_adjoint and pidm_darcy_residual_general_fwd / _bwd through the C ABI, on the host-emulated build and on gfx950.

References (tests/stencil_matrix_ref.py): the classed operator of tests/stencil_ref.py as a sparse matrix S assembled from the
stencil dictionary with its fp32-rounded coefficients; S @ x and autograd through it are the operator and its adjoint, in float64 on the
fp32 inputs the kernels see.  The general residual reference is darcy_ref.residual's algebra on four such matrices.

Tolerances - both are the project's own:
  * operators: the per-pixel bound of test_stencil_engine.py, |y - y64| <= 2 n u (|S| |x|) (u = 2^-24, n = the longest tap list),
    against the float64 product, not a golden.  The adjoint of a K-operator launch is ONE fp32 chain over the K operators, so its
    bound is 2 n u sum_k (|S_k|^T |g_k|) with n = the sum of the K longest tap lists (the length of that chain).
  * residual and its adjoint: the rule of test_kernels_darcy_f64.py, err(kernel) <= 4 * err(ref32) + 4 * 2^-23 with
    err(q) = max|q - q64| / max|q64| and ref32 = the same reference in float32 inside the test.

Every operator plan case asserts the (TR, TC, ntr, ntc, h, LDS bytes) pidm_stencil_plan gives it, and no two of them share
(TR, TC, ntr, ntc, h, periodic): a later change of st_plan cannot turn the cases into repeats of one plan.

Four mutations of k_stencil.hip were tried on the emulator against this module, tests/test_stencil_engine.py and
tests/test_darcy_general.py:
  (a) st_class with `>` for `>=` (the first high-edge pixel takes the centre list): every non-periodic case here fails, the
      smallest images (op-1x10x10-acc6, op-2x7x7-acc4, op-2x4x4-acc2) among them.  The older modules' golden, adjoint-identity and
      polynomial tests fail as well.
  (b) st_stage_tile with rows wrapped and columns outside the image read as zero: every periodic case here fails, among them
      op-1x8x131-acc6-per and general P131-B1-acc4-periodic, the only ones where the wrap crosses column tiles.  The older
      modules' periodic golden tests fail as well.
  (c) TC forced to 128 (no column tiles): the VALUES stay right, so no valued comparison can see it and no older test fails; the
      plan tuples of op-1x10x131-acc6, op-1x12x129-acc2, op-1x8x131-acc6-per and of both general P131 cases fail.
  (d) the adjoint's `pure` test with inner = 2 * mio: op-2x21x13-acc4, op-512x32x32-acc2, op-1x12x129-acc2 and the general cases
      from P = 16 up fail (not op-1x10x131-acc6: ten rows have no pure row at fd_acc 6).  The older modules' golden and
      adjoint-identity tests fail as well.

Worst figures over the cases of this module (every test prints its figures before it asserts): for the operators the largest share
of the per-pixel bound, for the residual err(kernel) / err(ref32) with the share of the bound in brackets.

    quantity                  emulator                      MI355X
    operator forward          0.423 of the bound            0.423 of the bound            3x3x3 fd_acc 2 periodic, d_d1
    operator adjoint          0.091 of the bound            0.346 of the bound            512x32x32 fd_acc 2 / 1024x33x128 (gfx950 only)
    residual                  1.7e-07 / 1.7e-07 (0.15)      1.7e-07 / 1.7e-07 (0.15)      P = 16, fd_acc 4, periodic, inv_h = (3, -9)
    residual adjoint          2.8e-07 / 1.6e-07 (0.25)      2.8e-07 / 1.6e-07 (0.25)      P = 32, B = 512, fd_acc 6

No quantity uses half of its bound.  Every torch.equal of this module holds on the gfx950 build (fma contraction on) as on the emulator.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from physicsinformeddiffusionmodels_amd._lib import ptr, stream_ptr
from physicsinformeddiffusionmodels_amd.grad_utils import StencilGradientComputation, StencilGradients, _ops_array
from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
from tests import darcy_ref as R
from tests.stencil_matrix_ref import apply_matrix, operator_matrix, residual_general
from tests.stencil_ref import U, apply_np, fp32_stencils, longest_list
from tests.test_kernels_darcy_f64 import err, make_inputs

ULP = 2.0 ** -23
F64, F32 = torch.float64, torch.float32
NAN = float("nan")
MODES = StencilGradients.MODES
D0, D1 = 1.0 / 63, -1.0 / 63
HALO_DICT = {("C", "C"): {(0, 0): 0.0, (0, -32): 1.0, (32, 0): 1.0}}


def _lib(backend):
    L, dev = backend
    return L, (L if dev.type == "cpu" else None), dev


def blank(shape, dev):
    return torch.full(shape, NAN, device=dev)


def plan_of(L, comps, dev, N, H, W, periodic):
    ops, keep = _ops_array(tuple(comps), dev)
    out = (C.c_int * 6)(*([-1] * 6))
    L.check(L.pidm_stencil_plan(ops, len(comps), N, H, W, int(periodic), out), "pidm_stencil_plan")
    return tuple(out)


def lds_bytes(comps, TR, TC, h):
    """One tile with its halo plus, per operator, 18 words of class ranges and 3 words per tap."""
    return ((TR + 2 * h) * (TC + 2 * h) + sum(18 + 3 * c.ntaps for c in comps)) * 4


def assert_plan(L, comps, dev, N, H, W, periodic, want5):
    TR, TC, ntr, ntc, h = want5
    got = plan_of(L, comps, dev, N, H, W, periodic)
    assert got == (TR, TC, ntr, ntc, h, lds_bytes(comps, TR, TC, h)), (got, want5)


# ------------------------------------------------------------------------------------------------------------------------------
# the references pin each other
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc,periodic,H,W", [(2, False, 4, 5), (4, False, 7, 9), (6, False, 10, 11), (2, True, 3, 3), (4, True, 5, 8),
                                              (6, True, 7, 9)])
def test_operator_matrix_equals_the_loop_reference(acc, periodic, H, W):
    sg = StencilGradients(d0=D0, d1=D1, fd_acc=acc, periodic=periodic)
    x = torch.randn(2, H, W, generator=torch.Generator().manual_seed(H * W), dtype=F64)
    for mode in MODES:
        st = getattr(sg, mode).stencils
        S, A = operator_matrix(st, H, W, periodic), operator_matrix(st, H, W, periodic, absolute=True)
        f32 = fp32_stencils(st)
        pairs = ((apply_matrix(S, x), apply_np(f32, x.numpy(), periodic)),
                 (apply_matrix(S.t().coalesce(), x), apply_np(f32, x.numpy(), periodic, transpose=True)),
                 (apply_matrix(A, x.abs()), apply_np(f32, x.numpy(), periodic, absolute=True)),
                 (apply_matrix(A.t().coalesce(), x.abs()), apply_np(f32, x.numpy(), periodic, absolute=True, transpose=True)))
        for got, want in pairs:
            assert err(got, want) < 1e-13, mode
        xr = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad(apply_matrix(S, xr), xr, x)
        assert err(gx, pairs[1][1]) < 1e-13, mode
        assert operator_matrix(st, H, W, periodic, dtype=F32).dtype == F32


def mats_of(sg, P, periodic, dt):
    return tuple(operator_matrix(getattr(sg, m).stencils, P, P, periodic, dt) for m in MODES[:4])


def test_general_reference_equals_the_second_order_reference():
    """Spacings that are powers of two: every second-order coefficient is exact in fp32, so the matrices hold what darcy_ref's
    closed forms hold and the two references are one function."""
    P = 9
    x = make_inputs(P, 2)["pred"].double()
    fs = make_inputs(P, 2)["fs"].double()
    for h0, h1 in ((1.0 / 16, -1.0 / 8), (0.25, 0.5)):
        sg = StencilGradients(d0=h0, d1=h1, fd_acc=2)
        s = R.bc1_sign_of(h1)
        assert err(residual_general(x, fs, mats_of(sg, P, False, F64), s), R.residual(x, fs, h0, h1, s)) < 1e-13


def test_general_reference_agrees_with_the_oracle_on_its_geometry():
    """P = 17: the oracle's spacing 1 / (P - 1) is a power of two (see above)."""
    from oracle import pidm_oracle as O
    P = 17
    x = make_inputs(P, 2)["pred"].double()
    sg = StencilGradients(d0=1.0 / (P - 1), d1=-1.0 / (P - 1), fd_acc=2)
    ours = residual_general(x, O.darcy_source_field(P).reshape(-1).double(), mats_of(sg, P, False, F64), 1.0)
    assert err(ours, O.darcy_residual(x)) < 1e-13


@pytest.mark.parametrize("acc,bcs,rev", [(4, "none", True), (6, "none", True), (4, "none", False), (2, "periodic", True),
                                         (4, "periodic", True)])
def test_general_reference_vs_reference_golden(acc, bcs, rev):
    """The genuine reference's fp32 outputs (g27_darcy_general) within the figures tests/test_darcy_general.py holds the kernels to."""
    import os
    from oracle import pidm_oracle as O
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "g27_darcy_general.npz"))
    tag, P = f"{acc}_{bcs}_{int(rev)}", 16
    d0 = 1.0 / (P - 1)
    sg = StencilGradients(d0=d0, d1=-d0 if rev else d0, fd_acc=acc, periodic=bcs == "periodic")
    xr = torch.from_numpy(g["x0"]).double().requires_grad_(True)
    res = residual_general(xr, O.darcy_source_field(P).reshape(-1).double(), mats_of(sg, P, bcs == "periodic", F64),
                             1.0 if rev else -1.0)
    (gx,) = torch.autograd.grad((torch.from_numpy(g["w"]).double() * res).sum(), xr)
    ef, ea = err(g["res_" + tag], res), err(g["gx_" + tag], gx)
    print(f"STENCIL_F64 golden {tag} | reference fp32 against float64: fwd {ef:.3e} adj {ea:.3e}")
    assert ef < 2e-6 and ea < 5e-6


# ------------------------------------------------------------------------------------------------------------------------------
# operators: plan cases
# ------------------------------------------------------------------------------------------------------------------------------
# (N, H, W, fd_acc, periodic, (TR, TC, ntr, ntc, h))
OP_CASES = [
    (1, 10, 10, 6, False, (8, 10, 2, 1, 7)),        # smallest fd_acc 6 image: every pixel in an edge class; bands of 8 + 2 rows
    (2, 7, 7, 4, False, (7, 7, 1, 1, 5)),           # smallest at fd_acc 4
    (2, 4, 4, 2, False, (4, 4, 1, 1, 3)),           # smallest at fd_acc 2
    (2, 7, 7, 6, True, (7, 7, 1, 1, 3)),            # the wrap covers the whole image
    (3, 3, 3, 2, True, (3, 3, 1, 1, 1)),
    (2, 21, 13, 4, False, (8, 13, 3, 1, 5)),        # bands 8 + 8 + 5; QC = 4 with a one-pixel last quad; unaligned rows
    (1024, 16, 16, 6, False, (16, 16, 1, 1, 7)),    # want == 1: one whole-image tile
    (512, 32, 32, 2, False, (16, 32, 2, 1, 3)),     # two thick bands
    (1, 10, 131, 6, False, (8, 64, 2, 3, 7)),       # three column tiles, the last 3 columns wide (all class H, a ragged quad)
    (1, 12, 129, 2, False, (8, 64, 2, 3, 3)),       # last column tile one pixel wide
    (1, 8, 131, 6, True, (8, 64, 1, 3, 3)),         # periodic with column tiles: the halos of tile 0 and the last tile wrap
    (1, 130, 9, 4, True, (8, 9, 17, 1, 2)),         # 17 row bands, the first and last wrap rows
]
OP_IDS = [f"op-{N}x{H}x{W}-acc{acc}" + ("-per" if per else "") for N, H, W, acc, per, _ in OP_CASES]
GPU_CASE = (1024, 33, 128, 2, False, (32, 128, 2, 1, 3))     # d_d00 only: QC = 32, the thread cap binds (TR = 32 of 33 rows)
HALO_CASES = [(65, 65, (32, 65, 3, 1, 32)),       # thin = h = 32: bands 32 + 32 + 1
              (65, 128, (21, 128, 4, 1, 32))]     # cap_lds binds: 16384 / (128 + 64) - 64 = 21 rows


def test_no_two_operator_cases_share_a_plan():
    keys = [(p, per) for _, _, _, _, per, p in OP_CASES] + [(GPU_CASE[5], False)] + [(p, True) for _, _, p in HALO_CASES]
    assert len(set(keys)) == len(keys)


@functools.lru_cache(maxsize=None)
def op_mats(acc, periodic, H, W, mode):
    st = getattr(StencilGradients(d0=D0, d1=D1, fd_acc=acc, periodic=periodic), mode).stencils
    return (operator_matrix(st, H, W, periodic), operator_matrix(st, H, W, periodic, absolute=True),
            longest_list(fp32_stencils(st), periodic))


def op_inputs(N, H, W, K):
    g = torch.Generator().manual_seed(100 * H + W + N)
    return torch.randn(N, H, W, generator=g), [torch.randn(N, H, W, generator=g) for _ in range(K)]


def run_ops(L, dev, comps, x, gs, periodic):
    """(outputs of the K operators, the adjoint of the K cotangents) of one forward and one adjoint launch."""
    N, H, W = x.shape
    K = len(comps)
    ops, keep = _ops_array(tuple(comps), dev)
    xd, gd = x.to(dev), [g.to(dev) for g in gs]
    outs, gx = [blank((N, H, W), dev) for _ in range(K)], blank((N, H, W), dev)
    optr = (C.c_void_p * K)(*[o.data_ptr() for o in outs])
    gptr = (C.c_void_p * K)(*[g.data_ptr() for g in gd])
    L.check(L.pidm_stencil_apply(ptr(xd), H * W, ops, optr, K, H * W, N, H, W, int(periodic), stream_ptr(dev)), "pidm_stencil_apply")
    L.check(L.pidm_stencil_apply_adjoint(gptr, H * W, ops, K, None, 0, ptr(gx), H * W, N, H, W, int(periodic), stream_ptr(dev)),
            "pidm_stencil_apply_adjoint")
    return [o.cpu() for o in outs], gx.cpu()


def check_ops(case, modes, acc, periodic, x, gs, outs, gx):
    N, H, W = x.shape
    xr = x.double().requires_grad_(True)
    ys, bound_T, n_T = [], torch.zeros(N, H, W, dtype=F64), 0
    for mode, g, y in zip(modes, gs, outs):
        S, A, n = op_mats(acc, periodic, H, W, mode)
        y64 = apply_matrix(S, xr)
        ys.append(y64)
        bound = 2 * n * U * apply_matrix(A, x.double().abs())
        e = (y.double() - y64.detach()).abs()
        print(f"STENCIL_F64 {case} | {mode} forward: {float((e / bound.clamp_min(1e-300)).max()):.3f} of the bound")
        assert not torch.isnan(y).any() and (e <= bound).all(), (case, mode)
        bound_T += apply_matrix(A.t().coalesce(), g.double().abs())
        n_T += n
    (gx64,) = torch.autograd.grad(ys, xr, [g.double() for g in gs])
    bound_T *= 2 * n_T * U
    e = (gx.double() - gx64).abs()
    print(f"STENCIL_F64 {case} | adjoint of {len(modes)}: {float((e / bound_T.clamp_min(1e-300)).max()):.3f} of the bound")
    assert not torch.isnan(gx).any() and (e <= bound_T).all(), case


def op_case(backend, N, H, W, acc, periodic, plan, modes=MODES):
    L, lib, dev = _lib(backend)
    sg = StencilGradients(d0=D0, d1=D1, fd_acc=acc, periodic=periodic, device=dev, lib=lib)
    comps = [getattr(sg, m) for m in modes]
    assert_plan(L, comps, dev, N, H, W, periodic, plan)
    x, gs = op_inputs(N, H, W, len(modes))
    outs, gx = run_ops(L, dev, comps, x, gs, periodic)
    check_ops(f"op {N}x{H}x{W} acc {acc} periodic {int(periodic)}", modes, acc, periodic, x, gs, outs, gx)
    return L, dev, comps, x, gs, outs, gx


@pytest.mark.parametrize("N,H,W,acc,periodic,plan", OP_CASES, ids=OP_IDS)
def test_operator_plan_case_vs_float64(backend, N, H, W, acc, periodic, plan):
    L, dev, comps, x, gs, outs, gx = op_case(backend, N, H, W, acc, periodic, plan)
    if plan[2] == 1 and N == 1024:
        # the whole-image tile against the same images run alone (bands of 8 rows): other plans, the same taps in the same order
        assert plan_of(L, comps, dev, 1, H, W, periodic)[:4] == (8, W, 2, 1)
        for i in (0, 511, 1023):
            o1, g1 = run_ops(L, dev, comps, x[i:i + 1], [g[i:i + 1] for g in gs], periodic)
            assert all(torch.equal(a, b[i:i + 1]) for a, b in zip(o1, outs)) and torch.equal(g1, gx[i:i + 1]), i


@pytest.mark.gpu
def test_operator_thread_cap_case_vs_float64():
    """QC = 32 quads per row: 1024 / 32 = 32 rows per workgroup bind below the 33 the batch asks for; the second band is one row.
    Four million pixels: too many for the emulator's one fiber per thread."""
    from physicsinformeddiffusionmodels_amd._lib import get_lib
    assert torch.cuda.is_available() and get_lib().backend == "hip"
    N, H, W, acc, periodic, plan = GPU_CASE
    op_case((get_lib(), torch.device("cuda:0")), N, H, W, acc, periodic, plan, modes=("d_d00",))


@pytest.mark.parametrize("H,W,plan", HALO_CASES, ids=[f"{H}x{W}" for H, W, _ in HALO_CASES])
def test_halo_limit_is_two_exact_rolls(backend, H, W, plan):
    """A user dictionary that reaches kStMaxHalo = 32 pixels, periodic: y = x[i, j - 32] + x[i + 32, j] on wrapped indices is one
    fp32 sum of two pixels, the adjoint likewise - exact."""
    L, lib, dev = _lib(backend)
    op = StencilGradientComputation(HALO_DICT, periodic=True, device=dev, lib=lib)
    assert op.max_inner_offset == 32 and op.min_size() == 65
    assert_plan(L, [op], dev, 1, H, W, True, plan)
    x, (g,) = op_inputs(1, H, W, 1)
    (y,), gx = run_ops(L, dev, [op], x, [g], True)
    assert torch.equal(y, torch.roll(x, 32, dims=-1) + torch.roll(x, -32, dims=-2))
    assert torch.equal(gx, torch.roll(g, -32, dims=-1) + torch.roll(g, 32, dims=-2))


def test_a_tap_beyond_the_halo_limit_is_refused(backend):
    L, lib, dev = _lib(backend)
    op = StencilGradientComputation({("C", "C"): {(0, 0): 0.0, (0, -33): 1.0, (32, 0): 1.0}}, periodic=True, device=dev, lib=lib)
    ops, keep = _ops_array((op,), dev)
    H = W = 67
    x, y = torch.full((H, W), 7.5, device=dev), torch.full((H, W), 7.5, device=dev)
    out = (C.c_int * 6)(*([-1] * 6))
    outs = (C.c_void_p * 1)(y.data_ptr())
    for rc in (L.pidm_stencil_plan(ops, 1, 1, H, W, 1, out),
               L.pidm_stencil_apply(ptr(x), H * W, ops, outs, 1, H * W, 1, H, W, 1, stream_ptr(dev)),
               L.pidm_stencil_apply_adjoint(outs, H * W, ops, 1, None, 0, ptr(x), H * W, 1, H, W, 1, stream_ptr(dev))):
        assert rc != 0 and "reaches 33 pixels" in L.pidm_last_error().decode()
    assert tuple(out) == (-1,) * 6 and (x == 7.5).all() and (y == 7.5).all()


def test_plan_query_refuses_what_the_launch_refuses(backend):
    L, lib, dev = _lib(backend)
    sg = StencilGradients(d0=D0, d1=D1, fd_acc=6, device=dev, lib=lib)
    ops, keep = _ops_array((sg.d_d00,), dev)
    out = (C.c_int * 6)()
    for args, what in (((None, 1, 1, 16, 16, 0, out), "null operator array"), ((ops, 0, 1, 16, 16, 0, out), "operators per launch"),
                       ((ops, 6, 1, 16, 16, 0, out), "operators per launch"), ((ops, 1, 0, 16, 16, 0, out), "need N, H, W > 0"),
                       ((ops, 1, 1, 9, 16, 0, out), "too small"), ((ops, 1, 1, 16, 9, 0, out), "too small"),
                       ((ops, 1, 1, 6, 7, 1, out), "too small"), ((ops, 1, 1, 16, 16, 0, None), "null buffer")):
        assert L.pidm_stencil_plan(*args) != 0 and what in L.pidm_last_error().decode(), what
    assert L.pidm_stencil_plan(ops, 1, 1, 10, 10, 0, out) == 0 and L.pidm_stencil_plan(ops, 1, 1, 7, 7, 1, out) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# general Darcy residual
# ------------------------------------------------------------------------------------------------------------------------------
def default_geom(P):
    return (float(P - 1), -float(P - 1))


GEN_MIN = [(4, 3, 2, "none"), (7, 3, 4, "none"), (10, 3, 6, "none"), (3, 2, 2, "periodic"), (5, 2, 4, "periodic"), (7, 2, 6, "periodic")]
GEN_ORDERS = [(P, 2, acc, bcs) for P in (21, 64) for acc in (2, 4, 6) for bcs in ("none", "periodic")]
GEN_GEOM = [(16, 2, acc, bcs) + geom for acc in (4, 6) for bcs in ("none", "periodic")
            for geom in ((15.0, -7.0), (3.0, -9.0), (15.0, 22.0), default_geom(16))]
GEN_CASES = [c + default_geom(c[0]) for c in GEN_MIN + GEN_ORDERS] + GEN_GEOM


def gen_id(c):
    P, B, acc, bcs, ih0, ih1 = c
    return f"P{P}-B{B}-acc{acc}-{bcs}" + ("" if (ih0, ih1) == default_geom(P) else f"-ih({ih0:g},{ih1:g})")


def gen_reference_of(inp, acc, bcs, ih0, ih1):
    sg = StencilGradients(d0=1.0 / ih0, d1=1.0 / ih1, fd_acc=acc, periodic=bcs == "periodic")
    P, s, ref = inp["pred"].shape[-1], R.bc1_sign_of(1.0 / ih1), {}
    for dt in (F64, F32):
        xr = inp["pred"].to(dt).requires_grad_(True)
        res = residual_general(xr, inp["fs"].to(dt), mats_of(sg, P, bcs == "periodic", dt), s)
        (ga,) = torch.autograd.grad(res, xr, inp["gr"].to(dt))
        ref[dt] = {"residual": res.detach(), "adjoint": ga}
    return ref[F64], {k: err(ref[F32][k], v) for k, v in ref[F64].items()}


@functools.lru_cache(maxsize=2)
def gen_reference(P, B, acc, bcs, ih0, ih1):
    inp = make_inputs(P, B)
    return (inp,) + gen_reference_of(inp, acc, bcs, ih0, ih1)


def gen_comps(backend, acc, bcs, ih0, ih1):
    L, lib, dev = _lib(backend)
    sg = StencilGradients(d0=1.0 / ih0, d1=1.0 / ih1, fd_acc=acc, periodic=bcs == "periodic", device=dev, lib=lib)
    return [getattr(sg, m) for m in MODES[:4]]


def run_general(backend, comps, inp, bcs, ih1):
    L, lib, dev = _lib(backend)
    B, _, P, _ = inp["pred"].shape
    ops, keep = _ops_array(tuple(comps), dev)
    per, s, st = int(bcs == "periodic"), R.bc1_sign_of(1.0 / ih1), stream_ptr(dev)
    x, fs, gr = inp["pred"].to(dev).contiguous(), inp["fs"].to(dev), inp["gr"].to(dev).contiguous()
    res, gx = blank((B, P * P, 3), dev), blank((B, 2, P, P), dev)
    ws = torch.empty(L.pidm_darcy_general_ws(B, P), dtype=torch.uint8, device=dev)
    assert ws.numel() == 12 * B * P * P * 4
    L.check(L.pidm_darcy_residual_general_fwd(ptr(x), ptr(fs), ops, per, s, ptr(res), ptr(ws), B, P, st), "general_fwd")
    L.check(L.pidm_darcy_residual_general_bwd(ptr(x), ptr(gr), ops, per, s, ptr(gx), ptr(ws), B, P, st), "general_bwd")
    return {"residual": res.cpu(), "adjoint": gx.cpu()}


def check(case, name, got, e32, q64):
    ek = err(got, q64)
    print(f"STENCIL_F64 {case} | {name}: err(kernel) {ek:.3e} err(ref32) {e32:.3e}")
    assert ek <= 4 * e32 + 4 * ULP, (case, name, ek, e32)


def gen_case(backend, P, B, acc, bcs, ih0, ih1):
    comps = gen_comps(backend, acc, bcs, ih0, ih1)
    inp, r64, e32 = gen_reference(P, B, acc, bcs, ih0, ih1)
    got = run_general(backend, comps, inp, bcs, ih1)
    for k in ("residual", "adjoint"):
        check(f"general {gen_id((P, B, acc, bcs, ih0, ih1))}", k, got[k], e32[k], r64[k])
    return comps, inp, got


@pytest.mark.parametrize("P,B,acc,bcs,ih0,ih1", GEN_CASES, ids=[gen_id(c) for c in GEN_CASES])
def test_general_residual_vs_float64(backend, P, B, acc, bcs, ih0, ih1):
    comps, _, _ = gen_case(backend, P, B, acc, bcs, ih0, ih1)
    if (P, B, acc, bcs) in GEN_MIN:
        assert max(c.min_size() for c in comps) == P           # one pixel less is refused (test_general_guards)


# (P, B, fd_acc, bcs, plan of the four-operator launches, plan of the two-operator launches)
GEN_PLANS = [(16, 1024, 4, "none", (16, 16, 1, 1, 5), (16, 16, 1, 1, 4)),       # whole-image tiles
             (131, 1, 6, "none", (8, 64, 17, 3, 7), (8, 64, 17, 3, 6)),         # column tiles in all four stencil launches
             (131, 1, 4, "periodic", (8, 64, 17, 3, 2), (8, 64, 17, 3, 2)),     # ... wrapped; the second adjoint launch has `add`
             (32, 512, 6, "none", (16, 32, 2, 1, 7), (16, 32, 2, 1, 6))]


@pytest.mark.parametrize("P,B,acc,bcs,plan4,plan2", GEN_PLANS, ids=[f"P{c[0]}-B{c[1]}-acc{c[2]}-{c[3]}" for c in GEN_PLANS])
def test_general_residual_plan_case_vs_float64(backend, P, B, acc, bcs, plan4, plan2):
    L, lib, dev = _lib(backend)
    ih0, ih1 = default_geom(P)
    comps, inp, got = gen_case(backend, P, B, acc, bcs, ih0, ih1)
    assert_plan(L, comps, dev, B, P, P, bcs == "periodic", plan4)
    assert_plan(L, comps[:2], dev, B, P, P, bcs == "periodic", plan2)
    if B == 1024:
        assert plan_of(L, comps, dev, 1, P, P, False)[:4] == (8, P, 2, 1)
        for i in (0, 1023):
            one = {k: (v[i:i + 1] if k != "fs" else v) for k, v in inp.items()}
            alone = run_general(backend, comps, one, bcs, ih1)
            assert torch.equal(alone["residual"], got["residual"][i:i + 1]) and torch.equal(alone["adjoint"], got["adjoint"][i:i + 1])


def test_general_residual_is_bit_identical_run_to_run(backend):
    P, B, acc, bcs = 21, 2, 6, "none"
    ih0, ih1 = default_geom(P)
    comps, inp = gen_comps(backend, acc, bcs, ih0, ih1), make_inputs(P, B)
    a, b = run_general(backend, comps, inp, bcs, ih1), run_general(backend, comps, inp, bcs, ih1)
    assert torch.equal(a["residual"], b["residual"]) and torch.equal(a["adjoint"], b["adjoint"])
    assert not torch.isnan(a["residual"]).any() and not torch.isnan(a["adjoint"]).any()


SENTINEL = 7.5


@pytest.mark.parametrize("entry", ["fwd", "bwd"])
def test_general_guards(backend, entry):
    """Status non-zero, the message, and nothing written: every refusal happens on the host before the first launch."""
    L, lib, dev = _lib(backend)
    B, P = 2, 12
    comps = gen_comps(backend, 6, "none", *default_geom(P))
    ops, keep = _ops_array(tuple(comps), dev)
    f = lambda *s: torch.full(s, SENTINEL, device=dev)   # noqa: E731
    t = {"x0": f(B, 2, P, P), "aux": f(B, P * P, 3), "out": f(B, P * P, 3) if entry == "fwd" else f(B, 2, P, P),
         "ws": torch.full((L.pidm_darcy_general_ws(B, P),), 0x5A, dtype=torch.uint8, device=dev)}
    fn = L.pidm_darcy_residual_general_fwd if entry == "fwd" else L.pidm_darcy_residual_general_bwd

    def refused(what, null=None, B=B, P=P, ops=ops):
        a = {k: (None if k == null else ptr(v)) for k, v in t.items()}
        rc = fn(a["x0"], a["aux"], ops, 0, 1.0, a["out"], a["ws"], B, P, stream_ptr(dev))
        msg = L.pidm_last_error().decode()
        assert rc != 0 and what in msg, (rc, msg)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert (t["out"] == SENTINEL).all() and (t["ws"] == 0x5A).all()
    for name in t:
        refused("darcy_residual_general: null buffer", null=name)
    refused("null operator array", ops=None)
    refused("out of range", B=0)
    refused("out of range", P=1)
    assert max(c.min_size() for c in comps) == 10
    refused("too small", P=9)
    assert L.pidm_darcy_general_ws(0, P) == 0 and L.pidm_darcy_general_ws(B, 0) == 0


@pytest.mark.parametrize("bcs", ["none", "periodic"])
@pytest.mark.parametrize("acc", [4, 6])
def test_residuals_darcy_vs_float64(backend, acc, bcs):
    """The Python level with pixels off the boundary and d1 not reversed: spacings 1 / P both positive, bc1_sign = -1."""
    L, lib, dev = _lib(backend)
    P, B = 12, 2
    rd = ResidualsDarcy(model=None, fd_acc=acc, pixels_per_dim=P, pixels_at_boundary=False, reverse_d1=False, device=dev, bcs=bcs, lib=lib)
    assert not rd.specialised
    inp = make_inputs(P, B)
    inp["fs"] = rd._f_s_flat.cpu()
    r64, e32 = gen_reference_of(inp, acc, bcs, float(P), float(P))
    xr = inp["pred"].to(dev).requires_grad_(True)
    res = rd.compute_residual(xr, pass_through=True)["residual"]
    (gx,) = torch.autograd.grad(res, xr, inp["gr"].to(dev))
    check(f"ResidualsDarcy P={P} acc {acc} {bcs}", "residual", res, e32["residual"], r64["residual"])
    check(f"ResidualsDarcy P={P} acc {acc} {bcs}", "adjoint", gx, e32["adjoint"], r64["adjoint"])
