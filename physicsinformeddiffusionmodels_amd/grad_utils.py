"""Numerics helper layer: mirror of reference `src/grad_utils.py` on the gfx950 stencil engine (csrc/k_stencil.hip).

Same public names and signatures (`StencilGradientComputation`, `StencilGradients`, `GradientsHelper`, the two `generalized_*`
converters).  The nine depthwise convolutions + nine slice scatters of the reference's `StencilGradientComputation.forward`
(src/grad_utils.py:64-146) are ONE launch of `pidm_stencil_apply` for up to five operators, its autograd adjoint is ONE launch of
`pidm_stencil_apply_adjoint` (a gather: no atomics, bit-identical run to run).  No CPU fallback, no findiff / sympy / scipy: the
finite-difference coefficients are computed here (`fd_coefficients`, `fd_stencil_set`).
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn as nn

from ._lib import PidmError, StencilOp, get_lib, ptr, stream_ptr

__all__ = ['generalized_image_to_b_xy_c', 'generalized_b_xy_c_to_image', 'fd_coefficients', 'fd_stencil_set',
           'StencilGradientComputation', 'StencilGradients', 'GradientsHelper', 'stencil_apply']

_CLASSES = 'LCH'
MAX_OPS = 5          # operators per launch (PIDM_STENCIL_MAX_OPS)
MAX_TAPS = 49        # taps per position class (the order-6 mixed derivative is 7 x 7)
TABLE_HEADER = 24    # int32 words in front of the (di, dj, coefficient) triples


def generalized_image_to_b_xy_c(tensor):
    """[B, c..., X, Y] -> [B, X*Y, c...]  (reference: src/grad_utils.py:9-15)."""
    nd = tensor.dim()
    perm = [0, nd - 2, nd - 1] + list(range(1, nd - 2))
    t = tensor.permute(*perm)
    return t.reshape(t.shape[0], t.shape[1] * t.shape[2], *t.shape[3:])


def generalized_b_xy_c_to_image(tensor, pixels_x=None, pixels_y=None):
    """[B, X*Y, c...] -> [B, c..., X, Y]  (reference: src/grad_utils.py:17-25)."""
    if pixels_x is None or pixels_y is None:
        pixels_x = pixels_y = int(math.sqrt(tensor.shape[1]))
    t = tensor.reshape(tensor.shape[0], pixels_x, pixels_y, *tensor.shape[2:])
    nd = t.dim()
    perm = [0] + list(range(3, nd)) + [1, 2]
    return t.permute(*perm)


# --------------------------------------------------------------------------------------------------------------------------
# finite-difference coefficients (what the reference takes from findiff: src/grad_utils.py:154-159)
# --------------------------------------------------------------------------------------------------------------------------
def fd_offsets(deriv, acc, cls):
    """Offsets of the `acc`-th order stencil of the `deriv`-th derivative in position class `cls` (findiff's rule): central
    n_c = 2*floor((deriv+1)/2) - 1 + acc points; one-sided n_c points for odd `deriv`, n_c + 1 for even `deriv`."""
    if deriv not in (1, 2) or acc not in (2, 4, 6) or cls not in _CLASSES:
        raise ValueError(f'fd_coefficients: deriv in (1, 2), acc in (2, 4, 6), cls in L/C/H (got {deriv}, {acc}, {cls!r})')
    n_c = 2 * ((deriv + 1) // 2) - 1 + acc
    if cls == 'C':
        return list(range(-(n_c // 2), n_c // 2 + 1))
    n = n_c if deriv % 2 else n_c + 1
    return [k if cls == 'L' else -k for k in range(n)]


def _fd_weights_exact(offsets, deriv):
    """Rational weights c_k with sum_k c_k o_k^m = m! [m == deriv], m = 0 .. n-1 (unique for distinct offsets)."""
    n = len(offsets)
    A = [[Fraction(o) ** m for o in offsets] + [Fraction(math.factorial(m) if m == deriv else 0)] for m in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if A[r][c] != 0)
        A[c], A[piv] = A[piv], A[c]
        A[c] = [v / A[c][c] for v in A[c]]
        for r in range(n):
            if r != c and A[r][c] != 0:
                A[r] = [a - A[r][c] * b for a, b in zip(A[r], A[c])]
    return [A[r][n] for r in range(n)]


def fd_coefficients(deriv, acc, cls):
    """{offset: coefficient} at unit spacing; exact rational solve rounded once to float64; zero coefficients are dropped."""
    offs = fd_offsets(deriv, acc, cls)
    return {o: float(w) for o, w in zip(offs, _fd_weights_exact(offs, deriv)) if w != 0}


def fd_stencil_set(terms, acc):
    """What findiff's `FinDiff(*terms, acc=acc).stencil(shape).data` returns for a 2-D grid: {(row class, column class):
    {(di, dj): value}} with `terms = [(axis, h, deriv), ...]`, each axis term divided by h**deriv, the product over the axes
    (float64)."""
    terms = [tuple(t) for t in terms]
    data = {}
    for key in itertools.product(_CLASSES, repeat=2):
        per_axis = [{0: 1.0}, {0: 1.0}]
        for axis, h, deriv in terms:
            per_axis[axis] = {o: v / (h ** deriv) for o, v in fd_coefficients(deriv, acc, key[axis]).items()}
        st = {}
        for (oi, vi), (oj, vj) in itertools.product(per_axis[0].items(), per_axis[1].items()):
            val = vi * vj
            if val != 0.0:
                st[(oi, oj)] = st.get((oi, oj), 0.0) + val
        data[key] = st
    return data


# --------------------------------------------------------------------------------------------------------------------------
# classed stencil operators on the device
# --------------------------------------------------------------------------------------------------------------------------
def _lib_for(lib, t):
    if lib is None:
        if not t.is_cuda:
            raise PidmError('grad_utils needs tensors on an MI355X: the gfx950 stencil kernels have no CPU fallback')
        lib = get_lib()
    return lib


def _collapse_images(x):
    """View of x [..., H, W] as N images with ONE image stride (in elements), copying only when the strides do not allow it."""
    H, W = x.shape[-2:]
    if x.stride(-1) != 1 or x.stride(-2) != W:
        x = x.contiguous()
    lead = [(n, s) for n, s in zip(x.shape[:-2], x.stride()[:-2]) if n != 1]
    for (_, s0), (n1, s1) in zip(lead[:-1], lead[1:]):
        if s0 != n1 * s1:
            x = x.contiguous()
            return x, H * W
    return x, (lead[-1][1] if lead else H * W)


def _ops_array(comps, device):
    arr = (StencilOp * len(comps))()
    keep = []
    for k, c in enumerate(comps):
        tab = c.table_on(device)
        keep.append(tab)
        arr[k].table, arr[k].mio, arr[k].max_offset, arr[k].ntaps = tab.data_ptr(), c.max_inner_offset, c.max_offset, c.ntaps
    return arr, keep


def _check_fit(comps, periodic, H, W):
    for c in comps:
        need = c.min_size(periodic)
        if H < need or W < need:
            raise ValueError(f'a {H} x {W} image is too small for this stencil set (needs at least {need} pixels per axis: '
                             f'max_inner_offset={c.max_inner_offset}, max_offset={c.max_offset}, periodic={periodic})')


class _StencilApplyFn(torch.autograd.Function):
    """(y_1 .. y_K) = (S_1 x .. S_K x) in one launch; backward gx = sum_k S_k^T g_k in one launch."""

    @staticmethod
    def forward(ctx, x, comps, periodic, lib, stacked):
        xs, xstride = _collapse_images(x.float())
        H, W = x.shape[-2:]
        N = x.numel() // (H * W) if H * W else 0
        K = len(comps)
        if stacked:     # [.., K, H, W]: the operators' outputs interleaved per image (compute_jacobian_finite_diff)
            out = torch.empty(*x.shape[:-2], K, H, W, dtype=torch.float32, device=x.device)
            outs = [out[..., k, :, :] for k in range(K)]
            ostride = K * H * W
        else:
            outs = [torch.empty(x.shape, dtype=torch.float32, device=x.device) for _ in range(K)]
            ostride = H * W
        if N:
            ops, keep = _ops_array(comps, x.device)
            optr = (C.c_void_p * K)(*[o.data_ptr() for o in outs])
            lib.check(lib.pidm_stencil_apply(ptr(xs), xstride, ops, optr, K, ostride, N, H, W, int(periodic), stream_ptr(x.device)),
                      'pidm_stencil_apply')
        ctx.meta = (comps, periodic, lib, stacked, x.shape, x.dtype)
        if stacked:
            return out
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        comps, periodic, lib, stacked, shape, dtype = ctx.meta
        H, W = shape[-2:]
        if stacked:
            g = grads[0].float().contiguous()
            gs = [g[..., k, :, :] for k in range(len(comps))]
            gstride = len(comps) * H * W
            use = list(comps)
        else:
            pairs = [(c, g) for c, g in zip(comps, grads) if g is not None]
            if not pairs:
                return None, None, None, None, None
            use = [c for c, _ in pairs]
            gs = [g.float().contiguous() for _, g in pairs]
            gstride = H * W
        dev = gs[0].device
        gx = torch.empty(shape, dtype=torch.float32, device=dev)
        N = gx.numel() // (H * W) if H * W else 0
        if N:
            ops, keep = _ops_array(use, dev)
            gptr = (C.c_void_p * len(use))(*[g.data_ptr() for g in gs])
            lib.check(lib.pidm_stencil_apply_adjoint(gptr, gstride, ops, len(use), None, 0, ptr(gx), H * W, N, H, W, int(periodic),
                                               stream_ptr(dev)), 'pidm_stencil_apply_adjoint')
        return gx.to(dtype), None, None, None, None


def stencil_apply(x, comps, periodic=False, lib=None, stacked=False):
    """Apply 1..5 `StencilGradientComputation` operators to x [B, *channels, H, W] (any strides) in one launch.  Returns a tuple of
    tensors shaped like x, or with `stacked=True` one tensor [B, *channels, K, H, W]."""
    comps = tuple(comps)
    if not 1 <= len(comps) <= MAX_OPS:
        raise ValueError(f'1 to {MAX_OPS} operators per launch (got {len(comps)})')
    if x.dim() < 2:
        raise ValueError('stencil operators act on the last two axes of an image tensor')
    lib = _lib_for(lib or comps[0]._lib, x)
    _check_fit(comps, periodic, x.shape[-2], x.shape[-1])
    return _StencilApplyFn.apply(x, comps, bool(periodic), lib, bool(stacked))


class StencilGradientComputation(nn.Module):
    """One classed stencil operator (reference: src/grad_utils.py:27-146).

    `stencils` is a findiff-shaped dictionary {(row class, column class): {(di, dj): value}} over 'L', 'C', 'H' - users can hand
    in their own.  A pixel (i, j) of an H x W image has row class L if i < max_inner_offset, H if i >= H - max_inner_offset, else
    C (columns alike with W); its value is the sum over the taps of its class.  That one rule is the reference's interior
    convolution plus its eight boundary convolutions in their overwrite order.  `periodic=True` uses the ('C', 'C') list on wrapped
    indices.  Coefficients are rounded to fp32 when the device table is built, which is where the reference rounds them.

    Sizes the operator does not fit (H or W < max(2*max_inner_offset, max_inner_offset + max_offset), or smaller than the central
    width when periodic) raise ValueError: the reference silently differentiates its zero padding there.
    """

    def __init__(self, stencils, periodic=False, device='cpu', lib=None):
        super().__init__()
        self.stencils = {tuple(k): dict(v) for k, v in stencils.items()}
        if ('C', 'C') not in self.stencils:
            raise ValueError("a stencil set needs its ('C', 'C') entry")
        self.max_inner_offset = 0
        self.max_offset = 0
        for key, st in self.stencils.items():
            if len(key) != 2 or key[0] not in _CLASSES or key[1] not in _CLASSES:
                raise ValueError(f'unknown position class {key!r}')
            if len(st) > MAX_TAPS:
                raise ValueError(f'{len(st)} taps in class {key}: the kernels take up to {MAX_TAPS}')
            for (i, j) in st:
                if key == ('C', 'C'):
                    self.max_inner_offset = max(self.max_inner_offset, abs(i), abs(j))
                else:
                    self.max_offset = max(self.max_offset, abs(i), abs(j))
        self.max_inner_kernel_size = 2 * self.max_inner_offset + 1
        self.max_kernel_size = 2 * self.max_offset + 1
        self.periodic = periodic
        self._lib = lib
        # device table: 9 x (first tap, taps) in class order LL LC LH CL CC CH HL HC HH, then (di, dj, fp32 bits) per tap
        words = [0] * TABLE_HEADER
        taps = []
        for c, key in enumerate(itertools.product(_CLASSES, repeat=2)):
            st = self.stencils.get(key, {})
            words[2 * c], words[2 * c + 1] = len(taps) // 3, len(st)
            for (di, dj), v in st.items():
                taps += [int(di), int(dj), int(np.float32(v).view(np.int32))]
        self.ntaps = len(taps) // 3
        words[18], words[19], words[20] = self.max_inner_offset, self.max_offset, self.ntaps
        self._table_host = torch.from_numpy(np.asarray(words + taps, dtype=np.int64).astype(np.int32))
        self._tables = {}
        self.table_on(torch.device(device))

    def table_on(self, device):
        device = torch.device(device)
        key = (device.type, device.index)
        if key not in self._tables:
            self._tables[key] = self._table_host.to(device)
        return self._tables[key]

    def min_size(self, periodic=None):
        periodic = self.periodic if periodic is None else periodic
        if periodic:
            return self.max_inner_kernel_size
        return max(2 * self.max_inner_offset, self.max_inner_offset + self.max_offset, 1)

    def forward(self, x):
        return stencil_apply(x, (self,), self.periodic, self._lib)[0]


class StencilGradients(nn.Module):
    """First / second / mixed derivatives of images at accuracy order 2, 4 or 6 (reference: src/grad_utils.py:148-175)."""

    MODES = ('d_d0', 'd_d1', 'd_d00', 'd_d11', 'd_d01')

    def __init__(self, d0=1, d1=1, fd_acc=2, periodic=False, device='cpu', lib=None):
        super().__init__()
        if fd_acc not in (2, 4, 6):
            raise NotImplementedError(f'fd_acc={fd_acc}: the coefficient generator covers orders 2, 4 and 6')
        self.periodic = periodic
        self.fd_acc = fd_acc
        self._lib = lib
        mk = lambda terms: StencilGradientComputation(fd_stencil_set(terms, fd_acc), periodic, device, lib)  # noqa: E731
        self.d_d0 = mk([(0, d0, 1)])
        self.d_d1 = mk([(1, d1, 1)])
        self.d_d00 = mk([(0, d0, 2)])
        self.d_d11 = mk([(1, d1, 2)])
        self.d_d01 = mk([(0, d0, 1), (1, d1, 1)])

    def forward(self, x, mode):
        if mode == 'all':
            return stencil_apply(x, [getattr(self, m) for m in self.MODES], self.periodic, self._lib)
        if mode in self.MODES:
            return getattr(self, mode)(x)
        raise NotImplementedError


class GradientsHelper:
    """Reference: src/grad_utils.py:177-291.  The numeric / autograd Jacobian and Hessian helpers wrap a user function and are
    plain torch, as in the reference; `compute_jacobian_finite_diff` is one stencil launch that writes the stacked result."""

    def __init__(self, d0, d1, fd_acc, periodic=False, device='cpu', eps=1e-6, lib=None):
        self.eps = eps
        self.stencil_gradients = StencilGradients(d0=d0, d1=d1, fd_acc=fd_acc, periodic=periodic, device=device, lib=lib)

    def compute_jacobian_num(self, func, branch_in, input, aux=False):
        input = input.clone().detach().requires_grad_(False)
        input_dim = input.shape[1]
        first = func(branch_in, input)
        jacobian = torch.zeros(*(first[0] if aux else first).shape, input_dim, device=branch_in.device)
        for i in range(input_dim):
            perturb = torch.zeros_like(input)
            perturb[:, i] = self.eps
            plus, minus = func(branch_in, input + perturb), func(branch_in, input - perturb)
            if aux:
                plus, minus = plus[0], minus[0]
            jacobian[..., i] = (plus - minus) / (2 * self.eps)
        if aux:
            return (jacobian, *first[1:])
        return jacobian

    def compute_hessian_num(self, func, input, branch_in):
        if self.eps < 1e-6:
            print('WARNING: Epsilon too small. Hessian computation may be unstable.')
        input_dim = input.shape[1]
        output = func(branch_in, input)
        hessian = torch.zeros(*output.shape, input_dim, input_dim, device=input.device)
        for i in range(input_dim):
            for j in range(input_dim):
                in_i, in_j, in_ij = input.clone(), input.clone(), input.clone()
                in_i[:, i] += self.eps
                in_j[:, j] += self.eps
                in_ij[:, i] += self.eps
                in_ij[:, j] += self.eps
                hessian[..., i, j] = (func(branch_in, in_ij) - func(branch_in, in_i) - func(branch_in, in_j) + output) / self.eps ** 2
        return hessian

    def compute_jacobian_finite_diff(self, tensor, aux=False):
        """[B, *channels, H, W] -> [B, *channels, 2, H, W] (d/d0, d/d1 before the pixel axes)."""
        if tensor.ndim < 4:
            raise ValueError('Tensor must be at least 4-dimensional. We expect an image-based representation as input!')
        sg = self.stencil_gradients
        jacobian = stencil_apply(tensor, (sg.d_d0, sg.d_d1), sg.periodic, sg._lib, stacked=True)
        if aux:
            return jacobian, tensor
        return jacobian

    def compute_jacobian_autograd(self, func, branch_in, trunk_in, aux=False, arg_grad=1, batched=False, mode='rev'):
        from torch.func import jacfwd, jacrev, vmap
        if mode == 'rev':
            ag_mode = jacrev
        elif mode == 'fwd':
            ag_mode = jacfwd
        else:
            raise ValueError('Unknown differentiation mode.')
        if batched:
            jacobian = vmap(vmap(ag_mode(func, argnums=arg_grad, has_aux=aux), in_dims=(0, None)), in_dims=(None, 0), out_dims=1)
        else:
            jacobian = ag_mode(func, argnums=arg_grad, has_aux=aux)
        return jacobian(branch_in, trunk_in)

    def compute_hessian_autograd(self, func, branch_in, trunk_in, arg_grad, batched=False):
        from torch.func import jacfwd, jacrev, vmap
        if batched:
            batch_hessian = vmap(vmap(jacfwd(jacrev(func, argnums=arg_grad), argnums=arg_grad), in_dims=(0, None)),
                                 in_dims=(None, 0), out_dims=1)
            return batch_hessian(branch_in, trunk_in).squeeze(2, 3)
        return jacfwd(jacrev(func, argnums=arg_grad), argnums=arg_grad)(branch_in, trunk_in)
