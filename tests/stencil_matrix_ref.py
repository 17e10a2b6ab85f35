"""The classed stencil operator of tests/stencil_ref.py as a torch sparse matrix, and the Darcy residual of tests/darcy_ref.py on four
such matrices (what pidm_darcy_residual_general_fwd computes for any stencil set), in float64 or float32.  The matrices serve the
sizes the explicit loops of `apply_np` are too slow for, and autograd through `S @ x` gives the adjoint.  No project imports."""
import numpy as np
import torch

from tests.stencil_ref import _cls, fp32_stencils


def operator_matrix(stencils, H, W, periodic=False, dtype=torch.float64, absolute=False):
    """The classed operator on an H x W image as a sparse [H*W, H*W] matrix S (row = output pixel i*W + j, column = the pixel a
    tap reads), assembled by the class rule of `apply_np`: the tap list of (row class, column class), taps outside the image
    dropped, or the ('C', 'C') list on wrapped indices.  Coefficients are the fp32-rounded ones, held in `dtype`; taps that land on
    one pixel (a wrap around a small image) are summed.  absolute=True: |S|, the sum of the absolute coefficients."""
    st = fp32_stencils(stencils)
    mio = max(max(abs(i), abs(j)) for (i, j) in st[('C', 'C')])
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ri = np.array([_cls(i, H, mio) for i in range(H)])[:, None].repeat(W, 1)
    cj = np.array([_cls(j, W, mio) for j in range(W)])[None, :].repeat(H, 0)
    rows, cols, vals = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
    for key in ([('C', 'C')] if periodic else list(st)):
        sel = np.ones((H, W), dtype=bool) if periodic else (ri == key[0]) & (cj == key[1])
        for (di, dj), v in st[key].items():
            ti, tj = ii[sel] + di, jj[sel] + dj
            if periodic:
                ti, tj, ok = ti % H, tj % W, slice(None)
            else:
                ok = (ti >= 0) & (ti < H) & (tj >= 0) & (tj < W)
            rows.append((ii[sel] * W + jj[sel])[ok])
            cols.append((ti * W + tj)[ok])
            vals.append(np.full(rows[-1].shape, abs(v) if absolute else v))
    idx = torch.from_numpy(np.stack([np.concatenate(rows), np.concatenate(cols)]))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(np.concatenate(vals)).to(dtype), (H * W, H * W)).coalesce()


def apply_matrix(S, x):
    """S applied to the last two axes of x (any leading axes), differentiable in x: autograd gives S^T."""
    H, W = x.shape[-2:]
    return torch.sparse.mm(S, x.reshape(-1, H * W).t()).t().reshape(x.shape)


def residual_general(x, f_s, mats, bc1_sign):
    """darcy_ref.residual for any stencil set: mats = the operators d/d0, d/d1, d2/d0^2, d2/d1^2 as sparse [P*P, P*P] matrices in
    the dtype of x; the six derivative fields are matrix products, the algebra and the (eq, bc0, bc1) layout are darcy_ref's.
    bc0 / bc1 sit on the first and last row / column whatever the matrices wrap, as in the kernel."""
    B, _, P, _ = x.shape
    p, K = x[:, 0], x[:, 1]
    S0, S1, S00, S11 = mats
    p0, p1, p00, p11 = apply_matrix(S0, p), apply_matrix(S1, p), apply_matrix(S00, p), apply_matrix(S11, p)
    K0, K1 = apply_matrix(S0, K), apply_matrix(S1, K)
    eq = (-K * p00 - K0 * p0) + (-K * p11 - K1 * p1) - f_s.reshape(P, P).to(x.dtype)
    edge = torch.zeros(P, dtype=x.dtype)        # -1 on the first row / column, +1 on the last, 0 between
    edge[0], edge[-1] = -1.0, 1.0
    bc0 = edge[:, None] * p0
    bc1 = (-bc1_sign * edge) * p1
    return torch.stack([eq, bc0, bc1], dim=-1).reshape(B, P * P, 3)
