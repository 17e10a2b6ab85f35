"""Plain-torch reference of the Darcy residual and the PIDM loss on it (what csrc/k_darcy.hip computes), in the dtype of its input.
No project imports.  x is [B,2,P,P] (channel 0 = pressure p, channel 1 = permeability K); h0 / h1 are the SIGNED grid spacings
along the rows / the columns of an image, independent of each other; f_s is any [P*P] source field.  Gradients: autograd."""
import torch


def bc1_sign_of(h1):
    """The kernels' convention: +1 when the column spacing is negative (the reference's reverse_d1), else -1."""
    return 1.0 if h1 < 0 else -1.0


def d1(a, h):
    """First derivative along the LAST axis, second order: central 3-point inside, one-sided 3-point at both edges."""
    mid = (a[..., 2:] - a[..., :-2]) * (0.5 / h)
    lo = (-1.5 * a[..., 0] + 2.0 * a[..., 1] - 0.5 * a[..., 2]) / h
    hi = (1.5 * a[..., -1] - 2.0 * a[..., -2] + 0.5 * a[..., -3]) / h
    return torch.cat([lo[..., None], mid, hi[..., None]], dim=-1)


def d2(a, h):
    """Second derivative along the LAST axis, second order: central 3-point inside, one-sided 4-point at both edges."""
    h2 = h * h
    mid = (a[..., 2:] - 2.0 * a[..., 1:-1] + a[..., :-2]) / h2
    lo = (2.0 * a[..., 0] - 5.0 * a[..., 1] + 4.0 * a[..., 2] - a[..., 3]) / h2
    hi = (2.0 * a[..., -1] - 5.0 * a[..., -2] + 4.0 * a[..., -3] - a[..., -4]) / h2
    return torch.cat([lo[..., None], mid, hi[..., None]], dim=-1)


def _rows(f, a, h):
    return f(a.transpose(-1, -2), h).transpose(-1, -2)


def residual(x, f_s, h0, h1, bc1_sign):
    """[B,2,P,P] -> [B,P*P,3] = (eq, bc0, bc1): eq = -div(K grad p) - f_s, bc0 = the outward row-direction flux condition on the
    first / last row, bc1 = bc1_sign * dp/dx1 on the first column and its negative on the last."""
    B, _, P, _ = x.shape
    p, K = x[:, 0], x[:, 1]
    p0, p00, K0 = _rows(d1, p, h0), _rows(d2, p, h0), _rows(d1, K, h0)
    p1, p11, K1 = d1(p, h1), d2(p, h1), d1(K, h1)
    eq = (-K * p00 - K0 * p0) + (-K * p11 - K1 * p1) - f_s.reshape(P, P).to(x.dtype)
    edge = torch.zeros(P, dtype=x.dtype)        # -1 on the first row / column, +1 on the last, 0 between
    edge[0], edge[-1] = -1.0, 1.0
    bc0 = edge[:, None] * p0
    bc1 = (-bc1_sign * edge) * p1
    return torch.stack([eq, bc0, bc1], dim=-1).reshape(B, P * P, 3)


def loss(x0, pred, f_s, p2w, inv_var, c_data, c_res, h0, h1, bc1_sign):
    """The training loss given the model output `pred` for the target x0, with per-sample weights p2w [B] and inverse posterior
    variances inv_var [B].  Returns (loss, c_data * data loss, mean |r|, residual)."""
    B = x0.shape[0]
    dt = pred.dtype
    res = residual(pred, f_s, h0, h1, bc1_sign)
    per = ((x0.to(dt) - pred) ** 2).reshape(B, -1).mean(dim=1)
    data = (per * p2w.to(dt)).mean() * c_data
    rl = (c_res * 0.5 * res ** 2 * inv_var.to(dt).reshape(B, 1, 1)).mean()
    return data + rl, data, res.abs().mean(), res


def jacobian_max(x, h0, h1, bc1_sign):
    """[B,2,P,P] -> [B]: the signed maximum over ALL entries of the dense Jacobian d residual[n,k] / d p[m] of each sample
    (structural zeros included), K held fixed.  f_s drops out of the derivative."""
    P = x.shape[-1]
    zero = torch.zeros(P * P, dtype=x.dtype)
    out = []
    for b in range(x.shape[0]):
        K = x[b, 1]
        J = torch.autograd.functional.jacobian(lambda p: residual(torch.stack([p, K])[None], zero, h0, h1, bc1_sign)[0], x[b, 0],
                                                vectorize=True)
        out.append(J.max())
    return torch.stack(out)
