"""Plain numpy (float64, explicit loops over pixels and taps) restatement of a classed stencil operator, for the tests of the
stencil engine: the operator itself, the operator with absolute coefficients (error bounds), and their transposes."""
import numpy as np

U = 2.0 ** -24      # unit roundoff of fp32


def fp32_stencils(stencils):
    """The dictionary with its values rounded to fp32 (what the device table and the reference's conv kernels hold)."""
    return {k: {o: float(np.float32(v)) for o, v in st.items()} for k, st in stencils.items()}


def longest_list(stencils, periodic):
    return len(stencils[('C', 'C')]) if periodic else max(len(st) for st in stencils.values())


def _cls(i, n, mio):
    return 'L' if i < mio else ('H' if i >= n - mio else 'C')


def apply_np(stencils, x, periodic=False, absolute=False, transpose=False):
    """y = S x (or S^T x) on the last two axes of x, in float64; absolute=True: |S| applied to |x|."""
    x = np.asarray(x, dtype=np.float64)
    if absolute:
        x = np.abs(x)
    H, W = x.shape[-2:]
    mio = max(max(abs(i), abs(j)) for (i, j) in stencils[('C', 'C')])
    y = np.zeros_like(x)
    for i in range(H):
        for j in range(W):
            key = ('C', 'C') if periodic else (_cls(i, H, mio), _cls(j, W, mio))
            for (di, dj), v in stencils[key].items():
                v = abs(v) if absolute else v
                ii, jj = i + di, j + dj
                if periodic:
                    ii, jj = ii % H, jj % W
                elif not (0 <= ii < H and 0 <= jj < W):
                    continue
                if transpose:
                    y[..., ii, jj] += v * x[..., i, j]
                else:
                    y[..., i, j] += v * x[..., ii, jj]
    return y
