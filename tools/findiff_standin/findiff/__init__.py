"""Stand-in for findiff >= 0.10 with what the reference's data generator (src/darcy_data_generation.py) uses: FinDiff(axis, h,
order, acc=2) applied to arrays and as a sparse matrix, Coef(array) * FinDiff, and sums / differences of such terms.
acc=2 only, with the SURVEY 8(c) coefficients (central in the interior, one-sided 3 / 4 points at the edges).
Used by tools/make_golden_darcy_data.py on the CPU only; nothing in the package imports it."""
import numpy as np
import scipy.sparse as sp

_C = {1: {"C": [-0.5, 0.0, 0.5], "L": [-1.5, 2.0, -0.5], "H": [0.5, -2.0, 1.5]},
      2: {"C": [1.0, -2.0, 1.0], "L": [2.0, -5.0, 4.0, -1.0], "H": [-1.0, 4.0, -5.0, 2.0]}}


def _d1(n, h, order):
    c = _C[order]
    M = np.zeros((n, n))
    M[0, :len(c["L"])] = c["L"]
    M[-1, n - len(c["H"]):] = c["H"]
    for i in range(1, n - 1):
        M[i, i - 1:i + 2] = c["C"]
    return M / h ** order


class _Op:
    def __init__(self, terms):
        self.terms = terms          # list of (coef array or scalar, axis, h, order)

    def matrix(self, shape):
        n = int(np.prod(shape))
        out = sp.csr_matrix((n, n))
        for coef, axis, h, order in self.terms:
            mats = [sp.identity(s, format="csr") for s in shape]
            mats[axis] = sp.csr_matrix(_d1(shape[axis], h, order))
            M = mats[0]
            for m in mats[1:]:
                M = sp.kron(M, m, format="csr")
            c = np.broadcast_to(np.asarray(coef, dtype=float), shape).reshape(-1)
            out = out + sp.diags(c) @ M
        return out

    def __call__(self, f):
        return (self.matrix(f.shape) @ f.reshape(-1)).reshape(f.shape)

    def __add__(self, o):
        return _Op(self.terms + o.terms)

    def __sub__(self, o):
        return _Op(self.terms + [(-np.asarray(c, dtype=float), a, h, k) for c, a, h, k in o.terms])

    def __neg__(self):
        return _Op([(-np.asarray(c, dtype=float), a, h, k) for c, a, h, k in self.terms])


class FinDiff(_Op):
    def __init__(self, axis, h, order, acc=2):
        assert acc == 2, "stand-in restates acc=2 only"
        super().__init__([(1.0, axis, h, order)])


class Coef:
    def __init__(self, value):
        self.value = np.asarray(value, dtype=float)

    def __mul__(self, op):
        return _Op([(self.value * c, a, h, k) for c, a, h, k in op.terms])
