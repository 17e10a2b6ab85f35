"""Stand-in for findiff >= 0.10 at acc 2, 4 and 6, with what the reference's data generator (src/darcy_data_generation.py) uses:
FinDiff(axis, h, order, acc=...) applied to arrays and as a sparse matrix, Coef(array) * FinDiff, and sums / differences of such
terms.  The sibling tools/findiff_standin restates acc=2 only; this one takes its coefficients from the project's own statement of
findiff's rule (grad_utils.fd_offsets / fd_coefficients: rows i < acc/2 forward, rows i > n-1-acc/2 backward, the others central)
and builds dense 1-D matrices by class, then Kronecker products.  Parity with the real findiff is unpinned, as for
oracle/shims/findiff.  Used by tools/make_golden_darcy_data_acc.py on the CPU only; nothing in the package imports it."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
from physicsinformeddiffusionmodels_amd.grad_utils import fd_coefficients  # noqa: E402


def _d1(n, h, order, acc):
    mio = acc // 2
    M = np.zeros((n, n))
    for i in range(n):
        cls = "L" if i < mio else ("H" if i > n - 1 - mio else "C")
        for o, w in fd_coefficients(order, acc, cls).items():
            M[i, i + o] = w
    return M / h ** order


class _Op:
    def __init__(self, terms):
        self.terms = terms          # list of (coef array or scalar, axis, h, order, acc)

    def matrix(self, shape):
        n = int(np.prod(shape))
        out = sp.csr_matrix((n, n))
        for coef, axis, h, order, acc in self.terms:
            mats = [sp.identity(s, format="csr") for s in shape]
            mats[axis] = sp.csr_matrix(_d1(shape[axis], h, order, acc))
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
        return _Op(self.terms + [(-np.asarray(c, dtype=float), *rest) for c, *rest in o.terms])

    def __neg__(self):
        return _Op([(-np.asarray(c, dtype=float), *rest) for c, *rest in self.terms])


class FinDiff(_Op):
    def __init__(self, axis, h, order, acc=2):
        assert acc in (2, 4, 6), "stand-in restates acc 2, 4, 6"
        super().__init__([(1.0, axis, h, order, acc)])


class Coef:
    def __init__(self, value):
        self.value = np.asarray(value, dtype=float)

    def __mul__(self, op):
        return _Op([(self.value * c, *rest) for c, *rest in op.terms])
