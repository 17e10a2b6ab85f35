"""Finite-difference coefficients and stencil sets of grad_utils (host, pure Python): no native library needed."""
import itertools
import math
import os
import sys
from fractions import Fraction

import pytest

from physicsinformeddiffusionmodels_amd.grad_utils import fd_coefficients, fd_offsets, fd_stencil_set

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D0, D1 = 1.0 / 63, -1.0 / 63
OPERATORS = {"d_d0": [(0, D0, 1)], "d_d1": [(1, D1, 1)], "d_d00": [(0, D0, 2)], "d_d11": [(1, D1, 2)],
             "d_d01": [(0, D0, 1), (1, D1, 1)]}


def _shim_findiff():
    import importlib.util
    spec = importlib.util.spec_from_file_location("findiff_shim_for_test", os.path.join(REPO, "oracle", "shims", "findiff", "__init__.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.FinDiff


def _ulp_close(a, b):
    return a == b or abs(a - b) <= math.ulp(max(abs(a), abs(b)))


@pytest.mark.parametrize("name", sorted(OPERATORS))
def test_acc2_equals_the_findiff_stand_in(name):
    FinDiff = _shim_findiff()
    terms = OPERATORS[name]
    ref = (FinDiff(*terms[0], acc=2) if len(terms) == 1 else FinDiff(*terms, acc=2)).stencil((99, 99)).data
    got = fd_stencil_set(terms, 2)
    assert set(got) == set(ref) and len(got) == 9
    for key in ref:
        assert set(got[key]) == set(ref[key]), key
        for off, v in ref[key].items():
            assert _ulp_close(got[key][off], v), (key, off, got[key][off], v)


@pytest.mark.parametrize("deriv,acc,cls", list(itertools.product((1, 2), (2, 4, 6), "LCH")))
def test_stencils_differentiate_monomials_exactly(deriv, acc, cls):
    offs = fd_offsets(deriv, acc, cls)
    c = fd_coefficients(deriv, acc, cls)
    n_c = 2 * ((deriv + 1) // 2) - 1 + acc
    assert len(offs) == (n_c if cls == "C" or deriv % 2 else n_c + 1)
    assert set(c) <= set(offs) and all(v != 0.0 for v in c.values())
    scale = sum(abs(v) for v in c.values())
    for m in range(len(offs)):
        # d^deriv/dx^deriv x^m at 0 = m! [m == deriv]; the offsets are small integers, so o**m is exact in float64
        got = math.fsum(v * float(Fraction(o) ** m) for o, v in c.items())
        want = float(math.factorial(m)) if m == deriv else 0.0
        mag = math.fsum(abs(v) * abs(float(Fraction(o) ** m)) for o, v in c.items())
        assert abs(got - want) <= 1e-12 * max(mag, scale), (m, got, want)


@pytest.mark.parametrize("deriv,acc,cls", list(itertools.product((1, 2), (2, 4, 6), "LCH")))
def test_coefficients_equal_sympy_finite_diff_weights(deriv, acc, cls):
    sympy = pytest.importorskip("sympy")
    offs = fd_offsets(deriv, acc, cls)
    w = sympy.finite_diff_weights(deriv, [sympy.Integer(o) for o in offs], 0)[deriv][-1]
    c = fd_coefficients(deriv, acc, cls)
    for o, wv in zip(offs, w):
        wv = float(wv)
        if wv == 0.0:
            assert o not in c
        else:
            assert abs(c[o] - wv) <= 1e-13 * abs(wv), (o, c[o], wv)


def test_mixed_derivative_is_the_product_of_the_axis_stencils():
    st = fd_stencil_set(OPERATORS["d_d01"], 6)
    assert len(st[("C", "C")]) == 36 and len(st[("L", "L")]) == 49 and len(st[("H", "C")]) == 42
    a, b = fd_coefficients(1, 6, "L"), fd_coefficients(1, 6, "C")
    for (di, dj), v in st[("L", "C")].items():
        assert v == (a[di] / D0) * (b[dj] / D1)


def test_package_does_not_import_findiff_sympy_or_scipy():
    import subprocess
    code = ("import sys; import physicsinformeddiffusionmodels_amd.grad_utils, src.grad_utils; "
            "bad = [m for m in ('findiff', 'sympy', 'scipy') if m in sys.modules]; assert not bad, bad")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO)


def test_src_grad_utils_reexports_the_reference_names():
    import src.grad_utils as gu
    for n in ("StencilGradientComputation", "StencilGradients", "GradientsHelper", "generalized_image_to_b_xy_c",
              "generalized_b_xy_c_to_image"):
        assert hasattr(gu, n), n
    import physicsinformeddiffusionmodels_amd.unet_model as um
    assert um.generalized_image_to_b_xy_c is gu.generalized_image_to_b_xy_c
    assert um.generalized_b_xy_c_to_image is gu.generalized_b_xy_c_to_image
    ns = {}
    exec("from src.grad_utils import *", ns)        # residuals_darcy.py of the reference starts with this line
    assert "GradientsHelper" in ns and "StencilGradients" in ns
