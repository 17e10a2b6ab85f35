"""Dense float64 NumPy restatement of one three-field SIMP step (simp_step_filtered_kernel, csrc/k_mech_gen.hip), for
tests/test_mechanics_data_generation_filtered.py.  TEST INFRASTRUCTURE: the mesh, the dense solve and the `perturb=` convention are
tests/simp_ref.py's; the density filter, the tanh projection, the chain rule and the fixed-count bisection on the volume of the
physical density are the kernel's."""
import numpy as np

from tests.simp_ref import oc_update


def _window(nel, rmin):
    """(dy, dx, h, element slices, neighbour slices) of every window offset with h = rmin - dist > 0."""
    win = int(np.ceil(rmin)) - 1
    for dy in range(-win, win + 1):
        for dx in range(-win, win + 1):
            h = rmin - np.sqrt(float(dy * dy + dx * dx))
            if h <= 0:
                continue
            ys, xs = slice(max(0, -dy), nel - max(0, dy)), slice(max(0, -dx), nel - max(0, dx))      # elements e with e + d inside
            yn, xn = slice(max(0, dy), nel - max(0, -dy)), slice(max(0, dx), nel - max(0, -dx))      # their neighbours e + d
            yield h, (ys, xs), (yn, xn)


def apply_H(nel, v, rmin):
    """(H v, Hs) of the element field v [E]: H_ej = max(0, rmin - dist(e, j)), clipped at the domain edge."""
    v = v.reshape(nel, nel)
    num, den = np.zeros((nel, nel)), np.zeros((nel, nel))
    for h, e, n in _window(nel, rmin):
        num[e] += h * v[n]
        den[e] += h
    return num.reshape(-1), den.reshape(-1)


def project(xt, mode, beta, eta):
    """(x^, dx^/dx~) of the filtered density x~."""
    if mode == "density":
        return xt, np.ones_like(xt)
    den = np.tanh(beta * eta) + np.tanh(beta * (1.0 - eta))
    return (np.tanh(beta * eta) + np.tanh(beta * (xt - eta))) / den, beta / (np.cosh(beta * (xt - eta)) ** 2 * den)


def physical(mesh, x, mode, beta, eta, rmin=1.5):
    num, hs = apply_H(mesh.nel, x, rmin)
    return project(num / hs, mode, beta, eta)[0]


def simp_step(mesh, x, bcs_b, vf, mode, beta=1., eta=0.5, penal=3., e_min=1e-3, rmin=1.5, move=0.2, n_bisect=60, perturb=None):
    """One step of one sample in float64.  x [E] design variables, mode 'density' or 'heaviside'.  perturb = (rng, scale) as in
    simp_ref.simp_step."""
    x = np.asarray(x, dtype=np.float64)
    num, hs = apply_H(mesh.nel, x, rmin)
    xp, d = project(num / hs, mode, beta, eta)
    Evec = e_min + xp ** penal * (1.0 - e_min)
    u = mesh.solve(Evec, bcs_b)
    if perturb is not None:
        rng, scale = perturb
        u = u * (1.0 + scale * rng.standard_normal(u.shape))
    ue = u[mesh.elem_dofs]
    ce = np.einsum("ea,ab,eb->e", ue, mesh.kloc, ue)
    c = float((Evec * ce).sum())
    g = -penal * xp ** (penal - 1.0) * (1.0 - e_min) * np.maximum(ce, 0.0)
    dc = apply_H(mesh.nel, g * (d / hs), rmin)[0]
    dv = apply_H(mesh.nel, d / hs, rmin)[0]
    ratio = dc / dv
    l1, l2 = 0.0, 1e9
    for _ in range(n_bisect):
        lmid = 0.5 * (l1 + l2)
        x_new = oc_update(x, ratio, lmid, move)
        x_phys = physical(mesh, x_new, mode, beta, eta, rmin)
        if x_phys.mean() > vf:
            l1 = lmid
        else:
            l2 = lmid
    return dict(x=x_new, x_phys=x_phys, u=u, compliance=c, change=float(np.abs(x_new - x).max()))
