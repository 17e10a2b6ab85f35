"""Float64 parity of the fused optimizer kernels (csrc/k_optim.hip): pidm_clip_adam_step, pidm_clip_adam_ema_step and
pidm_ema_update through the C ABI, on the host-emulated build and on gfx950.

Reference: `step64` below, the arithmetic of k_optim.hip's header comment written out in float64 on the fp32 state the kernel sees
(step_size and bc2_sqrt formed in double).  ref32 is fp32 torch.nn.utils.clip_grad_norm_ + torch.optim.Adam with its state preloaded.

Tolerance rule (that of test_kernels_darcy_f64.py).  For a compared tensor q:  err(q) = max|q - q64| / max|q64|, and a kernel passes
when  err(kernel) <= 4 * err(ref32) + 4 * 2^-23  for m, v, p and the reported norm.  With m / sqrt(v) drawn from a random state the
largest |p| of a big buffer is far above the typical one, so p is held to the same rule a second time on the half of the
elements the float64 step moves least ("p, quieter half": the split comes from the reference alone).

Every case is ONE step from a random state (m ~ N(0, 0.1), v = 0.01 N(0,1)^2, p ~ N(0,1)): trajectories amplify the m / sqrt(v)
sensitivity at near-zero gradients that both implementations share.  lr = 0.5 in the parity cases, so that the update is the size
of p and a wrong update cannot hide under the rounding of p; one case runs the training value 1e-3.

Sizes: 1, 2, 3 (tail only), 4, 1027, 525,315 (n / 4 > 512 * 256: some threads of sqsum_partial_kernel make a second pass) and
2,098,355 (n / 4 > 2048 * 256: the same in clip_adam_kernel), the last two with a tail of 3.

The EMA shadow is compared bit for bit with `(1. - mu) * p_new + mu * shadow` evaluated by torch in fp32 on the CPU - on the gfx950
build too, where a contraction of the two products and the sum into an fma would show.

Two mutations of k_optim.hip were tried on the emulator against this module and tests/test_fused_optimizer.py:
  (e) clip_adam_kernel's stride gridDim.x * 128: elements are updated twice at every n / 4 > 128, so test_sizes_vs_float64 fails
      from n = 1027 up (525,315 and 2,098,355 included), as do the hyperparameter, learning-rate, clipping and fused-EMA tests at
      n = 1027; test_fused_optimizer.py fails too.
  (f) ema_update_kernel's tail through fmaf: test_ema_update_is_the_reference_formula_bit_for_bit[0.99] fails (the n = 3 runs are
      tail only); no test of test_fused_optimizer.py does.

Worst err(kernel) / err(ref32) per quantity over the cases of this module, the share of the bound in brackets (every test prints
its figures before it asserts; ref32 runs on the host's CPU, so its error differs a little between the two machines):

    quantity                  emulator                      MI355X
    m                         1.2e-07 / 9.5e-08 (0.14)      8.7e-08 / 9.5e-08 (0.10)      n = 1027, (0.5, 0.9, 1e-3, step 7)
    v                         1.0e-07 / 2.8e-08 (0.18)      1.0e-07 / 2.8e-08 (0.18)      n = 1
    p                         9.2e-07 / 4.0e-07 (0.44)      9.2e-07 / 9.2e-07 (0.22)      n = 1
    p, quieter half           9.2e-07 / 4.0e-07 (0.44)      9.2e-07 / 9.2e-07 (0.22)      n = 1
    norm                      5.2e-08 / 6.7e-08 (0.07)      5.2e-08 / 6.7e-08 (0.07)      n = 1027, lr = 1e-3

No quantity uses half of its bound; the largest share belongs to the single element of n = 1, where max|q64| is that element.
"""
import math

import pytest
import torch

from physicsinformeddiffusionmodels_amd._lib import ptr, stream_ptr
from tests.test_kernels_darcy_f64 import err

ULP = 2.0 ** -23
NAN = float("nan")
DEFAULT_HP = (0.9, 0.999, 1e-8, 1)
SIZES = [1, 2, 3, 4, 1027, 525315, 2098355]


def make_state(n, seed=0, gscale=1.0):
    g = torch.Generator().manual_seed(7919 * seed + n)
    return {"p": torch.randn(n, generator=g), "m": 0.1 * torch.randn(n, generator=g),
            "v": 0.01 * torch.randn(n, generator=g) ** 2, "g": gscale * torch.randn(n, generator=g),
            "s": torch.randn(n, generator=g)}


def step64(st, lr, beta1, beta2, eps, step, max_norm):
    """One clipped Adam step in float64: (p, m, v, norm)."""
    p, m, v, g = (st[k].double() for k in "pmvg")
    norm = torch.sqrt((g * g).sum())
    coef = min(max_norm / (norm.item() + 1e-6), 1.0) if max_norm > 0 else 1.0
    gj = g * coef
    m = m + (1.0 - beta1) * (gj - m)
    v = v * beta2 + (1.0 - beta2) * gj * gj
    step_size, bc2_sqrt = lr / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step)
    p = p - step_size * (m / (torch.sqrt(v) / bc2_sqrt + eps))
    return {"p": p, "m": m, "v": v, "norm": norm}


def step32(st, lr, beta1, beta2, eps, step, max_norm):
    """The two calls of the reference training loop in fp32, the optimizer state preloaded."""
    p = torch.nn.Parameter(st["p"].clone())
    p.grad = st["g"].clone()
    opt = torch.optim.Adam([p], lr=lr, betas=(beta1, beta2), eps=eps)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": st["m"].clone(), "exp_avg_sq": st["v"].clone()}
    norm = torch.nn.utils.clip_grad_norm_([p], max_norm) if max_norm > 0 else p.grad.norm()
    opt.step()
    return {"p": p.detach(), "m": opt.state[p]["exp_avg"], "v": opt.state[p]["exp_avg_sq"], "norm": norm.detach()}


def run_step(backend, st, lr, beta1, beta2, eps, step, max_norm, with_norm=True, mu=None):
    """One kernel step on copies of the state; mu: through pidm_clip_adam_ema_step with the shadow st['s']."""
    L, dev = backend
    n = st["p"].numel()
    t = {k: st[k].clone().to(dev) for k in "pmvgs"}
    norm = torch.full((1,), NAN, device=dev) if with_norm else None
    ws = torch.empty(L.pidm_clip_adam_ws_bytes(), dtype=torch.uint8, device=dev)
    if mu is None:
        L.check(L.pidm_clip_adam_step(ptr(t["p"]), ptr(t["g"]), ptr(t["m"]), ptr(t["v"]), n, lr, beta1, beta2, eps, step, max_norm,
                                      ptr(norm), ptr(ws), stream_ptr(dev)), "pidm_clip_adam_step")
    else:
        L.check(L.pidm_clip_adam_ema_step(ptr(t["p"]), ptr(t["g"]), ptr(t["m"]), ptr(t["v"]), ptr(t["s"]), n, lr, beta1, beta2, eps, step,
                                          max_norm, mu, ptr(norm), ptr(ws), stream_ptr(dev)), "pidm_clip_adam_ema_step")
    out = {k: t[k].cpu() for k in "pmvs"}
    assert torch.equal(t["g"].cpu(), st["g"])
    out["norm"] = norm.cpu()[0] if with_norm else None
    return out


def check(case, name, got, q32, q64):
    ek, e32 = err(got, q64), err(q32, q64)
    print(f"OPTIM_F64 {case} | {name}: err(kernel) {ek:.3e} err(ref32) {e32:.3e}")
    assert ek <= 4 * e32 + 4 * ULP, (case, name, ek, e32)


def check_step(case, st, got, r32, r64, norm=True):
    for k in "mvp":
        check(case, k, got[k], r32[k], r64[k])
    quiet = (r64["p"] - st["p"].double()).abs()
    quiet = quiet <= quiet.median()
    check(case, "p, quieter half", got["p"][quiet], r32["p"][quiet], r64["p"][quiet])
    if norm:
        check(case, "norm", got["norm"], r32["norm"], r64["norm"])


def parity(backend, case, n, lr, hp, max_norm, seed=0, gscale=1.0):
    beta1, beta2, eps, step = hp
    st = make_state(n, seed, gscale)
    args = (lr, beta1, beta2, eps, step, max_norm)
    got, r32, r64 = run_step(backend, st, *args), step32(st, *args), step64(st, *args)
    check_step(case, st, got, r32, r64)
    return st, got, r64


# ------------------------------------------------------------------------------------------------------------------------------
# sizes, hyperparameters, learning rate
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes_vs_float64(backend, n):
    """The gradient norm is about sqrt(n), max_norm a tenth of it: every size is clipped."""
    parity(backend, f"n={n}", n, 0.5, DEFAULT_HP, 0.1 * math.sqrt(n))


@pytest.mark.parametrize("hp", [DEFAULT_HP, (0.9, 0.999, 1e-8, 100000), (0.5, 0.9, 1e-3, 7)], ids=str)
@pytest.mark.parametrize("n", [3, 1027])
def test_hyperparameters_vs_float64(backend, n, hp):
    parity(backend, f"n={n} hp={hp}", n, 0.5, hp, 0.1 * math.sqrt(n), seed=1)


def test_training_learning_rate_vs_float64(backend):
    parity(backend, "n=1027 lr=1e-3", 1027, 1e-3, DEFAULT_HP, 1.0, seed=2)


# ------------------------------------------------------------------------------------------------------------------------------
# clipping
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 1027])
def test_clipping(backend, n):
    hp, lr = DEFAULT_HP, 0.5
    # clipped: the norm is ten times max_norm
    st, got, r64 = parity(backend, f"n={n} clipped", n, lr, hp, 1.0, seed=3, gscale=10.0 / math.sqrt(n))
    assert 3.0 < r64["norm"].item() < 30.0
    # a max_norm nothing reaches, clipping off, clipping off without a norm: one set of bits
    args = (lr,) + hp
    big, off = run_step(backend, st, *args, 1e9), run_step(backend, st, *args, -1.0)
    nonorm = run_step(backend, st, *args, -1.0, with_norm=False)
    for k in "pmv":
        assert torch.equal(big[k], off[k]) and torch.equal(nonorm[k], off[k]), k
    check_step(f"n={n} max_norm=-1", st, off, step32(st, *args, -1.0), step64(st, *args, -1.0))     # the norm is still reported
    assert torch.equal(big["norm"], off["norm"])


@pytest.mark.parametrize("n", [3, 1027])
def test_zero_gradient_from_a_zero_state_moves_nothing(backend, n):
    st = make_state(n, seed=4)
    for k in "mvg":
        st[k].zero_()
    for max_norm in (1.0, -1.0):
        got = run_step(backend, st, 0.5, *DEFAULT_HP, max_norm)
        assert torch.equal(got["p"], st["p"]) and got["norm"].item() == 0.0
        assert (got["m"] == 0).all() and (got["v"] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------
# EMA
# ------------------------------------------------------------------------------------------------------------------------------
def ema_formula(p, shadow, mu):
    """src/denoising_utils.py:176, evaluated by torch in fp32 on the CPU."""
    return (1. - mu) * p + mu * shadow


EMA_RUNS = [(3, seed) for seed in range(16)] + [(1027, 0), (525315, 0)]


@pytest.mark.parametrize("mu", [0.99, 0.9999])
def test_ema_step_equals_the_plain_step_and_the_reference_formula_bit_for_bit(backend, mu):
    for n, seed in EMA_RUNS:
        st = make_state(n, seed=seed)
        args = (0.5,) + DEFAULT_HP + (0.1 * math.sqrt(n),)
        plain, fused = run_step(backend, st, *args), run_step(backend, st, *args, mu=mu)
        for k in ("p", "m", "v", "norm"):
            assert torch.equal(plain[k], fused[k]), (n, k)
        assert torch.equal(plain["s"], st["s"])
        assert torch.equal(fused["s"], ema_formula(fused["p"], st["s"], mu)), n


@pytest.mark.parametrize("mu", [0.99, 0.9999])
def test_ema_update_is_the_reference_formula_bit_for_bit(backend, mu):
    L, dev = backend
    for n, seed in EMA_RUNS:
        st = make_state(n, seed=seed)
        p, s = st["p"].to(dev), st["s"].clone().to(dev)
        L.check(L.pidm_ema_update(ptr(s), ptr(p), n, mu, stream_ptr(dev)), "pidm_ema_update")
        assert torch.equal(p.cpu(), st["p"])
        assert torch.equal(s.cpu(), ema_formula(st["p"], st["s"], mu)), n


# ------------------------------------------------------------------------------------------------------------------------------
# guards: refused on the host, nothing written
# ------------------------------------------------------------------------------------------------------------------------------
def test_guards(backend):
    L, dev = backend
    n, st = 64, stream_ptr(dev)
    buf = {k: torch.full((n + 1,), 7.5, device=dev) for k in "pgmvs"}
    ws = torch.empty(L.pidm_clip_adam_ws_bytes(), dtype=torch.uint8, device=dev)
    hp = (1e-3, 0.9, 0.999, 1e-8, 1, 1.0)

    def refused(rc, what):
        msg = L.pidm_last_error().decode()
        assert rc != 0 and what in msg, (rc, msg)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert all((b == 7.5).all() for b in buf.values())
    for off in "pgmvs":                                                  # one buffer 4 bytes into its allocation
        a = {k: ptr(b[1:] if k == off else b[:n]) for k, b in buf.items()}
        assert buf[off][1:].data_ptr() % 16 == 4
        refused(L.pidm_clip_adam_ema_step(a["p"], a["g"], a["m"], a["v"], a["s"], n, *hp, 0.99, None, ptr(ws), st), "16-byte aligned")
        if off != "s":
            refused(L.pidm_clip_adam_step(a["p"], a["g"], a["m"], a["v"], n, *hp, None, ptr(ws), st), "16-byte aligned")
    a = {k: ptr(b[:n]) for k, b in buf.items()}
    refused(L.pidm_clip_adam_ema_step(a["p"], a["g"], a["m"], a["v"], None, n, *hp, 0.99, None, ptr(ws), st), "null shadow buffer")
    refused(L.pidm_ema_update(None, a["p"], n, 0.99, st), "ema_update: null buffer")
    refused(L.pidm_ema_update(a["s"], None, n, 0.99, st), "ema_update: null buffer")
    refused(L.pidm_ema_update(ptr(buf["s"][1:]), a["p"], n, 0.99, st), "16-byte aligned")
    refused(L.pidm_ema_update(a["s"], ptr(buf["p"][1:]), n, 0.99, st), "16-byte aligned")
