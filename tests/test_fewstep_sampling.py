"""Few-step sampling: strided DDIM steps in p_sample_loop, p_sample_loop_guided and p_sample_loop_guided_mechanics
(DenoisingDiffusion.strided_step_coefs / sampling_timesteps) against the float64 restatement tests/fewstep_ref.py.  No kernel is
new: the three update kernels evaluate x_prev = c1 x0_hat + c2 x_t + sigma z (- g) with other host coefficients, and the tests pin
that algebra through them.  `backend` = host emulator or the gfx950 library (-m gpu).

Bounds: the loop tests keep the project's figures for a teacher-forced step, err <= 5e-5 max(|x_ref|, 1) (+ 2e-4 max|g_ref| on
guided steps), sums to 1e-4 relative (tests/test_guided_sampling.py, tests/test_guided_mechanics.py).  The coefficient identities
are float64 statements with float64 bounds.  Every test prints its figures before it asserts."""
import pytest
import torch

from oracle import pidm_oracle as O
from physicsinformeddiffusionmodels_amd._lib import PidmError
from physicsinformeddiffusionmodels_amd.denoising_utils import DenoisingDiffusion
from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
from tests import fewstep_ref as FR
from tests import guided_ref as GR
from tests import test_guided_mechanics as TM
from tests.test_guided_sampling import ZO, ZP, _loop_setup, _run

coefs = DenoisingDiffusion.strided_step_coefs


# ------------------------------------------------------------------------------------------------------------------------------
# 1. coefficient algebra (CPU, no library)
# ------------------------------------------------------------------------------------------------------------------------------
def schedule64(T):
    """the cosine schedule continued in float64 from the fp32 betas: abar = cumprod(1 - beta) holds to float64 rounding"""
    betas = DenoisingDiffusion._host_schedule(T)['betas'].double()
    alphas = 1.0 - betas
    return betas, alphas, torch.cumprod(alphas, 0)


@pytest.mark.parametrize("T", [100, 1000])
def test_consecutive_levels_with_eta_1_are_the_ancestral_posterior(T):
    """eta = 1 on (t, t-1): c1 = beta_t sqrt(p) / (1-a), c2 = (1-p) sqrt(alpha_t) / (1-a), sigma^2 = beta_t (1-p) / (1-a), to 1e-10
    absolute (measured 2.9e-15 at T = 100, 1.9e-13 at T = 1000).  This is a statement about a float64 schedule: on the engine's fp32
    tables 1 - abar_t / abar_{t-1} loses the small beta_t to the fp32 rounding of abar (measured 5.8e-6 at T = 100, 1.3e-4 at
    T = 1000), so the identity is NOT asserted there."""
    betas, alphas, ap = schedule64(T)
    worst = 0.0
    for t in range(T):
        c1, c2, sigma = coefs(ap, t, t - 1, 1.0)
        assert all(type(v) is float for v in (c1, c2, sigma))
        a, p = ap[t].item(), (ap[t - 1].item() if t > 0 else 1.0)
        b, al = betas[t].item(), alphas[t].item()
        ref = (b * p ** 0.5 / (1 - a), (1 - p) * al ** 0.5 / (1 - a), b * (1 - p) / (1 - a))
        worst = max(worst, abs(c1 - ref[0]), abs(c2 - ref[1]), abs(sigma * sigma - ref[2]))
    print(f"T={T}: worst deviation from the ancestral posterior {worst:.3e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("T", [100, 1000])
def test_eta_0_keeps_the_noise_direction(T):
    """eta = 0, any t_prev < t: a noised sample sqrt(a) x0 + sqrt(1-a) eps maps onto sqrt(p) x0 + sqrt(1-p) eps"""
    _, _, ap = schedule64(T)
    g = torch.Generator().manual_seed(T)
    worst = 0.0
    for _ in range(300):
        t = int(torch.randint(0, T, (1,), generator=g))
        t_prev = int(torch.randint(-1, t, (1,), generator=g))
        c1, c2, sigma = coefs(ap, t, t_prev, 0.0)
        a, p = ap[t].item(), (ap[t_prev].item() if t_prev >= 0 else 1.0)
        assert sigma == 0.0
        worst = max(worst, abs(c1 + c2 * a ** 0.5 - p ** 0.5), abs(c2 * (1 - a) ** 0.5 - (1 - p) ** 0.5))
    print(f"T={T}: worst deviation {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("T", [100, 1000])
def test_step_to_the_clean_sample_and_the_restatement(T):
    tabs = DenoisingDiffusion._host_schedule(T)
    for ap in (tabs['alphas_prod'], schedule64(T)[2], tabs['alphas_prod'].numpy()):
        for eta in (0, 0.5, 1):
            for t in (0, 1, T // 2, T - 1):
                assert coefs(ap, t, -1, eta) == (1.0, 0.0, 0.0)
    # the independent restatement of tests/fewstep_ref.py says the same as the product function, on the fp32 table the loops read
    ap = tabs['alphas_prod']
    g = torch.Generator().manual_seed(T + 1)
    worst = 0.0
    for _ in range(200):
        t = int(torch.randint(0, T, (1,), generator=g))
        t_prev = int(torch.randint(-1, t, (1,), generator=g))
        eta = float(torch.rand(1, generator=g))
        got, ref = coefs(ap, t, t_prev, eta), FR.step_coefs(ap.double(), t, t_prev, eta)
        worst = max(worst, *(abs(a - b.item()) for a, b in zip(got, ref)))
    print(f"T={T}: product vs restatement {worst:.3e}")
    assert worst <= 1e-12
    with pytest.raises(PidmError, match="eta"):
        coefs(ap, 5, 2, -0.1)


def test_sampling_timesteps():
    T = 100
    diff = DenoisingDiffusion(T, torch.device("cpu"))
    assert diff.sampling_steps is None and diff.sampling_eta == 0.0
    for S in (2, 7, T):
        lv = diff.sampling_timesteps(S)
        assert len(lv) == S and all(type(v) is int for v in lv)
        assert all(hi > lo for hi, lo in zip(lv, lv[1:]))
        assert lv[0] == T - 1 and lv[-1] == 0
    assert diff.sampling_timesteps(T) == list(reversed(range(T)))
    assert diff.sampling_timesteps(4) == [99, 66, 33, 0]
    assert diff.sampling_timesteps([5, 60, 99]) == [99, 60, 5]
    assert diff.sampling_timesteps((7,)) == [7]
    assert diff.sampling_timesteps(torch.tensor([0, 99])) == [99, 0]
    for bad in (1, 0, -3, T + 1, [5, 5, 60], [T], [-1, 3], [], 4.0, [3.5, 1], "12", True, object()):
        with pytest.raises(PidmError) as e:
            diff.sampling_timesteps(bad)
        assert repr(bad) in str(e.value), (bad, str(e.value))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. convergence to the probability-flow solution through the real update kernel
# ------------------------------------------------------------------------------------------------------------------------------
MU, SD = 0.7, 0.5


def test_gaussian_chain_converges_first_order(backend):
    """The model is the exact posterior mean of N(mu, s^2) data, so the eta = 0 chain integrates a linear ODE whose end point is
    known in closed form.  err(S) = max|x_final - exact|: halving the step must cut it (err(40) < 0.6 err(20); float64 numpy on
    N(0,1) draws gave 0.146 -> 0.076 at T = 100), and the engine's fp32 chain must sit on the float64 restatement's error to 1e-3
    relative: 10 x the fp32 chain error of 40 steps x 6e-8 x |x| ~ 3 over an err of at least 0.07."""
    L, dev = backend
    lib = L if dev.type == "cpu" else None
    P, B, T = 16, 2, 100
    diff = DenoisingDiffusion(T, dev, lib=lib)
    abar = diff._host_tables['alphas_prod'].double()

    def model(x_bxyc, time):
        t = int(time[0])
        x0 = FR.gaussian_posterior_mean(x_bxyc, abar[t], MU, SD)
        return x0.reshape(B, P, P, 2).permute(0, 3, 1, 2).contiguous()

    res = ResidualsDarcy(model=model, fd_acc=2, pixels_per_dim=P, pixels_at_boundary=True, reverse_d1=True, device=dev, lib=lib)
    g = torch.Generator().manual_seed(17)
    x_T = torch.randn(B, 2, P, P, generator=g)
    zs = [torch.randn(B, 2, P, P, generator=g) for _ in range(40)]
    exact = FR.gaussian_flow_endpoint(x_T, abar[T - 1], MU, SD)
    err, err_ref = {}, {}
    for S in (20, 40):
        x_seq, _ = _run(diff, dev, [x_T] + zs, lambda: diff.p_sample_loop(None, (B, 2, P, P), residual_func=res, keep_history=False,
                                                                          sampling_steps=S, eta=0.0))
        assert len(x_seq) == 1
        levels = diff.sampling_timesteps(S)
        x_ref = FR.gaussian_chain(abar, levels, x_T, MU, SD)
        err[S] = (x_seq[0].cpu().double() - exact).abs().max().item()
        err_ref[S] = (x_ref - exact).abs().max().item()
        print(f"S={S}: err {err[S]:.6e} err_ref {err_ref[S]:.6e} |err - err_ref| / err_ref {abs(err[S] - err_ref[S]) / err_ref[S]:.3e}")
    print(f"err(40) / err(20) = {err[40] / err[20]:.4f}")
    assert err[40] < 0.6 * err[20]
    for S in (20, 40):
        assert abs(err[S] - err_ref[S]) <= 1e-3 * err_ref[S], S


# ------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. teacher-forced strided Darcy chains with the dim-8 UNet
# ------------------------------------------------------------------------------------------------------------------------------
T_LOOP, S_LOOP = 100, 4
LEVELS = [99, 66, 33, 0]


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_strided_loop_teacher_forced(backend, eta):
    m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps) = _loop_setup(backend, n_steps=T_LOOP)
    (x_seq, interm), aux = _run(diff, dev, noises, lambda: diff.p_sample_loop(
        None, (B, 2, P, P), save_output=True, residual_func=res, eval_residuals=True, sampling_steps=S_LOOP, eta=eta))
    assert len(x_seq) == S_LOOP + 1 and len(interm) == S_LOOP + 1
    assert aux['timesteps'] == LEVELS and aux['residual'].shape[0] == B
    cfg = O.UnetCfg(dim=dim, channels=2)
    p64 = GR.params64(m.state_dict())
    abar = GR.tables64(n_steps)['alphas_prod']
    assert torch.equal(x_seq[0], noises[0])
    for k, (t, t_prev) in enumerate(FR.pairs(LEVELS)):
        # teacher forcing: the restatement advances the engine's own previous state
        x_ref, x0_ref = FR.plain_step_strided(p64, cfg, abar, x_seq[k], t, t_prev, noises[1 + k], eta)
        err = (x_seq[1 + k].double() - x_ref).abs().max().item()
        bound = 5e-5 * max(x_ref.abs().max().item(), 1.0)
        c = FR.step_coefs(abar, t, t_prev, eta)
        print(f"eta={eta} t={t}->{t_prev}: err {err:.3e} bound {bound:.3e} coefs {[v.item() for v in c]}")
        assert err <= bound, f"step t={t}"
        assert (interm[1 + k].double() - x0_ref).abs().max().item() <= 5e-5 * max(x0_ref.abs().max().item(), 1.0), f"step t={t}"
        assert (c[2] > 0) == (eta > 0 and t_prev >= 0)          # the noise term is live exactly where the test means it to be
    # the last step lands on its x0 estimate
    last = (x_seq[-1].double() - interm[-1].double()).abs().max().item()
    print(f"eta={eta}: |x_final - x0_hat| {last:.3e}")
    assert last <= 5e-5 * max(interm[-1].abs().max().item(), 1.0)
    # eval_residuals reports the residual of the last visited level's estimate
    r_ref = O.darcy_residual(interm[-1].double())
    assert (aux['residual'].cpu().double() - r_ref).abs().max().item() <= 1e-3 * r_ref.abs().max().item()


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_strided_guided_loop_teacher_forced(backend, eta):
    m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps) = _loop_setup(backend, n_steps=T_LOOP)
    guide_below = 50
    (x_seq, interm), aux = _run(diff, dev, noises, lambda: diff.p_sample_loop_guided(
        (B, 2, P, P), res, obs.to(dev), mask.to(dev), zeta_obs=ZO, zeta_pde=ZP, guide_below=guide_below, sampling_steps=S_LOOP, eta=eta))
    assert len(x_seq) == S_LOOP + 1 and len(interm) == S_LOOP + 1
    assert aux['guidance'].shape == (S_LOOP, B, 2) and aux['guidance'].device.type == dev.type
    assert aux['timesteps'] == LEVELS
    assert aux['residual'].shape == (B,)
    cfg = O.UnetCfg(dim=dim, channels=2)
    p64 = GR.params64(m.state_dict())
    abar = GR.tables64(n_steps)['alphas_prod']
    assert torch.equal(x_seq[0], noises[0])
    for k, (t, t_prev) in enumerate(FR.pairs(LEVELS)):
        s = aux['guidance'][k].cpu().double()
        if t >= guide_below:
            assert (s == 0).all(), f"step t={t}"
            x_ref, _ = FR.plain_step_strided(p64, cfg, abar, x_seq[k], t, t_prev, noises[1 + k], eta)
            gmax = 0.0
        else:
            x_ref, s_ref, g_ref = FR.guided_step_strided(p64, cfg, abar, x_seq[k], t, t_prev, noises[1 + k], eta, obs, mask, ZO, ZP)
            gmax = g_ref.abs().max().item()
            assert gmax > 0
            print("sums", s.tolist(), "ref", s_ref.tolist())
            assert ((s - s_ref).abs() <= 1e-4 * s_ref.abs()).all(), f"step t={t}"
        err = (x_seq[1 + k].double() - x_ref).abs().max().item()
        bound = 5e-5 * max(x_ref.abs().max().item(), 1.0) + 2e-4 * gmax
        print(f"eta={eta} t={t}->{t_prev}: err {err:.3e} bound {bound:.3e} |g| {gmax:.3e}")
        assert err <= bound, f"step t={t}"
    r_ref = O.darcy_residual(x_seq[-1].double()).abs().mean(dim=(1, 2))
    assert ((aux['residual'].cpu().double() - r_ref).abs() <= 1e-4 * r_ref).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 5. guided mechanics, strided
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("fewstep_mech_meshes")


def test_strided_guided_mechanics_loop_teacher_forced(backend, mesh_dir):
    S, eta = 3, 0.5
    m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, n_steps) = TM._loop_setup(backend, mesh_dir, n_steps=T_LOOP)
    nn = nel + 1
    levels = [99, 50, 0]                                # linspace(0, 99, 3) = 0, 49.5, 99; 49.5 rounds to even
    (x_seq, interm), aux = TM._run(dev, noises, lambda: diff.p_sample_loop_guided_mechanics(
        (cond.to(dev), bcs.to(dev)), (B, 3, nn, nn), res, obs.to(dev), mask.to(dev), *TM.ZETAS, sampling_steps=S, eta=eta))
    assert len(x_seq) == S + 1 and len(interm) == S + 1
    assert aux['guidance'].shape == (S, B, 3) and aux['timesteps'] == levels
    cfg = O.UnetCfg(dim=dim, channels=10, out_dim=3, sigmoid_last_channel=True)
    p64 = GR.params64(m.state_dict())
    abar = GR.tables64(n_steps)['alphas_prod']
    kloc, ed = TM.tables(res)
    assert torch.equal(x_seq[0], noises[0])
    for k, (t, t_prev) in enumerate(FR.pairs(levels)):
        x_ref, s_ref, g_ref = FR.guided_mech_step_strided(p64, cfg, abar, x_seq[k], cond, bcs, t, t_prev, noises[1 + k], eta, obs, mask,
                                                          TM.ZETAS, kloc, ed)
        err = (x_seq[1 + k].double() - x_ref).abs().max().item()
        bound = 5e-5 * max(x_ref.abs().max().item(), 1.0) + 2e-4 * g_ref.abs().max().item()
        print(f"t={t}->{t_prev}: err {err:.3e} bound {bound:.3e} |g| {g_ref.abs().max().item():.3e} |x| {x_ref.abs().max().item():.3e}")
        s = aux['guidance'][k].cpu().double()
        print("sums", s.tolist(), "ref", s_ref.tolist())
        assert g_ref.abs().max().item() > 0
        assert err <= bound, f"step t={t}"
        assert ((s - s_ref).abs() <= 1e-4 * s_ref.abs()).all(), f"step t={t}"
    r_ref = TM.final_residual_ref(x_seq[-1].double(), bcs, kloc, ed)
    print("final mean |r|", aux['residual'].tolist(), "ref", r_ref.tolist())
    assert ((aux['residual'].cpu().double() - r_ref).abs() <= 1e-4 * r_ref).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 6. bookkeeping
# ------------------------------------------------------------------------------------------------------------------------------
def test_instance_attributes_are_the_keyword_defaults(backend):
    m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps) = _loop_setup(backend, n_steps=T_LOOP)
    shape = (B, 2, P, P)
    by_kw, _ = _run(diff, dev, noises, lambda: diff.p_sample_loop(None, shape, residual_func=res, keep_history=False,
                                                                  sampling_steps=3, eta=0.5))
    diff.sampling_steps, diff.sampling_eta = 3, 0.5
    by_attr, _ = _run(diff, dev, noises, lambda: diff.p_sample_loop(None, shape, residual_func=res, keep_history=False))
    assert torch.equal(by_kw[0], by_attr[0])
    for bad in (dict(sampling_steps=1), dict(sampling_steps=[3, 3]), dict(sampling_steps=4, eta=-0.5)):
        with pytest.raises(PidmError):
            diff.p_sample_loop(None, shape, residual_func=res, keep_history=False, **bad)


def test_guided_loop_reads_the_instance_attributes_too(backend):
    """... and a keyword wins over them; an explicit list of levels ends at its lowest level (guide_below = 10: one guided step per
    run keeps this quick on the emulator)"""
    m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps) = _loop_setup(backend, n_steps=T_LOOP)
    shape = (B, 2, P, P)
    guided = lambda **kw: _run(diff, dev, noises, lambda: diff.p_sample_loop_guided(
        shape, res, obs.to(dev), mask.to(dev), zeta_obs=ZO, zeta_pde=ZP, guide_below=10, keep_history=False, **kw))
    diff.sampling_steps, diff.sampling_eta = [5, 60], 0.5
    (g_attr, _), aux = guided()
    assert aux['timesteps'] == [60, 5] and aux['guidance'].shape == (2, B, 2)
    assert (aux['guidance'][0] == 0).all() and (aux['guidance'][1] > 0).all()
    diff.sampling_steps, diff.sampling_eta = 50, 0.0
    (g_kw, _), aux_kw = guided(sampling_steps=(60, 5), eta=0.5)
    assert torch.equal(g_kw[0], g_attr[0]) and torch.equal(aux_kw['guidance'], aux['guidance'])
    for bad in (dict(sampling_steps=1), dict(sampling_steps=[3, 3]), dict(sampling_steps=4, eta=-0.5)):
        with pytest.raises(PidmError):
            diff.p_sample_loop_guided(shape, res, obs.to(dev), mask.to(dev), **bad)


def test_n_correction_counts_on_the_visited_levels(backend):
    m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps) = _loop_setup(backend, n_steps=T_LOOP)
    calls = []
    inner = res.residual_correction

    def counting(x):
        calls.append(tuple(x.shape))
        return inner(x)

    res.residual_correction = counting
    (x_seq, _), aux = _run(diff, dev, noises, lambda: diff.p_sample_loop(
        None, (B, 2, P, P), save_output=True, residual_func=res, N_correction=40, correction_mode='x0', sampling_steps=S_LOOP))
    # the visited levels below 40 are 33 and 0
    assert len(calls) == 2, calls
    assert len(x_seq) == S_LOOP + 1 and aux['timesteps'] == LEVELS and 'residual' in aux


def test_eta_does_not_change_what_the_generator_is_asked_for(backend):
    L, dev = backend
    m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps) = _loop_setup(backend, n_steps=T_LOOP)
    state = (lambda: torch.cuda.get_rng_state(dev)) if dev.type == "cuda" else torch.get_rng_state
    after, finals = [], []
    for eta in (0.0, 0.5):
        torch.manual_seed(1234)
        x_seq, _ = diff.p_sample_loop(None, (B, 2, P, P), residual_func=res, keep_history=False, sampling_steps=3, eta=eta)
        after.append(state())
        finals.append(x_seq[0].cpu())
    assert torch.equal(after[0], after[1])
    assert not torch.equal(finals[0], finals[1])        # eta = 0.5 did use its draws
    torch.manual_seed(1234)
    torch.randn((B, 2, P, P), device=dev)
    for _ in range(3):
        torch.randn((B, 2, P, P), device=dev)
    ref_state = state()
    assert torch.equal(after[0], ref_state)             # the initial noise + one tensor per visited level, nothing else
