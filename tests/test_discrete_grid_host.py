"""Host: generation on the discrete DDPM grid (schedule='scaled_linear' with config.timestep_spacing) — the integer grid against the
numpy restatements of diffusers' two spacings, the step scalars against fp64 in abar form, `sample` / `invert` / `invert_ddpm` /
`counterfactual` in eager torch on a tiny foreign module against loops written here in fp64, and the cosine grid's bytes.  No GPU.

Measured on the CPU (this file prints them):
  scalars      worst relative error of a step coefficient against the fp64 abar form, over both spacings, n in {4, 50}, N in {40, 1000},
               from_t in {1, 0.5}: 3.84e-6 (the upward DDIM pass 0 -> 249 under eps, N = 1000, n = 4).  The source is the fp32 rounding
               of the log-SNR table: a coefficient like k2 = -alpha_s expm1(-h) inherits the absolute error of lam (|lam| 2^-24, about
               4e-7 at |lam| = 7) relative to its own size.  SCALAR_BOUND = 1.6e-5 is 4 x the measured value, for other platforms' libm.
  sample       fp32 against the fp64 loop, inputs x 3: 7.5e-7 .. 6.8e-5 at scales 3 .. 185, at most 3.7e-7 x scale (bound 2.4e-6 ..
               2.9e-6 x scale, derived in the test)
  invert       DDIM inversion then decode, cfg_w = 0, from_t = 0.5: max |back - x| 4.8e-1 at 10 steps, 3.6e-2 at 50
  invert_ddpm  the decode under invert_class against the inversion's latents, worst step 7.2e-7 at |latents| up to 10.4
"""
import contextlib
import copy
import io
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import discrete as DG
from diffusion_classifier_amd import solver as S
from diffusion_classifier_amd import trajectory as TJ
import draws_fixture
from test_ddpm_invert_host import TOL_DECODE
from test_sd_unet_host import _ref_schedule

SCALAR_BOUND = 1.6e-5
NS = (1, 2, 4, 5, 8, 10, 20, 25, 40, 50, 100, 125, 200, 250, 500)


def _hip_dc(**over):
    """The small HIP UNet on the host (nothing runs): for the grid and the refusals."""
    return draws_fixture.classifier(over.pop("schedule", "scaled_linear"), **over)


# ------------------------------------------------------------------------------------------------ 1. the grid
@pytest.mark.parametrize("n", NS)
def test_grid_at_from_t_1_is_the_two_published_spacings(n):
    N = 1000
    dc = _hip_dc(sampling_steps=n, timestep_spacing="trailing")
    ks = TJ.discrete_steps(dc, 1.0)
    assert all(isinstance(k, int) for k in ks) and len(ks) == n + 1 and ks[-1] == 0
    assert ks[:n] == (np.round(np.arange(N, 0, -N / n)) - 1).astype(np.int64).tolist()
    dl = _hip_dc(sampling_steps=n, timestep_spacing="leading", steps_offset=1)
    kl = TJ.discrete_steps(dl, 1.0)
    assert kl[:n] == ((np.arange(n) * (N // n))[::-1] + 1).astype(np.int64).tolist() and kl[-1] == 0 and len(kl) == n + 1


@pytest.mark.parametrize("spacing, off", [("trailing", 0), ("leading", 1)])
@pytest.mark.parametrize("from_t", [0.3, 0.5, 0.999])
def test_grid_below_from_t_1_and_the_inversion_grid_is_its_reverse(from_t, spacing, off):
    for n in (1, 4, 50):
        dc = _hip_dc(sampling_steps=n, timestep_spacing=spacing, steps_offset=off)
        ks = TJ.discrete_steps(dc, from_t)
        assert ks[0] <= int(dc.ddpm_step(from_t)) and ks[-1] == 0 and len(ks) == n + 1
        assert all(a > b for a, b in zip(ks, ks[1:]))
        down, up = TJ.grid(dc, from_t, 0.0), TJ.grid(dc, 0.0, from_t)
        assert down.steps == ks and up.steps == ks[::-1]
        assert [float(v) for v in down.label] == [float(k) for k in ks] and all(v.dtype == torch.float32 and v.dim() == 0 for v in down.label)
        assert all(torch.equal(l, dc.ddpm_logsnr[k]) and l.dim() == 0 for l, k in zip(down.lam, ks))
        assert all(torch.equal(a, b) for a, b in zip(up.lam, down.lam[::-1]))
        assert all(torch.equal(a, b) for a, b in zip(S.grid_lams(dc, from_t, 0.0), down.lam))
    if spacing == "trailing":
        assert TJ.discrete_steps(_hip_dc(sampling_steps=4, timestep_spacing=spacing), from_t)[0] == int(dc.ddpm_step(from_t))


def test_impossible_grids_and_keys_raise_value_errors_before_any_draw():
    x, lab = torch.zeros(2, 3, 32, 32), torch.tensor([0, 1])
    calls = lambda dc, t: (lambda: dc.sample(x, lab, t), lambda: dc.counterfactual(x, None, t), lambda: dc.invert(x, lab, t),      # noqa: E731
                           lambda: dc.invert_ddpm(x, lab, t))
    dc = _hip_dc(train_timesteps=10, sampling_steps=8, timestep_spacing="trailing")
    dl = _hip_dc(sampling_steps=4, timestep_spacing="leading")                       # offset 0: k_{n-1} = 0 = k_n
    torch.manual_seed(5)
    first = torch.rand(1)
    torch.manual_seed(5)
    for call in calls(dc, 0.5):
        with pytest.raises(ValueError, match=r"sampling_steps = 8.*from_t = 0\.5.*N = 10.*'trailing'"):
            call()
    for call in calls(dl, 1.0):
        with pytest.raises(ValueError, match=r"sampling_steps = 4.*from_t = 1\.0.*N = 1000.*'leading'.*steps_offset = 0"):
            call()
    assert torch.equal(first, torch.rand(1))
    with pytest.raises(ValueError, match="sampling_steps"):                          # k_0 = 3 * 250 + 300 > N - 1
        TJ.discrete_steps(_hip_dc(sampling_steps=4, timestep_spacing="leading", steps_offset=300), 1.0)
    with pytest.raises(ValueError, match="timestep_spacing"):
        _hip_dc(timestep_spacing="linspace")
    for schedule in ("cosine", "shifted_cosine"):
        with pytest.raises(ValueError, match="timestep_spacing"):
            _hip_dc(schedule=schedule, timestep_spacing="trailing")
    with pytest.raises(ValueError, match="steps_offset"):
        _hip_dc(timestep_spacing="leading", steps_offset=1.5)


def test_without_the_key_the_entry_points_name_it():
    dc = _hip_dc(sampling_steps=4)
    x = torch.zeros(2, 3, 32, 32)
    for call in (lambda: dc.sample(x, torch.tensor([0, 1])), lambda: dc.counterfactual(x), lambda: dc.invert(x), lambda: dc.invert_ddpm(x)):
        with pytest.raises(NotImplementedError, match=r"scaled_linear.*timestep_spacing"):
            call()


def test_steps_offset_is_read_from_the_scheduler_file_and_the_config_wins(tmp_path):
    import json
    (tmp_path / "scheduler_config.json").write_text(json.dumps(dict(beta_schedule="scaled_linear", steps_offset=1, timestep_spacing="leading")))
    assert _hip_dc(scheduler_path=str(tmp_path)).steps_offset == 1 and _hip_dc().steps_offset == 0
    assert _hip_dc(scheduler_path=str(tmp_path), steps_offset=2).steps_offset == 2
    assert _hip_dc(scheduler_path=str(tmp_path)).timestep_spacing is None          # the spacing is the config's choice alone


def test_a_hip_backbone_refuses_latents_that_are_not_its_plans_extent():
    """`_feed` writes x into a buffer sized for config.sample_size: any other extent is an error before the first launch (no GPU needed
    to be told so)."""
    from diffusion_classifier_amd import _lib as L
    bb = _hip_dc().ema.ema_model                                               # 3 channels at 32x32
    for shape in ((1, 3, 16, 16), (1, 3, 64, 64), (1, 3, 32, 16), (1, 4, 32, 32)):
        with pytest.raises(L.DcamdError, match="sample_size"):
            bb._feed(None, torch.zeros(shape), 0.0)


# ------------------------------------------------------------------------------------------------ 2. the scalars
def _abar(N):
    return [1.0 / (1.0 + math.exp(-l)) for l in _ref_schedule(N)]


def _coefficients64(ab_t, ab_s, ab_p=None):
    """fp64, abar form -> {name: (coefficient of z, coefficient of the prediction)} of one step t -> s for eps and v, the posterior
    variance, and the 2M history weight (ab_p: abar of the point before t)."""
    at, st, as_, ss = math.sqrt(ab_t), math.sqrt(1 - ab_t), math.sqrt(ab_s), math.sqrt(1 - ab_s)
    # x0 = (z - st e) / at  |  at z - st v
    x_eps, x_v = (1 / at, -st / at), (at, -st)
    # DDIM: z_s = as x0 + ss (z - at x0) / st
    ddim = lambda x: (as_ * x[0] + ss * (1 - at * x[0]) / st, as_ * x[1] + ss * (-at * x[1]) / st)      # noqa: E731
    beta = 1 - ab_t / ab_s
    a, b = math.sqrt(ab_t / ab_s) * (1 - ab_s) / (1 - ab_t), as_ * beta / (1 - ab_t)
    ddpm = lambda x: (a + b * x[0], b * x[1])                                                          # noqa: E731
    out = {"ddim_eps": ddim(x_eps), "ddim_v": ddim(x_v), "ddpm_eps": ddpm(x_eps), "ddpm_v": ddpm(x_v),
           "var": ((1 - ab_s) / (1 - ab_t) * beta,)}
    if ab_p is not None:
        lam = lambda ab: math.log(ab / (1 - ab))                                                       # noqa: E731
        out["k3"] = (0.5 * (lam(ab_s) - lam(ab_t)) / (lam(ab_t) - lam(ab_p)),)
    return out


def _coefficients32(sc, ps, k3):
    """The same from the product's fp32 scalars (Python floats), combined in fp64."""
    alpha_t, sigma_t, k1, k2 = sc[:4]
    _, _, a, b, sd = ps
    x_eps, x_v = (1 / alpha_t, -sigma_t / alpha_t), (alpha_t, -sigma_t)
    out = {"ddim_eps": (k1 + k2 * x_eps[0], k2 * x_eps[1]), "ddim_v": (k1 + k2 * x_v[0], k2 * x_v[1]),
           "ddpm_eps": (a + b * x_eps[0], b * x_eps[1]), "ddpm_v": (a + b * x_v[0], b * x_v[1]), "var": (sd * sd,)}
    if k3 is not None:
        out["k3"] = (k3,)
    return out


def test_step_scalars_against_fp64_in_abar_form():
    worst, where = 0.0, None
    for N in (40, 1000):
        abar = _abar(N)
        for spacing, off in (("trailing", 0), ("leading", 1)):
            for n in (4, 50):
                if n > N // 2:
                    continue                                                   # 50 steps do not fit 40 train steps
                for from_t in (1.0, 0.5):
                    if spacing == "leading" and (int(from_t * N) // n) < 1:
                        continue
                    dc = _hip_dc(train_timesteps=N, sampling_steps=n, timestep_spacing=spacing, steps_offset=off)
                    g = TJ.grid(dc, from_t, 0.0)
                    ks = g.steps
                    inv = S.step_scalars(g.lam, "ddim", "denoise", clip=False)
                    two = S.step_scalars(g.lam, "dpmpp_2m", "denoise", clip=False)
                    assert len(inv) == len(two) == n and inv[-1][2:] == (0.0, 1.0, None, False) and not any(sc[5] for sc in inv + two)
                    full = S.step_scalars(g.lam, "ddim", "invert")              # first order throughout: the scalars of every step
                    up = S.step_scalars(g.lam[::-1], "ddim", "invert")
                    for i in range(n):
                        ps = DG.posterior_scalars(g.lam[i], g.lam[i + 1])
                        k3 = two[i][4]
                        assert (k3 is not None) == (1 <= i <= n - 2)
                        assert i == n - 1 or inv[i][:4] == full[i][:4] == two[i][:4]
                        want = _coefficients64(abar[ks[i]], abar[ks[i + 1]], abar[ks[i - 1]] if k3 is not None else None)
                        got = _coefficients32(full[i], ps, k3)
                        # the upward pass over the same pair of points: t and s swap
                        want["up_eps"], want["up_v"] = (_coefficients64(abar[ks[i + 1]], abar[ks[i]])[k] for k in ("ddim_eps", "ddim_v"))
                        u = _coefficients32(up[n - 1 - i], ps, None)
                        got["up_eps"], got["up_v"] = u["ddim_eps"], u["ddim_v"]
                        for name, vals in want.items():
                            for w64, g32 in zip(vals, got[name]):
                                rel = abs(g32 - w64) / abs(w64)
                                if rel > worst:
                                    worst, where = rel, (N, spacing, n, from_t, i, name)
    print(f"fp32 step scalars against the fp64 abar form: worst relative error {worst:.2e} at {where} (bound {SCALAR_BOUND:g})")
    assert worst < SCALAR_BOUND, (worst, where)


# ------------------------------------------------------------------------------------------------ 3. eager generation, a foreign module
class LabelNet(nn.Module):
    """Linear in x; the gain depends on the context and on the time input, so a wrong label moves the output; records what it is fed."""

    def __init__(self, ch=3, hid=4, freq=0.37):
        super().__init__()
        self.freq = freq
        self.config = SimpleNamespace(encoder_hid_dim=hid)
        self.mix = nn.Parameter(torch.randn(ch, ch) * 0.4)
        self.lin = nn.Linear(hid, ch)
        self.seen, self.seen_x = [], []

    def forward(self, x, noise_labels, encoder_hidden_states=None):
        self.seen.append(noise_labels.detach().clone())
        self.seen_x.append(x.detach().clone())
        t = noise_labels.to(x.dtype).reshape(-1, 1).expand(x.shape[0], 1)
        gain = 0.5 + 0.3 * torch.tanh(self.lin(encoder_hidden_states[:, 0])) + 0.2 * torch.cos(self.freq * t)
        return torch.einsum("oc,bchw->bohw", self.mix, x) * gain[:, :, None, None]


def _dc(N=1000, n=4, spacing="trailing", pred_param="eps", sampler=None, cfg_w=1.5, seed=3, freq=0.37):
    torch.manual_seed(seed)
    cfg = dict(pred_param=pred_param, schedule="scaled_linear", noise_d=8, image_size=8, cfg_w=cfg_w, ema_beta=0.999, ema_warmup=0,
               ema_update_freq=1, encoder_type="nn", classes=3, n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2,
               sampling_steps=n, train_timesteps=N, timestep_spacing=spacing, steps_offset=int(spacing == "leading"), sampler=sampler)
    with contextlib.redirect_stdout(io.StringIO()):
        return dca.DiffusionClassifier(LabelNet(freq=freq), dca.Config(**cfg))


def _net(dc):
    return dc.ema.ema_model


def _forget(dc):
    _net(dc).seen.clear()
    _net(dc).seen_x.clear()


def _sample64(dc, x, lab, from_t, sampler, e0, draws, label_of=float):
    """`sample` in fp64 from the abar table: the start, then the sampler's passes written in abar form -> (result, the largest
    magnitude the loop handled)."""
    N, w, v = dc.train_timesteps, dc.cfg_w, dc.pred_param == "v"
    abar = _abar(N)
    ks = TJ.discrete_steps(dc, from_t)
    n = len(ks) - 1
    net = copy.deepcopy(_net(dc)).double()
    cond = dc.encoder(lab).unsqueeze(1).double()
    null = dc.encoder(torch.full_like(lab, dc.null_token)).unsqueeze(1).double()
    z = e0.double() if from_t == 1 else math.sqrt(abar[ks[0]]) * x.double() + math.sqrt(1 - abar[ks[0]]) * e0.double()
    scale = float(z.abs().max())

    def x0_of(z, k):
        t = torch.tensor([label_of(k)], dtype=torch.float64)
        pr = (1 + w) * net(z, t, cond) - w * net(z, t, null)
        at, st = math.sqrt(abar[k]), math.sqrt(1 - abar[k])
        return at * z - st * pr if v else (z - st * pr) / at

    x_prev = h_prev = None
    passes = n + 1 if sampler == "ddpm" else n
    for p in net.parameters():
        p.requires_grad_(False)
    for i in range(passes):
        kt, ks_ = (ks[i], ks[i + 1]) if i < n else (ks[n - 1], ks[n])
        ab_t, ab_s = abar[kt], abar[ks_]
        x0 = x0_of(z, kt)
        scale = max(scale, float(x0.abs().max()))
        if sampler == "ddpm":
            beta = 1 - ab_t / ab_s
            mu = math.sqrt(ab_t / ab_s) * (1 - ab_s) / (1 - ab_t) * z + math.sqrt(ab_s) * beta / (1 - ab_t) * x0
            z = mu if i == n else mu + math.sqrt((1 - ab_s) / (1 - ab_t) * beta) * draws[i].double()
        elif i == n - 1:
            z = x0                                                             # the last deterministic pass: the data prediction
        else:
            D = x0
            h = 0.5 * (math.log(ab_s / (1 - ab_s)) - math.log(ab_t / (1 - ab_t)))
            if sampler == "dpmpp_2m" and i >= 1:
                D = x0 + 0.5 * h / h_prev * (x0 - x_prev)
            if sampler == "ddim":
                z = math.sqrt(ab_s) * x0 + math.sqrt(1 - ab_s) * (z - math.sqrt(ab_t) * x0) / math.sqrt(1 - ab_t)
            else:
                z = math.sqrt((1 - ab_s) / (1 - ab_t)) * z - math.sqrt(ab_s) * math.expm1(-h) * D
            x_prev, h_prev = x0, h
        scale = max(scale, float(z.abs().max()))
    return z, scale


@pytest.mark.parametrize("pred_param", ["eps", "v"])
@pytest.mark.parametrize("spacing", ["trailing", "leading"])
@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp_2m"])
def test_sample_equals_the_fp64_loop_feeds_the_steps_and_clips_nothing(sampler, spacing, pred_param):
    """Bound, relative to `scale`, the largest magnitude the fp64 loop handles.  (a) The log-SNR table is fp32: |lam| < 8, so a lam is
    off by at most 8 x 2^-24 = 2^-21; alpha and sigma move by at most half of that relatively, a pass reads two lams, so what a pass
    adds to z is off by at most 2^-21 x scale — systematic, it adds up over the passes.  (SCALAR_BOUND is a RELATIVE bound on
    coefficients that cancel, such as k2 at near-adjacent steps; their absolute error is this one.)  (b) A pass rounds about 16 times
    at 2^-24 (the guidance mix, the data prediction, the update, a 3-channel mix) with unrelated signs: sqrt(16 passes) x 2^-24.  The
    module is a contraction (|mix| gain < 1), so earlier errors are not amplified beyond the 1 / alpha_t <= 15 (eps) that `scale` holds.
    bound = (passes x 2^-21 + sqrt(16 passes) x 2^-24) x scale, 2.9e-6 x scale at 5 passes; measured: at most 3.7e-7 x scale."""
    n = 4
    for N, from_t in ((1000, 1.0), (40, 0.5)):
        dc = _dc(N=N, n=n, spacing=spacing, pred_param=pred_param, sampler=sampler)
        x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1)) * 3
        lab = torch.tensor([2, 0])
        _forget(dc)
        torch.manual_seed(9)
        got = dc.sample(x, lab, from_t=from_t)
        torch.manual_seed(9)
        e0 = torch.randn(x.shape) if from_t == 1 else torch.randn_like(x)
        draws = [torch.randn_like(x) for _ in range(n)]
        ks = TJ.discrete_steps(dc, from_t)
        passes = n + 1 if sampler == "ddpm" else n
        fed = [ks[min(i, n - 1)] for i in range(passes)]
        seen = _net(dc).seen
        assert len(seen) == 2 * passes and all(s.dtype == torch.float32 and s.tolist() == [float(fed[i // 2])] for i, s in enumerate(seen)), seen
        want, scale = _sample64(dc, x, lab, from_t, sampler, e0, draws)
        bound = (passes * 2.0 ** -21 + math.sqrt(16 * passes) * 2.0 ** -24) * scale
        d = float((got.double() - want).abs().max())
        print(f"{sampler} {spacing} {pred_param} N={N} from_t={from_t}: steps {ks}, |got - fp64| {d:.2e} (bound {bound:.2e}, scale {scale:.1f}), "
              f"|got|.max {float(got.abs().max()):.2f}")
        assert got.dtype == torch.float32 and d <= bound, (d, bound)
        assert float(got.abs().max()) > 1.0                                    # nothing was clipped to [-1, 1]
        # the time input steers: a module fed the log-SNR in place of the step gives another result, far outside the bound
        lam_of = lambda k: float(dc.ddpm_logsnr[k])                            # noqa: E731
        far = float((_sample64(dc, x, lab, from_t, sampler, e0, draws, label_of=lam_of)[0] - want).abs().max())
        assert far > 10 * bound, (far, bound)


def test_ddim_inversion_then_decode_comes_closer_with_more_steps():
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(2)) * 3
    lab = torch.tensor([1, 2])
    err = {}
    for n in (10, 50):
        dc = _dc(n=n, sampler="ddim", cfg_w=0.0, freq=0.004)                   # smooth in the step: an ODE a solver can converge on
        _forget(dc)
        z = dc.invert(x, lab, 0.5)
        ks = TJ.discrete_steps(dc, 0.5)
        assert [s.tolist() for s in _net(dc).seen] == [[float(k)] for k in ks[::-1][:n] for _ in range(2)]      # upwards: k_n = 0 first
        back = S.decode_eager(dc, z, lab, 0.5, "ddim")
        err[n] = float((back - x).abs().max())
        assert float(z.abs().max()) > 1.0 and float(back.abs().max()) > 1.0
    print(f"invert then decode, ddim, cfg_w = 0, from_t = 0.5: max |back - x| at 10 steps {err[10]:.3e}, at 50 steps {err[50]:.3e}")
    assert err[50] < err[10]


# ------------------------------------------------------------------------------------------------ 4. invert_ddpm there and back
@pytest.mark.parametrize("pred_param", ["eps", "v"])
@pytest.mark.parametrize("spacing", ["trailing", "leading"])
def test_ddpm_inversion_decodes_back_step_by_step(spacing, pred_param):
    """Under invert_class the ancestral decode of `counterfactual(start="ddpm_invert")` is fed, pass after pass, the latents the
    inversion drew: the module records its inputs.  Bound: TOL_DECODE of tests/test_ddpm_invert_host.py (the cosine case, whose
    latents lie in [-1, 1] after the clip) times max(1, |latents|.max()), since the unclipped latents of x 3 inputs are larger."""
    n = 4
    dc = _dc(N=40, n=n, spacing=spacing, pred_param=pred_param)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(4)) * 3
    c0, cl = torch.tensor([1, 2]), torch.tensor([[1, 0], [2, 1]])
    g = TJ.grid(dc, 0.5, 0.0)
    torch.manual_seed(21)
    draws = [torch.randn_like(x) for _ in range(n + 1)]
    lat = [torch.sqrt(torch.sigmoid(l)) * x + torch.sqrt(torch.sigmoid(-l)) * e for l, e in zip(g.lam, draws)]
    torch.manual_seed(21)
    inv = dc.invert_ddpm(x, c0, 0.5)
    assert torch.equal(inv.start, lat[0]) and tuple(inv.noise.shape) == (n,) + tuple(x.shape) and torch.isfinite(inv.noise).all()
    _forget(dc)
    torch.manual_seed(21)
    cf = dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=c0)
    net = _net(dc)
    assert len(net.seen) == 2 * n + (n + 1) * 2 * 2                            # the inversion, then n + 1 passes x K = 2 x (cond, null)
    assert [s.tolist() for s in net.seen[:2 * n]] == [[float(k)] for k in g.steps[:n] for _ in range(2)]
    decode_x, decode_k = net.seen_x[2 * n:], net.seen[2 * n:]
    scale = max(1.0, max(float(v.abs().max()) for v in lat))
    worst = 0.0
    for i in range(n + 1):
        own, other = decode_x[4 * i], decode_x[4 * i + 2]                      # column 0 (the inversion's class), column 1
        assert all(s.tolist() == [float(g.steps[min(i, n - 1)])] for s in decode_k[4 * i:4 * i + 4])
        worst = max(worst, float((own - lat[i]).abs().max()))
        assert i == 0 or float((other - lat[i]).abs().max()) > 100 * TOL_DECODE * scale      # another class leaves the path
    print(f"{spacing} {pred_param}: decode under invert_class against the inversion's latents, worst step {worst:.2e} "
          f"(bound {TOL_DECODE * scale:.2e}, |latents|.max {scale:.2f})")
    assert worst <= TOL_DECODE * scale
    assert float(cf.maps[:, 1].max()) > 0 and tuple(cf.samples.shape) == (2, 2, 3, 8, 8) and float(cf.samples.abs().max()) > 1.0
    # the own-class sample is the last pass, the unclipped mean, on the last latent
    cond, null, _ = TJ.contexts(dc, c0, x.device, net)
    lab_n = g.label[n - 1].unsqueeze(0)
    mu = DG.mean_eager(dc, lat[n], net(lat[n], lab_n, cond), net(lat[n], lab_n, null), DG.posterior_scalars(g.lam[n - 1], g.lam[n]), dc.cfg_w)
    assert float((cf.samples[:, 0] - mu).abs().max()) <= TOL_DECODE * scale


def test_counterfactual_is_k_reseeded_samples_on_every_sampler():
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(6)) * 3
    for sampler in ("ddpm", "ddim", "dpmpp_2m"):
        dc = _dc(N=40, sampler=sampler)
        torch.manual_seed(8)
        cf = dc.counterfactual(x, None, 0.5)
        for k in range(3):
            torch.manual_seed(8)
            assert torch.equal(dc.sample(x, torch.full((2,), k), from_t=0.5), cf.samples[:, k])
    inv = dc.counterfactual(x, None, 0.5, start="invert", invert_class=torch.tensor([0, 1]))      # dpmpp_2m decode of a DDIM inversion
    z = dc.invert(x, torch.tensor([0, 1]), 0.5)
    assert torch.equal(inv.samples[:, 2], S.decode_eager(dc, z, torch.tensor([2, 2]), 0.5, "dpmpp_2m"))


# ------------------------------------------------------------------------------------------------ 5. the cosine schedules
@pytest.mark.parametrize("schedule", ["cosine", "shifted_cosine"])
def test_cosine_grid_labels_are_the_lambdas(schedule):
    dc = _hip_dc(schedule=schedule, sampling_steps=7)
    for a, b in ((0.5, 0.0), (0.0, 0.7), (1.0, 0.0)):
        g = TJ.grid(dc, a, b)
        pts = torch.linspace(a, b, 8)
        assert g.steps is None and g.label is g.lam and len(g.lam) == 8
        assert all(g.label[i] is g.lam[i] and torch.equal(g.lam[i], dc.schedule(pts[i])) and g.lam[i].dim() == 0 for i in range(8))
        assert all(torch.equal(u, v) for u, v in zip(S.grid_lams(dc, a, b), g.lam))
