"""Host: config.variance = "learned" (the learned-range ancestral step) — the refusals of the key, the step scalars against an independent
fp64 evaluation, the eager step kind on a small foreign module that returns eps and a variance interpolation against fp64 loops
(tests/learned_var_oracle.py), and the argument checks of the two extended entries.  No GPU.

Measured on the CPU (this file prints them):
  scalars      log_hi / log_lo against fp64: at most 5.1e-8 relative (bound 2^-23 = 1.19e-7), neighbouring steps k -> k - 1 included
  sample       fp32 against the fp64 loop, n = 3: 1.7e-6 .. 3.4e-5 at scales 3.4 .. 52 (bounds 8.1e-6 .. 1.2e-4), 1.1e-3 at scale 3113
               (eps from pure noise at k = 999, where 1 / alpha_t = 157; bound 7.4e-3); the fixed-variance fp64 loop is 0.3 .. 17 away
  invert_ddpm  (noise[i] - fp64) * deviation 1.8e-6 (bound 1.3e-5); the decode under invert_class against the inversion's latents,
               worst step 7.1e-7, the last mean 1.1e-6 (bound 5.4e-5)
"""
import contextlib
import copy
import ctypes as C
import io
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import diffusion_classifier_amd as dca
import learned_var_oracle as LV
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import ancestral as AN
from diffusion_classifier_amd import trajectory as TJ
from test_ddpm_invert_host import TOL_DECODE, TOL_NOISE


class VarNet(nn.Module):
    """A foreign module with learned-variance outputs: C eps channels, linear in x with a gain that depends on the context and the
    step, then C variance channels in (-1.5, 1.5); records what it is fed."""

    def __init__(self, ch=3, hid=4, out=None, freq=0.37):
        super().__init__()
        self.freq = freq
        self.config = SimpleNamespace(encoder_hid_dim=hid, in_channels=ch, out_channels=2 * ch if out is None else out)
        self.mix = nn.Parameter(torch.randn(ch, ch) * 0.4)
        self.vmix = nn.Parameter(torch.randn(ch, ch) * 0.3)
        self.lin = nn.Linear(hid, ch)
        self.vlin = nn.Linear(hid, ch)
        self.seen, self.seen_x = [], []

    def forward(self, x, noise_labels, encoder_hidden_states=None):
        self.seen.append(noise_labels.detach().clone())
        self.seen_x.append(x.detach().clone())
        t = noise_labels.to(x.dtype).reshape(-1, 1).expand(x.shape[0], 1)
        ctx = encoder_hidden_states[:, 0]
        gain = 0.5 + 0.3 * torch.tanh(self.lin(ctx)) + 0.2 * torch.cos(self.freq * t)
        eps = torch.einsum("oc,bchw->bohw", self.mix, x) * gain[:, :, None, None]
        v = 1.5 * torch.tanh(torch.einsum("oc,bchw->bohw", self.vmix, x) + self.vlin(ctx)[:, :, None, None] + torch.sin(self.freq * t)[:, :, None, None])
        return torch.cat([eps, v], dim=1)[:, :self.config.out_channels]


def _dc(N=1000, n=3, spacing="trailing", pred_param="eps", variance="learned", seed=3, schedule="ddpm_linear", net=None, **over):
    torch.manual_seed(seed)
    cfg = dict(pred_param=pred_param, schedule=schedule, noise_d=8, image_size=8, cfg_w=1.5, ema_beta=0.999, ema_warmup=0,
               ema_update_freq=1, encoder_type="nn", classes=3, n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2,
               sampling_steps=n, train_timesteps=N, timestep_spacing=spacing, steps_offset=int(spacing == "leading"))
    if variance != "unset":
        cfg["variance"] = variance
    cfg.update(over)
    with contextlib.redirect_stdout(io.StringIO()):
        return dca.DiffusionClassifier(VarNet() if net is None else net, dca.Config(**cfg))


def _net64(dc):
    """The classifier's module in fp64 as the oracle loops' net(z, k, labels): labels are class ids, encoded by the classifier's table."""
    net = copy.deepcopy(dc.ema.ema_model).double().requires_grad_(False)
    table = dc.encoder.weight.detach().double()

    @torch.no_grad()
    def call(z, k, lab):
        return net(z, torch.tensor([float(k)], dtype=torch.float64), table[lab].unsqueeze(1))
    return call


# ------------------------------------------------------------------------------------------------ 1. the key
def test_refusals_of_the_key_come_before_any_draw():
    good, narrow = VarNet(), VarNet(out=3)
    torch.manual_seed(3)                                                         # _dc's seed: the constructor draws nothing before it refuses
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="discrete"):
        _dc(net=good, schedule="cosine", timestep_spacing=None)
    assert torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError, match="out_channels == 2 \\* in_channels"):
        _dc(net=narrow)
    assert torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError, match="ancestral sampler"):
        _dc(net=good, sampler="ddim")
    assert torch.equal(torch.get_rng_state(), state)
    for bad in ("range", "learned_range", True, 1):
        with pytest.raises(ValueError, match="config.variance must be"):
            _dc(net=good, variance=bad)
        assert torch.equal(torch.get_rng_state(), state)
    # config.sampler is read per call: set after construction, the entry points refuse before they draw
    dc = _dc()
    x = torch.zeros(2, 3, 8, 8)
    dc.config.sampler = "dpmpp_2m"
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="ancestral sampler"):
        dc.sample(x, torch.tensor([0, 1]), from_t=0.5)
    with pytest.raises(ValueError, match="ancestral sampler"):
        dc.counterfactual(x, None, 0.5)
    assert torch.equal(torch.get_rng_state(), state)
    assert not dc.ema.ema_model.seen


@pytest.mark.parametrize("value", ["unset", None, "fixed"])
def test_without_the_key_the_step_kinds_are_as_before(value):
    dc = _dc(variance=value)
    assert dc.variance is None
    kind = AN.step_kind(dc, TJ.grid(dc, 1.0, 0.0), 1.5)
    assert type(kind) is AN.Linear and not kind.variance
    cos = _dc(variance=value, schedule="cosine", timestep_spacing=None)
    assert type(AN.step_kind(cos, TJ.grid(cos, 1.0, 0.0), 1.5)) is AN.Clipped
    learned = _dc()
    kind = AN.step_kind(learned, TJ.grid(learned, 1.0, 0.0), 1.5)
    assert learned.variance == "learned" and type(kind) is AN.LearnedRange and kind.variance


# ------------------------------------------------------------------------------------------------ 2. the scalars
def _check_scalars(got, lin, abar, kt, ks, what):
    want = LV.scalars64(abar, kt, ks)
    assert got[:4] == lin[:4], (what, got, lin)                                  # alpha_t, sigma_t, a, b: Linear's, identically
    rel = [abs(g - want[k]) / abs(want[k]) for g, k in ((got[4], "log_hi"), (got[5], "log_lo"))]
    assert all(float(torch.tensor(g, dtype=torch.float32)) == g for g in got[4:])  # fp32 values: rounded once, on the host
    assert max(rel) <= 2.0 ** -23, (what, kt, ks, rel)
    assert got[5] <= got[4] <= 0.0
    return max(rel)


@pytest.mark.parametrize("schedule", ["ddpm_linear", "scaled_linear"])
def test_scalars_against_fp64_from_the_betas(schedule):
    b0, b1 = (1e-4, 0.02) if schedule == "ddpm_linear" else (0.00085, 0.012)
    abar = LV.abar64(1000, b0, b1, scaled=schedule == "scaled_linear")
    worst = 0.0
    for spacing, n, from_t in (("trailing", 4, 1.0), ("leading", 4, 1.0), ("leading", 5, 0.5)):
        dc = _dc(n=n, spacing=spacing, schedule=schedule)
        g = TJ.grid(dc, from_t, 0.0)
        assert spacing == "trailing" or dc.steps_offset == 1
        kind, lin = AN.step_kind(dc, g, 1.5), AN.Linear(dc, g, 1.5)
        assert len(kind.scal) == n
        for t in range(n):
            worst = max(worst, _check_scalars(kind.scal[t], lin.scal[t], abar, g.steps[t], g.steps[t + 1], (spacing, n, t)))
    # the cancellation case: neighbouring steps, 1 - abar_t / abar_s is a difference of two numbers that agree to 2 .. 3 digits
    dc = _dc(schedule=schedule)
    assert dc.abar.dtype == torch.float64 and not isinstance(dc.abar, nn.Parameter) and "abar" not in dc.state_dict()
    for k in (999, 500, 2, 1):
        got = AN.LearnedRange.scalars(dc.ddpm_logsnr[k], dc.ddpm_logsnr[k - 1], dc.abar[k], dc.abar[k - 1])
        lin = AN.Linear.scalars(dc.ddpm_logsnr[k], dc.ddpm_logsnr[k - 1])
        worst = max(worst, _check_scalars(got, lin, abar, k, k - 1, "neighbours"))
    print(f"{schedule}: log_hi / log_lo against fp64, worst relative error {worst:.2e} (bound 2^-23 = {2.0 ** -23:.2e})")


# ------------------------------------------------------------------------------------------------ 3. the eager kind
@pytest.mark.parametrize("pred_param", ["eps", "v"])
@pytest.mark.parametrize("spacing", ["trailing", "leading"])
def test_eager_sample_equals_the_fp64_loop(spacing, pred_param):
    """Bound: that of tests/test_discrete_grid_host.py for `Linear` against its fp64 loop, (passes x 2^-21 + sqrt(16 passes) x 2^-24) x
    scale, scale the largest magnitude the fp64 loop handles (latents and data predictions)."""
    n = 3
    for N, from_t in ((1000, 1.0), (40, 0.5)):
        dc = _dc(N=N, n=n, spacing=spacing, pred_param=pred_param)
        x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1)) * 3
        lab = torch.tensor([2, 0])
        torch.manual_seed(9)
        got = dc.sample(x, lab, from_t=from_t)
        torch.manual_seed(9)
        e0 = torch.randn(x.shape) if from_t == 1 else torch.randn_like(x)
        draws = [torch.randn_like(x) for _ in range(n)]
        ks = TJ.discrete_steps(dc, from_t)
        abar = LV.abar64(N)
        z0 = e0.double() if from_t == 1 else math.sqrt(abar[ks[0]]) * x.double() + math.sqrt(1 - abar[ks[0]]) * e0.double()
        null = torch.full_like(lab, dc.null_token)
        args = (_net64(dc), z0, lab, null, ks, abar, dc.cfg_w, pred_param == "v", draws)
        want, _, scale = LV.sample64(*args)
        fixed, _, _ = LV.sample64(*args, learned=False)
        passes = n + 1
        bound = (passes * 2.0 ** -21 + math.sqrt(16 * passes) * 2.0 ** -24) * scale
        d, far = float((got.double() - want).abs().max()), float((fixed - want).abs().max())
        print(f"{spacing} {pred_param} N={N} from_t={from_t}: steps {ks}, |got - fp64| {d:.2e} (bound {bound:.2e}, scale {scale:.1f}); the "
              f"fixed-variance fp64 loop is {far:.2e} away")
        seen = dc.ema.ema_model.seen
        assert len(seen) == 2 * passes and all(s.tolist() == [float(ks[min(i // 2, n - 1)])] for i, s in enumerate(seen))
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(x.shape) and d <= bound, (d, bound)
        assert far > 100 * bound, (far, bound)                                 # ignoring the key is far outside the bound


@pytest.mark.parametrize("pred_param", ["eps", "v"])
def test_eager_inversion_maps_and_the_decode_back(pred_param):
    """`invert_ddpm` against the fp64 maps (scaled by the deviation, bound TOL_NOISE of tests/test_ddpm_invert_host.py times
    max(1, |latents|.max()) as the discrete grid's tests scale it), then `counterfactual(start="ddpm_invert")`: under invert_class every
    pass is fed the inversion's next latent (bound TOL_DECODE x the same scale, tests/test_discrete_grid_host.py test 4), another class
    leaves the path, and the own-class sample is the unclipped mean of the last pass."""
    n, N = 3, 40
    dc = _dc(N=N, n=n, pred_param=pred_param)
    net = dc.ema.ema_model
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(4)) * 3
    c0, cl = torch.tensor([1, 2]), torch.tensor([[1, 0], [2, 1]])
    ks, abar = TJ.discrete_steps(dc, 0.5), LV.abar64(N)
    torch.manual_seed(21)
    draws = [torch.randn_like(x) for _ in range(n + 1)]
    null = torch.full_like(c0, dc.null_token)
    lat, maps, devs = LV.noise_maps64(_net64(dc), x, c0, null, ks, abar, dc.cfg_w, pred_param == "v", draws)
    scale = max(1.0, max(float(v.abs().max()) for v in lat))
    torch.manual_seed(21)
    inv = dc.invert_ddpm(x, c0, 0.5)
    assert tuple(inv.noise.shape) == (n,) + tuple(x.shape) and inv.noise.dtype == torch.float32 and torch.isfinite(inv.noise).all()
    d0 = float((inv.start.double() - lat[0]).abs().max())
    dn = max(float(((inv.noise[i].double() - maps[i]) * devs[i]).abs().max()) for i in range(n))
    assert d0 <= TOL_NOISE * scale and dn <= TOL_NOISE * scale, (d0, dn, TOL_NOISE * scale)
    assert min(float(v.std()) for v in devs) > 0.0                               # a deviation per element, not a scalar
    net.seen.clear(), net.seen_x.clear()
    torch.manual_seed(21)
    cf = dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=c0)
    decode_x = net.seen_x[2 * n:]
    assert len(net.seen) == 2 * n + (n + 1) * 2 * 2
    worst = 0.0
    for i in range(n + 1):
        own, other = decode_x[4 * i], decode_x[4 * i + 2]                        # column 0 (the inversion's class), column 1
        worst = max(worst, float((own.double() - lat[i]).abs().max()))
        assert i == 0 or float((other.double() - lat[i]).abs().max()) > 100 * TOL_DECODE * scale
    sc = LV.scalars64(abar, ks[n - 1], ks[n])
    mu, _, _ = LV.step64(_net64(dc), lat[n], ks[n - 1], c0, null, sc, dc.cfg_w, pred_param == "v", True)
    dl = float((cf.samples[:, 0].double() - mu).abs().max())
    print(f"{pred_param}: (noise[i] - fp64) * deviation {dn:.2e} (bound {TOL_NOISE * scale:.2e}); decode under invert_class against the "
          f"inversion's latents, worst step {worst:.2e}, last mean {dl:.2e} (bound {TOL_DECODE * scale:.2e}, |latents|.max {scale:.2f})")
    assert worst <= TOL_DECODE * scale and dl <= TOL_DECODE * scale
    assert float(cf.maps[:, 1].max()) > 0 and tuple(cf.samples.shape) == (2, 2, 3, 8, 8)


def test_step_fields_under_the_learned_kind():
    """mode and fstride = out_channels for a backbone whose pair plans keep the variance; another width is refused by naming both
    numbers, and so is a backbone without such plans (a HIP UNet with 2C outputs: its conv_out is not part of this)."""
    dc = _dc()
    cfg = lambda oc: SimpleNamespace(out_channels=oc, patch_size=2)              # noqa: E731
    dit = SimpleNamespace(config=cfg(8), variance_pair_plans=True, eps_rows_only=True)
    f = TJ.step_fields(dc, dit, (2, 4, 8, 8), 1.5, variance=True)
    assert (f["mode"], f["fstride"], f["C"], f["patch"]) == (L.STEP_LEARNED_RANGE, 8, 4, 2)
    assert f["v_param"] == L.STEP_MODE_BLOCK                                     # eps, and the flag that announces the mode block
    assert TJ.step_fields(dc, dit, (2, 4, 8, 8), 1.5)["v_param"] == 0
    assert "mode" not in TJ.step_fields(dc, dit, (2, 4, 8, 8), 1.5) and "fstride" not in TJ.step_fields(dc, dit, (2, 4, 8, 8), 1.5)
    with pytest.raises(L.DcamdError, match="got 6 vs 2 \\* 4 = 8"):
        TJ.step_fields(dc, SimpleNamespace(config=cfg(6), variance_pair_plans=True), (2, 4, 8, 8), 1.5, variance=True)
    with pytest.raises(L.DcamdError, match="got 4 vs 2 \\* 4 = 8"):
        TJ.step_fields(dc, SimpleNamespace(config=cfg(4), variance_pair_plans=True), (2, 4, 8, 8), 1.5, variance=True)
    unet = dca.UNetCondition2D(**dict(dca.small_unet_kwargs(), in_channels=4, out_channels=8))
    with pytest.raises(L.DcamdError, match="UNetCondition2D"):
        TJ.step_fields(dc, unet, (2, 4, 32, 32), 1.5, variance=True)
    with pytest.raises(L.DcamdError, match="out_channels == in_channels"):
        TJ.step_fields(dc, unet, (2, 4, 32, 32), 1.5)


# ------------------------------------------------------------------------------------------------ 4. the entries' argument checks
def _params(cls, **over):
    """A valid learned-range call on 2 x 4 x 8 x 8 latents in patches of 2 (ld = 32); the pointers are host memory nothing reads: every
    case below is refused before the launch."""
    buf = torch.zeros(16)
    kw = dict(z=buf.data_ptr(), pred=buf.data_ptr(), out=buf.data_ptr() + 4, n=2, C=4, H=8, W=8, ld=32, patch=2, v_param=L.STEP_MODE_BLOCK, w=1.5,
              one_plus_w=2.5, alpha_t=0.5, sigma_t=0.5, alpha_s=0.0, c=0.0, sd=0.0, mode=L.STEP_LEARNED_RANGE, fstride=8, k1=0.5, k2=0.5,
              log_hi=-0.1, log_lo=-2.0)
    kw.update(noise=None, noise_div=1, pad_=0) if cls is L.DdpmStepSharedParams else kw.update(x_next=buf.data_ptr())
    kw.update(over)
    return TJ.mode_params(cls)(**kw), buf


@pytest.mark.parametrize("entry, cls", [("dc_ddpm_step_shared", L.DdpmStepSharedParams), ("dc_ddpm_noise_map", L.DdpmNoiseMapParams)])
def test_the_entries_refuse_bad_mode_fields(entry, cls):
    fn = getattr(L.lib(), entry)
    cases = [(dict(mode=2), -1), (dict(mode=-1), -1),                     # DC_ERR_ARG
             (dict(fstride=7), -2), (dict(fstride=0), -2),                                          # DC_ERR_SHAPE: fstride < 2C
             (dict(ld=31), -2), (dict(fstride=12), -2),                                             # ld < p * p * fstride
             (dict(patch=0, ld=7), -2),                                                             # patch <= 1: ld < 2C
             (dict(log_hi=float("inf")), -1), (dict(log_hi=float("nan")), -1), (dict(log_lo=float("-inf")), -1),
             (dict(log_lo=float("nan")), -1), (dict(log_hi=0.5), -1), (dict(log_hi=-3.0), -1)]      # not finite, > 0, lo > hi
    for over, code in cases:
        p, keep = _params(cls, **over)
        rc = fn(C.cast(C.pointer(p), C.POINTER(cls)), None)
        assert rc == code, (entry, over, rc, L.lib().dc_last_error().decode())
        assert entry in L.lib().dc_last_error().decode()
    assert (L.STEP_FIXED, L.STEP_LEARNED_RANGE, L.STEP_MODE_BLOCK) == (0, 1, 256)
    # the struct itself is as it was; the block lies at its sizeof, in the order of the header's comment
    ext = TJ.mode_params(cls)
    assert C.sizeof(cls) == (96 if cls is L.DdpmStepSharedParams else 88) and not {"mode", "fstride"} & {n for n, _ in cls._fields_}
    assert [n for n, _ in ext._fields_] == [n for n, _ in cls._fields_] + ["mode", "fstride", "k1", "k2", "log_hi", "log_lo"]
    assert [getattr(ext, n).offset - C.sizeof(cls) for n in ("mode", "fstride", "k1", "k2", "log_hi", "log_lo")] == [0, 4, 8, 12, 16, 20]
