"""CPU: edit-friendly DDPM inversion on foreign backbones — the C-ABI surface of dc_ddpm_noise_map and its refusals, the derived
round-trip bound of one step, `invert_ddpm` and `counterfactual(start="ddpm_invert")` against the float64 statement
(ddpm_invert_oracle.py), the own-class property, determinism and generator use, the refusals and the untouched default path."""
import ctypes
import math
import os
import re

import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
import ddpm_invert_oracle as O
from helpers import load_case, standin_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 17
STEPS, BS = 4, 2

# fp32 run against the float64 statement on the same draws (stand-in backbone, sampling_steps = 4, cfg_w = 1.5, from_t = 0.5, eps and v),
# 4 x the largest max-abs difference seen over the cases of this file:
TOL_START = 4 * 1.3e-7       # x_0 = alpha_0 x + sigma_0 e_0, two roundings of values below 4: 1.27e-7 (eps and v: the same draws)
TOL_NOISE = 4 * 3.2e-7       # noise[i] * sd_i = x_{i+1} - mu_i, a latent minus a mean behind one backbone pass: 3.20e-7 (eps, i = 3;
#                              v: 2.72e-7; the raw noise[3] is this divided by sd_3 = 5.5e-4, hence the scaling)
TOL_DECODE = 4 * 1.3e-6      # a sample of counterfactual(start="ddpm_invert") (5 backbone passes): 1.26e-6 (eps, another class; own
#                              class 7.05e-7; v: 7.20e-7 / 7.07e-7).  Its maps sum three channels, 3 * TOL_DECODE: seen 1.24e-6


def _dc(pred_param="eps", **extra):
    g, cfg = load_case("1stage_eps")
    cfg.update(pred_param=pred_param, cfg_w=1.5, sampling_steps=STEPS)
    cfg.update(extra)
    dc = dca.DiffusionClassifier(standin_from(g, cfg), dca.Config(**cfg))
    dc.encoder.weight.data.copy_(torch.from_numpy(g["encoder.weight"]))
    return dc, torch.from_numpy(g["x"])[:BS].contiguous(), cfg


def _draws(x, n):
    """The n + 1 draws of `invert_ddpm(rng="reference")` from the generator as it stands."""
    return [torch.randn_like(x) for _ in range(n + 1)]


# ------------------------------------------------------------------------------------------------ C-ABI
def test_struct_fields_match_the_header_and_the_abi_version_stays():
    src = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    fields = L.DdpmNoiseMapParams._fields_
    assert [f[0] for f in fields if f[1] is L.vp] == ["z", "pred", "x_next", "out"]
    assert [f[0] for f in fields if f[1] is L.i32] == ["n", "C", "H", "W", "ld", "patch", "v_param"]
    assert [f[0] for f in fields if f[1] is L.f32] == ["w", "one_plus_w", "alpha_t", "sigma_t", "alpha_s", "c", "sd"]
    assert ctypes.sizeof(L.DdpmNoiseMapParams) == 4 * ptr + 14 * 4              # 88 bytes on a 64-bit host: no pad needed
    lib = L.lib()
    assert "dc_ddpm_noise_map" in L.EXPORTS and lib.dc_ddpm_noise_map is not None
    assert re.search(r"\bint dc_ddpm_noise_map\(", src)
    assert lib.dc_abi_version() == 5 and L.ABI_VERSION == 5
    assert re.search(r"#define DC_ABI_VERSION 5\b", src)
    # the older step entries keep their structs
    assert ctypes.sizeof(L.DdpmStepParams) == 4 * ptr + 14 * 4 and ctypes.sizeof(L.DdpmStepSharedParams) == 4 * ptr + 16 * 4
    assert ctypes.sizeof(L.SolverStepParams) == 5 * ptr + 16 * 4


def _map_params(**over):
    buf = (ctypes.c_float * 64)()
    buf2 = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    kw = dict(z=a, pred=a, x_next=a, out=ctypes.addressof(buf2), n=6, C=1, H=2, W=2, ld=4, patch=0, v_param=0,
              w=1.0, one_plus_w=2.0, alpha_t=1.0, sigma_t=1.0, alpha_s=0.5, c=0.5, sd=0.5)
    kw.update(over)
    return L.DdpmNoiseMapParams(**kw), (buf, buf2)


@pytest.mark.parametrize("over,code,word", [
    (dict(z=None), -1, "null"), (dict(pred=None), -1, "null"), (dict(x_next=None), -1, "null"), (dict(out=None), -1, "null"),
    (dict(sd=0.0), -1, "sd="), (dict(sd=-1.0), -1, "sd="), (dict(sd=float("inf")), -1, "sd="), (dict(sd=float("nan")), -1, "sd="),
    (dict(n=0), -2, "extents"), (dict(C=0), -2, "extents"), (dict(H=0), -2, "extents"), (dict(W=-1), -2, "extents"),
    (dict(ld=0), -2, "extents"), (dict(patch=2, ld=3), -2, "extents"), (dict(patch=3, ld=16), -2, "patch=3"),
])
def test_noise_map_refuses_before_any_launch(over, code, word):
    """Every argument check answers without a GPU and touches no memory (a call that passed them would launch: none does here)."""
    lib = L.lib()
    assert lib.dc_ddpm_noise_map(None, None) == -1 and "null" in lib.dc_last_error().decode()      # the entry is reached at all
    p, _keep = _map_params()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.dc_ddpm_noise_map(ctypes.byref(p), None) == code
    assert word in lib.dc_last_error().decode()


# ------------------------------------------------------------------------------------------------ one step there and back
@pytest.mark.parametrize("w", [0.0, 1.5])
@pytest.mark.parametrize("pred_param", ["eps", "v"])
def test_one_step_round_trip_stays_inside_the_derived_bound(pred_param, w):
    """out = mu + ((x_next - mu) / sd) * sd in fp32: the subtraction, the division, the product and the sum round once each, relative
    2^-24 — |out - x_next| <= 2^-24 (3 |x_next - mu| + |x_next|) to first order, asserted with a 4/3 margin as
    2^-22 (|x_next| + |x_next - mu|).  On the eager statement (`ddpm_sampler_step`) for every step of the grids from 0.5 and 1 (sd from
    5.5e-4, the step onto u = 0, to 0.9), data scales 0.01 .. 3 and predictions large enough to drive the data prediction into the clip."""
    dc, _, _ = _dc(pred_param, sampling_steps=3)
    g = torch.Generator().manual_seed(23)
    worst, sds, clipped = 0.0, [], False
    for from_t in (0.5, 1.0):
        steps = torch.linspace(from_t, 0.0, 4)
        for i in range(3):
            lam_t, lam_s = dc.schedule(steps[i]).unsqueeze(0), dc.schedule(steps[i + 1]).unsqueeze(0)
            for scale in (0.01, 0.3, 3.0):
                z, x_next = torch.randn(BS, 3, 8, 8, generator=g) * scale, torch.randn(BS, 3, 8, 8, generator=g) * scale
                pred, u_pred = torch.randn(BS, 3, 8, 8, generator=g) * 2, torch.randn(BS, 3, 8, 8, generator=g) * 2
                mu, var = dc.ddpm_sampler_step(z, pred, u_pred, lam_t, lam_s, w=w)
                sd = torch.sqrt(var)
                pr = (1 + w) * pred - w * u_pred
                a_t, s_t = torch.sqrt(torch.sigmoid(lam_t)), torch.sqrt(torch.sigmoid(-lam_t))
                clipped |= bool(((a_t * z - s_t * pr if pred_param == "v" else (z - s_t * pr) / a_t).abs() > 1).any())
                out = mu + ((x_next - mu) / sd) * sd
                bound = 2.0 ** -22 * (x_next.abs() + (x_next - mu).abs())
                assert bool(((out - x_next).abs() <= bound).all()), (from_t, i, scale, float(sd))
                worst = max(worst, float(((out - x_next).abs() / bound.clamp_min(1e-30)).max()))
                sds.append(float(sd))
    print(f"{pred_param} w={w}: sd {min(sds):.2e} .. {max(sds):.2e}, worst |out - x_next| / bound = {worst:.2f}")
    assert clipped and min(sds) < 1e-3 and max(sds) > 0.5
    # w = None is config.cfg_w: the argument is additive
    a = dc.ddpm_sampler_step(z, pred, u_pred, lam_t, lam_s)
    b = dc.ddpm_sampler_step(z, pred, u_pred, lam_t, lam_s, w=dc.cfg_w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ the float64 statement
@pytest.fixture(scope="module", params=["eps", "v"])
def case(request):
    """One inversion and one counterfactual per parametrisation, and their float64 statement on the same draws; left unchanged."""
    dc, x, cfg = _dc(request.param)
    lab = torch.tensor([1, 2])
    cl = torch.tensor([[1, 0, 3], [2, 3, 0]])                                 # column 0: the inversion's own class
    torch.manual_seed(SEED)
    inv = dc.invert_ddpm(x, lab, 0.5)
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=lab)
    torch.manual_seed(SEED)
    draws = _draws(x, STEPS)
    lat, noise, sds = O.invert64(dc, x, lab, 0.5, 1.5, draws)
    want = O.counterfactual64(dc, lat[0], noise, cl, 0.5, 1.5)
    return dict(dc=dc, x=x, lab=lab, cl=cl, inv=inv, cf=cf, draws=draws, lat=lat, noise=noise, sds=sds, want=want, pp=request.param)


def test_inversion_equals_the_float64_statement(case):
    inv, lat, noise, sds = case["inv"], case["lat"], case["noise"], case["sds"]
    assert isinstance(inv, dca.DdpmInversion) and inv.from_t == 0.5 and inv.guidance == 1.5          # None: config.cfg_w
    assert inv.start.dtype == inv.noise.dtype == torch.float32
    assert tuple(inv.start.shape) == (BS, 3, 8, 8) and tuple(inv.noise.shape) == (STEPS, BS, 3, 8, 8)
    d0 = (inv.start - lat[0]).abs().max().item()
    dn = [((inv.noise[i] - noise[i]) * sds[i]).abs().max().item() for i in range(STEPS)]
    print(f"{case['pp']}: start vs float64 {d0:.2e}; noise[i] * sd_i vs float64 {[f'{v:.2e}' for v in dn]}; sd_i {[f'{v:.2e}' for v in sds]}")
    assert d0 <= TOL_START and max(dn) <= TOL_NOISE
    assert sds[-1] < 1e-3                                                     # the raw last map is divided by this: compared scaled
    # another guidance weight gives other maps from the same latents, and is stored
    torch.manual_seed(SEED)
    other = case["dc"].invert_ddpm(case["x"], case["lab"], 0.5, guidance=0.0)
    assert other.guidance == 0.0 and torch.equal(other.start, inv.start) and not torch.equal(other.noise, inv.noise)
    _, n0, _ = O.invert64(case["dc"], case["x"], case["lab"], 0.5, 0.0, case["draws"])
    d_w0 = max(((other.noise[i] - n0[i]) * sds[i]).abs().max().item() for i in range(STEPS))
    # text None: the null token
    torch.manual_seed(SEED)
    nul = case["dc"].invert_ddpm(case["x"], None, 0.5)
    _, nn, _ = O.invert64(case["dc"], case["x"], torch.full((BS,), 4), 0.5, 1.5, case["draws"])
    d_nul = max(((nul.noise[i] - nn[i]) * sds[i]).abs().max().item() for i in range(STEPS))
    print(f"{case['pp']}: noise[i] * sd_i vs float64 under guidance 0: {d_w0:.2e}, under the null token: {d_nul:.2e}")
    assert d_w0 <= TOL_NOISE and d_nul <= TOL_NOISE


def test_counterfactual_equals_the_float64_statement(case):
    cf, want, x, cl = case["cf"], case["want"], case["x"], case["cl"]
    assert cf.samples.dtype == torch.float32 and tuple(cf.samples.shape) == (BS, 3, 3, 8, 8) and torch.equal(cf.classes, cl)
    own, other = (cf.samples[:, 0] - want[:, 0]).abs().max().item(), (cf.samples[:, 1:] - want[:, 1:]).abs().max().item()
    maps64 = (want - x.double()[:, None]).abs().sum(dim=2)
    dm = (cf.maps - maps64).abs().max().item()
    print(f"{case['pp']}: samples vs float64: own class {own:.2e}, other classes {other:.2e}; maps {dm:.2e}")
    assert own <= TOL_DECODE and other <= TOL_DECODE and dm <= 3 * TOL_DECODE
    assert (want[:, 0] - want[:, 1]).abs().max().item() > 0.1                 # the labels do matter
    maps = torch.zeros_like(cf.maps)
    for c in range(3):
        maps = maps + (cf.samples[:, :, c] - x[:, None, c]).abs()
    assert torch.equal(cf.maps, maps)
    # against a class: the maps are taken to that class's trajectory
    torch.manual_seed(SEED)
    ag = case["dc"].counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=case["lab"], against=cl[:, 0])
    assert torch.equal(ag.samples, cf.samples) and float(ag.maps[:, 0].max()) == 0.0 and float(ag.maps[:, 1].min()) >= 0.0


def test_own_class_trajectory_is_the_last_pass_applied_to_the_last_latent(case):
    """Under the inversion's class and weight every step lands on the next latent again, so the own-class sample is the sampler's last
    pass (the clipped mean) applied to x_n = alpha_n x + sigma_n e_n, recomputed here from the re-seeded generator.  It is NOT asserted
    to be close to x: with untrained weights the last mean pass is not the identity (a trained denoiser at sigma_n ~ 5e-4 is)."""
    dc, x = case["dc"], case["x"]
    torch.manual_seed(SEED)
    e_n = _draws(x, STEPS)[-1]
    lam_n = float(dc.schedule(torch.tensor(0.0, dtype=torch.float64)))
    x_n = math.sqrt(1 / (1 + math.exp(-lam_n))) * x.double() + math.sqrt(1 / (1 + math.exp(lam_n))) * e_n.double()
    want = O.last_pass64(dc, x_n, case["lab"], 0.5, 1.5)
    d = (case["cf"].samples[:, 0] - want).abs().max().item()
    far = (case["cf"].samples[:, 1] - want).abs().max().item()
    print(f"{case['pp']}: own-class sample vs the last pass on x_n: {d:.2e} (another class: {far:.2e})")
    assert d <= TOL_DECODE
    assert far > 1e-3                                                          # another class does not come back


# ------------------------------------------------------------------------------------------------ determinism, generator use
def test_reference_rng_takes_n_plus_one_draws_and_repeats_bit_for_bit():
    dc, x, _ = _dc("v")
    lab = torch.tensor([0, 3])
    torch.manual_seed(SEED)
    a = dc.invert_ddpm(x, lab, 0.5)
    after = torch.rand(1)
    torch.manual_seed(SEED)
    _draws(x, STEPS)
    assert torch.equal(after, torch.rand(1))                                  # exactly n + 1 randn_like(x)
    torch.manual_seed(SEED)
    b = dc.invert_ddpm(x, lab, 0.5)
    assert torch.equal(a.start, b.start) and torch.equal(a.noise, b.noise)
    # the decode draws nothing: a counterfactual leaves the generator where the inversion alone leaves it
    torch.manual_seed(SEED)
    c1 = dc.counterfactual(x, None, 0.5, start="ddpm_invert", invert_class=lab)
    assert torch.equal(after, torch.rand(1))
    torch.manual_seed(SEED)
    c2 = dc.counterfactual(x, None, 0.5, start="ddpm_invert", invert_class=lab, seed=5)      # seed: Philox only
    assert torch.equal(c1.samples, c2.samples) and torch.equal(c1.maps, c2.maps)
    # a refused call consumes nothing
    torch.manual_seed(SEED)
    first = torch.rand(1)
    torch.manual_seed(SEED)
    dc.config.ddpm_invert_max_bytes = 8
    with pytest.raises(ValueError):
        dc.invert_ddpm(x, lab, 0.5)
    with pytest.raises(ValueError):
        dc.counterfactual(x, None, 0.5, start="ddpm_invert", invert_class=lab)
    dc.config.ddpm_invert_max_bytes = None
    with pytest.raises(ValueError):
        dc.invert_ddpm(x, torch.zeros(BS + 1, dtype=torch.int64), 0.5)
    assert torch.equal(first, torch.rand(1))


# ------------------------------------------------------------------------------------------------ the default path
def test_default_path_is_untouched():
    """counterfactual(x, None, 0.5) gives the same bits before and after an `invert_ddpm` call, and equals the K reseeded `sample` calls."""
    dc, x, cfg = _dc()
    torch.manual_seed(SEED)
    a = dc.counterfactual(x, None, 0.5)
    torch.manual_seed(SEED)
    dc.invert_ddpm(x, None, 0.5)
    torch.manual_seed(SEED)
    b = dc.counterfactual(x, None, 0.5)
    assert torch.equal(a.samples, b.samples) and torch.equal(a.maps, b.maps)
    for k in range(cfg["classes"]):
        torch.manual_seed(SEED)
        assert torch.equal(dc.sample(x, torch.full((BS,), k), from_t=0.5), a.samples[:, k])


# ------------------------------------------------------------------------------------------------ refusals
def test_error_paths():
    dc, x, cfg = _dc()
    lab = torch.zeros(BS, dtype=torch.int64)
    for bad in (0, 0.0, -0.5, 1.0001, 2, float("nan")):
        with pytest.raises(ValueError, match="from_t"):
            dc.invert_ddpm(x, None, bad)
        with pytest.raises(ValueError, match="from_t"):
            dc.counterfactual(x, None, bad, start="ddpm_invert")
    with pytest.raises(ValueError, match="x must be"):
        dc.invert_ddpm(x[0], None, 0.5)
    for bad in (torch.zeros(BS + 1, dtype=torch.int64), torch.zeros(BS, 1, dtype=torch.int64), torch.zeros(BS), torch.zeros(BS, dtype=torch.bool),
                torch.full((BS,), cfg["classes"] + 1), torch.full((BS,), -1)):
        with pytest.raises(ValueError, match="text"):
            dc.invert_ddpm(x, bad)
        with pytest.raises(ValueError, match="invert_class"):
            dc.counterfactual(x, start="ddpm_invert", invert_class=bad)
    with pytest.raises(ValueError, match="rng"):
        dc.invert_ddpm(x, lab, rng="torch")
    with pytest.raises(L.DcamdError, match="philox"):
        dc.invert_ddpm(x, lab, rng="philox")                                  # a foreign backbone has no device RNG
    with pytest.raises(L.DcamdError, match="philox"):
        dc.counterfactual(x, start="ddpm_invert", rng="philox")
    # the byte cap: 4 steps x [2, 3, 8, 8] f32 = 6144 bytes
    dc.config.ddpm_invert_max_bytes = 6143
    with pytest.raises(ValueError, match=r"6144 bytes.*ddpm_invert_max_bytes = 6143"):
        dc.invert_ddpm(x, lab)
    with pytest.raises(ValueError, match="ddpm_invert_max_bytes"):
        dc.counterfactual(x, start="ddpm_invert")
    dc.config.ddpm_invert_max_bytes = 6144
    assert tuple(dc.invert_ddpm(x, lab).noise.shape) == (STEPS, BS, 3, 8, 8)
    dc.config.ddpm_invert_max_bytes = "1G"
    with pytest.raises(ValueError, match="ddpm_invert_max_bytes"):
        dc.invert_ddpm(x, lab)
    dc.config.ddpm_invert_max_bytes = None
    # the decode needs the ancestral sampler; the inversion itself does not care
    for sampler in ("ddim", "dpmpp_2m"):
        dc.config.sampler = sampler
        with pytest.raises(ValueError, match=r"start='ddpm_invert'.*config\.sampler"):
            dc.counterfactual(x, start="ddpm_invert")
        assert torch.isfinite(dc.invert_ddpm(x, lab).noise).all()
    dc.config.sampler = "ddpm"
    assert torch.isfinite(dc.counterfactual(x, start="ddpm_invert").samples).all()
    # untouched: start="invert" under the ancestral sampler, unknown starts, invert_class without an inversion
    for sampler in (None, "ddpm"):
        dc.config.sampler = sampler
        with pytest.raises(ValueError, match="start='invert' needs a deterministic config.sampler"):
            dc.counterfactual(x, start="invert")
    with pytest.raises(ValueError, match="start"):
        dc.counterfactual(x, start="latent")
    with pytest.raises(ValueError, match="invert_class"):
        dc.counterfactual(x, invert_class=lab)


def test_ragged_table_in_front_of_a_foreign_backbone_is_refused():
    g, cfg = load_case("1stage_eps")
    cfg.update(cfg_w=1.5, sampling_steps=STEPS, encoder_type="prompt", prompt_tokens=2)
    dc = dca.DiffusionClassifier(standin_from(g, dict(cfg, encoder_type="nn")), dca.Config(**cfg))
    dc.encoder.set_lengths([2, 1, 2, 2, 1])
    x = torch.from_numpy(g["x"])[:BS]
    torch.manual_seed(SEED)
    first = torch.rand(1)
    torch.manual_seed(SEED)
    with pytest.raises(NotImplementedError, match="different lengths"):
        dc.invert_ddpm(x, torch.zeros(BS, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="different lengths"):
        dc.counterfactual(x, start="ddpm_invert")
    assert torch.equal(first, torch.rand(1))
