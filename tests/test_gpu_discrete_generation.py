"""GPU: generation on the discrete DDPM grid (schedule='scaled_linear' with config.timestep_spacing) on the two random-weight minis of
tests/test_gpu_sd_unet.py — `sample`, `counterfactual`, `invert`, `invert_ddpm` and decode=True on the HIP loops (pair plans) against
the eager statement driven through the same backbone's `forward` (two calls per pass), what the plans were fed, chunking, Philox and bf16.

f32, 16x16 latents, BS = 2, K = 3, sampling_steps = 4, cfg_w = 2.  Two cases: SD1-mini / eps / 1000 train steps and SD2-mini / v / 40
train steps (grid neighbours 5 to 10 steps apart).  The model bound is test_gpu_counterfactual.BOUND (3e-4, the project's bound for fp32
pair plans against two-call plans) times max(1, |eager|.max()): nothing clips these samples to [-1, 1].

Seen on an MI355X (max-abs against the eager statement):
  sd1_eps_1000  sample 3.3e-6 .. 2.3e-5 (the largest at from_t = 1, |eager| up to 75); counterfactual vs K samples 0, chunked 0; invert
                3.2e-6, start="invert" 1.1e-5; invert_ddpm noise[i] * sd_i 5.2e-7; decode under invert_class, worst step 8.1e-6 (bound 2.1e-5)
  sd2_v_40      all 0 but the decode under invert_class, worst step 9.5e-7 (bound 1.6e-5)
"""
import pytest
import torch

from diffusion_classifier_amd import discrete as DG
from diffusion_classifier_amd import solver as S
from diffusion_classifier_amd import trajectory as TJ
from test_ddpm_invert_host import TOL_DECODE
from test_gpu_counterfactual import BOUND
from test_gpu_sd_unet import DEV, MINIS, _classifier, make_pair
from test_gpu_vae_decoder import ENC_TINY, TINY, bits, random_decoder, write_directory

pytestmark = pytest.mark.gpu
SEED = 7
STEPS, BS, HW = 4, 2, 16
CASES = {"sd1_eps_1000": ("sd1", "eps", 1000), "sd2_v_40": ("sd2", "v", 40)}
assert all(c[0] in MINIS for c in CASES.values())
CL = torch.tensor([[1, 2, 0], [2, 0, 1]])
C0 = torch.tensor([1, 2])
_BUILT = {}


def mini(name, seed):
    """A mini of tests/test_gpu_sd_unet.py at 16x16 latents: SD2-mini is published there at 8x8, and a model's launch plans are built
    for config.sample_size (its weights do not depend on it).  `make_pair` hands its extra keywords to the oracle only, so the key is set
    on the model it returns — here, before the classifier copies the model and long before the first plan is built."""
    m, _, kw, Sx = make_pair(name, seed=seed)
    assert not m._plans
    m.config.sample_size = HW
    return m, dict(kw, sample_size=HW), Sx


def build(case, spacing="trailing", **over):
    """One classifier per (case, spacing, extra keys), built once and shared by the tests; config.sampler is set per test."""
    key = (case, spacing, tuple(sorted(over.items())))
    if key not in _BUILT:
        name, pred_param, N = CASES[case]
        m, kw, Sx = mini(name, 300 + len(case))
        dc = _classifier(m, kw, Sx, pred_param=pred_param, cfg_w=2.0, sampling_steps=STEPS, train_timesteps=N, timestep_spacing=spacing,
                         steps_offset=int(spacing == "leading"), **over)
        torch.manual_seed(301)
        dc.encoder.weight.data.normal_(0, 2.0)
        x = torch.randn(BS, 4, HW, HW)                                          # scaled latents: unit variance, not [-1, 1]
        _BUILT[key] = (dc.to(DEV), x.to(DEV))
    dc, x = _BUILT[key]
    dc.config.sampler = None
    dc.config.units_per_launch = None
    return dc, x


def eager_sample(dc, x, lab, from_t, sampler):
    """`sample` in eager torch on the same backbone: the start as ever, then two `forward` calls per pass."""
    if sampler != "ddpm":
        return S.sample_eager(dc, x, lab, from_t, sampler)
    z0 = TJ.initial_latent(dc, x, from_t)
    cond, null, lens = TJ.contexts(dc, lab, x.device, dc.ema.ema_model)
    return DG.ancestral_eager(dc, z0, [cond], null, TJ.grid(dc, from_t, 0.0), lens)[0]


def bound_of(want):
    return BOUND * max(1.0, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ 6. sample
@pytest.mark.parametrize("from_t", [1, 0.5])
@pytest.mark.parametrize("spacing", ["trailing", "leading"])
@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp_2m"])
@pytest.mark.parametrize("case", list(CASES))
def test_sample_matches_the_eager_statement(case, sampler, spacing, from_t):
    dc, x = build(case, spacing)
    dc.config.sampler = sampler
    lab, other = torch.tensor([1, 0]).to(DEV), torch.tensor([2, 1]).to(DEV)
    torch.manual_seed(SEED)
    got = dc.sample(x, lab, from_t=from_t)
    torch.manual_seed(SEED)
    want = eager_sample(dc, x, lab, from_t, sampler)
    assert got.shape == x.shape and got.dtype == torch.float32 and got.is_cuda and torch.isfinite(got).all()
    d, b = (got - want).abs().max().item(), bound_of(want)
    print(f"{case} {sampler} {spacing} from_t={from_t}: steps {TJ.discrete_steps(dc, from_t)}, sample vs the eager statement: "
          f"max abs difference {d:.2e} (bound {b:.2e}), |eager|.max {float(want.abs().max()):.2f}")
    assert d < b, (d, b)
    torch.manual_seed(SEED)
    far = (dc.sample(x, other, from_t=from_t) - got).abs().max().item()
    assert far > 10 * b, (far, b)                                              # the labels do steer these models: the bound can see a mix-up
    assert float(want.abs().max()) > 1.0 and float(got.abs().max()) > 1.0        # nothing is clipped to [-1, 1]


def test_latents_of_another_extent_are_refused_before_any_launch():
    """The plans are built for config.sample_size: 8x8 latents in front of a 16x16 model would under-fill the operand, 32x32 would
    write past it."""
    from diffusion_classifier_amd import _lib as L
    dc, x = build("sd2_v_40")
    for sampler in ("ddpm", "ddim"):
        dc.config.sampler = sampler
        for bad in (x[:, :, :8, :8].contiguous(), x.repeat(1, 1, 2, 2)):
            with pytest.raises(L.DcamdError, match="sample_size"):
                dc.sample(bad, C0.to(DEV), from_t=0.5)
            with pytest.raises(L.DcamdError, match="sample_size"):
                dc.counterfactual(bad, CL, 0.5)


# ------------------------------------------------------------------------------------------------ 7. what the plans were fed
def _record_feeds(monkeypatch, dc):
    bb, fed = dc.ema.ema_model, []
    real = bb._feed
    monkeypatch.setattr(bb, "_feed", lambda plan, x, labels: (fed.append((x.detach().clone(), torch.as_tensor(labels).detach().clone())),
                                                              real(plan, x, labels))[1])
    return fed


@pytest.mark.parametrize("case, spacing", [("sd1_eps_1000", "leading"), ("sd2_v_40", "trailing")])
def test_every_launch_is_fed_the_step_of_its_pass(monkeypatch, case, spacing):
    dc, x = build(case, spacing)
    fed = _record_feeds(monkeypatch, dc)
    labels = lambda: [v[1].reshape(-1).cpu().tolist() for v in fed]             # noqa: E731
    ks = TJ.discrete_steps(dc, 0.5)
    down = [float(k) for k in ks[:STEPS]]
    for sampler, passes in (("ddim", down), ("dpmpp_2m", down), ("ddpm", down + [down[-1]])):
        dc.config.sampler = sampler
        fed.clear()
        dc.sample(x, C0.to(DEV), from_t=0.5)
        assert labels() == [[k] for k in passes], (sampler, labels(), ks)
        dc.config.units_per_launch = 6                                         # 2 * K units an image: every image its own chunk
        fed.clear()
        dc.counterfactual(x, CL, 0.5)
        assert labels() == [[k] for k in passes for _ in range(BS)], (sampler, labels(), ks)
        assert all(tuple(v[0].shape) == (3, 4, HW, HW) for v in fed)
        dc.config.units_per_launch = None
    fed.clear()
    dc.invert(x, C0, 0.5)
    assert labels() == [[float(k)] for k in ks[::-1][:STEPS]]                  # upwards, from k_n = 0
    fed.clear()
    dc.invert_ddpm(x, C0, 0.5)
    assert labels() == [[k] for k in down]


# ------------------------------------------------------------------------------------------------ 8. counterfactual
@pytest.mark.parametrize("case, spacing", [("sd1_eps_1000", "trailing"), ("sd2_v_40", "leading")])
def test_ancestral_counterfactual_is_k_reseeded_samples_chunks_and_philox(case, spacing):
    dc, x = build(case, spacing)
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, CL, 0.5)
    want = []
    for k in range(3):
        torch.manual_seed(SEED)
        want.append(dc.sample(x, CL[:, k].to(DEV), from_t=0.5))
    want = torch.stack(want, dim=1)
    d, b = (cf.samples - want).abs().max().item(), bound_of(want)
    assert tuple(cf.samples.shape) == (BS, 3, 4, HW, HW) and tuple(cf.maps.shape) == (BS, 3, HW, HW) and torch.isfinite(cf.samples).all()
    dc.config.units_per_launch = 6
    torch.manual_seed(SEED)
    one = dc.counterfactual(x, CL, 0.5)
    dc.config.units_per_launch = None
    dchunk = (one.samples - cf.samples).abs().max().item()
    print(f"{case} {spacing}: ancestral counterfactual vs K reseeded sample() calls: max abs difference {d:.2e}; one image per chunk vs "
          f"one launch {dchunk:.2e} (bound {b:.2e})")
    assert d < b and dchunk < b, (d, dchunk, b)
    assert (want[:, 0] - want[:, 1]).abs().max().item() > 10 * b and float(cf.samples.abs().max()) > 1.0
    before = torch.cuda.get_rng_state(0), torch.get_rng_state()
    p1 = dc.counterfactual(x, CL, 0.5, rng="philox", seed=11)
    assert torch.equal(torch.cuda.get_rng_state(0), before[0]) and torch.equal(torch.get_rng_state(), before[1])
    p2 = dc.counterfactual(x, CL, 0.5, rng="philox", seed=11)
    p3 = dc.counterfactual(x, CL, 0.5, rng="philox", seed=12)
    assert torch.isfinite(p1.samples).all() and torch.equal(p1.samples, p2.samples) and torch.equal(p1.maps, p2.maps)
    assert not torch.equal(p1.samples, p3.samples)


@pytest.mark.parametrize("case, spacing", [("sd1_eps_1000", "leading"), ("sd2_v_40", "trailing")])
def test_inverted_counterfactual_is_k_decodes_of_the_inverted_latent(case, spacing):
    dc, x = build(case, spacing)
    dc.config.sampler = "dpmpp_2m"
    zinv = dc.invert(x, C0, 0.5)
    zinv_e = S.invert_eager(dc, x, C0, 0.5, 0.0)
    cf = dc.counterfactual(x, CL, 0.5, start="invert", invert_class=C0)
    want = torch.stack([S.decode_eager(dc, zinv, CL[:, k].to(DEV), 0.5, "dpmpp_2m") for k in range(3)], dim=1)
    d, di, b = (cf.samples - want).abs().max().item(), (zinv - zinv_e).abs().max().item(), bound_of(want)
    dc.config.units_per_launch = 6
    one = dc.counterfactual(x, CL, 0.5, start="invert", invert_class=C0)
    dc.config.units_per_launch = None
    dchunk = (one.samples - cf.samples).abs().max().item()
    print(f"{case} {spacing}: invert vs the eager statement {di:.2e} (bound {bound_of(zinv_e):.2e}); counterfactual(start='invert') vs K "
          f"decodes of invert(x, c0) {d:.2e}; one image per chunk vs one launch {dchunk:.2e} (bound {b:.2e})")
    assert di < bound_of(zinv_e) and d < b and dchunk < b, (di, d, dchunk, b)
    assert (want[:, 0] - want[:, 1]).abs().max().item() > 10 * b and float(zinv.abs().max()) > 1.0
    again = dc.counterfactual(x, CL, 0.5, start="invert", invert_class=C0)
    assert torch.equal(again.samples, cf.samples) and torch.equal(again.maps, cf.maps)


# ------------------------------------------------------------------------------------------------ 9. invert_ddpm
@pytest.mark.parametrize("case, spacing", [("sd1_eps_1000", "trailing"), ("sd2_v_40", "leading")])
def test_ddpm_inversion_decodes_back_step_by_step(monkeypatch, case, spacing):
    """Under invert_class the decode is fed, pass after pass, the latents the inversion drew (recomputed here from the reseeded
    generator by the product's own expressions).  Bound and scaling: test 4 of tests/test_discrete_grid_host.py, TOL_DECODE of
    tests/test_ddpm_invert_host.py times max(1, |latents|.max())."""
    dc, x = build(case, spacing)
    g = TJ.grid(dc, 0.5, 0.0)
    torch.manual_seed(SEED)
    alsg = DG.latent_scalars(g)
    lat = [(a.to(DEV) * x + s.to(DEV) * torch.randn_like(x)).contiguous() for a, s in alsg]
    torch.manual_seed(SEED)
    inv = dc.invert_ddpm(x, C0, 0.5)
    assert torch.equal(inv.start, lat[0]) and tuple(inv.noise.shape) == (STEPS,) + tuple(x.shape) and torch.isfinite(inv.noise).all()
    # against the eager statement on the same draws, scaled by sd_i as tests/test_gpu_ddpm_invert.py does
    torch.manual_seed(SEED)
    start_e, noise_e = DG.noise_maps_eager(dc, x, C0, g, 2.0)
    sds = [DG.posterior_scalars(g.lam[i], g.lam[i + 1])[4] for i in range(STEPS)]
    dn = max(((inv.noise[i] - noise_e[i]) * sds[i]).abs().max().item() for i in range(STEPS))
    fed = _record_feeds(monkeypatch, dc)
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, CL, 0.5, start="ddpm_invert", invert_class=C0)      # column 0 of CL is C0
    feeds = fed[STEPS:]                                                        # the inversion's passes come first
    assert len(fed) == STEPS + STEPS + 1 and all(tuple(v[0].shape) == (BS * 3, 4, HW, HW) for v in feeds)
    scale = max(1.0, max(float(v.abs().max()) for v in lat))
    worst = 0.0
    for i, (z, _) in enumerate(feeds):
        z = z.view(BS, 3, 4, HW, HW)
        worst = max(worst, float((z[:, 0] - lat[i]).abs().max()))
        assert i == 0 or float((z[:, 1] - lat[i]).abs().max()) > 100 * TOL_DECODE * scale      # another class leaves the path
    print(f"{case} {spacing}: invert_ddpm vs the eager statement, noise[i] * sd_i {dn:.2e} (bound {BOUND * scale:.2e}); the decode under "
          f"invert_class against the inversion's latents, worst step {worst:.2e} (bound {TOL_DECODE * scale:.2e}, |latents|.max {scale:.2f})")
    assert dn < BOUND * scale
    assert worst <= TOL_DECODE * scale, (worst, TOL_DECODE * scale)
    assert float(cf.maps[:, 1].min()) >= 0.0 and float(cf.maps[:, 1].max()) > 0.0 and float(cf.maps[:, 2].max()) > 0.0


# ------------------------------------------------------------------------------------------------ 10. decode=True
def test_decode_true_is_decode_latents_of_the_latents(tmp_path):
    dec = random_decoder(TINY, 81)
    torch.manual_seed(82)
    from diffusion_classifier_amd.nets.vae import VAEEncoder
    path = write_directory(str(tmp_path / "vae"), dec, VAEEncoder(**ENC_TINY))
    name, pred_param, N = CASES["sd2_v_40"]
    m, kw, Sx = mini(name, 310)
    dc = _classifier(m, kw, Sx, pred_param=pred_param, cfg_w=2.0, sampling_steps=STEPS, train_timesteps=N, timestep_spacing="trailing",
                     vae_path=path).to(DEV)
    x = torch.randn(BS, 4, HW, HW, generator=torch.Generator().manual_seed(311)).to(DEV)
    lab = torch.tensor([2, 0]).to(DEV)
    for sampler in ("ddpm", "ddim"):
        dc.config.sampler = sampler
        torch.manual_seed(SEED)
        lat = dc.sample(x, lab, from_t=0.5)
        torch.manual_seed(SEED)
        img = dc.sample(x, lab, from_t=0.5, decode=True)
        assert tuple(img.shape) == (BS, 3, 4 * HW, 4 * HW) and torch.equal(bits(img), bits(dc.decode_latents(lat)))
        torch.manual_seed(SEED)
        cf = dc.counterfactual(x, CL, 0.5, decode=True)
        assert tuple(cf.samples.shape) == (BS, 3, 3, 4 * HW, 4 * HW) and tuple(cf.maps.shape) == (BS, 3, 4 * HW, 4 * HW)
        assert torch.isfinite(cf.samples).all() and torch.isfinite(cf.maps).all()


# ------------------------------------------------------------------------------------------------ 11. bf16
@pytest.mark.parametrize("case", list(CASES))
def test_bf16_runs_finite(case):
    """The default compute dtype: shapes, devices and finiteness only, no parity claim."""
    dc, x = build(case, "trailing", compute_dtype="bf16")
    for sampler in ("ddpm", "dpmpp_2m"):
        dc.config.sampler = sampler
        got = dc.sample(x, C0.to(DEV), from_t=1)
        cf = dc.counterfactual(x, CL, 0.5)
        assert got.shape == x.shape and got.is_cuda and got.dtype == torch.float32 and torch.isfinite(got).all()
        assert tuple(cf.samples.shape) == (BS, 3, 4, HW, HW) and cf.samples.is_cuda and torch.isfinite(cf.samples).all()
        assert tuple(cf.maps.shape) == (BS, 3, HW, HW) and torch.isfinite(cf.maps).all()
    dc.check_device_errors()
