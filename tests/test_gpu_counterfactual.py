"""GPU: counterfactual sampling — dc_ddpm_step_shared against dc_ddpm_step on repeated noise and dc_abs_diff_map against its torch
statement (bit for bit), `DiffusionClassifier.counterfactual` on the small UNet / DiT against K calls of `sample` with the seed reset in
front of each, chunked launches, shared noise, the Philox mode, a ragged prompt table, pixel space, and the once-per-call context plan.

The model bound is 3e-4 max-abs: what test_sample_batch2_plan_with_fused_step_matches_the_two_call_path gives to fp32 plans of
different launch shapes on these models and step counts (here: BS * K images a launch against BS)."""
import ctypes

import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import counterfactual as CF
from diffusion_classifier_amd import engine as E
from diffusion_classifier_amd.utils.wavelet import wavelet_enc_2
from test_gpu_model import BASE, DEV, _small_dit_classifiers, make_pair
from test_gpu_prompt_model import BASE as PROMPT_BASE, _randomise_vectors

pytestmark = pytest.mark.gpu
BOUND = 3e-4
SEED = 7
FROM_T = 0.8


def ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ dc_ddpm_step_shared
@pytest.mark.parametrize("shape", [(2, 3, 3, 5, 7, 0, 3),            # an element count that is no multiple of 256
                                   (1, 1, 3, 8, 8, 0, 4),            # noise_div = 1
                                   (2, 3, 4, 8, 8, 4, 72),           # DiT's un-patchified layout, ld > C * 16
                                   (2, 3, 3, 384, 320, 0, 4)])       # > 8192 x 256 elements: the grid-stride loop wraps
def test_ddpm_step_shared_equals_ddpm_step_on_repeated_noise(shape):
    n_img, K, Cc, H, W, patch, ld = shape
    n = n_img * K
    lib = L.lib()
    g = torch.Generator(device=DEV).manual_seed(3)
    z = torch.randn(n, Cc, H, W, device=DEV, generator=g)
    noise = torch.randn(n_img, Cc, H, W, device=DEV, generator=g)
    pp = max(patch, 1)
    pred = torch.randn(2 * n, H // pp, W // pp, ld, device=DEV, generator=g) * 2
    rep = noise.repeat_interleave(K, dim=0).contiguous()
    if n * Cc * H * W > 8192 * 256:
        assert n_img * Cc * H * W < 8192 * 256                        # (the wrap is reached by the trajectories, not by the noise)
    sc = dict(w=1.5, alpha_t=0.8, sigma_t=0.6, alpha_s=0.9, c=0.3, sd=0.2, one_plus_w=2.5)
    for v_param in (0, 1):
        for with_noise in (True, False):
            want = torch.full_like(z, 9.0)
            got = torch.full_like(z, -9.0)
            p0 = L.DdpmStepParams(z=ptr(z), pred=ptr(pred), noise=ptr(rep) if with_noise else None, out=ptr(want), n=n, C=Cc, H=H, W=W,
                                  ld=ld, patch=patch, v_param=v_param, **sc)
            L.check(lib.dc_ddpm_step(ctypes.byref(p0), L.stream_ptr()), "dc_ddpm_step")
            p1 = L.DdpmStepSharedParams(z=ptr(z), pred=ptr(pred), noise=ptr(noise) if with_noise else None, out=ptr(got), n=n, C=Cc, H=H,
                                        W=W, ld=ld, patch=patch, v_param=v_param, noise_div=K, pad_=0, **sc)
            L.check(lib.dc_ddpm_step_shared(ctypes.byref(p1), L.stream_ptr()), "dc_ddpm_step_shared")
            assert torch.isfinite(want).all() and float(want.abs().max()) != 9.0
            assert torch.equal(got, want), (v_param, with_noise, (got - want).abs().max().item())
            if with_noise and K > 1:
                assert not torch.equal(got[0], got[1])                 # (trajectories of an image do differ: z and pred do)


# ------------------------------------------------------------------------------------------------ dc_abs_diff_map
@pytest.mark.parametrize("shape,r_of_a", [((6, 3, 5, 7), [3, 0, 3, 3, 5, 0]),          # rows 1, 2, 4 skipped, 0 and 3 repeated
                                          ((4, 12, 16, 16), [1, 1, 0, 1])])
def test_abs_diff_map_equals_the_sequential_torch_sum(shape, r_of_a):
    n, Cc, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(5)
    a = torch.randn(n, Cc, H, W, device=DEV, generator=g)
    r = torch.randn(max(r_of_a) + 1, Cc, H, W, device=DEV, generator=g)
    idx = torch.tensor(r_of_a)
    got = CF.abs_diff_map_hip(a, r, idx)
    want = torch.zeros(n, H, W, device=DEV)
    for c in range(Cc):                                               # c ascending, fp32
        want = want + (a[:, c] - r[idx.to(DEV), c]).abs()
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, H, W)
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert torch.equal(CF.abs_diff_map_torch(a, r, idx), want)
    # a row index outside r reads nothing and poisons its map
    bad = CF.abs_diff_map_hip(a, r, torch.tensor([r.shape[0]] + r_of_a[1:]))
    assert torch.isnan(bad[0]).all() and torch.equal(bad[1:], want[1:])


# ------------------------------------------------------------------------------------------------ models
def _reseeded(dc, x, cl, from_t=FROM_T):
    outs = []
    for k in range(cl.shape[1]):
        torch.manual_seed(SEED)
        outs.append(dc.sample(x, cl[:, k].to(DEV), from_t=from_t))
    return torch.stack(outs, dim=1)


def _build(kind):
    cfg = dict(BASE, cfg_w=2.0, sampling_steps=3, classes=4, pred_param="v" if kind == "unet_v" else "eps")
    if kind == "unet_v":
        m, _ = make_pair(dca.small_unet_kwargs(), seed=33)
        dc = dca.DiffusionClassifier(m, dca.Config(**cfg)).to(DEV)
        x = torch.rand(2, 3, 32, 32) * 2 - 1
    else:
        dc, _ = _small_dit_classifiers(dict(cfg, encoder_type="DiT", image_size=16, noise_d=16))
        x = torch.rand(2, 4, 16, 16) * 2 - 1
    return dc, x.to(DEV)


@pytest.fixture(scope="module", params=["unet_v", "dit_eps"])
def case(request):
    """The models and settings of test_sample_batch2_plan_with_fused_step_matches_the_two_call_path, BS = 2, K = 3; the K reseeded
    `sample` calls and the unchunked counterfactual call are computed once and left unchanged."""
    dc, x = _build(request.param)
    cl = torch.tensor([[1, 3, 0], [2, 0, 3]])
    want = _reseeded(dc, x, cl)
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, cl, FROM_T)
    return dict(kind=request.param, dc=dc, x=x, cl=cl, want=want, cf=cf)


def test_counterfactual_matches_k_reseeded_sample_calls(case):
    cf, want, x = case["cf"], case["want"], case["x"]
    assert cf.samples.dtype == torch.float32 and cf.samples.device == x.device
    assert tuple(cf.samples.shape) == (2, 3) + tuple(x.shape[1:]) and torch.isfinite(cf.samples).all()
    assert torch.equal(cf.classes.cpu(), case["cl"])
    d = (cf.samples - want).abs().max().item()
    print(f"{case['kind']}: counterfactual vs K reseeded sample() calls: max abs difference {d:.2e} (bound {BOUND:g})")
    assert d < BOUND, d
    far = (want[:, 0] - want[:, 1]).abs().max().item()
    assert far > 10 * BOUND, far                                       # the labels do steer these models: the bound can see a mix-up
    # the maps of the call are the statement on its own samples
    assert torch.equal(cf.maps, CF.abs_diff_map_torch(cf.samples.reshape((6,) + tuple(x.shape[1:])), x, torch.arange(2).repeat_interleave(3))
                       .view(cf.maps.shape))


def test_one_image_per_chunk_matches_the_unchunked_call(case):
    dc, x = case["dc"], case["x"]
    dc.config.units_per_launch = 6                                     # 2 * K units an image: every image its own chunk
    try:
        torch.manual_seed(SEED)
        got = dc.counterfactual(x, case["cl"], FROM_T)
    finally:
        dc.config.units_per_launch = None
    bb = dc.ema.ema_model
    assert {k[1] for k in bb._plans if k[0] == "pair_session" and k[2] == 3} == {0, 1}     # two sessions of K = 3 trajectories
    d = (got.samples - case["cf"].samples).abs().max().item()
    print(f"{case['kind']}: one image per chunk vs one launch: max abs difference {d:.2e} (bound {BOUND:g})")
    assert d < BOUND, d


def test_trajectories_of_one_class_share_their_noise(case):
    dc, x = case["dc"], case["x"]
    torch.manual_seed(SEED)
    got = dc.counterfactual(x, torch.tensor([2, 2, 2]), FROM_T).samples
    d = max((got[:, 0] - got[:, k]).abs().max().item() for k in (1, 2))
    print(f"{case['kind']}: three trajectories of class 2: max abs difference {d:.2e} (bound {BOUND:g}; unshared noise: O(1))")
    assert d < BOUND, d


def test_philox_noise_is_reproducible_and_keyed_by_the_seed(case):
    dc, x, cl = case["dc"], case["x"], case["cl"]
    torch.manual_seed(1)
    before = torch.cuda.get_rng_state(0), torch.get_rng_state()
    a = dc.counterfactual(x, cl, FROM_T, rng="philox", seed=11)
    assert torch.equal(torch.cuda.get_rng_state(0), before[0]) and torch.equal(torch.get_rng_state(), before[1])   # no generator touched
    torch.manual_seed(2)
    b = dc.counterfactual(x, cl, FROM_T, rng="philox", seed=11)
    c = dc.counterfactual(x, cl, FROM_T, rng="philox", seed=12)
    assert torch.isfinite(a.samples).all()
    assert torch.equal(a.samples, b.samples) and torch.equal(a.maps, b.maps)
    assert not torch.equal(a.samples, c.samples)
    full = dc.counterfactual(x, cl, 1, rng="philox", seed=11)          # from pure noise
    assert torch.isfinite(full.samples).all() and not torch.equal(full.samples, a.samples)


def test_against_a_class_on_the_device(case):
    dc, x, cl = case["dc"], case["x"], case["cl"]
    torch.manual_seed(SEED)
    got = dc.counterfactual(x, cl, FROM_T, against=torch.tensor([3, 2]).to(DEV))          # columns 1 and 0
    s = got.samples
    base = torch.stack([s[0, 1], s[1, 0]])
    want = torch.zeros_like(got.maps)
    for c in range(s.shape[2]):
        want = want + (s[:, :, c] - base[:, None, c]).abs()
    assert torch.equal(got.maps, want)
    assert float(got.maps[0, 1].max()) == 0.0 and float(got.maps[1, 0].max()) == 0.0 and float(got.maps[0, 0].max()) > 0.0


def test_context_plan_runs_once_per_call_and_once_per_step_through_sample(monkeypatch):
    dc, x = _build("unet_v")
    calls = []
    real = E.UNetPlan.run_ctx

    def counting(self):
        calls.append(self)
        return real(self)
    monkeypatch.setattr(E.UNetPlan, "run_ctx", counting)
    dc.counterfactual(x, torch.tensor([1, 3, 0]), FROM_T)              # 3 steps, one chunk
    assert len(calls) == 1
    del calls[:]
    dc.sample(x, torch.tensor([1, 3]).to(DEV), from_t=FROM_T)
    assert len(calls) == dc.config.sampling_steps + 1                  # unchanged: every pass of `sample` (3 steps + the final mean)


# ------------------------------------------------------------------------------------------------ a ragged prompt table
def test_ragged_prompt_table_matches_reseeded_sample():
    cfg = dict(PROMPT_BASE, cfg_w=2.0, sampling_steps=3, classes=3, pred_param="v", prompt_tokens=3)
    torch.manual_seed(133)
    m = dca.UNetCondition2D(**dca.small_unet_kwargs())
    _randomise_vectors(m)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg))
    with torch.no_grad():
        dc.encoder.weight.mul_(3.0)
    dc.encoder.set_lengths([3, 2, 3, 1])                               # class prompts of 3, 2, 3 tokens, a null prompt of 1
    dc = dc.to(DEV)
    x = (torch.rand(2, 3, 32, 32) * 2 - 1).to(DEV)
    cl = torch.tensor([[1, 0, 2], [2, 1, 1]])
    want = _reseeded(dc, x, cl)
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, cl, FROM_T)
    bb = dc.ema.ema_model
    (key,) = [k for k in bb._plans if k[0] == "pair_session"]
    assert key[-1] == "varlen"
    assert bb._plans[key].ctx_len.tolist() == [2, 1, 3, 1, 3, 1, 3, 1, 2, 1, 2, 1]        # 2u = cond, 2u + 1 = null of trajectory u
    d = (cf.samples - want).abs().max().item()
    print(f"ragged 3-token table: counterfactual vs K reseeded sample() calls: max abs difference {d:.2e} (bound {BOUND:g})")
    assert d < BOUND, d


# ------------------------------------------------------------------------------------------------ pixel space
def test_pixel_space_is_the_inverse_haar_transform_of_the_raw_samples():
    kw = dict(dca.small_unet_kwargs(), sample_size=16, in_channels=12, out_channels=12)
    cfg = dict(BASE, cfg_w=2.0, sampling_steps=2, classes=3, pred_param="v", image_size=16, noise_d=16)
    m, _ = make_pair(kw, seed=35)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg)).to(DEV)
    x = (torch.rand(2, 12, 16, 16) * 2 - 1).to(DEV)
    torch.manual_seed(SEED)
    raw = dc.counterfactual(x, None, 0.5)
    torch.manual_seed(SEED)
    pix = dc.counterfactual(x, None, 0.5, pixel_space=True)
    assert tuple(raw.samples.shape) == (2, 3, 12, 16, 16) and tuple(pix.samples.shape) == (2, 3, 3, 32, 32)
    assert tuple(pix.maps.shape) == (2, 3, 32, 32)
    want = wavelet_enc_2(raw.samples.reshape(6, 12, 16, 16) * 2).view(2, 3, 3, 32, 32)
    assert torch.equal(pix.samples, want)
    base = wavelet_enc_2(x * 2)
    maps = torch.zeros_like(pix.maps)
    for c in range(3):
        maps = maps + (want[:, :, c] - base[:, None, c]).abs()
    assert torch.equal(pix.maps, maps)
    torch.manual_seed(SEED)
    pa = dc.counterfactual(x, None, 0.5, against=torch.tensor([1, 2]), pixel_space=True)
    maps = torch.zeros_like(pix.maps)
    for c in range(3):
        maps = maps + (want[:, :, c] - torch.stack([want[0, 1, c], want[1, 2, c]])[:, None]).abs()
    assert torch.equal(pa.maps, maps)
