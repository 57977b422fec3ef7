"""GPU: deterministic samplers and DDIM inversion — dc_solver_step against the torch expressions (bit for bit), `sample`, `invert` and
`counterfactual(start="invert")` on the small UNet (v) / DiT (eps) against the eager statement of solver.py driven through the same HIP
backbone's `forward` (two calls per pass), chunked launches, repeatability, `against=` / pixel space, a ragged prompt table, and the
number of backbone passes and step launches.

The model bound is 3e-4 max-abs, the project's bound for fp32 pair plans against two-call plans (test_gpu_counterfactual.BOUND)."""
import ctypes

import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import counterfactual as CF
from diffusion_classifier_amd import engine as E
from diffusion_classifier_amd import solver as S
from diffusion_classifier_amd.nets import unet as U
from diffusion_classifier_amd.utils.wavelet import wavelet_enc_2
from test_gpu_model import BASE, DEV, _small_dit_classifiers, make_pair
from test_gpu_prompt_model import BASE as PROMPT_BASE, _randomise_vectors

pytestmark = pytest.mark.gpu
BOUND = 3e-4
SEED = 7
STEPS = 4                                    # passes 1 and 2 of dpmpp_2m are second order


def ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ dc_solver_step
def _pair_layout(pc, pu, patch, ld):
    """[n, C, H, W] x 2 -> the prediction buffer of a batch-2 plan, rows 2b / 2b+1; the padding of ld holds NaN (never read)."""
    n, Cc, H, W = pc.shape
    pp = max(patch, 1)
    pair = torch.full((2 * n, H // pp, W // pp, ld), float("nan"))
    for b in range(n):
        for u, src in ((2 * b, pc[b]), (2 * b + 1, pu[b])):
            if patch > 1:                    # token (ty, tx), k = (py * p + px) * C + c
                pair[u, :, :, :Cc * pp * pp] = src.reshape(Cc, H // pp, pp, W // pp, pp).permute(1, 3, 2, 4, 0).reshape(H // pp, W // pp, -1)
            else:
                pair[u, :, :, :Cc] = src.permute(1, 2, 0)
    return pair


@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 0, 3),               # an element count that is no multiple of 256
                                   (3, 4, 8, 8, 2, 24),              # DiT's un-patchified layout with a padded ld
                                   (1, 12, 16, 16, 0, 16)])          # ld > C
def test_solver_step_equals_the_torch_expressions(shape):
    """Bit-equal to the torch evaluation of the header's expressions for the same fp32 scalars: v / eps, w in {0, 1.5}, clamp on / off,
    no history, history written only (pass 0 of 2M), history read and written to another buffer, history read and written in place
    (xhat aliasing xprev), final on / off.  The torch side is written as in test_ddpm_step_equals_the_torch_expressions."""
    n, Cc, H, W, patch, ld = shape
    lib = L.lib()
    torch.manual_seed(44)
    z, xprev = torch.randn(n, Cc, H, W), torch.randn(n, Cc, H, W).clamp(-1, 1)
    pc, pu = torch.randn(n, Cc, H, W) * 2, torch.randn(n, Cc, H, W) * 2
    lp, lt, ls = torch.tensor(-2.5), torch.tensor(-1.25), torch.tensor(0.75)
    a_t, a_s = torch.sqrt(torch.sigmoid(lt)), torch.sqrt(torch.sigmoid(ls))
    s_t, s_s = torch.sqrt(torch.sigmoid(-lt)), torch.sqrt(torch.sigmoid(-ls))
    h, h_prev = (ls - lt) / 2, (lt - lp) / 2
    k1, k2, k3 = s_s / s_t, -a_s * torch.special.expm1(-h), 0.5 * h / h_prev
    zd, pd, xpd = z.to(DEV), _pair_layout(pc, pu, patch, ld).to(DEV), xprev.to(DEV)
    seen_clamp = seen_final_clamp = False
    for v_param in (0, 1):
        for w in (0.0, 1.5):
            pred = (1 + w) * pc - w * pu
            for clamp in (0, 1):
                x = a_t * z - s_t * pred if v_param else (z - s_t * pred) / a_t
                seen_clamp |= bool((x.abs() > 1).any())
                if clamp:
                    x = torch.clamp(x, -1, 1)
                for hist in ("off", "write", "on", "alias"):
                    D = x + k3 * (x - xprev) if hist in ("on", "alias") else x
                    seen_final_clamp |= bool((D.abs() > 1).any())
                    for final in (0, 1):
                        want = torch.clamp(D, -1, 1) if final else k1 * z + k2 * D
                        out = torch.full((n, Cc, H, W), 9.0, device=DEV)
                        hin = xpd.clone() if hist in ("on", "alias") else None
                        hout = hin if hist == "alias" else None if hist == "off" else torch.full_like(out, 9.0)
                        p = L.SolverStepParams(z=ptr(zd), pred=ptr(pd), xprev=ptr(hin), xhat=ptr(hout), out=ptr(out), n=n, C=Cc, H=H, W=W,
                                               ld=ld, patch=patch, v_param=v_param, clamp=clamp, final_pass=final, w=w,
                                               one_plus_w=float(1.0 + w), alpha_t=float(a_t), sigma_t=float(s_t), k1=float(k1),
                                               k2=float(k2), k3=float(k3))
                        L.check(lib.dc_solver_step(ctypes.byref(p), L.stream_ptr()), "dc_solver_step")
                        tag = (v_param, w, clamp, hist, final)
                        assert torch.equal(out.cpu(), want), (tag, (out.cpu() - want).abs().max())
                        if hout is not None:
                            assert torch.equal(hout.cpu(), x), (tag, (hout.cpu() - x).abs().max())
                        if hist == "on":
                            assert torch.equal(hin, xpd)                                  # a history that is only read stays
    assert seen_clamp and seen_final_clamp                                                # both clamps do engage on these inputs


# ------------------------------------------------------------------------------------------------ models
def _build(kind):
    cfg = dict(BASE, cfg_w=2.0, sampling_steps=STEPS, classes=4, pred_param="v" if kind == "unet_v" else "eps")
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
    """The two backbones of test_gpu_counterfactual.py, BS = 2, K = 3, sampling_steps = 4, cfg_w = 2; the inverted latent and the
    unchunked inverted counterfactual are computed once (under dpmpp_2m) and left unchanged."""
    torch.manual_seed(101)
    dc, x = _build(request.param)
    cl = torch.tensor([[1, 3, 0], [2, 0, 3]])
    c0 = torch.tensor([3, 2])
    dc.config.sampler = "dpmpp_2m"
    zinv = dc.invert(x, c0, 0.5)
    cf = dc.counterfactual(x, cl, 0.5, start="invert", invert_class=c0)
    dc.config.sampler = None
    return dict(kind=request.param, dc=dc, x=x, cl=cl, c0=c0, zinv=zinv, cf=cf)


@pytest.fixture
def with_sampler(case):
    def set_(name):
        case["dc"].config.sampler = name
    yield set_
    case["dc"].config.sampler = None


@pytest.mark.parametrize("from_t", [1, 0.5])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_sample_matches_the_eager_statement(case, with_sampler, sampler, from_t):
    dc, x = case["dc"], case["x"]
    with_sampler(sampler)
    lab, other = torch.tensor([1, 3]).to(DEV), torch.tensor([2, 0]).to(DEV)
    torch.manual_seed(SEED)
    got = dc.sample(x, lab, from_t=from_t)
    torch.manual_seed(SEED)
    want = S.sample_eager(dc, x, lab, from_t, sampler)
    assert got.shape == x.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    d = (got - want).abs().max().item()
    print(f"{case['kind']} {sampler} from_t={from_t}: sample vs the eager statement: max abs difference {d:.2e} (bound {BOUND:g})")
    assert d < BOUND, d
    torch.manual_seed(SEED)
    far = (dc.sample(x, other, from_t=from_t) - got).abs().max().item()
    assert far > 10 * BOUND, far                                       # the labels do steer these models: the bound can see a mix-up
    # only the initial draw came from torch's generators
    after = torch.get_rng_state(), torch.cuda.get_rng_state(0)
    torch.manual_seed(SEED)
    S.initial_latent(dc, x, from_t)
    assert torch.equal(after[0], torch.get_rng_state()) and torch.equal(after[1], torch.cuda.get_rng_state(0))


@pytest.mark.parametrize("text", ["labels", None])
def test_invert_matches_the_eager_statement_and_repeats(case, text):
    dc, x = case["dc"], case["x"]
    lab = case["c0"] if text == "labels" else None
    before = torch.cuda.get_rng_state(0), torch.get_rng_state()
    got = dc.invert(x, lab, 0.5) if lab is not None else dc.invert(x)
    assert torch.equal(torch.cuda.get_rng_state(0), before[0]) and torch.equal(torch.get_rng_state(), before[1])
    assert got.shape == x.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    want = S.invert_eager(dc, x, S.label_rows(lab, 2, dc.config.classes, "text"), 0.5, 0.0)
    d = (got - want).abs().max().item()
    print(f"{case['kind']} text={text}: invert vs the eager statement: max abs difference {d:.2e} (bound {BOUND:g})")
    assert d < BOUND, d
    assert torch.equal(dc.invert(x, lab, 0.5), got)
    if lab is not None:
        assert torch.equal(got, case["zinv"])                          # whatever config.sampler says
        assert (got - dc.invert(x, torch.tensor([0, 1]), 0.5)).abs().max().item() > 10 * BOUND


def test_inverted_counterfactual_matches_k_decodes_of_the_inverted_latent(case, with_sampler):
    dc, x, cl, cf = case["dc"], case["x"], case["cl"], case["cf"]
    with_sampler("dpmpp_2m")
    assert cf.samples.dtype == torch.float32 and tuple(cf.samples.shape) == (2, 3) + tuple(x.shape[1:]) and torch.isfinite(cf.samples).all()
    want = torch.stack([S.decode_eager(dc, case["zinv"], cl[:, k].to(DEV), 0.5, "dpmpp_2m") for k in range(3)], dim=1)
    d = (cf.samples - want).abs().max().item()
    print(f"{case['kind']}: counterfactual(start='invert') vs K decodes of invert(x, c0): max abs difference {d:.2e} (bound {BOUND:g})")
    assert d < BOUND, d
    far = (want[:, 0] - want[:, 1]).abs().max().item()
    assert far > 10 * BOUND, far
    assert torch.equal(cf.maps, CF.abs_diff_map_torch(cf.samples.reshape((6,) + tuple(x.shape[1:])), x, torch.arange(2).repeat_interleave(3))
                       .view(cf.maps.shape))
    # exactly repeatable, and no generator is touched
    before = torch.cuda.get_rng_state(0), torch.get_rng_state()
    again = dc.counterfactual(x, cl, 0.5, start="invert", invert_class=case["c0"])
    assert torch.equal(torch.cuda.get_rng_state(0), before[0]) and torch.equal(torch.get_rng_state(), before[1])
    assert torch.equal(again.samples, cf.samples) and torch.equal(again.maps, cf.maps)
    # against a class: the maps are taken to that class's trajectory of the same image
    ag = dc.counterfactual(x, cl, 0.5, start="invert", invert_class=case["c0"], against=torch.tensor([3, 2]).to(DEV))   # columns 1, 0
    base = torch.stack([ag.samples[0, 1], ag.samples[1, 0]])
    maps = torch.zeros_like(ag.maps)
    for c in range(x.shape[1]):
        maps = maps + (ag.samples[:, :, c] - base[:, None, c]).abs()
    assert torch.equal(ag.samples, cf.samples) and torch.equal(ag.maps, maps) and float(ag.maps[0, 1].max()) == 0.0


def test_one_image_per_chunk_matches_the_unchunked_call(case, with_sampler):
    dc, x = case["dc"], case["x"]
    with_sampler("dpmpp_2m")
    dc.config.units_per_launch = 6                                     # 2 * K units an image: every image its own chunk
    try:
        got = dc.counterfactual(x, case["cl"], 0.5, start="invert", invert_class=case["c0"])
    finally:
        dc.config.units_per_launch = None
    bb = dc.ema.ema_model
    assert {k[1] for k in bb._plans if k[0] == "pair_session" and k[2] == 3} == {0, 1}     # two sessions of K = 3 trajectories
    d = (got.samples - case["cf"].samples).abs().max().item()
    print(f"{case['kind']}: one image per chunk vs one launch: max abs difference {d:.2e} (bound {BOUND:g})")
    assert d < BOUND, d


def test_noise_start_under_a_deterministic_sampler(case, with_sampler):
    """start='noise': K deterministic trajectories from one draw — the reseeded `sample` calls, and Philox touches no generator."""
    dc, x, cl = case["dc"], case["x"], case["cl"]
    with_sampler("ddim")
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, cl, 0.5)
    want = []
    for k in range(3):
        torch.manual_seed(SEED)
        want.append(dc.sample(x, cl[:, k].to(DEV), from_t=0.5))
    d = (cf.samples - torch.stack(want, dim=1)).abs().max().item()
    print(f"{case['kind']}: ddim counterfactual vs K reseeded sample() calls: max abs difference {d:.2e} (bound {BOUND:g})")
    assert d < BOUND, d
    before = torch.cuda.get_rng_state(0), torch.get_rng_state()
    a = dc.counterfactual(x, cl, 0.5, rng="philox", seed=11)
    assert torch.equal(torch.cuda.get_rng_state(0), before[0]) and torch.equal(torch.get_rng_state(), before[1])
    b = dc.counterfactual(x, cl, 0.5, rng="philox", seed=11)
    c = dc.counterfactual(x, cl, 0.5, rng="philox", seed=12)
    assert torch.isfinite(a.samples).all() and torch.equal(a.samples, b.samples) and not torch.equal(a.samples, c.samples)


# ------------------------------------------------------------------------------------------------ pass counts
def test_context_plan_runs_once_per_session_and_a_step_launch_per_step_and_chunk(monkeypatch):
    """A deterministic counterfactual: the context plan once per call and chunk, sampling_steps backbone passes and step launches per
    chunk (ancestral DDPM: sampling_steps + 1).  start='invert' adds the inversion's own session per chunk (its contexts are those of
    invert_class: one more context-plan run) and sampling_steps more passes and launches."""
    dc, x = _build("unet_v")
    dc.config.sampler = "dpmpp_2m"
    ctx, passes, launches = [], [], []
    real_ctx, real_step = E.UNetPlan.run_ctx, U.PairSession.step
    lib = L.lib()
    real_launch = lib.dc_solver_step
    monkeypatch.setattr(E.UNetPlan, "run_ctx", lambda self: (ctx.append(self), real_ctx(self))[1])
    monkeypatch.setattr(U.PairSession, "step", lambda self, *a: (passes.append(self), real_step(self, *a))[1])
    monkeypatch.setattr(lib, "dc_solver_step", lambda *a: (launches.append(a), real_launch(*a))[1])
    cl = torch.tensor([1, 3, 0])
    dc.counterfactual(x, cl, 0.5)                                      # one chunk
    assert (len(ctx), len(passes), len(launches)) == (1, STEPS, STEPS)
    for lst in (ctx, passes, launches):
        del lst[:]
    dc.counterfactual(x, cl, 0.5, start="invert", invert_class=torch.tensor([1, 2]))
    assert (len(ctx), len(passes), len(launches)) == (2, 2 * STEPS, 2 * STEPS)
    for lst in (ctx, passes, launches):
        del lst[:]
    dc.config.units_per_launch = 2                                     # every image its own chunk, in the inversion too
    dc.counterfactual(x, cl, 0.5, start="invert", invert_class=torch.tensor([1, 2]))
    assert (len(ctx), len(passes), len(launches)) == (2 + 2, 2 * 2 * STEPS, 2 * 2 * STEPS)
    for lst in (ctx, passes, launches):
        del lst[:]
    dc.config.units_per_launch = None
    dc.config.sampler = None                                           # the ancestral path launches none of the new steps
    dc.counterfactual(x, cl, 0.5)
    assert (len(ctx), len(passes), len(launches)) == (1, STEPS + 1, 0)


# ------------------------------------------------------------------------------------------------ a ragged prompt table
def test_ragged_prompt_table_matches_the_eager_statement():
    cfg = dict(PROMPT_BASE, cfg_w=2.0, sampling_steps=STEPS, classes=3, pred_param="v", prompt_tokens=3, sampler="dpmpp_2m")
    torch.manual_seed(133)
    m = dca.UNetCondition2D(**dca.small_unet_kwargs())
    _randomise_vectors(m)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg))
    with torch.no_grad():
        dc.encoder.weight.mul_(3.0)
    dc.encoder.set_lengths([3, 2, 3, 1])                               # class prompts of 3, 2, 3 tokens, a null prompt of 1
    dc = dc.to(DEV)
    x = (torch.rand(2, 3, 32, 32) * 2 - 1).to(DEV)
    cl, c0 = torch.tensor([[1, 0, 2], [2, 1, 1]]), torch.tensor([1, 0])
    cf = dc.counterfactual(x, cl, 0.5, start="invert", invert_class=c0)
    bb = dc.ema.ema_model
    assert all(k[-1] == "varlen" for k in bb._plans if k[0] == "pair_session")
    zinv = S.invert_eager(dc, x, c0, 0.5, 0.0)
    want = torch.stack([S.decode_eager(dc, zinv, cl[:, k].to(DEV), 0.5, "dpmpp_2m") for k in range(3)], dim=1)
    d = (cf.samples - want).abs().max().item()
    print(f"ragged 3-token table: counterfactual(start='invert') vs the eager statement: max abs difference {d:.2e} (bound {BOUND:g})")
    assert d < BOUND, d


# ------------------------------------------------------------------------------------------------ pixel space
def test_pixel_space_is_the_inverse_haar_transform_of_the_raw_samples():
    kw = dict(dca.small_unet_kwargs(), sample_size=16, in_channels=12, out_channels=12)
    cfg = dict(BASE, cfg_w=2.0, sampling_steps=2, classes=3, pred_param="v", image_size=16, noise_d=16, sampler="ddim")
    m, _ = make_pair(kw, seed=35)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg)).to(DEV)
    x = (torch.rand(2, 12, 16, 16) * 2 - 1).to(DEV)
    c0 = torch.tensor([0, 2])
    raw = dc.counterfactual(x, None, 0.5, start="invert", invert_class=c0)
    pix = dc.counterfactual(x, None, 0.5, start="invert", invert_class=c0, pixel_space=True)
    assert tuple(raw.samples.shape) == (2, 3, 12, 16, 16) and tuple(pix.samples.shape) == (2, 3, 3, 32, 32)
    want = wavelet_enc_2(raw.samples.reshape(6, 12, 16, 16) * 2).view(2, 3, 3, 32, 32)
    assert torch.equal(pix.samples, want)
    base = wavelet_enc_2(x * 2)
    maps = torch.zeros_like(pix.maps)
    for c in range(3):
        maps = maps + (want[:, :, c] - base[:, None, c]).abs()
    assert torch.equal(pix.maps, maps)
