"""GPU: edit-friendly DDPM inversion — dc_ddpm_noise_map against the torch expressions (bit for bit) and there and back through
dc_ddpm_step_shared (the derived bound), `invert_ddpm` and `counterfactual(start="ddpm_invert")` on the small UNet (v) / DiT (eps)
against the eager statement driven through the same HIP backbone's `forward` (two calls per pass), the own-class property, chunked
launches, Philox, `against=` / pixel space, a ragged prompt table, and the launch counts.

The model bound is 3e-4 max-abs, the project's bound for fp32 pair plans against two-call plans (test_gpu_counterfactual.BOUND).  Seen
on an MI355X (max-abs against the eager statement; start / noise[i] * sd_i / samples):
  unet_v   0 / 5.73e-7 / 4.22e-6;  own-class sample against the last pass on x_n: 4.51e-6
  dit_eps  0 / 4.30e-7 / 9.54e-7;  own-class sample against the last pass on x_n: 1.37e-6
  ragged 3-token table: noise[i] * sd_i 4.30e-7, samples 3.76e-6;  one image per chunk against one launch: the same bits on both models
The round trip of one step through the two kernels stays at 0.56 of the derived bound at most (0.35 / 0.53 / 0.56 on the three shapes)."""
import ctypes

import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import counterfactual as CF
from diffusion_classifier_amd import ddpm_invert as DI
from diffusion_classifier_amd import engine as E
from diffusion_classifier_amd import solver as S
from diffusion_classifier_amd.nets import unet as U
from diffusion_classifier_amd.utils.wavelet import wavelet_enc_2
from test_gpu_model import BASE, DEV, _small_dit_classifiers, make_pair
from test_gpu_prompt_model import BASE as PROMPT_BASE, _randomise_vectors

pytestmark = pytest.mark.gpu
BOUND = 3e-4
SEED = 7
STEPS, BS = 4, 2
SHAPES = [(2, 3, 5, 7, 0, 3),                # an element count that is no multiple of 256
          (3, 4, 8, 8, 2, 24),               # DiT's un-patchified layout with a padded ld
          (1, 12, 16, 16, 0, 16)]            # ld > C


def ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ dc_ddpm_noise_map
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


def _operands(shape):
    n, Cc, H, W, patch, ld = shape
    torch.manual_seed(44)
    z, x_next = torch.randn(n, Cc, H, W), torch.randn(n, Cc, H, W)
    pc, pu = torch.randn(n, Cc, H, W) * 2, torch.randn(n, Cc, H, W) * 2
    lt, ls = torch.tensor(-1.25), torch.tensor(0.75)
    c = -torch.special.expm1(lt - ls)
    a_t, a_s, s_t = torch.sqrt(torch.sigmoid(lt)), torch.sqrt(torch.sigmoid(ls)), torch.sqrt(torch.sigmoid(-lt))
    return z, x_next, pc, pu, c, a_t, a_s, s_t


def _mean(z, pc, pu, w, v_param, c, a_t, a_s, s_t):
    """(mu, the unclipped data prediction) by the header's expressions, written as test_ddpm_step_equals_the_torch_expressions does."""
    pred = (1 + w) * pc - w * pu
    xp = a_t * z - s_t * pred if v_param else (z - s_t * pred) / a_t
    return a_s * (z * (1 - c) / a_t + c * torch.clamp(xp, -1, 1)), xp


@pytest.mark.parametrize("shape", SHAPES)
def test_noise_map_equals_the_torch_expressions(shape):
    """Bit-equal to the torch evaluation of the header's expressions for the same fp32 scalars: v / eps, w in {0, 1.5}, sd in {5.5e-4,
    0.4}, out in a buffer of its own (x_next stays) and out aliasing x_next."""
    n, Cc, H, W, patch, ld = shape
    lib = L.lib()
    z, x_next, pc, pu, c, a_t, a_s, s_t = _operands(shape)
    zd, pd = z.to(DEV), _pair_layout(pc, pu, patch, ld).to(DEV)
    seen_clip = False
    for v_param in (0, 1):
        for w in (0.0, 1.5):
            mu, xp = _mean(z, pc, pu, w, v_param, c, a_t, a_s, s_t)
            seen_clip |= bool((xp.abs() > 1).any())
            for sd in (torch.tensor(5.5e-4), torch.tensor(0.4)):
                want = (x_next - mu) / sd
                for alias in (False, True):
                    xn = x_next.to(DEV)
                    out = xn if alias else torch.full((n, Cc, H, W), 9.0, device=DEV)
                    p = L.DdpmNoiseMapParams(z=ptr(zd), pred=ptr(pd), x_next=ptr(xn), out=ptr(out), n=n, C=Cc, H=H, W=W, ld=ld, patch=patch,
                                             v_param=v_param, w=w, one_plus_w=float(1.0 + w), alpha_t=float(a_t), sigma_t=float(s_t),
                                             alpha_s=float(a_s), c=float(c), sd=float(sd))
                    L.check(lib.dc_ddpm_noise_map(ctypes.byref(p), L.stream_ptr()), "dc_ddpm_noise_map")
                    tag = (v_param, w, float(sd), alias)
                    assert torch.equal(out.cpu(), want), (tag, (out.cpu() - want).abs().max())
                    if not alias:
                        assert torch.equal(xn.cpu(), x_next), tag                         # an x_next that is only read stays
    assert seen_clip                                                                      # the clip does engage on these inputs


@pytest.mark.parametrize("shape", SHAPES)
def test_noise_map_and_shared_step_are_inverse_within_the_derived_bound(shape):
    """dc_ddpm_step_shared fed the maps of dc_ddpm_noise_map lands on x_next again: mu + ((x_next - mu) / sd) * sd rounds four times,
    |out - x_next| <= 2^-22 (|x_next| + |x_next - mu|) per element (test_ddpm_invert_host.py derives it).  noise_div = 1: a map per
    trajectory; noise_div = 3: three trajectories of an image (the same z and prediction) read its one map."""
    n, Cc, H, W, patch, ld = shape
    lib = L.lib()
    z, x_next, pc, pu, c, a_t, a_s, s_t = _operands(shape)
    worst = 0.0
    for v_param in (0, 1):
        for w in (0.0, 1.5):
            mu, _ = _mean(z, pc, pu, w, v_param, c, a_t, a_s, s_t)
            bound = 2.0 ** -22 * (x_next.abs() + (x_next - mu).abs())
            for sd in (5.5e-4, 0.4):
                sc = dict(w=w, one_plus_w=float(1.0 + w), alpha_t=float(a_t), sigma_t=float(s_t), alpha_s=float(a_s), c=float(c), sd=sd)
                zd, xn, pd = z.to(DEV), x_next.to(DEV), _pair_layout(pc, pu, patch, ld).to(DEV)
                maps = torch.full((n, Cc, H, W), 9.0, device=DEV)
                p = L.DdpmNoiseMapParams(z=ptr(zd), pred=ptr(pd), x_next=ptr(xn), out=ptr(maps), n=n, C=Cc, H=H, W=W, ld=ld, patch=patch,
                                         v_param=v_param, **sc)
                L.check(lib.dc_ddpm_noise_map(ctypes.byref(p), L.stream_ptr()), "dc_ddpm_noise_map")
                for K in (1, 3):
                    zk = zd.repeat_interleave(K, dim=0).contiguous()
                    pk = _pair_layout(pc.repeat_interleave(K, dim=0), pu.repeat_interleave(K, dim=0), patch, ld).to(DEV)
                    out = torch.full((n * K, Cc, H, W), 9.0, device=DEV)
                    q = L.DdpmStepSharedParams(z=ptr(zk), pred=ptr(pk), noise=ptr(maps), out=ptr(out), n=n * K, C=Cc, H=H, W=W, ld=ld,
                                               patch=patch, v_param=v_param, noise_div=K, pad_=0, **sc)
                    L.check(lib.dc_ddpm_step_shared(ctypes.byref(q), L.stream_ptr()), "dc_ddpm_step_shared")
                    err = (out.cpu().view(n, K, Cc, H, W) - x_next[:, None]).abs()
                    worst = max(worst, float((err / bound[:, None].clamp_min(1e-30)).max()))
                    assert bool((err <= bound[:, None]).all()), (v_param, w, sd, K, float(err.max()))
    print(f"{shape}: worst |step(map) - x_next| / bound = {worst:.2f}")


# ------------------------------------------------------------------------------------------------ models
def _build(kind):
    cfg = dict(BASE, cfg_w=2.0, sampling_steps=STEPS, classes=4, pred_param="v" if kind == "unet_v" else "eps")
    if kind == "unet_v":
        m, _ = make_pair(dca.small_unet_kwargs(), seed=33)
        dc = dca.DiffusionClassifier(m, dca.Config(**cfg)).to(DEV)
        x = torch.rand(BS, 3, 32, 32) * 2 - 1
    else:
        dc, _ = _small_dit_classifiers(dict(cfg, encoder_type="DiT", image_size=16, noise_d=16))
        x = torch.rand(BS, 4, 16, 16) * 2 - 1
    return dc, x.to(DEV)


def _sds(dc, from_t=0.5):
    lams = S.grid_lams(dc, from_t, 0.0)
    return [dc._sampler_step_scalars(lams[i], lams[i + 1])[4] for i in range(len(lams) - 1)]


def _eager_pass(dc, z, lab, lam_t, lam_s):
    """(mu, var) of one ancestral step at z under labels `lab`: two calls of the backbone's forward and `ddpm_sampler_step`."""
    cond, null, lens = S.contexts(dc, lab.to(DEV), DEV, dc.ema.ema_model)
    kc = {"encoder_lengths": lens["cond"]} if lens else {}
    kn = {"encoder_lengths": lens["null"]} if lens else {}
    lam_t, lam_s = lam_t.to(DEV).unsqueeze(0), lam_s.to(DEV).unsqueeze(0)
    pred = dc.ema(z, lam_t, encoder_hidden_states=cond, **kc)
    u_pred = dc.ema(z, lam_t, encoder_hidden_states=null, **kn)
    return dc.ddpm_sampler_step(z, pred, u_pred, lam_t.clone(), lam_s.clone())


def _eager_decode(dc, start, noise, lab, from_t=0.5):
    """The ancestral sampler from `start` adding noise[i] in step i, then its last pass (the lambda and scalars of step n - 1)."""
    lams = S.grid_lams(dc, from_t, 0.0)
    n = len(lams) - 1
    z = start
    for i in range(n):
        mu, var = _eager_pass(dc, z, lab, lams[i], lams[i + 1])
        z = mu + noise[i] * torch.sqrt(var)
    return dc.clip(_eager_pass(dc, z, lab, lams[n - 1], lams[n])[0])


@pytest.fixture(scope="module", params=["unet_v", "dit_eps"])
def case(request):
    """The two backbones of test_gpu_counterfactual.py, BS = 2, K = 3, sampling_steps = 4, cfg_w = 2; the inversion, the unchunked
    counterfactual (column 0: the inversion's own class) and the eager inversion are computed once and left unchanged."""
    torch.manual_seed(101)
    dc, x = _build(request.param)
    c0 = torch.tensor([3, 2])
    cl = torch.tensor([[3, 1, 0], [2, 0, 3]])
    torch.manual_seed(SEED)
    inv = dc.invert_ddpm(x, c0, 0.5)
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=c0)
    torch.manual_seed(SEED)
    start_e, noise_e = DI.run_eager(dc, x, c0, 0.5, 2.0)
    return dict(kind=request.param, dc=dc, x=x, cl=cl, c0=c0, inv=inv, cf=cf, start_e=start_e, noise_e=noise_e)


def test_inversion_matches_the_eager_statement(case):
    dc, x, inv = case["dc"], case["x"], case["inv"]
    assert isinstance(inv, dca.DdpmInversion) and inv.from_t == 0.5 and inv.guidance == 2.0
    assert inv.start.dtype == inv.noise.dtype == torch.float32 and inv.noise.device == x.device
    assert tuple(inv.start.shape) == tuple(x.shape) and tuple(inv.noise.shape) == (STEPS,) + tuple(x.shape)
    assert torch.isfinite(inv.noise).all()
    sds = _sds(dc)
    d0 = (inv.start - case["start_e"]).abs().max().item()
    dn = [((inv.noise[i] - case["noise_e"][i]) * sds[i]).abs().max().item() for i in range(STEPS)]
    print(f"{case['kind']}: invert_ddpm vs the eager statement: start {d0:.2e}, noise[i] * sd_i {[f'{v:.2e}' for v in dn]} (bound {BOUND:g})")
    assert d0 < BOUND and max(dn) < BOUND
    torch.manual_seed(SEED)
    far = dc.invert_ddpm(x, torch.tensor([0, 1]), 0.5)
    assert max(((far.noise[i] - inv.noise[i]) * sds[i]).abs().max().item() for i in range(STEPS)) > 10 * BOUND     # the labels do steer


def test_counterfactual_matches_the_eager_statement_and_the_own_class_comes_back(case):
    dc, x, cl, cf = case["dc"], case["x"], case["cl"], case["cf"]
    assert cf.samples.dtype == torch.float32 and tuple(cf.samples.shape) == (BS, 3) + tuple(x.shape[1:]) and torch.isfinite(cf.samples).all()
    want = torch.stack([_eager_decode(dc, case["start_e"], case["noise_e"], cl[:, k]) for k in range(3)], dim=1)
    d = (cf.samples - want).abs().max().item()
    print(f"{case['kind']}: counterfactual(start='ddpm_invert') vs the eager statement: max abs difference {d:.2e} (bound {BOUND:g})")
    assert d < BOUND, d
    far = (want[:, 0] - want[:, 1]).abs().max().item()
    assert far > 10 * BOUND, far
    assert torch.equal(cf.maps, CF.abs_diff_map_torch(cf.samples.reshape((BS * 3,) + tuple(x.shape[1:])), x, torch.arange(BS).repeat_interleave(3))
                       .view(cf.maps.shape))
    # against a class: the maps are taken to that class's trajectory of the same image
    torch.manual_seed(SEED)
    ag = dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=case["c0"], against=torch.tensor([1, 2]).to(DEV))   # columns 1, 0
    base = torch.stack([ag.samples[0, 1], ag.samples[1, 0]])
    maps = torch.zeros_like(ag.maps)
    for c in range(x.shape[1]):
        maps = maps + (ag.samples[:, :, c] - base[:, None, c]).abs()
    assert torch.equal(ag.samples, cf.samples) and torch.equal(ag.maps, maps) and float(ag.maps[0, 1].max()) == 0.0


def test_philox_repeats_touches_no_generator_and_the_own_class_is_the_last_pass_on_the_last_latent(case):
    """rng="philox": row i * BS + b is the draw of latent i of image b.  The own-class sample is the sampler's last pass applied to
    x_n = alpha_n x + sigma_n e_n with e_n the rows n * BS + b, recomputed here.  (Not asserted to be close to x: with untrained
    weights the last mean pass is not the identity.)"""
    dc, x, cl, c0 = case["dc"], case["x"], case["cl"], case["c0"]
    torch.manual_seed(1)
    before = torch.cuda.get_rng_state(0), torch.get_rng_state()
    a = dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=c0, rng="philox", seed=11)
    ia = dc.invert_ddpm(x, c0, 0.5, rng="philox", seed=11)
    assert torch.equal(torch.cuda.get_rng_state(0), before[0]) and torch.equal(torch.get_rng_state(), before[1])
    torch.manual_seed(2)
    b = dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=c0, rng="philox", seed=11)
    ib = dc.invert_ddpm(x, c0, 0.5, rng="philox", seed=11)
    c = dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=c0, rng="philox", seed=12)
    assert torch.isfinite(a.samples).all()
    assert torch.equal(a.samples, b.samples) and torch.equal(a.maps, b.maps) and not torch.equal(a.samples, c.samples)
    assert torch.equal(ia.start, ib.start) and torch.equal(ia.noise, ib.noise)
    CHW = x[0].numel()
    e_n = torch.empty_like(x)
    rows = torch.arange(STEPS * BS, (STEPS + 1) * BS, dtype=torch.int64, device=DEV)
    L.check(L.lib().dc_philox_normal(e_n.data_ptr(), BS, CHW, rows.data_ptr(), 11, L.stream_ptr()), "dc_philox_normal")
    lams = S.grid_lams(dc, 0.5, 0.0)
    lam_n = lams[STEPS].detach().float().cpu().reshape(())
    x_n = torch.sqrt(torch.sigmoid(lam_n)).to(DEV) * x + torch.sqrt(torch.sigmoid(-lam_n)).to(DEV) * e_n
    want = dc.clip(_eager_pass(dc, x_n, c0, lams[STEPS - 1], lams[STEPS])[0])
    d = (a.samples[:, 0] - want).abs().max().item()
    far = (a.samples[:, 1] - want).abs().max().item()
    print(f"{case['kind']}: own-class sample vs the last pass on x_n: {d:.2e} (bound {BOUND:g}; another class: {far:.2e})")
    assert d < BOUND, d
    assert far > 10 * BOUND, far


def test_one_image_per_chunk_matches_the_unchunked_call(case):
    dc, x = case["dc"], case["x"]
    dc.config.units_per_launch = 2                                     # a launch holds one image at least: every image its own chunk, in
    #                                                                    the inversion (2 units an image) and in the decode (2 * K)
    try:
        torch.manual_seed(SEED)
        inv = dc.invert_ddpm(x, case["c0"], 0.5)
        torch.manual_seed(SEED)
        got = dc.counterfactual(x, case["cl"], 0.5, start="ddpm_invert", invert_class=case["c0"])
    finally:
        dc.config.units_per_launch = None
    bb = dc.ema.ema_model
    assert {k[1] for k in bb._plans if k[0] == "pair_session" and k[2] == 3} == {0, 1}     # two sessions of K = 3 trajectories
    assert {k[1] for k in bb._plans if k[0] == "pair_session" and k[2] == 1} == {0, 1}     # and two of one image for the inversion
    sds = _sds(dc)
    dn = max(((inv.noise[i] - case["inv"].noise[i]) * sds[i]).abs().max().item() for i in range(STEPS))
    d = (got.samples - case["cf"].samples).abs().max().item()
    print(f"{case['kind']}: one image per chunk vs one launch: noise[i] * sd_i {dn:.2e}, samples {d:.2e} (bound {BOUND:g})")
    assert torch.equal(inv.start, case["inv"].start)
    assert dn < BOUND and d < BOUND                                    # plans of different launch shapes may differ, within BOUND


# ------------------------------------------------------------------------------------------------ launch counts
def test_launches_per_chunk(monkeypatch):
    """Per chunk: sampling_steps backbone passes and dc_ddpm_noise_map launches for the inversion, sampling_steps + 1 passes and
    dc_ddpm_step_shared launches for the decode; the context plan once per session; Philox draws belong to the inversion alone."""
    dc, x = _build("unet_v")
    ctx, passes, maps, steps, draws = [], [], [], [], []
    real_ctx, real_step = E.UNetPlan.run_ctx, U.PairSession.step
    lib = L.lib()
    real_map, real_shared, real_philox = lib.dc_ddpm_noise_map, lib.dc_ddpm_step_shared, lib.dc_philox_normal
    monkeypatch.setattr(E.UNetPlan, "run_ctx", lambda self: (ctx.append(self), real_ctx(self))[1])
    monkeypatch.setattr(U.PairSession, "step", lambda self, *a: (passes.append(self), real_step(self, *a))[1])
    monkeypatch.setattr(lib, "dc_ddpm_noise_map", lambda *a: (maps.append(a), real_map(*a))[1])
    monkeypatch.setattr(lib, "dc_ddpm_step_shared", lambda *a: (steps.append(len(draws)), real_shared(*a))[1])
    monkeypatch.setattr(lib, "dc_philox_normal", lambda *a: (draws.append(a), real_philox(*a))[1])
    lists = (ctx, passes, maps, steps, draws)
    cl, c0 = torch.tensor([1, 3, 0]), torch.tensor([1, 2])
    dc.invert_ddpm(x, c0, 0.5)                                         # one chunk, torch's generator
    assert [len(v) for v in lists] == [1, STEPS, STEPS, 0, 0]
    for lst in lists:
        del lst[:]
    dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=c0, rng="philox", seed=3)
    assert [len(v) for v in lists] == [2, 2 * STEPS + 1, STEPS, STEPS + 1, STEPS + 1]
    assert steps == [STEPS + 1] * (STEPS + 1)                          # every draw precedes the first decode step: the decode draws nothing
    for lst in lists:
        del lst[:]
    dc.config.units_per_launch = 2                                     # every image its own chunk, in the inversion too
    dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=c0)
    assert [len(v) for v in lists] == [4, 2 * (2 * STEPS + 1), 2 * STEPS, 2 * (STEPS + 1), 0]
    for lst in lists:
        del lst[:]
    dc.config.units_per_launch = None
    dc.counterfactual(x, cl, 0.5)                                      # the default start launches no noise map
    assert [len(v) for v in lists] == [1, STEPS + 1, 0, STEPS + 1, 0]


# ------------------------------------------------------------------------------------------------ a ragged prompt table
def test_ragged_prompt_table_matches_the_eager_statement():
    cfg = dict(PROMPT_BASE, cfg_w=2.0, sampling_steps=STEPS, classes=3, pred_param="v", prompt_tokens=3)
    torch.manual_seed(133)
    m = dca.UNetCondition2D(**dca.small_unet_kwargs())
    _randomise_vectors(m)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg))
    with torch.no_grad():
        dc.encoder.weight.mul_(3.0)
    dc.encoder.set_lengths([3, 2, 3, 1])                               # class prompts of 3, 2, 3 tokens, a null prompt of 1
    dc = dc.to(DEV)
    x = (torch.rand(BS, 3, 32, 32) * 2 - 1).to(DEV)
    cl, c0 = torch.tensor([[1, 0, 2], [0, 1, 1]]), torch.tensor([1, 0])
    torch.manual_seed(SEED)
    inv = dc.invert_ddpm(x, c0, 0.5)
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, cl, 0.5, start="ddpm_invert", invert_class=c0)
    bb = dc.ema.ema_model
    assert all(k[-1] == "varlen" for k in bb._plans if k[0] == "pair_session")
    torch.manual_seed(SEED)
    start_e, noise_e = DI.run_eager(dc, x, c0, 0.5, 2.0)
    sds = _sds(dc)
    dn = max(((inv.noise[i] - noise_e[i]) * sds[i]).abs().max().item() for i in range(STEPS))
    want = torch.stack([_eager_decode(dc, start_e, noise_e, cl[:, k]) for k in range(3)], dim=1)
    d = (cf.samples - want).abs().max().item()
    print(f"ragged 3-token table vs the eager statement: noise[i] * sd_i {dn:.2e}, samples {d:.2e} (bound {BOUND:g})")
    assert (inv.start - start_e).abs().max().item() < BOUND and dn < BOUND and d < BOUND


# ------------------------------------------------------------------------------------------------ pixel space
def test_pixel_space_and_against_on_a_dwt_shaped_case():
    kw = dict(dca.small_unet_kwargs(), sample_size=16, in_channels=12, out_channels=12)
    cfg = dict(BASE, cfg_w=2.0, sampling_steps=2, classes=3, pred_param="v", image_size=16, noise_d=16)
    m, _ = make_pair(kw, seed=35)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg)).to(DEV)
    x = (torch.rand(BS, 12, 16, 16) * 2 - 1).to(DEV)
    c0 = torch.tensor([0, 2])
    kws = dict(start="ddpm_invert", invert_class=c0, rng="philox", seed=5)
    raw = dc.counterfactual(x, None, 0.5, **kws)
    pix = dc.counterfactual(x, None, 0.5, pixel_space=True, **kws)
    assert tuple(raw.samples.shape) == (BS, 3, 12, 16, 16) and tuple(pix.samples.shape) == (BS, 3, 3, 32, 32)
    want = wavelet_enc_2(raw.samples.reshape(BS * 3, 12, 16, 16) * 2).view(BS, 3, 3, 32, 32)
    assert torch.equal(pix.samples, want)
    base = wavelet_enc_2(x * 2)
    maps = torch.zeros_like(pix.maps)
    for c in range(3):
        maps = maps + (want[:, :, c] - base[:, None, c]).abs()
    assert torch.equal(pix.maps, maps)
    pa = dc.counterfactual(x, None, 0.5, against=c0, pixel_space=True, **kws)
    maps = torch.zeros_like(pix.maps)
    for c in range(3):
        maps = maps + (want[:, :, c] - torch.stack([want[0, 0, c], want[1, 2, c]])[:, None]).abs()
    assert torch.equal(pa.samples, want) and torch.equal(pa.maps, maps)
