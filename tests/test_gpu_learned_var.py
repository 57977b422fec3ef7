"""GPU: config.variance = "learned", the learned-range ancestral step — `dc_ddpm_step_shared` / `dc_ddpm_noise_map` in
DC_STEP_LEARNED_RANGE against fp64 from the same fp32 inputs and scalars, and `sample` / `counterfactual` / `invert_ddpm` on a small DiT
with learned-variance outputs (2 heads x 32, 2 layers, 8x8x4 latents in patches of 2, out_channels 8, f32) against the fp64 loops of
tests/learned_var_oracle.py over `oracle.OracleDiT` in fp64.

Op bounds (derived, see the tests): the step adds noise * sde with sde = expf(0.5 (fr log_hi + (1 - fr) log_lo)); the exp argument is at
most 23 in magnitude (0.5 |log 1e-20|), three roundings in front of it and expf's 1-2 ulp give about 5e-6 relative in sde, times 4 for
the 0.5f multiply and the interpolation: |out - mu - sde64 noise| <= 2e-5 |sde64 noise| + 2^-23 |out|, mu the kernel's own mean (the
noise = NULL launch, which equals `dc_solver_step` bit for bit).  Map then step: 4 x 2^-24 (|x_next| + |mu|).
Model bounds: the error of the FIXED-variance run against its own fp64 loop on the same model and draws, times 4 (one expf with a
23x-amplified argument per element and step), and at least test_gpu_counterfactual.BOUND x max(1, |fp64|.max()), the suite's bound
for f32 trajectories.

Seen on an MI355X (first complete run): step, worst |out - mu - sde64 noise| / bound 0.50 over all shapes and both scalar sets (sde from
1.0e-12 to 1); map then step 0.92 of its bound, the map against fp64 3.4e-6 relative at most; pinned head 0.48 / 0.44 of the step bound;
max-abs against fp64, learned / fixed: sample 7.17e-6 / 7.05e-6 (reference draws), 7.14e-6 / 6.85e-6 (Philox), counterfactual 1.01e-5 /
8.89e-6, invert_ddpm noise x deviation 2.47e-6 / 2.39e-6 (floors 3e-3 .. 8e-3); learned against fixed 6.5e-2 .. 8.2e-2 relative L2;
decode under invert_class, worst step 3.82e-6 (bound 1.79e-5); the variance pair plan equals `DiT.forward`'s channels bit for bit.
"""
import ctypes as C
import math

import pytest
import torch

import dit_dir_oracle as DO
import learned_var_oracle as LV
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import ancestral as AN
from diffusion_classifier_amd import trajectory as TJ
from test_ddpm_invert_host import TOL_DECODE
from test_gpu_counterfactual import BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ================================================================================================ the ops
SHAPES = {
    "patch0_5x5": dict(n=2, C=3, H=5, W=5, patch=0, ld=8, fstride=6, noise_div=1),            # odd extents, a partial block, padded rows
    "patch2_8x8": dict(n=4, C=4, H=8, W=8, patch=2, ld=32, fstride=8, noise_div=2),
    "patch4_16x16": dict(n=2, C=4, H=16, W=16, patch=4, ld=128, fstride=8, noise_div=1),
    "patch2_256x256": dict(n=9, C=4, H=256, W=256, patch=2, ld=32, fstride=8, noise_div=3),   # 9216 blocks > the 8192 cap: a second trip
}
# (alpha_t, sigma_t, k1, k2, log_hi, log_lo) as fp32 values: a middle step of a 4-step walk, and the clamped posterior variance 1e-20
SCALARS = {"mid": (0.28033417, 0.95990247, 0.20000905, 0.66786808, -0.16246155, -0.82313114),
           "clamped": (0.99994999, 0.01000, 0.0001521, 0.99983984, -9.2104502, -46.0517006)}
SCALARS = {k: tuple(float(torch.tensor(v, dtype=torch.float32)) for v in t) for k, t in SCALARS.items()}
_OPS = {}


def op_case(name):
    """Inputs of one shape, once: NCHW f32 tensors on the host, the prediction in both layouts on the device (unread slots NaN)."""
    if name not in _OPS:
        s = SHAPES[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        shp = (s["n"], s["C"], s["H"], s["W"])
        z, pc, pu, xn = (torch.randn(shp, generator=g) for _ in range(4))
        vc = torch.rand(shp, generator=g) * 3.0 - 1.5                          # not clamped: fr in [-0.25, 1.25]
        vc.view(-1)[:3] = torch.tensor([-1.0, 1.0, 0.0])
        noise = torch.randn((s["n"] // s["noise_div"],) + shp[1:], generator=g)
        p = max(s["patch"], 1)
        pred = LV.pack_pred(pc, pu, vc, s["patch"], s["ld"], s["fstride"])
        eps_ld = max(p * p * s["C"], 1) + 1
        pred_eps = LV.pack_pred(pc, pu, None, s["patch"], eps_ld, s["C"])      # what dc_solver_step and the fixed step read
        assert int(torch.isnan(pred).sum()) > 0
        host = dict(z=z, pc=pc, pu=pu, vc=vc, noise=noise, xn=xn)
        dev = {k: v.to(DEV).contiguous() for k, v in dict(host, pred=pred, pred_eps=pred_eps).items()}
        _OPS[name] = (s, host, dev, eps_ld)
    return _OPS[name]


def ptr(t):
    return None if t is None else t.data_ptr()


def common(s, dev, v_param, w, sc, pred="pred", ld=None):
    return dict(z=ptr(dev["z"]), pred=ptr(dev[pred]), n=s["n"], C=s["C"], H=s["H"], W=s["W"], ld=s["ld"] if ld is None else ld,
                patch=s["patch"], v_param=v_param, w=w, one_plus_w=float(1.0 + w), alpha_t=sc[0], sigma_t=sc[1])


def learned(sc, s):
    return dict(mode=L.STEP_LEARNED_RANGE, fstride=s["fstride"], k1=sc[2], k2=sc[3], log_hi=sc[4], log_lo=sc[5])


def call(entry, cls, fields):
    """The entry on its struct, or — when the fields carry a mode — on the struct with the mode block behind it and the flag that
    announces the block in v_param (dcamd.h DC_STEP_MODE_BLOCK)."""
    if "mode" in fields:
        fields = dict(fields, v_param=fields["v_param"] | L.STEP_MODE_BLOCK)
        p = TJ.mode_params(cls)(**fields)
    else:
        p = cls(**fields)
    L.check(getattr(L.lib(), entry)(C.cast(C.pointer(p), C.POINTER(cls)), L.stream_ptr()), entry)


def run_step(s, dev, v_param, w, sc, noise, noise_div, **mode):
    out = torch.full_like(dev["z"], float("nan"))
    call("dc_ddpm_step_shared", L.DdpmStepSharedParams, dict(noise=ptr(noise), out=ptr(out), noise_div=noise_div, pad_=0, alpha_s=0.0, c=0.0,
                                                             sd=0.0, **common(s, dev, v_param, w, sc), **mode))
    return out


def sde_of(host, sc):
    fr = 0.5 * host["vc"].double() + 0.5
    return torch.exp(0.5 * (fr * sc[4] + (1.0 - fr) * sc[5]))


@pytest.mark.parametrize("w", [0.0, 1.5])
@pytest.mark.parametrize("v_param", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_step_mean_is_the_solver_steps_bits_and_the_noise_term_is_within_the_bound(name, v_param, w):
    s, host, dev, eps_ld = op_case(name)
    for which, sc in SCALARS.items():
        mu = run_step(s, dev, v_param, w, sc, None, s["noise_div"], **learned(sc, s))
        want = torch.full_like(mu, float("nan"))
        p = L.SolverStepParams(xprev=None, xhat=None, out=ptr(want), clamp=0, final_pass=0, k1=sc[2], k2=sc[3], k3=0.0,
                               **common(s, dev, v_param, w, sc, pred="pred_eps", ld=eps_ld))
        L.check(L.lib().dc_solver_step(C.byref(p), L.stream_ptr()), "dc_solver_step")
        assert torch.isfinite(mu).all() and torch.equal(mu.view(torch.int32), want.view(torch.int32)), (name, which)
        out = run_step(s, dev, v_param, w, sc, dev["noise"], s["noise_div"], **learned(sc, s)).cpu().double()
        term = sde_of(host, sc) * host["noise"].double().repeat_interleave(s["noise_div"], dim=0)
        err = (out - mu.cpu().double() - term).abs()
        bound = 2e-5 * term.abs() + 2.0 ** -23 * out.abs()
        worst = float((err / bound).max())
        print(f"{name} v_param={v_param} w={w} {which}: |out - mu - sde64 noise| / bound, worst {worst:.3f}; "
              f"sde in [{float(sde_of(host, sc).min()):.2e}, {float(sde_of(host, sc).max()):.2e}]")
        assert torch.isfinite(out).all() and bool((err <= bound).all()), (name, which, worst)
        # the three pinned variance values: v = -1 -> exp(0.5 log_lo), v = 1 -> exp(0.5 log_hi), v = 0 -> the geometric middle
        pinned = sde_of(host, sc).view(-1)[:3].tolist()
        for got, arg in zip(pinned, (sc[5], sc[4], 0.5 * (sc[4] + sc[5]))):
            assert abs(got - math.exp(0.5 * arg)) <= 1e-12 * got


@pytest.mark.parametrize("name", ["patch0_5x5", "patch2_8x8"])
def test_mode_zero_ignores_the_new_fields(name):
    """DC_STEP_FIXED in a mode block with garbage in fstride, k1, k2, log_hi, log_lo, and in one of zeros: the bits of the same call on
    the plain struct, without flag and block (step and map)."""
    s, host, dev, eps_ld = op_case(name)
    sc = SCALARS["mid"]
    fixed = dict(alpha_s=0.9, c=0.4, sd=0.3)
    garbage = dict(mode=L.STEP_FIXED, fstride=-7, k1=float("nan"), k2=1e30, log_hi=float("inf"), log_lo=5.0)
    zeros = dict(mode=0, fstride=0, k1=0.0, k2=0.0, log_hi=0.0, log_lo=0.0)
    outs = []
    for extra in ({}, zeros, garbage):
        kw = common(s, dev, 1, 1.5, sc, pred="pred_eps", ld=eps_ld)
        o1, o2, o3 = (torch.full_like(dev["z"], float("nan")) for _ in range(3))
        for noise, o in ((dev["noise"], o1), (None, o2)):
            call("dc_ddpm_step_shared", L.DdpmStepSharedParams,
                 dict(noise=ptr(noise), out=ptr(o), noise_div=s["noise_div"], pad_=0, **fixed, **kw, **extra))
        call("dc_ddpm_noise_map", L.DdpmNoiseMapParams, dict(x_next=ptr(dev["xn"]), out=ptr(o3), **fixed, **kw, **extra))
        outs.append((o1, o2, o3))
    for a, b, c in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert float(outs[0][1].abs().max()) <= 1.0                                  # the fixed last pass still clips


@pytest.mark.parametrize("v_param", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_map_then_step_lands_on_x_next(name, v_param):
    """A division and a multiply-add on the same sde bits: |step(map) - x_next| <= 4 x 2^-24 (|x_next| + |mu|); in place the same bits."""
    s, host, dev, _ = op_case(name)
    w = 1.5
    for which, sc in SCALARS.items():
        mode = learned(sc, s)
        kw = dict(alpha_s=0.0, c=0.0, sd=0.0, **common(s, dev, v_param, w, sc), **mode)
        m = torch.full_like(dev["z"], float("nan"))
        call("dc_ddpm_noise_map", L.DdpmNoiseMapParams, dict(x_next=ptr(dev["xn"]), out=ptr(m), **kw))
        inplace = dev["xn"].clone()
        call("dc_ddpm_noise_map", L.DdpmNoiseMapParams, dict(x_next=ptr(inplace), out=ptr(inplace), **kw))
        assert torch.isfinite(m).all() and torch.equal(m.view(torch.int32), inplace.view(torch.int32)), (name, which)
        mu = run_step(s, dev, v_param, w, sc, None, 1, **mode)
        back = run_step(s, dev, v_param, w, sc, m, 1, **mode)
        err = (back.double() - dev["xn"].double()).abs()
        bound = 4 * 2.0 ** -24 * (dev["xn"].double().abs() + mu.double().abs())
        worst = float((err / bound).max())
        # the map is the fp64 one up to the roundings of mu, sde and the division
        m64 = (host["xn"].double() - mu.cpu().double()) / sde_of(host, sc)
        rel = float(((m.cpu().double() - m64).abs() / (m64.abs() + 1e-30)).max())
        print(f"{name} v_param={v_param} {which}: |step(map) - x_next| / bound, worst {worst:.3f}; map against fp64, worst relative {rel:.2e}")
        assert bool((err <= bound).all()), (name, which, worst)
        assert rel <= 2e-5 + 2.0 ** -22, rel


# ================================================================================================ the model
N_STEPS, BS, SEED = 3, 2, 7
GEN = dict(cfg_w=1.5, sampling_steps=N_STEPS, timestep_spacing="trailing")
_MODEL = {}


def model():
    """The small DiT with learned-variance outputs, its fp64 oracle, and two classifiers over copies of it on the device — the key set
    and unset — once, shared and left unchanged."""
    if not _MODEL:
        m = DO.make_dit(DO.DIT_A, seed=71)
        dcl, _ = DO.classifier(m, variance="learned", **GEN)
        dcf, _ = DO.classifier(m, **GEN)
        torch.manual_seed(72)
        x = torch.rand(BS, 4, 8, 8) * 2 - 1
        _MODEL.update(m=m, net=LV.dit64(m), learned=dcl.to(DEV), fixed=dcf.to(DEV), x=x, abar=LV.abar64(1000))
    return _MODEL


def reference_draws(x, n, from_t=1):
    """The draws of `sample` under torch.manual_seed(SEED): the start — from pure noise on the CPU generator, below from_t = 1 the
    `randn_like` of `diffuse` on the device's — then one `randn_like` per pass on the device's."""
    torch.manual_seed(SEED)
    like = torch.empty(x.shape, device=DEV)
    e0 = torch.randn(x.shape) if from_t == 1 else torch.randn_like(like).cpu()
    return e0, [torch.randn_like(like).cpu() for _ in range(n)]


def philox_draws(x, n, seed):
    ns = TJ.NoiseSource(x.to(DEV), "philox", seed, n + 1)
    return [ns(i).clone().cpu() for i in range(n + 1)]


def start64(c, x, ks, e0, from_t):
    return e0.double() if from_t == 1 else math.sqrt(c["abar"][ks[0]]) * x.double() + math.sqrt(1 - c["abar"][ks[0]]) * e0.double()


def check_against_fp64(what, got_l, got_f, want_l, want_f):
    """The bound of the model tests: the fixed run's error against its own fp64 loop x 4, at least the suite's f32 trajectory bound."""
    el, ef = float((got_l.cpu().double() - want_l).abs().max()), float((got_f.cpu().double() - want_f).abs().max())
    floor = BOUND * max(1.0, float(want_l.abs().max()))
    bound = max(4 * ef, floor)
    rel = float((want_l - want_f).norm() / want_f.norm())
    print(f"{what}: learned against fp64 {el:.2e}, fixed against its fp64 {ef:.2e} (bound max(4 x fixed, {floor:.1e}) = {bound:.2e}); "
          f"learned and fixed differ by {rel:.2e} relative L2")
    assert torch.isfinite(got_l).all() and ef <= floor, (ef, floor)
    assert el <= bound, (el, bound)
    return el, ef


def _pin(m, bias):
    """The model with the variance rows of proj_out_2 zeroed and their bias set: v = bias everywhere, exactly."""
    import copy
    m = copy.deepcopy(m)
    with torch.no_grad():
        Wt, b = m.proj_out_2.weight.view(4, 8, -1), m.proj_out_2.bias.view(4, 8)
        Wt[:, 4:] = 0.0
        b[:, 4:] = bias
    return m


def _record_feeds(monkeypatch, dc):
    bb, fed = dc.ema.ema_model, []
    real = bb._feed
    monkeypatch.setattr(bb, "_feed", lambda plan, x, labels: (fed.append(x.detach().clone()), real(plan, x, labels))[1])
    return fed


@pytest.mark.parametrize("bias", [-1.0, 1.0])
def test_pinned_variance_head_gives_the_two_fixed_variances(monkeypatch, bias):
    """v = -1: sde = sqrt(beta~), `Linear`'s sd, so every pass of `sample` under the key equals the key-unset step from the same latent
    within the step bound of the op test; v = +1: sde = sqrt(beta), against fp64.  Pass by pass on the latents the learned run was fed:
    a bound on one step says nothing about what a network makes of it two passes later."""
    c = model()
    m = _pin(c["m"], bias)
    dcl, _ = DO.classifier(m, variance="learned", **GEN)
    dcf, _ = DO.classifier(m, **GEN)
    dcl, dcf, x = dcl.to(DEV), dcf.to(DEV), c["x"].to(DEV)
    lab = torch.tensor([2, 0]).to(DEV)
    fed = _record_feeds(monkeypatch, dcl)
    torch.manual_seed(SEED)
    got = dcl.sample(x, lab, from_t=1)
    _, draws = reference_draws(x, N_STEPS)
    assert len(fed) == N_STEPS + 1
    lat = fed + [got]
    g = TJ.grid(dcf, 1.0, 0.0)
    lin, bb = AN.step_kind(dcf, g, dcf.cfg_w), dcf.ema.ema_model
    assert type(lin) is AN.Linear
    fields = TJ.step_fields(dcf, bb, x.shape, dcf.cfg_w)
    null = torch.full_like(lab, dcf.null_token)
    worst = 0.0
    for i in range(N_STEPS + 1):
        t = min(i, N_STEPS - 1)
        z = lat[i].contiguous()
        pair = bb.forward_pair(z, g.label[t].to(DEV).unsqueeze(0), lab, null)
        f = dict(fields, z=z.data_ptr(), pred=pair.data_ptr(), n=BS, ld=pair.shape[-1])
        mu = torch.empty_like(z)
        lin.mean_hip(f, mu, t)
        if i == N_STEPS:
            assert torch.equal(lat[i + 1], mu)                                   # the last pass: the unclipped mean, the same bits
            break
        sc = LV.scalars64(c["abar"], g.steps[t], g.steps[t + 1])
        sd64 = math.sqrt(math.exp(sc["log_lo" if bias < 0 else "log_hi"]))
        e = draws[i].to(DEV).double()
        nxt = lat[i + 1].double()
        bound = 2e-5 * (sd64 * e).abs() + 2.0 ** -23 * nxt.abs()
        err = (nxt - mu.double() - sd64 * e).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (bias, i, float((err / bound).max()))
        if bias < 0:                                                             # the key-unset step from the same latent
            out = torch.empty_like(z)
            lin.step_hip(f, out, t, draws[i].to(DEV))
            e2 = (nxt - out.double()).abs()
            b2 = 2e-5 * (lin.scal[t][4] * e).abs() + 2.0 ** -23 * nxt.abs()
            worst = max(worst, float((e2 / b2).max()))
            assert bool((e2 <= b2).all()), (i, float((e2 / b2).max()))
    print(f"variance head pinned at {bias:+.0f}: per pass, worst error / step bound {worst:.3f}")


def test_sample_against_the_fp64_oracle():
    """from_t = 0.5, steps 499 -> 332 -> 165 -> 0: from pure noise this random-weight eps model's data prediction at k = 999
    (1 / alpha_t = 157) reaches 1e3 and buries the noise term — the fp64 learned and fixed runs then differ by 3e-3 relative L2, here
    by 7e-2."""
    c = model()
    x, lab, from_t = c["x"], torch.tensor([2, 0]), 0.5
    null = torch.full_like(lab, 3)
    ks = TJ.discrete_steps(c["learned"], from_t)
    out = {}
    # rng = "reference": `sample`, the draws reproduced from the seed
    e0, draws = reference_draws(x, N_STEPS, from_t)
    for who in ("learned", "fixed"):
        torch.manual_seed(SEED)
        out[who] = c[who].sample(x.to(DEV), lab.to(DEV), from_t=from_t)
    args = (c["net"], start64(c, x, ks, e0, from_t), lab, null, ks, c["abar"], 1.5, False, draws)
    want_l, want_f = LV.sample64(*args)[0], LV.sample64(*args, learned=False)[0]
    check_against_fp64("sample, reference draws", out["learned"], out["fixed"], want_l, want_f)
    rel = float((out["learned"] - out["fixed"]).double().norm() / out["fixed"].double().norm())
    assert rel > 1e-2, rel                                                       # ignoring the key fails here
    # rng = "philox": `sample` has no such argument; one class column of `counterfactual` is `sample` on Philox noise
    pd = philox_draws(x, N_STEPS, 11)
    for who in ("learned", "fixed"):
        out[who] = c[who].counterfactual(x.to(DEV), lab.view(BS, 1), from_t, rng="philox", seed=11).samples[:, 0]
    args = (c["net"], start64(c, x, ks, pd[0], from_t), lab, null, ks, c["abar"], 1.5, False, pd[1:])
    want_l, want_f = LV.sample64(*args)[0], LV.sample64(*args, learned=False)[0]
    check_against_fp64("sample, philox draws", out["learned"], out["fixed"], want_l, want_f)
    assert float((out["learned"] - out["fixed"]).double().norm() / out["fixed"].double().norm()) > 1e-2
    c["learned"].check_device_errors()


def test_counterfactual_is_two_fp64_runs_on_shared_noise():
    c = model()
    x, cl, from_t = c["x"], torch.tensor([[1, 2], [0, 1]]), 0.5
    ks = TJ.discrete_steps(c["learned"], from_t)
    pd = philox_draws(x, N_STEPS, 5)
    got = {who: c[who].counterfactual(x.to(DEV), cl, from_t, rng="philox", seed=5) for who in ("learned", "fixed")}
    null = torch.full((BS,), 3)
    z0 = start64(c, x, ks, pd[0], from_t)
    want = {who: torch.stack([LV.sample64(c["net"], z0, cl[:, k], null, ks, c["abar"], 1.5, False, pd[1:], learned=who == "learned")[0]
                              for k in range(2)], dim=1) for who in got}
    assert tuple(got["learned"].samples.shape) == (BS, 2, 4, 8, 8) and tuple(got["learned"].maps.shape) == (BS, 2, 8, 8)
    check_against_fp64("counterfactual, K = 2", got["learned"].samples, got["fixed"].samples, want["learned"], want["fixed"])
    s = got["learned"].samples
    assert float((s[:, 0] - s[:, 1]).abs().max()) > 100 * BOUND                  # the two classes' trajectories differ
    assert float((s - got["fixed"].samples).double().norm() / got["fixed"].samples.double().norm()) > 1e-2


def test_inversion_maps_and_the_decode_back(monkeypatch):
    """`invert_ddpm` against the fp64 maps (scaled by the deviation; the bound of `check_against_fp64`), then
    `counterfactual(start="ddpm_invert")`: under the image's own class every pass is fed the inversion's next latent — bound:
    TOL_DECODE x max(1, |latents|.max()), the discrete grid's round-trip bound (tests/test_gpu_discrete_generation.py test 9) — and
    another class leaves the path."""
    c = model()
    x, c0, cl, from_t = c["x"], torch.tensor([1, 2]), torch.tensor([[1, 0], [2, 1]]), 0.5
    ks = TJ.discrete_steps(c["learned"], from_t)
    pd = philox_draws(x, N_STEPS, 9)
    null = torch.full((BS,), 3)
    inv = {who: c[who].invert_ddpm(x.to(DEV), c0, from_t, rng="philox", seed=9) for who in ("learned", "fixed")}
    scaled, want = {}, {}
    for who in inv:
        lat, maps, devs = LV.noise_maps64(c["net"], x, c0, null, ks, c["abar"], 1.5, False, pd, learned=who == "learned")
        devs = [d if torch.is_tensor(d) else torch.full_like(maps[0], d) for d in devs]
        want[who] = torch.stack([m * d for m, d in zip(maps, devs)])
        scaled[who] = inv[who].noise.cpu().double() * torch.stack(devs)
        assert tuple(inv[who].noise.shape) == (N_STEPS, BS, 4, 8, 8) and torch.isfinite(inv[who].noise).all()
    el, ef = check_against_fp64("invert_ddpm, noise[i] x deviation", scaled["learned"], scaled["fixed"], want["learned"], want["fixed"])
    scale = max(1.0, max(float(v.abs().max()) for v in lat))
    fed = _record_feeds(monkeypatch, c["learned"])
    cf = c["learned"].counterfactual(x.to(DEV), cl, from_t, start="ddpm_invert", invert_class=c0, rng="philox", seed=9)
    feeds = fed[N_STEPS:]                                                        # the inversion's passes come first
    assert len(fed) == 2 * N_STEPS + 1
    worst = 0.0
    for i, z in enumerate(feeds):
        z = z.view(BS, 2, 4, 8, 8).cpu().double()
        worst = max(worst, float((z[:, 0] - lat[i]).abs().max()))
        assert i == 0 or float((z[:, 1] - lat[i]).abs().max()) > 100 * TOL_DECODE * scale
    print(f"decode under invert_class against the inversion's latents, worst step {worst:.2e} (bound {TOL_DECODE * scale:.2e})")
    assert worst <= TOL_DECODE * scale, (worst, TOL_DECODE * scale)
    assert float(cf.maps[:, 1].max()) > 0.0 and torch.isfinite(cf.samples).all()


def test_pair_plans_with_and_without_the_variance():
    c = model()
    bb = c["learned"].ema.ema_model
    x = c["x"].to(DEV)
    lab, null, step = torch.tensor([2, 0]).to(DEV), torch.tensor([3, 3]).to(DEV), torch.tensor([431.0], device=DEV)
    pair = bb.forward_pair(x, step, lab, null, variance=True).clone()
    assert tuple(pair.shape) == (2 * BS, 4, 4, 2 * 2 * 8) and pair.dtype == torch.float32
    full = torch.stack([bb(x, step.expand(BS), lab), bb(x, step.expand(BS), null)], dim=1).reshape(2 * BS, 8, 8, 8)
    feat = pair.view(2 * BS, 4, 4, 2, 2, 8).permute(0, 5, 1, 3, 2, 4).reshape(2 * BS, 8, 8, 8)      # un-patchify: nhwpqc -> nchpwq
    assert torch.equal(feat[:, 4:], full[:, 4:]) and torch.equal(feat[:, :4], full[:, :4])          # same GEMM, same packed rows
    ses = bb.pair_session(BS, DEV, lab, null, slot=3, variance=True)
    assert torch.equal(ses.step(x, step), pair)
    kinds = {k[0] for k in bb._plans}
    assert {"pair_var", "pair_session_var", "fwd"} <= kinds
    assert all(pl.pred.C == 32 for k, pl in bb._plans.items() if k[0] in ("pair_var", "pair_session_var", "fwd"))
    # with the key unset the eps-only pair plans are still the ones built and used
    fb = c["fixed"].ema.ema_model
    torch.manual_seed(SEED)
    c["fixed"].sample(x, lab, from_t=1)
    c["fixed"].counterfactual(x, None, 0.5)
    assert any(k[0] == "pair" for k in fb._plans) and any(k[0] == "pair_session" for k in fb._plans)
    assert all(pl.pred.C == 16 for k, pl in fb._plans.items() if k[0] != "fwd") and not any("_var" in k[0] for k in fb._plans)
    with pytest.raises(L.DcamdError, match="out_channels == 2 \\* in_channels"):
        DO.eps_twin(c["m"]).to(DEV).forward_pair(x, step, lab, null, variance=True)
