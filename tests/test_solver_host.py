"""CPU: deterministic samplers and DDIM inversion on foreign backbones — the C-ABI surface of dc_solver_step, the step scalars against a
float64 evaluation, the solvers' order of convergence, exactness on a line, `sample` / `invert` / `counterfactual` against the float64
statement (solver_oracle.py), determinism, the untouched default path and the refusals."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import solver as S
import solver_oracle as O
from helpers import load_case, standin_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 17

# fp32 run against the float64 statement on the same inputs (stand-in backbone, sampling_steps = 4, cfg_w = 1.5), 4 x the largest
# max-abs difference seen over the cases of this file:
TOL_DECODE = 4 * 9.9e-7      # a decode from a given latent (`sample` from_t in {0.5, 1}, `counterfactual` from noise at 0.5): 9.83e-7
TOL_INVERT = 4 * 1.91e-4     # anything behind an inversion to 0.5: the first pass from u = 0 forms k1 z + k2 x with k1 = sigma_s / sigma_t
#                              ~ 1.3e3 and k2 ~ -k1, so the rounding of z and x (6e-8) comes out ~1e-4: 1.58e-4 on the stand-in, 1.91e-4 on
#                              the line backbone
TOL_LINE_DECODE = 4 * 1.2e-7  # the decode on the line backbone returns the clipped data prediction, one rounding from x*: 1.19e-7


def _dc(pred_param="eps", backbone=None, **extra):
    g, cfg = load_case("1stage_eps")
    cfg.update(pred_param=pred_param, cfg_w=1.5, sampling_steps=4)
    cfg.update(extra)
    dc = dca.DiffusionClassifier(backbone if backbone is not None else standin_from(g, cfg), dca.Config(**cfg))
    dc.encoder.weight.data.copy_(torch.from_numpy(g["encoder.weight"]))
    return dc, torch.from_numpy(g["x"]), cfg


# ------------------------------------------------------------------------------------------------ C-ABI
def test_struct_fields_match_the_header_and_the_abi_version_stays():
    src = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in L.SolverStepParams._fields_ if f[1] is L.vp] == ["z", "pred", "xprev", "xhat", "out"]
    assert ctypes.sizeof(L.SolverStepParams) == 5 * ptr + 16 * 4
    lib = L.lib()
    assert "dc_solver_step" in L.EXPORTS and lib.dc_solver_step is not None
    assert re.search(r"\bint dc_solver_step\(", src)
    assert lib.dc_abi_version() == 5 and L.ABI_VERSION == 5
    assert re.search(r"#define DC_ABI_VERSION 5\b", src)
    # the older step entries keep their structs
    assert ctypes.sizeof(L.DdpmStepParams) == 4 * ptr + 14 * 4 and ctypes.sizeof(L.DdpmStepSharedParams) == 4 * ptr + 16 * 4


def _step_params(**over):
    buf = (ctypes.c_float * 64)()
    buf2 = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    kw = dict(z=a, pred=a, xprev=a, xhat=a, out=ctypes.addressof(buf2), n=6, C=1, H=2, W=2, ld=4, patch=0, v_param=0, clamp=1, final_pass=0,
              w=1.0, one_plus_w=2.0, alpha_t=1.0, sigma_t=1.0, k1=0.5, k2=0.5, k3=0.5)
    kw.update(over)
    return L.SolverStepParams(**kw), (buf, buf2)


@pytest.mark.parametrize("over,code,word", [
    (dict(z=None), -1, "null"), (dict(pred=None), -1, "null"), (dict(out=None), -1, "null"), (dict(out="z"), -1, "alias"),
    (dict(n=0), -2, "extents"), (dict(C=0), -2, "extents"), (dict(W=-1), -2, "extents"), (dict(ld=0), -2, "extents"),
    (dict(patch=2, ld=3), -2, "extents"), (dict(patch=3, ld=16), -2, "patch=3"),
])
def test_solver_step_refuses_before_any_launch(over, code, word):
    """Every argument check answers without a GPU and touches no memory."""
    lib = L.lib()
    p, _keep = _step_params()
    for k, v in over.items():
        setattr(p, k, p.z if v == "z" else v)
    assert lib.dc_solver_step(ctypes.byref(p), None) == code
    assert word in lib.dc_last_error().decode()
    assert lib.dc_solver_step(None, None) == -1


# ------------------------------------------------------------------------------------------------ scalars
@pytest.mark.parametrize("schedule", ["cosine", "shifted_cosine"])
def test_step_scalars_match_a_float64_evaluation(schedule):
    """Grids from from_t in {0.5, 1.0} with n in {1, 2, 4}, both directions, both samplers: relative difference <= 1e-6 to the float64
    evaluation of the same formulas on the same lambdas (measured: 4.9e-7 at most — k2 of the first inversion pass of the shifted
    schedule; expm1 near the grid end needed no more), the identity k2 = alpha_s - alpha_t sigma_s / sigma_t to the same tolerance, and
    identical lists for "ddim" and "dpmpp_2m" when n <= 2."""
    worst = 0.0
    for from_t in (0.5, 1.0):
        for n in (1, 2, 4):
            dc, _, _ = _dc(schedule=schedule, sampling_steps=n, noise_d=64 if schedule == "shifted_cosine" else 32)
            for direction, (a, b) in (("denoise", (from_t, 0.0)), ("invert", (0.0, from_t))):
                lams = S.grid_lams(dc, a, b)
                assert len(lams) == n + 1
                got = {s: S.step_scalars(lams, s, direction) for s in S.SAMPLERS}
                for s in S.SAMPLERS:
                    want = O.scalars64(lams, s, direction)
                    assert len(got[s]) == n                                      # n passes, not n + 1
                    for i, (gp, wp) in enumerate(zip(got[s], want)):
                        assert all(isinstance(v, float) for v in gp[:4]) and isinstance(gp[5], bool)
                        assert gp[5] == wp[5] == (direction == "denoise" and i == n - 1)
                        assert (gp[4] is None) == (wp[4] is None) == (not (s == "dpmpp_2m" and direction == "denoise" and 1 <= i <= n - 2))
                        for j in range(5):
                            if wp[j] is not None:
                                rel = abs(gp[j] - wp[j]) / abs(wp[j])
                                worst = max(worst, rel)
                                assert rel <= 1e-6, (from_t, n, direction, s, i, j, gp[j], wp[j])
                        lt, ls = float(lams[i]), float(lams[i + 1])
                        sig = lambda v: 1.0 / (1.0 + math.exp(-v))               # noqa: E731
                        ident = math.sqrt(sig(ls)) - math.sqrt(sig(lt)) * math.sqrt(sig(-ls)) / math.sqrt(sig(-lt))
                        assert abs(gp[3] - ident) <= 1e-6 * abs(ident), (from_t, n, direction, s, i, gp[3], ident)
                if n <= 2 or direction == "invert":
                    assert got["ddim"] == got["dpmpp_2m"]
                else:
                    assert got["ddim"] != got["dpmpp_2m"]
    print(f"{schedule}: largest relative difference of a step scalar to float64: {worst:.2e}")
    with pytest.raises(ValueError, match="sampler"):
        S.step_scalars(lams, "ddpm", "denoise")
    with pytest.raises(ValueError, match="direction"):
        S.step_scalars(lams, "ddim", "up")


# ------------------------------------------------------------------------------------------------ order of convergence
def _midpoint_error(n, sampler):
    """Gaussian data of standard deviation s = 0.5: the exact denoiser is x_hat = alpha s^2 / (alpha^2 s^2 + sigma^2) z and the
    probability-flow solution z(lam) = z0 f(lam) / f(lam0), f = sqrt(sigmoid(lam) s^2 + sigmoid(-lam)).  Integrated in float64 with the
    scalars of `step_scalars` from from_t = 0.5 to the grid's midpoint (pass n / 2) on the cosine schedule."""
    dc, _, _ = _dc(sampling_steps=n)
    lams = S.grid_lams(dc, 0.5, 0.0)
    scal = S.step_scalars(lams, sampler, "denoise")
    s2 = 0.25
    z0 = 0.2 * torch.randn(64, dtype=torch.float64, generator=torch.Generator().manual_seed(0))      # |x_hat| << 1: no clamp
    z, x_prev = z0.clone(), None
    for i in range(n // 2):
        _, _, k1, k2, k3, final = scal[i]
        assert not final
        lam = float(lams[i])
        a2, sg2 = 1.0 / (1.0 + math.exp(-lam)), 1.0 / (1.0 + math.exp(lam))
        x = math.sqrt(a2) * s2 / (a2 * s2 + sg2) * z
        assert float(x.abs().max()) < 1.0
        D = x if k3 is None else x + k3 * (x - x_prev)
        z, x_prev = k1 * z + k2 * D, x
    f = lambda lam: math.sqrt(s2 / (1.0 + math.exp(-lam)) + 1.0 / (1.0 + math.exp(lam)))             # noqa: E731
    return float((z - z0 * f(float(lams[n // 2])) / f(float(lams[0]))).abs().max())


def test_order_of_convergence():
    """DDIM is first order, 2M second: halving the step halves / quarters the error at the midpoint.  Seen here (max-abs over the 64
    draws of seed 0; the absolute values scale with the draw, the ratios do not): DDIM 5.24e-3 (n = 16), 2.63e-3 (32); 2M 3.94e-4, 9.15e-5
    — ratios 1.99 and 4.31, 2M 13.3 x below DDIM at 16.  A wrong k2 or k3 breaks these."""
    e = {(s, n): _midpoint_error(n, s) for s in S.SAMPLERS for n in (16, 32)}
    print({k: f"{v:.3e}" for k, v in e.items()})
    assert 1.7 <= e["ddim", 16] / e["ddim", 32] <= 2.3
    assert e["dpmpp_2m", 16] / e["dpmpp_2m", 32] >= 3.5
    assert e["dpmpp_2m", 16] <= e["ddim", 16] / 5


# ------------------------------------------------------------------------------------------------ exactness on a line
class LineBackbone(nn.Module):
    """Answers every call with the prediction that belongs to the fixed image x*: eps = (z - alpha x*) / sigma, v = alpha eps - sigma x*."""

    def __init__(self, xstar, pred_param, hid=8):
        super().__init__()
        self.config = SimpleNamespace(encoder_hid_dim=hid)
        self.pred_param = pred_param
        self.register_buffer("xstar", xstar)
        self.unused = nn.Parameter(torch.zeros(1))

    def forward(self, x, noise_labels, encoder_hidden_states=None):
        lam = noise_labels.to(x.dtype).view(-1, 1, 1, 1)
        al, sg = torch.sqrt(torch.sigmoid(lam)), torch.sqrt(torch.sigmoid(-lam))
        eps = (x - al * self.xstar) / sg
        return eps if self.pred_param == "eps" else al * eps - sg * self.xstar


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("pred_param", ["eps", "v"])
def test_inversion_and_decode_are_exact_on_a_line(pred_param, sampler):
    """With the data prediction pinned to x*, every pass keeps z = alpha x*: the inverted latent is alpha_u x* and its decode is x*.
    Tolerances: the fp32 run against the float64 statement (TOL_INVERT, TOL_LINE_DECODE above; seen: latent 1.91e-4 (eps) / 1.34e-4 (v),
    decode 6.0e-8 / 1.2e-7) — the float64 statement itself is within 4e-8 of the line."""
    xs = torch.rand(5, 3, 8, 8, generator=torch.Generator().manual_seed(5)) * 2 - 1
    dc, _, _ = _dc(pred_param, backbone=LineBackbone(xs, pred_param), sampler=sampler)
    lab = torch.zeros(5, dtype=torch.int64)
    z = dc.invert(xs, lab, 0.5)
    z64 = O.invert64(dc, xs, lab, 0.5)
    alpha_u = torch.sqrt(torch.sigmoid(dc.schedule(torch.tensor(0.5, dtype=torch.float64))))
    assert z.dtype == torch.float32 and z.shape == xs.shape
    dz, dl = (z - z64).abs().max().item(), (z - alpha_u * xs).abs().max().item()
    assert (z64 - alpha_u * xs).abs().max().item() < 1e-6
    cl = torch.tensor([0, 2])
    cf = dc.counterfactual(xs, cl, 0.5, start="invert", invert_class=lab)
    d64 = O.counterfactual64(dc, z64, cl.expand(5, 2), 0.5, sampler)
    dd, dx = (cf.samples - d64).abs().max().item(), (cf.samples - xs[:, None]).abs().max().item()
    print(f"{pred_param} {sampler}: latent vs float64 {dz:.2e}, vs alpha_u x* {dl:.2e}; decode vs float64 {dd:.2e}, vs x* {dx:.2e}")
    assert dz <= TOL_INVERT and dl <= TOL_INVERT
    assert dd <= TOL_LINE_DECODE and dx <= TOL_LINE_DECODE
    assert float(cf.maps.max()) <= 3 * TOL_LINE_DECODE                   # the maps against the input: three channels of nothing


# ------------------------------------------------------------------------------------------------ the float64 statement
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("pred_param", ["eps", "v"])
def test_foreign_paths_equal_the_float64_statement(pred_param, sampler):
    dc, x, cfg = _dc(pred_param, sampler=sampler)
    BS = x.shape[0]
    lab = torch.arange(BS) % cfg["classes"]
    cl = torch.stack([(torch.arange(3) + b) % cfg["classes"] for b in range(BS)])
    seen = {}
    for from_t in (0.5, 1):
        torch.manual_seed(SEED)
        got = dc.sample(x, lab, from_t=from_t)
        torch.manual_seed(SEED)
        z0 = S.initial_latent(dc, x, from_t)
        want = O.decode64(dc, z0, lab, from_t, sampler)
        assert got.dtype == torch.float32 and got.shape == x.shape
        seen[f"sample {from_t}"] = (got - want).abs().max().item()
        assert seen[f"sample {from_t}"] <= TOL_DECODE
    # counterfactual from shared noise: the K classes decoded from the one draw
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, cl, 0.5)
    torch.manual_seed(SEED)
    z0 = S.initial_latent(dc, x, 0.5)
    want = O.counterfactual64(dc, z0, cl, 0.5, sampler)
    seen["counterfactual"] = (cf.samples - want).abs().max().item()
    assert seen["counterfactual"] <= TOL_DECODE
    assert (want[:, 0] - want[:, 1]).abs().max().item() > 0.1                 # the labels do matter
    assert torch.equal(cf.classes, cl) and tuple(cf.maps.shape) == (BS, 3) + tuple(x.shape[2:])
    # inversion, under a class with guidance and under the null token without
    z = dc.invert(x, lab, 0.5, guidance=0.5)
    seen["invert w=0.5"] = (z - O.invert64(dc, x, lab, 0.5, 0.5)).abs().max().item()
    zn = dc.invert(x)
    null = torch.full((BS,), cfg["classes"], dtype=torch.int64)
    zn64 = O.invert64(dc, x, null, 0.5)
    seen["invert null"] = (zn - zn64).abs().max().item()
    assert seen["invert w=0.5"] <= TOL_INVERT and seen["invert null"] <= TOL_INVERT
    # counterfactual from the inverted latent, against a class
    cfi = dc.counterfactual(x, cl, 0.5, start="invert", invert_class=lab, against=cl[:, 1])
    want = O.counterfactual64(dc, O.invert64(dc, x, lab, 0.5), cl, 0.5, sampler)
    seen["counterfactual invert"] = (cfi.samples - want).abs().max().item()
    assert seen["counterfactual invert"] <= TOL_INVERT
    maps = torch.zeros_like(cfi.maps)
    for c in range(x.shape[1]):
        maps = maps + (cfi.samples[:, :, c] - cfi.samples[:, 1:2, c]).abs()
    assert torch.equal(cfi.maps, maps)
    cfn = dc.counterfactual(x, cl, 0.5, start="invert")                       # invert_class None: the null token
    assert (cfn.samples - O.counterfactual64(dc, zn64, cl, 0.5, sampler)).abs().max().item() <= TOL_INVERT
    print(pred_param, sampler, {k: f"{v:.2e}" for k, v in seen.items()})


# ------------------------------------------------------------------------------------------------ determinism
def test_inverted_counterfactual_touches_no_generator_and_repeats_bit_for_bit():
    dc, x, cfg = _dc("v", sampler="dpmpp_2m")
    lab = torch.arange(x.shape[0]) % cfg["classes"]
    torch.manual_seed(SEED)
    before = torch.get_rng_state()
    a = dc.counterfactual(x, None, 0.5, start="invert", invert_class=lab)
    assert torch.equal(torch.get_rng_state(), before)
    torch.manual_seed(SEED + 1)
    b = dc.counterfactual(x, None, 0.5, start="invert", invert_class=lab)
    assert torch.equal(a.samples, b.samples) and torch.equal(a.maps, b.maps)
    # start="noise" under a deterministic sampler takes the initial draw alone: the generator stands where `diffuse` leaves it
    torch.manual_seed(SEED)
    dc.counterfactual(x, None, 0.5)
    after = torch.rand(1)
    torch.manual_seed(SEED)
    S.initial_latent(dc, x, 0.5)
    assert torch.equal(after, torch.rand(1))


# ------------------------------------------------------------------------------------------------ the default path
def test_default_path_is_untouched():
    """config.sampler unset: `sample` gives the reference golden as test_next_rows.py reads it, and "ddpm" is the same bits."""
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "sample_cases.npz")))
    for tag in ("eps", "v_from_t"):
        outs = []
        for sampler in (None, "ddpm"):
            dc, _, _ = _dc("v" if tag.startswith("v") else "eps", **({} if sampler is None else {"sampler": sampler}))
            torch.manual_seed(int(g[tag + ".seed"]))
            outs.append(dc.sample(torch.from_numpy(g[tag + ".x"]), torch.from_numpy(g[tag + ".labels"]), from_t=float(g[tag + ".from_t"])))
        np.testing.assert_allclose(outs[0].numpy(), g[tag + ".out"], rtol=0, atol=2e-6)
        assert torch.equal(outs[0], outs[1])
    dc, x, _ = _dc()
    torch.manual_seed(SEED)
    a = dc.counterfactual(x, None, 0.5)
    dc.config.sampler = "ddpm"
    torch.manual_seed(SEED)
    assert torch.equal(dc.counterfactual(x, None, 0.5).samples, a.samples)
    dc.config.sampler = "ddim"
    torch.manual_seed(SEED)
    assert not torch.equal(dc.counterfactual(x, None, 0.5).samples, a.samples)


# ------------------------------------------------------------------------------------------------ refusals
def test_error_paths():
    dc, x, cfg = _dc(sampler="euler")
    BS = x.shape[0]
    for call in (lambda: dc.sample(x, torch.zeros(BS, dtype=torch.int64)), lambda: dc.counterfactual(x)):
        with pytest.raises(ValueError, match="'ddpm', 'ddim', 'dpmpp_2m'"):
            call()
    assert torch.isfinite(dc.invert(x)).all()                                 # always DDIM, whatever config.sampler says
    for sampler in (None, "ddpm"):
        dc.config.sampler = sampler
        with pytest.raises(ValueError, match="start='invert'"):
            dc.counterfactual(x, start="invert")
    dc.config.sampler = "ddim"
    with pytest.raises(ValueError, match="start"):
        dc.counterfactual(x, start="latent")
    with pytest.raises(ValueError, match="invert_class"):
        dc.counterfactual(x, invert_class=torch.zeros(BS, dtype=torch.int64))            # belongs to start="invert"
    for bad in (torch.zeros(BS + 1, dtype=torch.int64), torch.zeros(BS, 1, dtype=torch.int64), torch.zeros(BS), torch.zeros(BS, dtype=torch.bool),
                torch.full((BS,), cfg["classes"] + 1), torch.full((BS,), -1)):
        with pytest.raises(ValueError, match="invert_class"):
            dc.counterfactual(x, start="invert", invert_class=bad)
        with pytest.raises(ValueError, match="text"):
            dc.invert(x, bad)
    for bad in (0, 0.0, -0.5, 1.0001, 2, float("nan")):
        with pytest.raises(ValueError, match="to_t"):
            dc.invert(x, None, bad)
        with pytest.raises(ValueError, match="from_t"):
            dc.counterfactual(x, None, bad, start="invert")
    with pytest.raises(L.DcamdError, match="philox"):
        dc.counterfactual(x, rng="philox")                                    # kept: a foreign backbone has no device RNG
    # a refusal consumed no random numbers
    torch.manual_seed(SEED)
    a = torch.rand(1)
    torch.manual_seed(SEED)
    with pytest.raises(ValueError):
        dc.counterfactual(x, start="invert", invert_class=torch.zeros(BS + 1, dtype=torch.int64))
    assert torch.equal(a, torch.rand(1))
