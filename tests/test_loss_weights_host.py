"""CPU: the weights of the scoring loss — config.trial_weighting (with config.min_snr_gamma), classify(..., pixel_weight=),
config.pixel_weight_key and DiffusionClassifier.loss — on foreign stand-in backbones (the `_ForeignRunner` path, loss.py's torch
statements): the refusals by name, "train" against the reference's formula restated here, a callable and a step table under
'scaled_linear', the two exactness properties of the definition (ones give the unweighted bits; errors_w == errors * w), a 0/1 mask
against the unweighted run on inputs zeroed outside it, a mask that changes the label, `loss` against a value captured from the
reference's own `loss` (tools/capture_loss_golden.py -> tests/golden/loss_cases.npz), and the weights block behind the two (unchanged) structs."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import evidence as EV
from diffusion_classifier_amd import loss as LS
import early_stop_oracle as SO
import loss_weights_oracle as WO
import score_loss_oracle as O
from standin import TinyBackbone
from test_abi_host import _c_compiler

HERE = os.path.dirname(os.path.abspath(__file__))
ONE_STAGE = dict(n_stages=1, evaluation_per_stage=[7], n_keep_per_stage=[1])
DISCRETE = dict(schedule="scaled_linear", train_timesteps=50, **ONE_STAGE)


def _bits(v):
    v = v.cpu().contiguous()
    return v.view(torch.int32) if v.dtype == torch.float32 else v


def _reference_weight(logsnr, pred_param, gamma=5.0):
    """Reference diffusion_classifier.py:331-337, restated."""
    snr = torch.exp(logsnr).clamp(max=gamma)
    return 1 / (1 + snr) if pred_param == "v" else 1 / snr


# ------------------------------------------------------------------------------------------------ refusals, each by name
def test_uniform_and_none_resolve_to_no_weights():
    for cfg in (dict(), dict(trial_weighting=None), dict(trial_weighting="uniform")):
        assert LS.trial_weighting_of(dca.Config(**cfg)) is None
        dc, x, t, eps = SO.standin_classifier(dca, **cfg)
        assert dc.trial_weighting is None and "weight" not in dc._trial_draws(x, 7, t, eps, "reference", 0)
    assert LS.trial_weighting_of(dca.Config(trial_weighting="train")) == ("train", 5.0)
    assert LS.trial_weighting_of(dca.Config(trial_weighting="train", min_snr_gamma=3)) == ("train", 3.0)


@pytest.mark.parametrize("bad", ["Train", "min_snr", "", 1, 0.5, True, {"a": 1}])
def test_an_unknown_trial_weighting_is_refused_by_name(bad):
    with pytest.raises(ValueError, match="trial_weighting.*'uniform'.*'train'.*callable"):
        LS.trial_weighting_of(dca.Config(trial_weighting=bad))
    with pytest.raises(ValueError, match="trial_weighting"):
        SO.standin_classifier(dca, trial_weighting=bad)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), "5", True, [5.0]])
def test_a_bad_min_snr_gamma_is_refused(bad):
    with pytest.raises(ValueError, match="min_snr_gamma"):
        SO.standin_classifier(dca, trial_weighting="train", min_snr_gamma=bad)


@pytest.mark.parametrize("other", [None, "uniform", (lambda l: torch.ones_like(l))])
def test_min_snr_gamma_next_to_another_weighting_is_refused(other):
    with pytest.raises(ValueError, match="min_snr_gamma.*trial_weighting"):
        SO.standin_classifier(dca, min_snr_gamma=4.0, **({} if other is None else {"trial_weighting": other}))


def test_a_step_table_is_refused_outside_the_discrete_schedules_and_at_a_wrong_length():
    with pytest.raises(ValueError, match="trial_weighting.*discrete"):
        SO.standin_classifier(dca, trial_weighting=[1.0] * 50)
    for bad in ([1.0] * 49, torch.ones(51), torch.ones(2, 25), np.ones(7)):
        with pytest.raises(ValueError, match="trial_weighting.*train_timesteps = 50"):
            SO.standin_classifier(dca, trial_weighting=bad, **DISCRETE)
    for bad in ([1.0] * 49 + [-1.0], [float("nan")] + [1.0] * 49, [float("inf")] * 50):
        with pytest.raises(ValueError, match="trial_weighting.*finite and >= 0"):
            SO.standin_classifier(dca, trial_weighting=bad, **DISCRETE)
    with pytest.raises(ValueError, match="trial_weighting"):
        SO.standin_classifier(dca, trial_weighting=["a"] * 50, **DISCRETE)


@pytest.mark.parametrize("f,word", [
    (lambda l: torch.ones(3), "shape"), (lambda l: [1.0], "shape"), (lambda l: torch.ones_like(l).long(), "float"),
    (lambda l: -torch.ones_like(l), "finite and >= 0"), (lambda l: l * float("nan"), "finite and >= 0"),
    (lambda l: torch.full_like(l, float("inf")), "finite and >= 0")])
def test_a_callable_that_returns_no_weights_is_refused_at_the_call(f, word):
    dc, x, t, eps = SO.standin_classifier(dca, trial_weighting=f)
    with pytest.raises(ValueError, match="trial_weighting.*" + word):
        dc.classify(x, t=t, eps=eps)


def test_trial_weighting_with_simulate_rank_is_refused():
    dc, x, t, eps = SO.standin_classifier(dca, trial_weighting="train", simulate_rank=(0, 2))
    with pytest.raises(ValueError, match="trial_weighting.*simulate_rank"):
        dc.classify(x, t=t, eps=eps)


def test_a_bad_pixel_weight_is_refused_by_name():
    dc, x, t, eps = SO.standin_classifier(dca)
    BS, _, H, W = x.shape
    for bad in (torch.ones(BS, H), torch.ones(BS, 3, H, W), torch.ones(BS, H, W + 1), torch.ones(BS - 1, H, W), torch.ones(H, W),
                torch.ones(BS, 1, 1, H, W), torch.ones(BS, H, W, dtype=torch.int64), torch.ones(BS, H, W, dtype=torch.bool),
                np.ones((BS, H, W), dtype=np.float32), [[1.0]], 1.0):
        with pytest.raises(ValueError, match="pixel_weight"):
            dc.classify(x, t=t, eps=eps, pixel_weight=bad)
    for ok in (torch.ones(BS, H, W), torch.ones(BS, 1, H, W), torch.ones(BS, H, W, dtype=torch.float64), torch.ones(BS, H, W, dtype=torch.bfloat16)):
        m = LS.pixel_weight_of(ok, BS, H, W)
        assert m.dtype == torch.float32 and tuple(m.shape) == (BS, H, W) and m.is_contiguous()


# ------------------------------------------------------------------------------------------------ the trial weights
@pytest.mark.parametrize("pred_param", ["eps", "v"])
@pytest.mark.parametrize("gamma", [None, 2.0])
def test_train_is_the_references_weight_and_the_errors_are_the_fp32_product(pred_param, gamma):
    keys = dict(pred_param=pred_param, **({} if gamma is None else {"min_snr_gamma": gamma}))
    dc, x, t, eps = SO.standin_classifier(dca, trial_weighting="train", **keys, **ONE_STAGE)      # (one stage: no pruning, every cell scored)
    dc0, _, _, _ = SO.standin_classifier(dca, pred_param=pred_param, **ONE_STAGE)
    T, BS = t.shape
    lam = torch.stack([dc.schedule(t[j].clone()) for j in range(T)])
    want = torch.stack([_reference_weight(lam[j], pred_param, 5.0 if gamma is None else gamma) for j in range(T)])
    w = dc._trial_draws(x, T, t, eps, "reference", 0)["weight"]
    assert w.dtype == torch.float32 and tuple(w.shape) == (T, BS) and torch.equal(_bits(w), _bits(want))
    snr = torch.exp(lam)
    assert bool((snr > 5).any()) and bool((snr < 2).any())                    # draws on both sides of the clamp
    _, err_w = dc.classify(x, t=t, eps=eps, return_errors=True)
    _, err = dc0.classify(x, t=t, eps=eps, return_errors=True)
    fin = torch.isfinite(err)
    assert torch.equal(torch.isfinite(err_w), fin) and int(fin.sum()) > 0
    prod = err * w.t()[:, None, :]                                            # errors[b, c, j] * w[j, b], one fp32 multiply
    assert torch.equal(_bits(err_w[fin]), _bits(prod[fin]))
    assert not torch.equal(_bits(err_w[fin]), _bits(err[fin]))


def test_a_callable_and_a_step_table_under_scaled_linear():
    table = torch.linspace(2.0, 0.5, 50)
    seen = []

    def f(logsnr):
        seen.append(logsnr.clone())
        return torch.sigmoid(logsnr) + 0.25

    dc0, x, t, eps = SO.standin_classifier(dca, **DISCRETE)
    _, err = dc0.classify(x, t=t, eps=eps, return_errors=True)
    fin = torch.isfinite(err)
    T, BS = t.shape
    for spec in (table, table.tolist(), tuple(table.tolist()), table.double().numpy()):
        dc, _, _, _ = SO.standin_classifier(dca, trial_weighting=spec, **DISCRETE)
        d = dc._trial_draws(x, T, t, eps, "reference", 0)
        steps = dc.ddpm_step(t)
        assert torch.equal(d["label"], steps.float()) and torch.equal(_bits(d["weight"]), _bits(table[steps]))
        _, err_w = dc.classify(x, t=t, eps=eps, return_errors=True)
        assert torch.equal(_bits(err_w[fin]), _bits((err * d["weight"].t()[:, None, :])[fin]))
    assert len(set(dc.ddpm_step(t).reshape(-1).tolist())) > 10
    dc, _, _, _ = SO.standin_classifier(dca, trial_weighting=f, **DISCRETE)
    _, err_w = dc.classify(x, t=t, eps=eps, return_errors=True)
    lam = torch.stack([dc.schedule(t[j].clone()) for j in range(T)])
    assert len(seen) == 1 and seen[0].dtype == torch.float32 and not seen[0].is_cuda and torch.equal(_bits(seen[0]), _bits(lam))
    assert torch.equal(_bits(err_w[fin]), _bits((err * (torch.sigmoid(lam) + 0.25).t()[:, None, :])[fin]))


@pytest.mark.parametrize("kind", ["l2", "l1", "huber"])
def test_ones_give_the_unweighted_bits_for_errors_posterior_and_maps(kind):
    dc0, x, t, eps = SO.standin_classifier(dca, score_loss=kind)
    dc, _, _, _ = SO.standin_classifier(dca, score_loss=kind, trial_weighting=lambda l: torch.ones_like(l))
    BS, _, H, W = x.shape
    want = dc0.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, return_evidence=True)
    for m in (torch.ones(BS, H, W), torch.ones(BS, 1, H, W, dtype=torch.float64)):
        got = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, return_evidence=True, pixel_weight=m)
        assert torch.equal(got[0], want[0]) and torch.equal(_bits(got[1]), _bits(want[1]))
        for a, b in zip(tuple(got[2]) + tuple(got[3]), tuple(want[2]) + tuple(want[3])):
            assert torch.equal(_bits(a), _bits(b))
    assert torch.isfinite(want[3].mean_map).any()


# ------------------------------------------------------------------------------------------------ the pixel weights
class PixelwiseBackbone(nn.Module):
    """pred[b, :, y, x] = gain(class, t) * (M z[b, :, y, x]): no bias and no neighbourhood, written with elementwise ops, so a pixel's
    prediction has the same bits whatever the other pixels hold, and a zero pixel predicts an exact zero."""

    def __init__(self, ch=3, hid=8):
        super().__init__()
        self.config = SimpleNamespace(encoder_hid_dim=hid)
        self.mix = nn.Parameter(torch.randn(ch, ch) * 0.5)
        self.lin, self.tl = nn.Linear(hid, ch), nn.Linear(1, ch)

    def forward(self, x, noise_labels, encoder_hidden_states=None):
        gain = 1.0 + 0.5 * torch.tanh(self.lin(encoder_hidden_states[:, 0]) + self.tl(noise_labels[:, None].float()))
        return (x[:, None] * self.mix[None, :, :, None, None]).sum(2) * gain[:, :, None, None]


def _pixelwise(seed=3, **over):
    torch.manual_seed(seed)
    dc = dca.DiffusionClassifier(PixelwiseBackbone(), dca.Config(**dict(SO.STANDIN_CFG, **over)))
    BS, T = 4, 7
    return dc, torch.rand(BS, 3, 8, 8) * 2 - 1, torch.rand(T, BS), torch.randn(T, BS, 3, 8, 8)


@pytest.mark.parametrize("kind", ["l2", "l1", "huber"])
@pytest.mark.parametrize("pred_param", ["eps", "v"])
def test_a_mask_is_the_unweighted_run_on_inputs_zeroed_outside_it(kind, pred_param):
    """Exact by construction: outside the mask x = eps = 0 make z = 0, the pixelwise bias-free stand-in predicts 0 there, so d = 0 and
    the term is 0 for every loss; inside, every d has the bits of the full run.  The sums then add the same numbers (zeros for the
    hidden pixels on both sides) in the same order."""
    dc, x, t, eps = _pixelwise(score_loss=kind, pred_param=pred_param)
    BS, _, H, W = x.shape
    m = (torch.rand(BS, H, W, generator=torch.Generator().manual_seed(5)) < 0.6).float()
    m[0] = 0.0
    m[0, 2:5, 1:7] = 1.0
    assert 0.2 < float(m.mean()) < 0.8
    lab_m, err_m, ev_m = dc.classify(x, t=t, eps=eps, return_errors=True, return_evidence=True, pixel_weight=m)
    lab_z, err_z, ev_z = dc.classify(x * m[:, None], t=t, eps=eps * m[None, :, None], return_errors=True, return_evidence=True)
    _, err_f = dc.classify(x, t=t, eps=eps, return_errors=True)
    assert torch.equal(lab_m, lab_z) and torch.equal(_bits(err_m), _bits(err_z))
    for a, b in zip(ev_m, ev_z):
        assert torch.equal(_bits(a), _bits(b))
    fin = torch.isfinite(err_f) & torch.isfinite(err_m)                       # (pruning may differ between the two runs)
    assert int(fin.sum()) > 0 and bool((err_m[fin] < err_f[fin]).all())       # part of every image is hidden
    hidden = (m == 0)[:, None].expand_as(ev_m.mean_map)
    assert bool((torch.nan_to_num(ev_m.mean_map)[hidden] == 0).all())


class RegionBackbone(nn.Module):
    """pred = x + pattern[class]: class 2 is off everywhere, classes 0 and 1 differ in the rows [0, 3) only, where class 0 is off."""

    def __init__(self, H=8, W=8):
        super().__init__()
        self.config = SimpleNamespace(encoder_hid_dim=3)
        p = torch.zeros(3, H, W)
        p[0, :3] = 1.0
        p[2] = 3.0
        self.register_buffer("pattern", p)
        self.dummy = nn.Parameter(torch.zeros(1))

    def forward(self, x, noise_labels, encoder_hidden_states=None):
        cls = encoder_hidden_states[:, 0].argmax(dim=1)
        return x + self.pattern[cls][:, None]


def test_a_mask_that_hides_the_only_region_where_two_classes_differ_changes_the_label():
    """On the whole image class 0 pays for its pattern in rows 0-2 (72 elements of (d + 1)^2 against d^2) and class 1 wins every
    image.  With those rows masked out nothing distinguishes 0 from 1 — their errors are the same bits — and the stage end's tie goes
    to the lower class id: every label moves from 1 to 0."""
    cfg = dict(SO.STANDIN_CFG, **ONE_STAGE)
    dc = dca.DiffusionClassifier(RegionBackbone(), dca.Config(**cfg))
    with torch.no_grad():
        dc.encoder.weight.copy_(torch.eye(4)[:, :3])      # one-hot rows: the backbone reads the class back from them
    torch.manual_seed(9)
    BS, T = 4, 7
    x, t, eps = torch.rand(BS, 3, 8, 8) * 2 - 1, torch.rand(T, BS), torch.randn(T, BS, 3, 8, 8)
    lab, err = dc.classify(x, t=t, eps=eps, return_errors=True)
    assert lab.tolist() == [1] * BS
    m = torch.ones(BS, 8, 8)
    m[:, :3] = 0.0
    lab_m, err_m = dc.classify(x, t=t, eps=eps, return_errors=True, pixel_weight=m)
    assert torch.equal(_bits(err_m[:, 0]), _bits(err_m[:, 1])) and bool((err_m[:, 2] > err_m[:, 1]).all())
    assert not torch.equal(_bits(err[:, 0]), _bits(err[:, 1]))
    assert lab_m.tolist() == [0] * BS
    # hiding the rows where they do NOT differ keeps the label
    lab_k = dc.classify(x, t=t, eps=eps, pixel_weight=1.0 - m)
    assert lab_k.tolist() == [1] * BS


def test_a_nan_weight_poisons_its_image_and_is_counted_by_the_posterior():
    dc, x, t, eps = SO.standin_classifier(dca, **ONE_STAGE)
    BS, _, H, W = x.shape
    m = torch.ones(BS, H, W)
    m[2, 3, 4] = float("nan")
    lab, err, post = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, pixel_weight=m)
    assert torch.isnan(err).all(dim=2).all(dim=1).tolist() == [b == 2 for b in range(BS)]
    assert post.invalid.tolist() == [err.shape[1] * err.shape[2] if b == 2 else 0 for b in range(BS)]


def test_weighted_statements_against_the_float64_oracle():
    """loss.error_torch / evidence.err_map_torch with general weights (m in [0, 2] with exact zeros, w in [0.25, 4]) against
    tests/loss_weights_oracle.py; torch's summation order is its own (adds = N - 1 covers every order), and the l2 statement's
    sqrt(m) d costs two more roundings per term than the model's one (sqrt, and the square's second factor)."""
    g = torch.Generator().manual_seed(21)
    n, C, H, W = 6, 3, 5, 7
    pred, e = torch.randn(n, C, H, W, generator=g), torch.randn(n, C, H, W, generator=g)
    m = torch.rand(n, H, W, generator=g) * 2
    m[:, 1:3, 2:5] = 0.0
    w = 0.25 + 3.75 * torch.rand(n, generator=g)
    d, h = O.differences(pred.numpy(), e.numpy(), None, None, None, np.arange(n), None, False)
    N = C * H * W
    for kind, k in LS.KINDS.items():
        o = WO.weighted_sums(d, h, kind, 1.0, m.double().numpy(), w.double().numpy())
        got = LS.error_torch(pred, e, k, 1.0, pixel_w=m, trial_w=w).double().numpy()
        bound = WO.scalar_bound(o, kind, adds=N - 1 + (2 if kind == "l2" else 0))
        r_sc = float((np.abs(got - WO.scalar_value(o)) / bound).max())
        acc, bad = EV.new_slabs(1, n, H * W, "cpu")
        EV.err_map_torch(pred, e, torch.arange(n), acc[0], bad[0], k, 1.0, pixel_w=m, trial_w=w)
        planes = acc[0, :n].double().numpy().reshape(n, H, W) * 2.0 ** -O.F
        r_pix = float((np.abs(planes - WO.pixel_value(o)) / WO.pixel_bound(o, kind, C)).max())
        print(f"weighted statements {kind}: error / bound — scalar {r_sc:.3g}, planes {r_pix:.3g}")
        assert int(bad.sum()) == 0 and r_sc <= 1.0 and r_pix <= 1.0, (kind, r_sc, r_pix)
        assert float(np.median(np.abs(got / O.sums(d, h, kind, 1.0)["err"] - 1))) > 1e-2          # not the unweighted sums


# ------------------------------------------------------------------------------------------------ evaluate / inference
def test_evaluate_hands_the_batchs_mask_to_classify():
    dc, x, t, eps = SO.standin_classifier(dca, pixel_weight_key="mask")
    BS, _, H, W = x.shape
    m = torch.ones(BS, 1, H, W)
    m[:, :, :4] = 0.0
    calls = []
    real = dc.classify
    dc.classify = lambda *a, **k: calls.append(k) or real(*a, t=t, eps=eps, **k)
    samples, _, _ = dc.evaluate([dict(images=x, mask=m)], classification=True)
    assert len(calls) == 1 and calls[0]["pixel_weight"] is m
    assert torch.equal(samples[0], real(x, t=t, eps=eps, pixel_weight=m))
    # without the key classify is called as it always was
    dc2, _, _, _ = SO.standin_classifier(dca)
    calls2 = []
    real2 = dc2.classify
    dc2.classify = lambda *a, **k: calls2.append(k) or real2(*a, t=t, eps=eps, **k)
    dc2.evaluate([dict(images=x, mask=m)], classification=True)
    assert calls2 == [dict(fast=dc2.config.fast_classification)]
    # a batch without the key named by the config is an error, not a silent unweighted run
    with pytest.raises(KeyError):
        dc.evaluate([dict(images=x)], classification=True)


# ------------------------------------------------------------------------------------------------ loss
def _golden(tag):
    g = dict(np.load(os.path.join(HERE, "golden", "loss_cases.npz")))
    cfg = {k[4:]: v.tolist() for k, v in g.items() if k.startswith("cfg.")}
    bb = TinyBackbone(ch=3, hid=8, n_classes=cfg["classes"], mode="nn")
    bb.load_state_dict({k[len(tag) + 4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(tag + ".bb.")})
    dc = dca.DiffusionClassifier(bb, dca.Config(pred_param=str(g[tag + ".pred_param"]), **cfg))
    with torch.no_grad():
        dc.encoder.weight.copy_(torch.from_numpy(g[tag + ".encoder.weight"]))
    return dc, {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + ".")}


@pytest.mark.parametrize("tag", ["eps", "v"])
def test_loss_is_the_references_own_value(tag):
    """The value the reference's `loss` returned for these inputs and draws.  Bound: both sides evaluate the same fp32 statements per
    element, so they can differ only in the order in which torch.mean adds the N = BS C H W non-negative terms and in the final
    division: each side is within gamma(N - 1 + 1) of the exact mean of those terms, hence |ours - theirs| <= 2 gamma(N) * loss."""
    dc, g = _golden(tag)
    x, labels = torch.from_numpy(g["x"]), torch.from_numpy(g["labels"])
    want = float(g["loss"])
    N = x.numel()
    bound = 2 * O.gamma(N) * want
    got = dc.loss(x, labels, t=torch.from_numpy(g["t"]), eps=torch.from_numpy(g["eps"]))
    assert got.dtype == torch.float32 and got.dim() == 0 and not got.requires_grad
    print(f"loss {tag}: {float(got):.9g} against the reference's {want:.9g}, |diff| {abs(float(got) - want):.3g}, bound {bound:.3g} (N = {N})")
    assert abs(float(got) - want) <= bound
    # the draws in the reference's order: the recorded seed reproduces the recorded draws, hence the value
    torch.manual_seed(int(g["seed"]))
    assert abs(float(dc.loss(x, labels)) - want) <= bound
    # ema=True scores the EMA copy: the same weights here
    assert abs(float(dc.loss(x, labels, t=torch.from_numpy(g["t"]), eps=torch.from_numpy(g["eps"]), ema=True)) - want) <= bound
    # the weight is "train"'s whatever trial_weighting says, and the loss is the squared error whatever score_loss says
    dc.trial_weighting, dc.score_loss = ("call", lambda l: 7 * torch.ones_like(l)), (L.LOSS_L1, 1.0)
    assert float(dc.loss(x, labels, t=torch.from_numpy(g["t"]), eps=torch.from_numpy(g["eps"]))) == float(got)


def test_loss_needs_no_text_on_a_foreign_backbone_only_where_the_backbone_takes_none():
    """text=None reaches a foreign backbone as encoder_hidden_states=None, the reference's behaviour; the HIP refusal is a GPU test."""
    class NoText(nn.Module):
        def forward(self, x, noise_labels, encoder_hidden_states=None):
            assert encoder_hidden_states is None
            return 0.5 * x

    dc = dca.DiffusionClassifier(NoText(), dca.Config(**dict(SO.STANDIN_CFG, encoder_type="DiT")))
    torch.manual_seed(2)
    x = torch.rand(3, 3, 8, 8)
    out = dc.loss(x)
    assert out.dim() == 0 and torch.isfinite(out)


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_the_weights_block_stands_behind_the_unchanged_structs(tmp_path):
    """The structs keep their fields (`loss`, `huber_delta` last); the flag is a #define; the class plan.py fills for a weighted op has
    the layout a C caller gets from `struct { params base; const float* pixel_w; const float* trial_w; int32_t w_T, w_cells; }`."""
    assert L.LOSS_WEIGHTED == 256 and not (L.LOSS_WEIGHTED & (L.LOSS_L1 | L.LOSS_HUBER))
    h = L.ABI
    assert (len(h.structs), len(h.functions), len(h.enums["dc_op_kind"])) == (32, 77, 23) and L.ABI_VERSION == 5
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "dcamd.h"']
    for s_ in ("dc_eps_mse_params", "dc_err_map_params"):
        lines.append(f"typedef struct {{ {s_} base; const float* pixel_w; const float* trial_w; int32_t w_T, w_cells; }} w_{s_};")
    lines.append("int main(void) {")
    for s_ in ("dc_eps_mse_params", "dc_err_map_params"):
        lines.append(f'  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof({s_}), sizeof(w_{s_}), offsetof(w_{s_}, pixel_w), offsetof(w_{s_}, trial_w), '
                     f"offsetof(w_{s_}, w_T), offsetof(w_{s_}, w_cells));")
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "block.c", tmp_path / "block"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_c_compiler(), "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)],
                   check=True)
    rows = [tuple(map(int, ln.split())) for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    for cls, theirs in zip((L.EpsMseParams, L.ErrMapParams), rows):
        assert cls._fields_[-2:] == [("loss", L.i32), ("huber_delta", L.f32)]
        ext = LS.weighted_params(cls)
        assert [n for n, _ in ext._fields_] == [n for n, _ in cls._fields_] + ["pixel_w", "trial_w", "w_T", "w_cells"]
        ours = (ctypes.sizeof(cls), ctypes.sizeof(ext), ext.pixel_w.offset, ext.trial_w.offset, ext.w_T.offset, ext.w_cells.offset)
        assert ours == theirs and ours[2] == ours[0], (ours, theirs)
        for name, _ in cls._fields_:
            assert getattr(ext, name).offset == getattr(cls, name).offset
        assert LS.weighted_params(cls) is ext


@pytest.mark.parametrize("entry,cls", [("dc_eps_mse", L.EpsMseParams), ("dc_err_map", L.ErrMapParams)])
def test_trial_weights_without_their_maps_are_refused_before_any_launch(entry, cls):
    """DC_ERR_ARG, answered without a GPU (a call that passed the checks would launch: none does here)."""
    lib = L.lib()
    ext = LS.weighted_params(cls)
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    base = dict(pred=a, eps=a, n_units=1, C=1, H=2, W=2, ld=1, trial_w=a, w_T=1, w_cells=1, loss=L.LOSS_WEIGHTED)
    base.update(dict(out=a) if cls is L.EpsMseParams else dict(acc=a, bad=a, T=1, cells=1))
    call = lambda **kw: getattr(lib, entry)(ctypes.cast(ctypes.pointer(ext(**kw)), ctypes.POINTER(cls)), None)
    for maps in (dict(), dict(out_index=a), dict(img_of_bj=a)):
        assert call(**dict(base, **maps)) == -1, maps
        msg = lib.dc_last_error().decode()
        assert entry in msg and "trial_w" in msg, msg
    if cls is L.EpsMseParams:                            # dc_err_map refuses its own T / cells <= 0 for every caller, by its older check
        for zero in (dict(w_T=0), dict(w_cells=0), dict(w_T=-1)):
            assert call(**dict(base, out_index=a, img_of_bj=a, **zero)) == -1 and "trial_w" in lib.dc_last_error().decode()
    # the guard against a stray flag bit: the block must look like one even without trial weights (dc_err_map: agree with T / cells)
    for zero in (dict(w_T=0), dict(w_cells=-3)) + ((dict(w_T=2), dict(w_cells=2)) if cls is L.ErrMapParams else ()):
        assert call(**dict(base, trial_w=None, pixel_w=a, **zero)) == -1 and "w_T" in lib.dc_last_error().decode(), zero
    # a bit that is neither a kind nor the flag is refused, an unknown kind under the flag too, and a shape error is still a shape error
    for bad in (7 | L.LOSS_WEIGHTED, 512, L.LOSS_WEIGHTED << 1 | 1):
        assert call(**dict(base, loss=bad)) == -1 and f"loss={bad}" in lib.dc_last_error().decode()
    assert call(**dict(base, H=0)) == -2
