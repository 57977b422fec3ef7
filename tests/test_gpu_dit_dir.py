"""GPU: a published-style DiT — learned-variance outputs (out_channels = 2 * in_channels), the 'ddpm_linear' schedule, 1000 classes,
and the route from a directory on disk to `classify` — against the test-side oracle (tests/dit_dir_oracle.py) and against the
out_channels = in_channels twin whose proj_out_2 holds exactly the eps rows.

  A   2 heads x 32, 2 layers, 8x8 latents in patches of 2: eps is 16 of the 32 projection columns (the XL/2 case, below one N tile)
  B   the same at 16x16 in patches of 4: eps is 64 of 128 columns

The plans that feed a scoring tail or a step kernel project the eps rows only (the slicing form): a 2C model and its twin launch the
same kernels on the same packed weights, so everything they compute through those plans agrees bit for bit.

Measured on an MI355X (first run): f32 forward rel-L2 3.3e-7 (A) / 4.1e-7 (B), bound 2e-5; f32 classify per-cell 2.7e-7, bound 1e-4; bf16
forward 2.66e-3 (A) / 2.73e-3 (XL heads), bound 5e-3; 1000 classes 4.0e-7, bound 1e-4.
"""
import pytest
import torch

import diffusion_classifier_amd as dca
import dit_dir_oracle as DO
import oracle
from diffusion_classifier_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEO = {"A": DO.DIT_A, "B": DO.DIT_B}
STEPS = torch.tensor([999.0, 17.0, 250.0])


def relerr(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


_CASES = {}


def case(name):
    """(model on the CPU, fp32 OracleDiT with its weights, forward inputs, the oracle's 8-channel output): once per geometry, shared
    and left unchanged."""
    if name not in _CASES:
        kw = GEO[name]
        m = DO.make_dit(kw, seed=50 + len(_CASES))
        o = oracle.OracleDiT(**kw)
        o.load_state_dict(m.state_dict())
        torch.manual_seed(51)
        hw = kw["sample_size"]
        x, lab = torch.randn(3, 4, hw, hw), torch.tensor([1, 10, 3])                  # 10: the null row of the tables
        with torch.no_grad():
            ref = o(x, STEPS, lab)
        _CASES[name] = (m, o, (x, STEPS, lab), ref)
    return _CASES[name]


def _po2(plan):
    (op,) = [(f, mt) for (_, _, f), mt in zip(plan.pb.ops, plan.pb.meta) if mt.get("name") == "proj_out_2"]
    return op


# ------------------------------------------------------------------------------------------------ 1. f32 forward, all channels
@pytest.mark.parametrize("name", list(GEO))
def test_forward_f32_returns_all_channels_against_the_oracle(name):
    m, _, (x, step, lab), ref = case(name)
    md = m.to(DEV).set_compute_dtype("f32")
    got = md(x.to(DEV), step.to(DEV), lab.to(DEV)).cpu()
    m.cpu()
    r, r_eps, r_var = relerr(got, ref), relerr(got[:, :4], ref[:, :4]), relerr(got[:, 4:], ref[:, 4:])
    print(f"{name} f32 forward, 8 channels: rel-L2 {r:.2e} (eps half {r_eps:.2e}, variance half {r_var:.2e}; bound 2e-5)")
    assert tuple(got.shape) == tuple(ref.shape) == (3, 8, x.shape[2], x.shape[3])
    assert r < 2e-5 and r_eps < 2e-5 and r_var < 2e-5, (r, r_eps, r_var)


# ------------------------------------------------------------------------------------------------ 2. f32 classify, ddpm_linear
_CLASSIFY = {}


def classify_case():
    """Model A under schedule='ddpm_linear': (classifier on the device, inputs, its labels and errors, the oracle's), computed once."""
    if not _CLASSIFY:
        m = case("A")[0]
        dc, cfg = DO.classifier(m)
        oc, fed = DO.oracle_classifier(m, cfg)
        torch.manual_seed(52)
        BS, T = 2, 4
        x = torch.rand(BS, 4, 8, 8) * 2 - 1
        t, eps = torch.tensor([[0.9995, 0.0172], [0.5, 0.25], [0.0, 0.731], [0.1234, 1.0]]), torch.randn(T, BS, 4, 8, 8)
        ref_l, ref_e = oc.classify(x, t=t, eps=eps, return_errors=True)
        dc = dc.to(DEV)
        got_l, got_e = dc.classify(x.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
        dc.check_device_errors()
        _CLASSIFY.update(dc=dc, cfg=cfg, x=x, t=t, eps=eps, got=(got_l.cpu(), got_e), ref=(ref_l, ref_e), fed=fed.seen_labels)
    return _CLASSIFY


def test_classify_f32_ddpm_linear_against_the_oracle():
    c = classify_case()
    (got_l, got_e), (ref_l, ref_e) = c["got"], c["ref"]
    rel = ((got_e - ref_e).abs() / ref_e).max().item()
    print(f"A f32 classify, ddpm_linear: per-cell eps-MSE max rel err {rel:.2e} (bound 1e-4); labels {got_l.tolist()} / {ref_l.tolist()}")
    assert tuple(got_e.shape) == (2, 3, 4) and torch.isfinite(got_e).all()
    assert rel < 1e-4, rel
    assert got_l.tolist() == ref_l.tolist()
    # every label the oracle backbone was fed is an integer step, k = min(floor(t * 1000), 999) — and so is every one the plan was fed
    steps = torch.tensor([[999.0, 17.0], [500.0, 250.0], [0.0, 731.0], [123.0, 999.0]])
    fed = c["fed"]
    assert len(fed) == 4 * 3 and all(torch.equal(s, steps[i // 3]) for i, s in enumerate(fed)), fed
    assert all(bool((s == s.round()).all()) and s.dtype == torch.float32 for s in fed)
    (sp,) = list(c["dc"]._score_plans.values())
    lam = sp["layout"].view(sp["ctl"], "lam").cpu()
    assert sorted(lam.tolist()) == sorted(steps.reshape(-1).tolist()), lam
    # the scoring plan projects the 16 eps rows, on the 32-wide tile
    f, mt = _po2(sp["plan"])
    assert f["Cout"] == 16 and f["tile_n"] == 32 and sp["plan"].pred.C == 16 and "invalid" not in mt["family"], (f["Cout"], mt)


# ------------------------------------------------------------------------------------------------ 3. the twin
GEN = dict(cfg_w=1.5, sampling_steps=4, timestep_spacing="trailing")


@pytest.mark.parametrize("name", list(GEO))
def test_a_learned_variance_model_and_its_eps_twin_agree_bit_for_bit(name):
    """The slicing form: scoring and pair plans of the 2C model run proj_out_2 on its eps rows alone — the twin's whole projection — so
    classify's errors, forward_pair, ancestral and DDIM sampling, the DDPM inversion and the counterfactuals decoded from it are the
    same bits.  (Before learned-variance outputs were served the 2C side compared the wrong numbers in classify and raised in the rest.)"""
    m = case(name)[0]
    tw = DO.eps_twin(m)
    hw = GEO[name]["sample_size"]
    torch.manual_seed(53)
    BS, T = 2, 4
    x = torch.rand(BS, 4, hw, hw) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 4, hw, hw)
    lab, cl = torch.tensor([2, 0]), torch.tensor([[0, 2, 1], [1, 0, 2]])
    out = {}
    for who, model in (("2C", m), ("twin", tw)):
        dc, _ = DO.classifier(model, **GEN)
        dc = dc.to(DEV)
        xd = x.to(DEV)
        r = {}
        r["labels"], r["errors"] = dc.classify(xd, t=t, eps=eps.to(DEV), return_errors=True)
        bb = dc.ema.ema_model
        r["pair"] = bb.forward_pair(xd, torch.tensor([431.0, 7.0], device=DEV), lab.to(DEV), torch.full_like(lab, 3).to(DEV)).clone()
        torch.manual_seed(54)
        r["sample"] = dc.sample(xd, lab.to(DEV), from_t=1)
        dc.config.sampler = "ddim"
        torch.manual_seed(54)
        r["ddim"] = dc.sample(xd, lab.to(DEV), from_t=1)
        dc.config.sampler = None
        torch.manual_seed(55)
        inv = dc.invert_ddpm(xd, lab.to(DEV), 0.6)
        r["inv_start"], r["inv_noise"] = inv.start, inv.noise
        torch.manual_seed(55)
        cf = dc.counterfactual(xd, cl, 0.6, start="ddpm_invert", invert_class=lab)
        r["cf_samples"], r["cf_maps"] = cf.samples, cf.maps
        dc.check_device_errors()
        if who == "2C":
            p = GEO[name]["patch_size"]
            assert tuple(r["pair"].shape) == (2 * BS, hw // p, hw // p, p * p * 4)          # eps alone, feature stride C
            plans = bb._plans
            assert all(pl.pred.C == p * p * 4 for k, pl in plans.items() if k[0] != "fwd") and any(k[0] == "pair" for k in plans)
        out[who] = {k: v.detach().cpu() for k, v in r.items()}
    for k, v in out["2C"].items():
        w = out["twin"][k]
        assert torch.isfinite(v.float()).all(), k
        assert torch.equal(v, w), (name, k, (v.double() - w.double()).abs().max().item())
    assert tuple(out["2C"]["sample"].shape) == (BS, 4, hw, hw) and tuple(out["2C"]["cf_samples"].shape) == (BS, 3, 4, hw, hw)
    assert not torch.equal(out["2C"]["sample"], out["2C"]["ddim"])
    # the plain forward still returns the variance half, and its eps half is the twin's whole output
    full = m.to(DEV)(x.to(DEV), STEPS[:2].to(DEV), lab.to(DEV)).cpu()
    half = tw.to(DEV)(x.to(DEV), STEPS[:2].to(DEV), lab.to(DEV)).cpu()
    m.cpu()
    assert tuple(full.shape) == (BS, 8, hw, hw) and tuple(half.shape) == (BS, 4, hw, hw)
    assert relerr(full[:, :4], half) < 2e-5          # two different GEMM shapes: the f32 forward bound, not bits


# ------------------------------------------------------------------------------------------------ 4. bf16 forward
DIT_XL_CUT = dict(num_attention_heads=16, attention_head_dim=72, in_channels=4, out_channels=8, num_layers=2, sample_size=32, patch_size=2,
                  num_embeds_ada_norm=10)


@pytest.mark.parametrize("name", ["A", "XL"])
def test_forward_bf16_against_the_low_precision_oracle(name):
    """Bound: 5e-3 rel-L2 against the oracle with bf16 storage rounding, what tests/test_gpu_head_width.py applies to its bf16 DiT
    forward.  XL: the published head geometry (16 x 72, padded to 96; D = 1152, 256 tokens) cut to 2 layers, with 8 output channels."""
    kw = GEO["A"] if name == "A" else DIT_XL_CUT
    m = DO.make_dit(kw, seed=56)
    o = oracle.OracleDiT(**kw, lowp=True, lowp_dtype=torch.bfloat16)
    o.load_state_dict(m.state_dict())
    torch.manual_seed(57)
    hw = kw["sample_size"]
    x, step, lab = torch.randn(2, 4, hw, hw), torch.tensor([640.0, 33.0]), torch.tensor([4, 7])
    with torch.no_grad():
        ref = o(x, step, lab)
    md = m.to(DEV).set_compute_dtype("bf16")
    got = md(x.to(DEV), step.to(DEV), lab.to(DEV)).cpu()
    r = relerr(got, ref)
    print(f"{name} bf16 forward, 8 channels: rel-L2 against the bf16-rounded oracle {r:.3e} (bound 5e-3)")
    assert tuple(got.shape) == (2, 8, hw, hw) and torch.isfinite(got).all()
    assert r < 5e-3, r
    f, mt = _po2(next(iter(md._plans.values())))
    assert f["Cout"] == 32 and "invalid" not in mt["family"]


# ------------------------------------------------------------------------------------------------ 5. 1000 classes
SEED_1000 = 61          # chosen on the CPU, in the oracle alone: see the assertion on `gap` below


def test_thousand_classes_through_stage_pruning():
    """Model A with 1000 classes, one image, two stages (1 trial keeping 8, then 2 more), 8 units per launch: stage 2 runs as two
    micro-batches.  Labels and the surviving classes equal the oracle's, errors within the f32 bound.  The seed is one at which, in the
    oracle alone, the 8th and 9th class means of stage 1 differ by more than 1e-3 relative: no tie at the cut."""
    kw = dict(DO.DIT_A, num_embeds_ada_norm=1000)
    m = DO.make_dit(kw, seed=SEED_1000)
    over = dict(classes=1000, n_stages=2, evaluation_per_stage=[1, 3], n_keep_per_stage=[8, 1], units_per_launch=8)
    dc, cfg = DO.classifier(m, **over)
    oc, _ = DO.oracle_classifier(m, cfg)
    torch.manual_seed(SEED_1000 + 1)
    x = torch.rand(1, 4, 8, 8) * 2 - 1
    t, eps = torch.tensor([[0.62], [0.35], [0.81]]), torch.randn(3, 1, 4, 8, 8)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # 1016 batch-1 forwards of a tiny model: a thread pool only costs (2 ms a call on one thread)
    try:
        ref_l, ref_e = oc.classify(x, t=t, eps=eps, return_errors=True)
    finally:
        torch.set_num_threads(threads)
    stage1 = ref_e[0, :, 0].sort().values
    gap = ((stage1[8] - stage1[7]) / stage1[7]).item()
    final = ref_e[0, torch.isfinite(ref_e[0, :, 2])].mean(1).sort().values
    assert gap > 1e-3 and (final[1] - final[0]) / final[0] > 1e-3, (gap, final)      # measured on the CPU: 3.4e-3 and 1.1e-2
    kept_ref = sorted(torch.isfinite(ref_e[0, :, 2]).nonzero().reshape(-1).tolist())
    assert len(kept_ref) == 8 and kept_ref == sorted(ref_e[0, :, 0].topk(8, largest=False).indices.tolist())
    dc = dc.to(DEV)
    got_l, got_e = dc.classify(x.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    dc.check_device_errors()
    kept = sorted(torch.isfinite(got_e[0, :, 2]).nonzero().reshape(-1).tolist())
    fin = torch.isfinite(ref_e)
    rel = ((got_e[fin] - ref_e[fin]).abs() / ref_e[fin]).max().item()
    print(f"1000 classes: kept {kept} / {kept_ref}; label {got_l.tolist()} / {ref_l.tolist()}; max rel err {rel:.2e} (bound 1e-4); "
          f"gap at the cut {gap:.2e}")
    assert kept == kept_ref and torch.equal(torch.isfinite(got_e), fin)
    assert torch.isfinite(got_e[0, :, 0]).all()                                      # all 1000 classes were scored in stage 1
    assert rel < 1e-4, rel
    assert got_l.cpu().tolist() == ref_l.tolist()
    sizes = sorted((sp["n_bj"], sp["k"]) for sp in dc._score_plans.values())
    assert sizes == [(1, 8), (1, 1000)], sizes                                       # stage 2: two launches of one pair x 8 classes


# ------------------------------------------------------------------------------------------------ 6. directory to classify
def test_from_a_directory_to_classify(tmp_path):
    c = classify_case()
    m = case("A")[0]
    d = DO.write_transformer(tmp_path, "transformer", GEO["A"], m.state_dict())
    sched = DO.write_scheduler(tmp_path)
    loaded = dca.DiT.from_directory(d)
    dc, _ = DO.classifier(loaded, scheduler_path=sched)
    assert dc.train_timesteps == 1000 and torch.equal(dc.ddpm_logsnr, c["dc"].ddpm_logsnr)
    dc = dc.to(DEV)
    got_l, got_e = dc.classify(c["x"].to(DEV), t=c["t"], eps=c["eps"].to(DEV), return_errors=True)
    dc.check_device_errors()
    assert torch.equal(got_l.cpu(), c["got"][0]) and torch.equal(got_e, c["got"][1])
    assert int(L.lib().dc_pn_timeouts()) == 0
