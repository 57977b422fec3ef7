"""GPU: StableDiffusionUNet end to end on two random-weight mini models — forward and classify (schedule='scaled_linear') against the
test-side oracle (tests/sd_unet_oracle.py), the plans' structure, the component kernels at the widths Stable Diffusion adds, and the
launch lists of UNetCondition2D plans against the lists recorded before this class existed.

Both minis: block_out_channels (128, 320), 32 GroupNorm groups, one layer per block, cross-attention at both levels, 4 latent channels.
  SD1-mini   attention_head_dim 2 (head widths 64 and 160), 1x1-conv projections, context 64, 16x16 latents, prompts of 7 tokens
  SD2-mini   attention_head_dim (2, 5) (64 and 64), linear projections, context 128, 8x8 latents, prompts of 5 tokens
They reach GroupNorm groups of 4, 10, 14 and 20 channels, a 160-wide head at 64 tokens and self-attention over 256 tokens.

bf16 forward, measured on an MI355X (the bound is 2 r_o, r_o the bf16-rounded oracle against the fp32 oracle, both on the CPU):
  SD1-mini  HIP 1.051e-2, r_o 1.180e-2;  SD2-mini  HIP 7.814e-3, r_o 8.825e-3  (DESIGN §6o).
"""
import contextlib
import io
import json

import pytest
import torch

import conv_halo_cases as G
import diffusion_classifier_amd as dca
import norm_cases as N
import plan_lists
import test_gpu_conv_halo as TC
import test_gpu_norms as TN
from diffusion_classifier_amd import _lib as L
from sd_unet_oracle import SDOracleUNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASE = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=(128, 320), layers_per_block=1, norm_num_groups=32,
            down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D"))
MINIS = {"sd1": (dict(BASE, cross_attention_dim=64, attention_head_dim=2, use_linear_projection=False), 7),
         "sd2": (dict(BASE, sample_size=8, cross_attention_dim=128, attention_head_dim=(2, 5), use_linear_projection=True), 5)}
CFG = dict(pred_param="eps", schedule="scaled_linear", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, encoder_type="prompt",
           classes=3, n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32")


def relerr(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _randomise_vectors(m):
    """Default inits leave norm affines at (1, 0) and biases tiny: randomise them so a dropped bias or a swapped pair shows."""
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)


def make_pair(name, seed, **oracle_kw):
    kw, S = MINIS[name]
    torch.manual_seed(seed)
    m = dca.StableDiffusionUNet(**kw)
    _randomise_vectors(m)
    o = SDOracleUNet(**kw, **oracle_kw)
    o.load_state_dict(m.state_dict())
    return m, o, kw, S


_INPUTS = {}


def forward_case(name):
    """(model, inputs, fp32 oracle output), computed once per mini and shared by the forward tests (left unchanged)."""
    if name not in _INPUTS:
        m, o, kw, S = make_pair(name, seed=160 + len(name))
        torch.manual_seed(161)
        hw = kw["sample_size"]
        x, step = torch.randn(2, 4, hw, hw) * 0.8, torch.tensor([999.0, 17.0])
        emb, lens = torch.randn(2, S, kw["cross_attention_dim"]), torch.tensor([S, S - 3], dtype=torch.int32)
        with torch.no_grad():
            ref = {"full": o(x, step, encoder_hidden_states=emb), "ragged": o(x, step, encoder_hidden_states=emb, encoder_lengths=lens)}
        _INPUTS[name] = (m, o, (x, step, emb, lens), ref)
    return _INPUTS[name]


def _plan_of(m):
    return list(m._plans.values())[-1]


def _ops(pb, kind):
    return [(f, mt) for (k, _, f), mt in zip(pb.ops, pb.meta) if k == kind]


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", list(MINIS))
def test_forward_f32_against_the_oracle(name):
    m, _, (x, step, emb, lens), ref = forward_case(name)
    m = m.to(DEV).set_compute_dtype("f32")
    got = m(x.to(DEV), step.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    got_r = m(x.to(DEV), step.to(DEV), encoder_hidden_states=emb.to(DEV), encoder_lengths=lens).cpu()
    r, rr = relerr(got, ref["full"]), relerr(got_r, ref["ragged"])
    print(f"{name} f32 forward: rel-L2 {r:.2e}, with prompt lengths {lens.tolist()} {rr:.2e} (bound 5e-5); lengths move the output by "
          f"{relerr(ref['ragged'], ref['full']):.2e}")
    assert r < 5e-5 and rr < 5e-5, (r, rr)
    assert relerr(ref["ragged"], ref["full"]) > 1e-3              # the lengths matter: the two references are different problems
    assert int(L.lib().dc_pn_timeouts()) == 0                  # what DiffusionClassifier.check_device_errors reads


@pytest.mark.parametrize("name", list(MINIS))
def test_forward_bf16_within_twice_the_oracles_own_rounding(name):
    """r_o: relative L2 between the oracle with lowp=True (bf16 storage rounding) and the fp32 oracle, on the CPU.  The HIP output must lie
    within 2 r_o of the fp32 oracle: two independent bf16 roundings of the same graph differ by about sqrt(2) r_o, and the factor 2 leaves
    room for accumulation order.
    Measured on an MI355X (first run of this test): sd1 r = 1.051e-2 against r_o = 1.180e-2 (bound 2.360e-2); sd2 r = 7.814e-3 against
    r_o = 8.825e-3 (bound 1.765e-2)."""
    m, _, (x, step, emb, _), ref = forward_case(name)
    _, o16, _, _ = make_pair(name, seed=160 + len(name), lowp=True)
    with torch.no_grad():
        r_o = relerr(o16(x, step, encoder_hidden_states=emb), ref["full"])
    m = m.to(DEV).set_compute_dtype("bf16")
    got = m(x.to(DEV), step.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    r = relerr(got, ref["full"])
    print(f"{name} bf16 forward: HIP against the fp32 oracle rel-L2 {r:.3e}; the bf16-rounded oracle against it r_o = {r_o:.3e} (bound 2 r_o = {2 * r_o:.3e})")
    assert torch.isfinite(got).all()
    assert r < 2 * r_o, (r, r_o)


# ------------------------------------------------------------------------------------------------ plans
def test_the_160_site_runs_both_attentions_on_the_strip_kernel_in_bf16():
    m, _, (x, step, emb, lens), _ = forward_case("sd1")
    m = m.to(DEV).set_compute_dtype("bf16")
    for kw in ({}, {"encoder_lengths": lens}):
        m(x.to(DEV), step.to(DEV), encoder_hidden_states=emb.to(DEV), **kw)
        plan = _plan_of(m)
        assert plan.varlen == bool(kw)
        for pb in (plan.pb, plan.ctx_pb):
            assert not any(mt["name"] == "ctx.hid_proj" for mt in pb.meta)
            assert not any(mt.get("variant") == "invalid" or "unsupported" in str(mt["family"]) or mt["family"] in ("invalid", "gn-not-fusable")
                           for mt in pb.meta), [mt for mt in pb.meta]
        cross = _ops(plan.pb, L.OP_CROSS_ATTENTION_LEN if kw else L.OP_CROSS_ATTENTION) + (_ops(plan.pb, L.OP_CROSS_ATTENTION) if kw else [])
        wide = [(f, mt) for f, mt in cross if f["d"] == 160]
        names = sorted(mt["name"].rsplit(".", 1)[1] for _, mt in wide)
        # down 1, mid, up 0 x 2: four sites of 320 channels in 2 heads, attn1 (self form) and attn2 each
        assert names == ["attn1"] * 4 + ["attn2"] * 4, names
        assert all(mt["variant"] == "mfma" for _, mt in wide), [(mt["name"], mt["variant"]) for _, mt in wide]
        for f, mt in wide:
            if mt["name"].endswith("attn1"):
                assert f["Lq"] == f["S"] == 64 and f["ld_q"] == f["ld_kv"] == 960 and f["q_map"] is None and f["kv_map"] is None
            else:
                assert f["S"] == 7 and f["Lq"] == 64
        # the 128-channel level (heads of 64, 256 tokens) stays on dc_attention's flash route
        att = _ops(plan.pb, L.OP_ATTENTION)
        assert len(att) == 3 and all(f["d"] == 64 and f["L"] == 256 and mt["variant"].startswith("flash") for f, mt in att), [mt for _, mt in att]
        assert not _ops(plan.pb, L.OP_TBLOCK_FRONT)
    assert int(L.lib().dc_pn_timeouts()) == 0


def test_the_linear_projection_mini_plans_serve_every_op_without_a_wide_head():
    """SD2-mini in bf16, full and ragged prompts: no projection of the context, nothing refused, every head 64 wide (dc_attention for
    attn1, the strip kernel's D = 64 instance for attn2), proj_in / proj_out and the proj_out fold launched as for conv projections."""
    m, _, (x, step, emb, lens), _ = forward_case("sd2")
    m = m.to(DEV).set_compute_dtype("bf16")
    for kw in ({}, {"encoder_lengths": lens}):
        m(x.to(DEV), step.to(DEV), encoder_hidden_states=emb.to(DEV), **kw)
        plan = _plan_of(m)
        for pb in (plan.pb, plan.ctx_pb):
            assert not any(mt["name"] == "ctx.hid_proj" for mt in pb.meta)
            assert not any(mt.get("variant") == "invalid" or "unsupported" in str(mt["family"]) or mt["family"] in ("invalid", "gn-not-fusable")
                           for mt in pb.meta), [mt for mt in pb.meta]
        cross = _ops(plan.pb, L.OP_CROSS_ATTENTION_LEN if kw else L.OP_CROSS_ATTENTION)
        assert len(cross) == 7 and all(f["d"] == 64 and f["S"] == 5 and mt["variant"] == "mfma" for f, mt in cross)      # 2 down, mid, 4 up
        assert bool(_ops(plan.pb, L.OP_CROSS_ATTENTION)) == (not kw)
        assert len(_ops(plan.pb, L.OP_ATTENTION)) == 7 and all(f["d"] == 64 for f, _ in _ops(plan.pb, L.OP_ATTENTION))
        names = [mt["name"] for mt in plan.pb.meta]
        assert sum(n.endswith(".proj_in") for n in names) == 7 and sum(n.endswith(".ff_proj_out") for n in names) == 7
    assert int(L.lib().dc_pn_timeouts()) == 0


def test_one_token_context_runs_on_the_class_vector_path_without_the_projection():
    """SD never uses S = 1, but the class must not break on it: the class vector of every site straight from the context rows."""
    m, o, kw, _ = make_pair("sd1", seed=170)
    torch.manual_seed(171)
    x, step, emb = torch.randn(2, 4, 16, 16), torch.tensor([500.0, 3.0]), torch.randn(2, 1, 64)
    with torch.no_grad():
        ref = o(x, step, encoder_hidden_states=emb)
    m = m.to(DEV)
    got = m(x.to(DEV), step.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    plan = _plan_of(m)
    assert [mt["name"] for mt in plan.ctx_pb.meta][0] == "ctx.to_v" and not _ops(plan.pb, L.OP_CROSS_ATTENTION_LEN)
    assert sorted(f["d"] for f, _ in _ops(plan.pb, L.OP_CROSS_ATTENTION)) == [160] * 4          # attn1 of the wide sites only
    r = relerr(got, ref)
    print(f"sd1 f32 forward, one-token context: rel-L2 {r:.2e} (bound 5e-5)")
    assert r < 5e-5, r


def test_unet_condition_2d_plans_launch_what_they_launched_before():
    with open(plan_lists.FIXTURE) as f:
        want = json.load(f)
    got = plan_lists.plan_lists(DEV)
    assert sorted(got) == sorted(want)
    for name in want:
        for part in ("ctx", "main"):
            assert got[name][part] == want[name][part], (name, part, [(a, b) for a, b in zip(got[name][part], want[name][part]) if a != b][:5])


# ------------------------------------------------------------------------------------------------ classify
def _classifier(backbone, kw, S, **over):
    cfg = dict(CFG, prompt_tokens=S, noise_d=kw["sample_size"], image_size=kw["sample_size"], **over)
    with contextlib.redirect_stdout(io.StringIO()):
        return dca.DiffusionClassifier(backbone, dca.Config(**cfg))


@pytest.mark.parametrize("name, ragged, pred_param", [("sd1", True, "eps"), ("sd2", False, "eps"), ("sd1", False, "v")])
def test_classify_f32_scaled_linear_against_the_oracle_as_a_foreign_backbone(name, ragged, pred_param):
    """The same DiffusionClassifier twice: over the HIP backbone (scoring plans, the step in the control block's lam slot) and over the
    test oracle as a foreign nn.Module (eager torch, the step as noise_labels).  Ragged prompts: the HIP side gets the table's lengths;
    the foreign call has no mask argument, so the oracle reads the zero rows `set_prompt` leaves behind a short prompt as padding."""
    m, o, kw, S = make_pair(name, seed=180 + len(pred_param), zero_rows_are_padding=ragged)
    dc, oc = _classifier(m, kw, S, pred_param=pred_param), _classifier(o, kw, S, pred_param=pred_param)
    torch.manual_seed(181)
    table = torch.randn(4, S, kw["cross_attention_dim"]) * 2.0
    lens = [S, S - 4, 2, S - 1] if ragged else [S] * 4
    for row, ln in enumerate(lens):
        dc.encoder.set_prompt(row, table[row, :ln])
        oc.encoder.weight.data[row] = dc.encoder.weight.data[row]      # zero pad rows, lengths left at S: a foreign backbone takes no ragged table
    assert dc.encoder.varlen == ragged and not oc.encoder.varlen
    BS, T, hw = 2, 2, kw["sample_size"]
    x = torch.rand(BS, 4, hw, hw) * 2 - 1
    t, eps = torch.tensor([[0.9995, 0.0172], [0.5, 0.25]]), torch.randn(T, BS, 4, hw, hw)
    ref_l, ref_e = oc.classify(x, t=t, eps=eps, return_errors=True)
    dc = dc.to(DEV)
    got_l, got_e = dc.classify(x.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    rel = ((got_e - ref_e).abs() / ref_e).max().item()
    print(f"{name} f32 classify, scaled_linear, pred_param={pred_param}, lengths {lens[:3]}: per-cell eps-MSE max rel err {rel:.2e} (bound 1e-4); "
          f"labels {got_l.cpu().tolist()} / {ref_l.tolist()}")
    assert rel < 1e-4, rel
    assert got_l.cpu().tolist() == ref_l.tolist()
    # both runners were fed the same step labels: k = floor(t * 1000)
    steps = torch.tensor([[999.0, 17.0], [500.0, 250.0]])
    seen = oc.ema.ema_model.seen_labels
    assert len(seen) == T * 3 and all(torch.equal(s.cpu(), steps[i // 3]) for i, s in enumerate(seen)), seen
    (sp,) = list(dc._score_plans.values())
    lam = sp["layout"].view(sp["ctl"], "lam").cpu()
    assert sp["n_bj"] == T * BS and sorted(lam.tolist()) == sorted(steps.reshape(-1).tolist()), lam
    assert sp["plan"].varlen == ragged and sp["plan"].S == S
    dc.check_device_errors()


# ------------------------------------------------------------------------------------------------ component kernels at the new widths
GN_SHAPES = [(320, 0), (448, 0), (960, 0), (128, 192), (320, 128), (640, 320)]      # (C, C1): one source, and the up path's h | skip pairs


def _gn_case(dt, C, C1):
    """GroupNorm + SiLU over 8x8 pixels in 32 groups: 10, 14 and 30 channels per group, which no 16-byte chunk lines up with."""
    c = N._gn(f"sd_gn_{C}+{C1}_{N.DTN[dt]}", dt, "?", n=3, HW=64, C=C, C1=C1, groups=32, silu=1, use=("x1", "map1") if C1 else (), tag="sd widths")
    p = L.GroupnormParams(**N.gn_fields(c, N.fake_ptrs(c)))
    c["expect"] = L.lib().dc_groupnorm_variant(p).decode()        # whichever route the library picks must hold the bound
    return c


@pytest.mark.parametrize("C, C1", GN_SHAPES)
@pytest.mark.parametrize("dt", N.DTS, ids=[N.DTN[d] for d in N.DTS])
def test_groupnorm_at_stable_diffusion_widths(dt, C, C1):
    c = _gn_case(dt, C, C1)
    assert c["expect"] != "invalid"
    o = N.make_operands(c)
    refs = N.reference(c, o)
    _, bufs = TN.launch(c, TN.device_operands(c, o))
    problems, worst = N.check_outputs(c, bufs, refs)
    print(f"{c['name']} [{c['expect']}]: {(C + C1) // 32} channels per group, worst err / bound {worst:.4f}")
    assert not problems, (c["name"], problems)


CONV_SHAPES = [(320, 0, 320), (320, 128, 320), (640, 320, 640)]          # (C0, C1, Cout): 320 -> 320, 448 -> 320, 960 -> 640


@pytest.mark.parametrize("C0, C1, Cout", CONV_SHAPES)
@pytest.mark.parametrize("dt", G.DTS, ids=[G.DTN[d] for d in G.DTS])
def test_halo_conv_at_stable_diffusion_widths(dt, C0, C1, Cout):
    """3x3 convs of 8x8 images with bias, the time vector and quad statistics, as a ResNet's conv1 runs them: Cout = 320 is two and a half
    N tiles, K = 9 x 320 / 448 / 960 an odd number of 64-channel chunks per tap."""
    c = G._case(f"sd_halo8_{G.DTN[dt]}_{C0}+{C1}_{Cout}", dt, "halo8", 8, 8, 3, expect="conv3_halo<%s,8w>", C0=C0, C1=C1, Cout=Cout,
                use={"bias", "rowvec", "qstats"} | ({"map1"} if C1 else set()), n_vec=3)
    o = G.make_operands(c)
    ref, bound, det = G.reference(c, o, detail=True)
    ptrs, keep = TC.device_operands(c, o)
    out, qs = G.new_output(c, DEV), G.new_qstats(c, DEV)
    TC.launch(c, ptrs, out, qs)
    torch.cuda.synchronize()
    problems, worst = G.check_output(c, out.cpu(), ref, bound, qs.cpu(), det["e"])
    print(f"{c['name']} {c['expect']} = {c['instance']}: worst err / bound (with the quad records) {worst:.4f}")
    assert not problems, (c["name"], problems)
