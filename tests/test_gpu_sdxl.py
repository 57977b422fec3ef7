"""GPU: Stable Diffusion XL scoring end to end on tiny random-weight models — CLIPTextEncoderWithProjection (penultimate state and
pooled output) against the pinned transformers outputs, StableDiffusionXLUNet (transformer depth, the text_time side path) against the
test-side oracle (tests/sdxl_oracle.py), `classify` under encoder_type='clip_dual' against the same classifier over the oracle as a
foreign backbone, a directory tree through both loaders, and the launch lists of the existing classes' plans against the lists recorded
before this class existed.  Geometry: tests/sdxl_cases.py.
"""
import json

import pytest
import torch

import diffusion_classifier_amd as dca
import sd_plan_lists
import sdxl_cases as X
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd.nets.clip import CLIPTextEncoder, CLIPTextEncoderWithProjection
from sdxl_oracle import SDXLOracleUNet, clip_encode_ext

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STORE = {"bf16": torch.bfloat16, "f16": torch.float16}


# ------------------------------------------------------------------------------------------------ 1. CLIP
def _clip(case, act):
    g, cfg, sd = X.golden()
    eos = 2 if case == "argmax" else int(g["eos_first"])
    m = CLIPTextEncoderWithProjection(**dict(cfg, hidden_act=act, eos_token_id=eos))
    m.load_state_dict(sd, strict=True)
    return m.to(DEV), torch.from_numpy(g["input_ids." + case]), torch.from_numpy(g["attention_mask"]), eos


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("case", ["argmax", "first"])
def test_clip_f32_penultimate_and_pooled_against_transformers(case, act):
    g = X.golden()[0]
    m, ids, mask, _ = _clip(case, act)
    lens = mask.sum(1).tolist()
    for tag, am in (("", mask), (".nomask", None)):
        hs, emb = m(ids.to(DEV), None if am is None else am.to(DEV), layer=-2, pooled=True)
        hs, emb = hs.cpu(), emb.cpu()
        want_h, want_e = torch.from_numpy(g[f"hidden_states_m2.{case}.{act}{tag}"]), torch.from_numpy(g[f"text_embeds.{case}.{act}{tag}"])
        n_of = lens if am is not None else [ids.shape[1]] * len(lens)
        r_h = max(X.relerr(hs[b, :n], want_h[b, :n]) for b, n in enumerate(n_of))
        r_e = X.relerr(emb, want_e)
        print(f"{case} {act}{tag} f32: hidden_states[-2] rel-L2 {r_h:.2e} (worst prompt), text_embeds {r_e:.2e} (bound 1e-4)")
        assert r_h < 1e-4 and r_e < 1e-4, (r_h, r_e)
        assert all(float(hs[b, n:].abs().max()) == 0.0 for b, n in enumerate(n_of) if n < ids.shape[1])      # pad rows are zero
        assert hs.dtype == torch.float32 and emb.dtype == torch.float32 and tuple(emb.shape) == (3, 64)
    last, emb2 = m(ids.to(DEV), mask.to(DEV), pooled=True)                       # layer=-1 next to the pooled output
    want_l = torch.from_numpy(g[f"last_hidden_state.{case}.{act}"])
    assert max(X.relerr(last.cpu()[b, :n], want_l[b, :n]) for b, n in enumerate(lens)) < 1e-4 and torch.equal(emb2.cpu(), emb)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_clip_16_bit_against_the_storage_rounded_oracle(dt):
    g, cfg, sd = X.golden()
    for case in ("argmax", "first"):
        m, ids, mask, eos = _clip(case, "quick_gelu")
        m.set_compute_dtype(dt)
        hs, emb = (t.cpu() for t in m(ids.to(DEV), mask.to(DEV), layer=-2, pooled=True))
        want_h, want_e = clip_encode_ext(sd, cfg, ids, mask, layer=-2, pooled=True, store=STORE[dt], eos_token_id=eos)
        r_h = max(X.relerr(hs[b, :n], want_h[b, :n]) for b, n in enumerate(mask.sum(1).tolist()))
        r_e = X.relerr(emb, want_e)
        print(f"{case} {dt}: hidden_states[-2] rel-L2 {r_h:.2e}, text_embeds {r_e:.2e} against the storage-rounded oracle (bound 2e-2)")
        assert r_h < 2e-2 and r_e < 2e-2, (r_h, r_e)


def test_clip_default_call_gives_the_parent_class_bits():
    g, cfg, sd = X.golden()
    m, ids, mask, _ = _clip("argmax", "quick_gelu")
    parent = CLIPTextEncoder(**{k: v for k, v in cfg.items() if k not in ("projection_dim", "eos_token_id")})
    parent.load_state_dict({k: v for k, v in sd.items() if k != "text_projection.weight"}, strict=True)
    parent = parent.to(DEV)
    for dt in ("f32", "bf16"):
        m.set_compute_dtype(dt), parent.set_compute_dtype(dt)
        a, b = m(ids.to(DEV), mask.to(DEV)), parent(ids.to(DEV), mask.to(DEV))
        assert torch.equal(a, b) and torch.equal(m(ids.to(DEV), mask.to(DEV), layer=-1, pooled=False), b)
        # the parent read at layer=-2 (SDXL's first encoder) is the projected class's penultimate state
        assert torch.equal(parent.hidden_state(ids.to(DEV), mask.to(DEV), layer=-2), m(ids.to(DEV), mask.to(DEV), layer=-2))
    assert [mt["name"] for mt in list(parent._plans.values())[0].pb.meta][-1] == "final.ln"


# ------------------------------------------------------------------------------------------------ 2 / 3. UNet forward
_CASES = {}


def make_pair(kw, seed, **oracle_kw):
    torch.manual_seed(seed)
    m = X.randomise(dca.StableDiffusionXLUNet(**kw), seed + 1)
    o = SDXLOracleUNet(**kw, **oracle_kw)
    o.load_state_dict(m.state_dict(), strict=True)
    return m, o


def forward_case(name):
    """(model, inputs, fp32 oracle outputs), computed once per geometry and shared (left unchanged)."""
    if name not in _CASES:
        kw = dict(tiny=X.TINY, tiny3=X.TINY3)[name]
        m, o = make_pair(kw, 300 + len(name))
        g = torch.Generator().manual_seed(301)
        x, step = torch.randn(2, 4, 16, 16, generator=g) * 0.8, torch.tensor([999.0, 17.0])
        emb, lens = torch.randn(2, X.S, 128, generator=g), torch.tensor([X.S, X.S - 3], dtype=torch.int32)
        pooled, tids = torch.randn(2, 2, X.POOLED, generator=g), torch.tensor([[[16.0, 16, 0, 0, 16, 16]] * 2, [[24.0, 20, 2, 3, 16, 12], [512.0, 512, 0, 0, 1024, 1024]]])
        ref = {}
        with torch.no_grad():
            for key, (p, t, ln) in dict(base=(0, 0, None), ragged=(0, 0, lens), ids=(0, 1, None), pooled=(1, 0, None)).items():
                ref[key] = o(x, step, encoder_hidden_states=emb, encoder_lengths=ln, added_cond_kwargs=dict(text_embeds=pooled[p], time_ids=tids[t]))
        _CASES[name] = (m, o, kw, (x, step, emb, lens, pooled, tids), ref)
    return _CASES[name]


def _run(m, x, step, emb, pooled, tids, lens=None):
    return m(x.to(DEV), step.to(DEV), emb.to(DEV), dict(text_embeds=pooled.to(DEV), time_ids=tids.to(DEV)), encoder_lengths=lens).cpu()


@pytest.mark.parametrize("name", ["tiny", "tiny3"])
def test_forward_f32_against_the_oracle(name):
    m, _, kw, (x, step, emb, lens, pooled, tids), ref = forward_case(name)
    m = m.to(DEV).set_compute_dtype("f32")
    got = dict(base=_run(m, x, step, emb, pooled[0], tids[0]), ragged=_run(m, x, step, emb, pooled[0], tids[0], lens),
               ids=_run(m, x, step, emb, pooled[0], tids[1]), pooled=_run(m, x, step, emb, pooled[1], tids[0]))
    for key in got:
        r = X.relerr(got[key], ref[key])
        moved = X.relerr(ref[key], ref["base"])
        print(f"{name} f32 forward, {key}: rel-L2 {r:.2e} (bound 5e-5); the oracle moves by {moved:.2e} against the base case")
        assert r < 5e-5, (key, r)
        assert key == "base" or moved > 5e-5, (key, moved)          # the comparison can see the lengths, the size ids and the pooled row
    plan = list(m._plans.values())[-1]
    names = [mt["name"] for mt in plan.pb.meta]
    sites = sum(n.endswith(".proj_in") for n in names)
    depth = kw["transformer_layers_per_block"]
    assert sites == (4 if name == "tiny" else 11) and sum(n.endswith(".ff_proj_out") for n in names) == sites      # the fold: the last block only
    assert sum(n.endswith("transformer_blocks.0.ff_out") for n in names) == sites and not any(n.endswith("transformer_blocks.1.ff_out") for n in names)
    assert sum(n.endswith(".attn2") for n in names) == 2 * sites and depth in ((1, 2), 2)
    assert [mt["name"] for mt in plan.ctx_pb.meta] == ["add.sin", "add.l1", "add.l2", "ctx.to_kv"]
    # the time vector is per unit: everything behind conv_in runs in the unit domain
    assert not any(mt.get("variant") == "invalid" or mt["family"] == "invalid" for pb in (plan.pb, plan.ctx_pb) for mt in pb.meta)
    assert int(L.lib().dc_pn_timeouts()) == 0


def test_forward_bf16_within_twice_the_oracles_own_rounding():
    """r_o: relative L2 between the oracle with lowp=True (bf16 storage rounding) and the fp32 oracle, on the CPU.  The HIP output must lie
    within 2 r_o of the fp32 oracle, computed exactly as tests/test_gpu_sd_unet.py does.
    Measured on an MI355X (first run of this test): r = 9.529e-3 against r_o = 9.927e-3 (bound 1.985e-2)."""
    m, _, kw, (x, step, emb, _, pooled, tids), ref = forward_case("tiny")
    _, o16 = make_pair(kw, 300 + len("tiny"), lowp=True)
    with torch.no_grad():
        r_o = X.relerr(o16(x, step, encoder_hidden_states=emb, added_cond_kwargs=dict(text_embeds=pooled[0], time_ids=tids[0])), ref["base"])
    m = m.to(DEV).set_compute_dtype("bf16")
    got = _run(m, x, step, emb, pooled[0], tids[0])
    r = X.relerr(got, ref["base"])
    print(f"tiny bf16 forward: HIP against the fp32 oracle rel-L2 {r:.3e}; the bf16-rounded oracle against it r_o = {r_o:.3e} (bound 2 r_o = {2 * r_o:.3e})")
    assert torch.isfinite(got).all()
    assert r < 2 * r_o, (r, r_o)


def test_zeroed_add_embedding_at_depth_one_agrees_with_the_sd_unet():
    """add_embedding.linear_2 zeroed (weight and bias): aug = 0, and at depth 1 the network is a StableDiffusionUNet of the same weights.
    Not in bits: the XL plan runs every ResNet per unit, the SD plan shares the trunk in front of the first cross-attention."""
    kw = dict(X.TINY, transformer_layers_per_block=1)
    torch.manual_seed(330)
    xl = X.randomise(dca.StableDiffusionXLUNet(**kw), 331)
    with torch.no_grad():
        xl.add_embedding.linear_2.weight.zero_(), xl.add_embedding.linear_2.bias.zero_()
    sd = dca.StableDiffusionUNet(**{k: v for k, v in kw.items() if k not in ("transformer_layers_per_block", "addition_embed_type",
                                                                            "addition_time_embed_dim", "projection_class_embeddings_input_dim")})
    sd.load_state_dict({k: v for k, v in xl.state_dict().items() if not k.startswith("add_embedding.")}, strict=True)
    g = torch.Generator().manual_seed(332)
    x, step, emb = torch.randn(2, 4, 16, 16, generator=g), torch.tensor([640.0, 3.0]), torch.randn(2, X.S, 128, generator=g)
    pooled, tids = torch.randn(2, X.POOLED, generator=g), torch.tensor([[16.0, 16, 0, 0, 16, 16]] * 2)
    a = _run(xl.to(DEV), x, step, emb, pooled, tids)
    b = sd.to(DEV)(x.to(DEV), step.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    r = X.relerr(a, b)
    print(f"XL with a zeroed add_embedding.linear_2 at depth 1 against StableDiffusionUNet, f32: rel-L2 {r:.2e} (bound 5e-5)")
    assert r < 5e-5, r


def test_one_token_contexts_are_refused_under_the_xl_class():
    m = dca.StableDiffusionXLUNet(**X.TINY).to(DEV)
    with pytest.raises(L.DcamdError, match="prompt"):
        m(torch.zeros(1, 4, 16, 16, device=DEV), 1.0, torch.zeros(1, 1, 128, device=DEV),
          dict(text_embeds=torch.zeros(1, X.POOLED, device=DEV), time_ids=torch.zeros(1, 6, device=DEV)))


# ------------------------------------------------------------------------------------------------ 4. classify
def _fill(dc, table, pooled, lens, foreign):
    for row, n in enumerate(lens):
        dc.encoder.set_prompt(row, table[row, :n])
        dc.set_pooled(row, pooled[row])
    if foreign:      # its call has no mask: the oracle reads the zero rows set_prompt left as padding
        dc.encoder.set_lengths([X.S] * len(lens))


@pytest.mark.parametrize("pred_param, stages", [("eps", None), ("v", None), ("eps", ([1, 2], [2, 1]))])
def test_classify_f32_against_the_oracle_classifier(tmp_path, pred_param, stages):
    m, o = make_pair(X.TINY, 340 + len(pred_param), zero_rows_are_padding=True)
    root = X.write_tree(tmp_path / "tree", X.TINY, {})
    over = dict(pred_param=pred_param, add_time_ids=(24.0, 20.0, 2.0, 3.0, 16.0, 12.0))
    if stages:
        over.update(n_stages=2, evaluation_per_stage=stages[0], n_keep_per_stage=stages[1])
    dc, oc = X.classifier(m, root, **over), X.classifier(o, root, **over)
    g = torch.Generator().manual_seed(341)
    table, pooled = torch.randn(4, X.S, 128, generator=g) * 2.0, torch.randn(4, X.POOLED, generator=g)
    lens = [X.S, 3, X.S - 2, 5]
    _fill(dc, table, pooled, lens, False), _fill(oc, table, pooled, lens, True)
    assert dc.encoder.varlen and not oc.encoder.varlen
    BS, T = 2, 2
    x = torch.rand(BS, 4, 16, 16, generator=g) * 2 - 1
    t, eps = torch.tensor([[0.9995, 0.0172], [0.5, 0.25]]), torch.randn(T, BS, 4, 16, 16, generator=g)
    ref_l, ref_e = oc.classify(x, t=t, eps=eps, return_errors=True)
    dc = dc.to(DEV)
    got_l, got_e = dc.classify(x.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    assert torch.equal(torch.isfinite(got_e), torch.isfinite(ref_e))             # with pruning stages: the same survivors
    fin = torch.isfinite(ref_e)
    rel = ((got_e[fin] - ref_e[fin]).abs() / ref_e[fin]).max().item()
    print(f"clip_dual f32 classify, pred_param={pred_param}, stages={stages}: per-cell eps-MSE max rel err {rel:.2e} (bound 1e-4); "
          f"labels {got_l.cpu().tolist()} / {ref_l.tolist()}; scored cells {int(fin.sum())} of {fin.numel()}")
    assert rel < 1e-4, rel
    assert got_l.cpu().tolist() == ref_l.tolist()
    if stages:
        assert int(fin.sum()) == BS * (3 * 1 + 2 * 1)
    sp = list(dc._score_plans.values())[0]
    assert sp["plan"].varlen and sp["plan"].S == X.S
    dc.check_device_errors()


# ------------------------------------------------------------------------------------------------ 5. directory to classify
def test_a_directory_tree_classifies_in_the_bits_of_the_in_memory_model(tmp_path):
    torch.manual_seed(350)
    m = X.randomise(dca.StableDiffusionXLUNet(**X.TINY), 351)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())                                              # what an fp16 file can hold
    root = X.write_tree(tmp_path / "sdxl", X.TINY, m.state_dict(), fp16_names=True)
    loaded = dca.StableDiffusionXLUNet.from_directory(root + "/unet", variant="fp16")
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in loaded.state_dict().items())
    ids1, ids2, mask = X.prompt_ids([X.S, 3, 6, 5])
    g = torch.Generator().manual_seed(352)
    x = torch.rand(2, 4, 16, 16, generator=g) * 2 - 1
    t, eps = torch.rand(2, 2, generator=g), torch.randn(2, 2, 4, 16, 16, generator=g)
    out = []
    for bb in (m, loaded):
        dc = X.classifier(bb, root, clip2_variant="fp16", scheduler_path=root + "/scheduler").to(DEV)
        dc.set_class_prompts(ids1, mask, input_ids_2=ids2, attention_mask_2=mask)
        assert dc.encoder.lengths.tolist() == [X.S, 3, 6, 5] and float(dc.encoder.weight.detach()[1, 3:].abs().max()) == 0.0
        assert float(dc.pooled_table.abs().min()) > 0.0
        out.append(dc.classify(x.to(DEV), t=t, eps=eps.to(DEV), return_errors=True))
        dc.check_device_errors()
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][0], out[1][0]) and bool(torch.isfinite(out[0][1]).all())
    # the table holds the two penultimate states side by side, encoder 1 first, and the pooled row is encoder 2's text_embeds
    (cfg1, sd1), (cfg2, sd2) = X.clip_pair()
    h1 = clip_encode_ext(sd1, dict(cfg1, eos_token_id=2), ids1, mask, layer=-2)
    h2, emb = clip_encode_ext(sd2, cfg2, ids2, mask, layer=-2, pooled=True)
    for row, n in enumerate([X.S, 3, 6, 5]):
        assert X.relerr(dc.encoder.weight.detach()[row, :n].cpu(), torch.cat([h1[row, :n], h2[row, :n]], dim=-1)) < 1e-4
    assert X.relerr(dc.pooled_table.cpu(), emb) < 1e-4


# ------------------------------------------------------------------------------------------------ 6. the existing classes' plans
def test_stable_diffusion_unet_plans_launch_what_they_launched_before():
    """(UNetCondition2D's lists: tests/test_gpu_sd_unet.py::test_unet_condition_2d_plans_launch_what_they_launched_before.)"""
    with open(sd_plan_lists.FIXTURE) as f:
        want = json.load(f)
    got = sd_plan_lists.plan_lists(DEV)
    assert sorted(got) == sorted(want)
    for name in want:
        for part in ("ctx", "main"):
            assert got[name][part] == want[name][part], (name, part, [(a, b) for a, b in zip(got[name][part], want[name][part]) if a != b][:5])
