"""Host: what Stable Diffusion XL scoring adds, without a GPU — the extended CLIP oracle against the pinned transformers outputs
(hidden_states[-2] and text_embeds under both EOS rules), the loaders of CLIPTextEncoderWithProjection and StableDiffusionXLUNet, the
envelope's refusals, the published geometry's parameter count, the UNet oracle's depth-1 form against SDOracleUNet, and
encoder_type='clip_dual' driving the oracle as a foreign backbone against the written-out loop.

(The launch lists of the existing classes' plans are compared in tests/test_gpu_sdxl.py: building a plan packs weights on the device.)"""
import math

import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd.nets.clip import CLIPTextEncoder, CLIPTextEncoderWithProjection
from diffusion_classifier_amd.nets.sd_unet import StableDiffusionUNet, StableDiffusionXLUNet
import sdxl_cases as X
from sd_unet_oracle import SDOracleUNet
from sdxl_oracle import SDXLOracleUNet, clip_encode_ext, eos_positions

ACTS = ("quick_gelu", "gelu")


# ------------------------------------------------------------------------------------------------ 1. the CLIP oracle
@pytest.mark.parametrize("case", ["argmax", "first"])
def test_extended_clip_oracle_reproduces_the_pinned_transformers_outputs(case):
    g, cfg, sd = X.golden()
    ids, mask = torch.from_numpy(g["input_ids." + case]), torch.from_numpy(g["attention_mask"])
    eos = 2 if case == "argmax" else int(g["eos_first"])
    lens = mask.sum(1)
    pos = eos_positions(ids, eos)
    if case == "argmax":
        assert pos.tolist() == (lens - 1).tolist() and bool((ids.max(1).values == cfg["vocab_size"] - 1).all())
    else:       # held twice: the first occurrence is neither the last position nor where the largest id stands
        assert ((ids == eos).sum(1) == 2).all() and (pos < lens - 1).all() and (pos != ids.argmax(1)).any()
    for act in ACTS:
        for tag, m in (("", mask), (".nomask", None)):
            hs, emb = clip_encode_ext(sd, cfg, ids, m, layer=-2, pooled=True, hidden_act=act, eos_token_id=eos)
            r_h = X.relerr(hs, torch.from_numpy(g[f"hidden_states_m2.{case}.{act}{tag}"]))
            r_e = X.relerr(emb, torch.from_numpy(g[f"text_embeds.{case}.{act}{tag}"]))
            print(f"{case} {act}{tag}: hidden_states[-2] rel-L2 {r_h:.2e}, text_embeds {r_e:.2e} (bound 1e-5)")
            assert r_h < 1e-5 and r_e < 1e-5, (case, act, tag, r_h, r_e)
        last = clip_encode_ext(sd, cfg, ids, mask, hidden_act=act)
        assert X.relerr(last, torch.from_numpy(g[f"last_hidden_state.{case}.{act}"])) < 1e-5
        # the penultimate state is neither the last state nor the first layer's output
        assert X.relerr(clip_encode_ext(sd, cfg, ids, mask, layer=-2, hidden_act=act), last) > 0.1
        assert X.relerr(clip_encode_ext(sd, cfg, ids, mask, layer=-2, hidden_act=act), clip_encode_ext(sd, cfg, ids, mask, layer=-3, hidden_act=act)) > 0.01


# ------------------------------------------------------------------------------------------------ 2. loaders and envelopes
def test_clip_with_projection_keys_loading_and_variant(tmp_path):
    _, cfg, sd = X.golden()
    m = CLIPTextEncoderWithProjection(**cfg)
    assert set(m.state_dict()) == set(sd) and tuple(m.text_projection.weight.shape) == (cfg["projection_dim"], cfg["hidden_size"])
    assert "text_projection.bias" not in m.state_dict() and m.config.eos_token_id == 2 and not any(p.requires_grad for p in m.parameters())
    same = lambda mod: all(torch.equal(v, sd[k]) for k, v in mod.state_dict().items())
    assert same(CLIPTextEncoderWithProjection.from_directory(X.write_clip(tmp_path / "ok", cfg, sd)))
    bare = {(k if k.startswith("text_projection.") else k[len("text_model."):]): v for k, v in sd.items()}
    assert same(CLIPTextEncoderWithProjection.from_directory(X.write_clip(tmp_path / "bare", cfg, bare)))
    extra = {"vision_model.embeddings.class_embedding": torch.randn(8), "visual_projection.weight": torch.randn(4, 8), "logit_scale": torch.tensor(2.6),
             "text_model.embeddings.position_ids": torch.arange(16)[None]}
    assert same(CLIPTextEncoderWithProjection.from_directory(X.write_clip(tmp_path / "towers", cfg, dict(sd, **extra))))
    fp16 = X.write_clip(tmp_path / "fp16", cfg, {k: v.half() for k, v in sd.items()}, "model.fp16.safetensors")
    assert same(CLIPTextEncoderWithProjection.from_directory(fp16, variant="fp16"))          # the golden's weights are fp16-representable
    with pytest.raises(FileNotFoundError, match=r"model\.safetensors"):
        CLIPTextEncoderWithProjection.from_directory(fp16)
    with pytest.raises(RuntimeError, match=r"text_projection\.weight"):
        CLIPTextEncoderWithProjection.from_directory(X.write_clip(tmp_path / "lost", cfg, {k: v for k, v in sd.items() if k != "text_projection.weight"}))
    with pytest.raises(RuntimeError, match=r"text_projection\.bias"):
        CLIPTextEncoderWithProjection.from_directory(X.write_clip(tmp_path / "stray", cfg, dict(sd, **{"text_projection.bias": torch.zeros(64)})))
    # the parent class is as it was: the projection is ignored, its keys and config do not know it
    p = CLIPTextEncoder.from_directory(X.write_clip(tmp_path / "parent", {k: v for k, v in cfg.items() if k not in ("projection_dim", "eos_token_id")}, sd))
    assert "text_projection.weight" not in p.state_dict() and CLIPTextEncoder.IGNORED == ("vision_model.", "visual_projection.", "text_projection.", "logit_scale")
    assert not hasattr(p.config, "projection_dim")


def test_eos_positions_follow_both_rules_and_refuse_by_row():
    g, cfg, _ = X.golden()
    mask = torch.from_numpy(g["attention_mask"])
    lens = mask.sum(1)
    legacy = CLIPTextEncoderWithProjection(**cfg)
    ids = torch.from_numpy(g["input_ids.argmax"])
    assert legacy._eos_positions(ids, lens).tolist() == ids.argmax(1).tolist()
    first = CLIPTextEncoderWithProjection(**dict(cfg, eos_token_id=int(g["eos_first"])))
    ids_f = torch.from_numpy(g["input_ids.first"])
    assert first._eos_positions(ids_f, lens).tolist() == eos_positions(ids_f, int(g["eos_first"])).tolist()
    bad = ids_f.clone()
    bad[1][bad[1] == int(g["eos_first"])] = 50
    with pytest.raises(ValueError, match="row 1"):
        first._eos_positions(bad, lens)
    with pytest.raises(ValueError, match="row 2"):                  # the EOS of row 2 lies in its padding
        legacy._eos_positions(ids, torch.tensor([16, 7, 1]))
    with pytest.raises(ValueError, match="layer"):
        legacy(ids, layer=-3)


def test_stable_diffusion_unet_still_refuses_what_sdxl_needs():
    base = {k: v for k, v in X.TINY.items() if k not in ("transformer_layers_per_block", "addition_embed_type", "addition_time_embed_dim",
                                                        "projection_class_embeddings_input_dim")}
    StableDiffusionUNet(**base)
    for bad, word in ((dict(addition_embed_type="text_time"), "addition_embed_type"), (dict(transformer_layers_per_block=2), "transformer_layers_per_block"),
                      (dict(transformer_layers_per_block=(1, 2)), "transformer_layers_per_block")):
        with pytest.raises(NotImplementedError, match=word) as e:
            StableDiffusionUNet(**dict(base, **bad))
        assert "Stable Diffusion 1.x / 2.x" in str(e.value)


@pytest.mark.parametrize("bad, word", [
    (dict(addition_embed_type="text"), "addition_embed_type"), (dict(addition_embed_type="text_image"), "addition_embed_type"),
    (dict(addition_embed_type=None), "addition_embed_type"), (dict(class_embed_type="timestep"), "class_embed_type"),
    (dict(class_embed_type="projection"), "class_embed_type"), (dict(reverse_transformer_layers_per_block=(2, 1)), "reverse_transformer_layers_per_block"),
    (dict(transformer_layers_per_block=(1, 2, 3)), "transformer_layers_per_block"), (dict(transformer_layers_per_block=0), "transformer_layers_per_block"),
    (dict(transformer_layers_per_block=((1, 2), (1, 2))), "transformer_layers_per_block"),
    (dict(addition_time_embed_dim=None), "addition_time_embed_dim"), (dict(addition_time_embed_dim=33), "addition_time_embed_dim"),
    (dict(projection_class_embeddings_input_dim=None), "projection_class_embeddings_input_dim"),
    (dict(projection_class_embeddings_input_dim=192), "projection_class_embeddings_input_dim"),
    (dict(dual_cross_attention=True), "dual_cross_attention"), (dict(only_cross_attention=True), "only_cross_attention"),
    (dict(time_cond_proj_dim=256), "time_cond_proj_dim"), (dict(attention_type="gated"), "attention_type"),
    (dict(encoder_hid_dim_type="text_proj", encoder_hid_dim=64), "encoder_hid_dim_type"), (dict(num_attention_heads=8), "num_attention_heads"),
    (dict(num_class_embeds=10), "num_class_embeds"), (dict(attention_head_dim=(2, 3)), "attention_head_dim"),
])
def test_the_xl_class_refuses_by_name(bad, word):
    with pytest.raises(NotImplementedError, match=word):
        StableDiffusionXLUNet(**dict(X.TINY, **bad))


def test_xl_unet_keys_loading_variant_and_refused_calls(tmp_path):
    torch.manual_seed(2)
    src = StableDiffusionXLUNet(**X.TINY)
    sd = src.state_dict()
    assert isinstance(src, StableDiffusionUNet) and dca.StableDiffusionXLUNet is StableDiffusionXLUNet
    assert src.config.transformer_layers_per_block == (1, 2) and src.config.addition_embed_type == "text_time"
    for k in ("add_embedding.linear_1.weight", "add_embedding.linear_1.bias", "add_embedding.linear_2.weight", "add_embedding.linear_2.bias",
              "down_blocks.1.attentions.0.transformer_blocks.1.attn2.to_k.weight", "mid_block.attentions.0.transformer_blocks.1.ff.net.2.bias",
              "up_blocks.0.attentions.1.transformer_blocks.1.norm3.weight"):
        assert k in sd, k
    assert tuple(sd["add_embedding.linear_1.weight"].shape) == (256, 256) and tuple(sd["add_embedding.linear_2.weight"].shape) == (256, 256)
    assert not any(".transformer_blocks.2." in k for k in sd) and tuple(sd["mid_block.attentions.0.proj_in.weight"].shape) == (128, 128)
    deep = StableDiffusionXLUNet(**X.TINY3)            # the int form: two blocks at every site; up blocks read the heads reversed
    assert deep.config.transformer_layers_per_block == (2, 2, 2)
    assert sum(k.endswith(".transformer_blocks.1.norm1.weight") for k in deep.state_dict()) == sum(k.endswith(".proj_in.weight") for k in deep.state_dict()) == 11
    m = StableDiffusionXLUNet.from_directory(X.write_unet(tmp_path / "ok", X.TINY, sd, upcast_attention=None, act_fn="silu"))
    assert list(m.state_dict()) == list(sd) and all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert all(not p.requires_grad for p in m.parameters())
    fp16 = X.write_unet(tmp_path / "fp16", X.TINY, {k: v.half() for k, v in sd.items()}, "diffusion_pytorch_model.fp16.safetensors")
    v = StableDiffusionXLUNet.from_directory(fp16, variant="fp16", sample_size=32)
    assert v.config.sample_size == 32 and all(torch.equal(p, sd[k].half().float()) for k, p in v.state_dict().items())
    with pytest.raises(FileNotFoundError, match=r"diffusion_pytorch_model\.safetensors"):
        StableDiffusionXLUNet.from_directory(fp16)
    lost = "add_embedding.linear_2.bias"
    with pytest.raises(RuntimeError, match=lost.replace(".", r"\.")):
        StableDiffusionXLUNet.from_directory(X.write_unet(tmp_path / "lost", X.TINY, {k: t for k, t in sd.items() if k != lost}))
    lost = "mid_block.attentions.0.transformer_blocks.1.attn1.to_q.weight"
    with pytest.raises(RuntimeError, match=lost.replace(".", r"\.")):
        StableDiffusionXLUNet.from_directory(X.write_unet(tmp_path / "lost2", X.TINY, {k: t for k, t in sd.items() if k != lost}))
    with pytest.raises(RuntimeError, match=r"transformer_blocks\.2"):
        extra = {"mid_block.attentions.0.transformer_blocks.2.norm1.weight": torch.zeros(128)}
        StableDiffusionXLUNet.from_directory(X.write_unet(tmp_path / "stray", X.TINY, dict(sd, **extra)))
    with pytest.raises(NotImplementedError, match="addition_embed_type"):     # the SD 1.x / 2.x class does not take this directory
        StableDiffusionUNet.from_directory(str(tmp_path / "ok"))
    x, ctx = torch.zeros(1, 4, 16, 16), torch.zeros(1, X.S, 128)
    for name, call in (("forward_pair", lambda: src.forward_pair(x, 1.0, ctx, ctx)), ("pair_session", lambda: src.pair_session(1, "cpu", ctx, ctx))):
        with pytest.raises(NotImplementedError, match="StableDiffusionXLUNet"):
            call()
    for kwargs in ({}, {"text_embeds": torch.zeros(1, 64)}, {"time_ids": torch.zeros(1, 6)}):
        with pytest.raises(ValueError, match="text_embeds|time_ids"):
            src(x, 1.0, ctx, kwargs)


def _resnet(cin, cout, temb):
    return 2 * cin + (9 * cin * cout + cout) + (temb * cout + cout) + 2 * cout + (9 * cout * cout + cout) + ((cin * cout + cout) if cin != cout else 0)


def _site(C, depth, xdim):
    attn1 = 3 * C * C + (C * C + C)                                         # q, k, v without bias; to_out with one
    attn2 = C * C + 2 * C * xdim + (C * C + C)
    ff = (C * 8 * C + 8 * C) + (4 * C * C + C)                              # GEGLU projection, ff.net.2
    return 2 * C + 2 * (C * C + C) + depth * (6 * C + attn1 + attn2 + ff)   # norm, proj_in / proj_out, the blocks (three LayerNorms each)


def test_published_sdxl_base_geometry_on_the_meta_device():
    kw = dca.sdxl_unet_kwargs()
    with torch.device("meta"):
        m = StableDiffusionXLUNet(**kw)
    s = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert s["add_embedding.linear_1.weight"] == (1280, 2816) and s["time_embedding.linear_1.weight"] == (1280, 320)
    assert s["down_blocks.2.attentions.1.transformer_blocks.9.attn2.to_k.weight"] == (1280, 2048)
    assert s["down_blocks.1.attentions.0.transformer_blocks.1.attn2.to_v.weight"] == (640, 2048) and s["down_blocks.1.attentions.0.proj_in.weight"] == (640, 640)
    assert not any(k.startswith(("down_blocks.0.attentions", "up_blocks.2.attentions")) for k in s)
    blocks = {}
    for k in s:
        if k.endswith(".norm1.weight") and ".transformer_blocks." in k:
            blocks[s[k][0]] = blocks.get(s[k][0], 0) + 1
    assert blocks == {640: 10, 1280: 60}                                     # 70 blocks; K | V of 2 * (10 * 640 + 60 * 1280) = 166,400 per token
    from diffusion_classifier_amd import engine as E
    assert {v[0] // E.site_heads(m.config, k[: -len(".proj_in.weight")]) for k, v in s.items() if k.endswith(".proj_in.weight")} == {64}
    T, X_ = 1280, 2048
    count = (320 * 4 * 9 + 320) + (320 * T + T) + (T * T + T) + (2816 * T + T) + (T * T + T)                   # conv_in, time_embedding, add_embedding
    count += 2 * _resnet(320, 320, T) + (9 * 320 * 320 + 320)                                                    # down 0 and its downsampler
    count += _resnet(320, 640, T) + _resnet(640, 640, T) + 2 * _site(640, 2, X_) + (9 * 640 * 640 + 640)        # down 1
    count += _resnet(640, 1280, T) + _resnet(1280, 1280, T) + 2 * _site(1280, 10, X_)                           # down 2
    count += 2 * _resnet(1280, 1280, T) + _site(1280, 10, X_)                                                    # mid
    count += 2 * _resnet(2560, 1280, T) + _resnet(1920, 1280, T) + 3 * _site(1280, 10, X_) + (9 * 1280 * 1280 + 1280)      # up 0
    count += _resnet(1920, 640, T) + _resnet(1280, 640, T) + _resnet(960, 640, T) + 3 * _site(640, 2, X_) + (9 * 640 * 640 + 640)    # up 1
    count += _resnet(960, 320, T) + 2 * _resnet(640, 320, T)                                                     # up 2
    count += 2 * 320 + (4 * 320 * 9 + 4)                                                                         # conv_norm_out, conv_out
    assert sum(math.prod(v) for v in s.values()) == count == 2567463684      # the published parameter count of the SDXL-base UNet


# ------------------------------------------------------------------------------------------------ 3. the UNet oracle at depth 1
@pytest.mark.parametrize("lowp", [False, True])
def test_xl_oracle_at_depth_one_without_text_time_is_the_sd_oracle(lowp):
    kw = {k: v for k, v in X.TINY.items() if k not in ("transformer_layers_per_block", "addition_embed_type", "addition_time_embed_dim",
                                                      "projection_class_embeddings_input_dim")}
    torch.manual_seed(11)
    a = X.randomise(SDOracleUNet(**kw, lowp=lowp), 12)
    b = SDXLOracleUNet(**kw, lowp=lowp)
    b.load_state_dict(a.state_dict(), strict=True)
    x, step, ctx = torch.randn(2, 4, 16, 16), torch.tensor([700.0, 12.0]), torch.randn(2, X.S, 128)
    with torch.no_grad():
        for lens in (None, torch.tensor([X.S, 3])):
            assert torch.equal(a(x, step, encoder_hidden_states=ctx, encoder_lengths=lens), b(x, step, encoder_hidden_states=ctx, encoder_lengths=lens))


# ------------------------------------------------------------------------------------------------ 4. clip_dual over a foreign backbone
def _oracle(kw, seed, **over):
    torch.manual_seed(seed)
    return X.randomise(SDXLOracleUNet(**kw, **over), seed + 1)


@pytest.mark.parametrize("time_ids", [None, (24.0, 20.0, 2.0, 3.0, 16.0, 12.0)])
def test_clip_dual_classify_on_a_foreign_backbone_is_the_written_out_loop(tmp_path, time_ids):
    o = _oracle(X.TINY, 21, zero_rows_are_padding=True)
    root = X.write_tree(tmp_path / "tree", X.TINY, {})
    dc = X.classifier(o, root, add_time_ids=time_ids)
    assert tuple(dc.encoder.weight.shape) == (X.CLASSES + 1, X.S, 128) and tuple(dc.pooled_table.shape) == (X.CLASSES + 1, X.POOLED)
    assert "pooled_table" in dc.state_dict()
    want_ids = (16.0, 16.0, 0.0, 0.0, 16.0, 16.0) if time_ids is None else time_ids
    assert tuple(dc.add_time_ids.shape) == (6,) and dc.add_time_ids.tolist() == list(want_ids)
    g = torch.Generator().manual_seed(22)
    table, pooled = torch.randn(X.CLASSES + 1, X.S, 128, generator=g) * 2.0, torch.randn(X.CLASSES + 1, X.POOLED, generator=g)
    lens = [X.S, 3, X.S - 2, 5]
    with pytest.raises(RuntimeError, match="set_class_prompts"):
        dc.classify(torch.zeros(2, 4, 16, 16))
    for row, n in enumerate(lens):
        dc.encoder.set_prompt(row, table[row, :n])
        dc.set_pooled(row, pooled[row])
    assert dc.encoder.varlen
    dc.encoder.set_lengths([X.S] * (X.CLASSES + 1))      # a foreign backbone's call has no mask: the oracle reads the zero rows set_prompt left as padding
    BS, T = 2, 2
    x = torch.rand(BS, 4, 16, 16, generator=g) * 2 - 1
    t, eps = torch.tensor([[0.9995, 0.0172], [0.5, 0.25]]), torch.randn(T, BS, 4, 16, 16, generator=g)
    labels, errors = dc.classify(x, t=t, eps=eps, return_errors=True)
    # the written-out loop over (trial, class)
    want = torch.empty(BS, X.CLASSES, T)
    tid = torch.tensor(want_ids).expand(BS, 6)
    with torch.no_grad():
        for j in range(T):
            lam = dc.schedule(t[j])
            al, sg = torch.sqrt(torch.sigmoid(lam)).view(-1, 1, 1, 1), torch.sqrt(torch.sigmoid(-lam)).view(-1, 1, 1, 1)
            z = al * x + sg * eps[j]
            for c in range(X.CLASSES):
                ctx = torch.zeros(BS, X.S, 128)
                ctx[:, :lens[c]] = table[c, :lens[c]]
                pred = o(x=z, noise_labels=dc.noise_labels(t[j]), encoder_hidden_states=ctx, encoder_lengths=torch.tensor([lens[c]] * BS),
                         added_cond_kwargs={"text_embeds": pooled[c].expand(BS, -1), "time_ids": tid})
                want[:, c, j] = torch.norm((pred - eps[j]).view(BS, -1), dim=1, p=2) ** 2
    assert torch.equal(errors, want), (errors - want).abs().max()
    assert labels.tolist() == want.mean(2).argmin(1).tolist()
    # the conditioning reaches the scores: another pooled row or other size ids give other errors
    dc.set_pooled(0, pooled[0] + 1.0)
    moved = dc.classify(x, t=t, eps=eps, return_errors=True)[1]
    assert not torch.equal(moved[:, 0], errors[:, 0]) and torch.equal(moved[:, 1:], errors[:, 1:])


# ------------------------------------------------------------------------------------------------ 5. construction refusals
def test_clip_dual_construction_and_prompt_refusals(tmp_path):
    o = _oracle(X.TINY, 31)
    root = X.write_tree(tmp_path / "tree", X.TINY, {})
    with pytest.raises(NotImplementedError, match="clip2_path"):
        X.classifier(o, root, clip2_path=None)
    with pytest.raises(NotImplementedError, match="clip_path"):
        X.classifier(o, root, clip_path=None)
    with pytest.raises(ValueError, match=r"64 \+ 64.*192"):
        X.classifier(_oracle(dict(X.TINY, cross_attention_dim=192), 32), root)
    with pytest.raises(ValueError, match=r"64 \+ 6 \* 16.*256"):
        X.classifier(_oracle(dict(X.TINY, addition_time_embed_dim=16), 33), root)
    with pytest.raises(ValueError, match="add_time_ids"):
        X.classifier(o, root, add_time_ids=(1.0, 2.0, 3.0))
    dc = X.classifier(o, root)
    ids1, ids2, mask = X.prompt_ids([X.S, 3, 6, 5])
    with pytest.raises(ValueError, match="input_ids_2"):
        dc.set_class_prompts(ids1, mask)
    short = mask.clone()
    short[2, 5] = 0
    with pytest.raises(ValueError, match="row 2"):
        dc.set_class_prompts(ids1, mask, input_ids_2=ids2, attention_mask_2=short)
    with pytest.raises(ValueError, match="row 1"):
        dc.set_pooled(1, torch.zeros(63))
    x = torch.zeros(2, 4, 16, 16)
    for call in (lambda: dc.sample(x, torch.tensor([0, 1])), lambda: dc.counterfactual(x), lambda: dc.invert(x), lambda: dc.invert_ddpm(x)):
        with pytest.raises(NotImplementedError, match="SDXL"):
            call()
    # every other encoder type keeps its state dict: no pooled table
    import draws_fixture
    assert "pooled_table" not in draws_fixture.classifier("scaled_linear").state_dict()
    with pytest.raises(RuntimeError, match="clip_dual"):
        draws_fixture.classifier("scaled_linear").set_pooled(0, torch.zeros(4))
