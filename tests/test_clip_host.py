"""CPU: the CLIP text encoder path without a GPU — the plain-torch restatement against the pinned transformers outputs, the mask
independence of the valid rows, CLIPTextEncoder's parameter names and local loading, every refusal, and the C-ABI of dc_attention_causal /
dc_layernorm_rows / dc_embed_rows_pos / dc_act_pass (struct order, exports, argument validation and routing)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine_clip as EC
from diffusion_classifier_amd.nets.clip import CLIPTextEncoder
from clip_oracle import clip_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(pred_param="eps", schedule="cosine", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, n_stages=1,
           evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32", image_size=32, noise_d=32)
ACTS = ("quick_gelu", "gelu")
PUBLISHED = (["text_model.embeddings.token_embedding.weight", "text_model.embeddings.position_embedding.weight",
              "text_model.final_layer_norm.weight", "text_model.final_layer_norm.bias"] +
             [f"text_model.encoder.layers.{i}.{m}.{p}" for i in range(2) for p in ("weight", "bias")
              for m in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "layer_norm1", "layer_norm2",
                        "mlp.fc1", "mlp.fc2")])
_G = {}


def golden():
    if not _G:
        g = np.load(os.path.join(ROOT, "tests", "golden", "clip_tiny.npz"))
        _G.update(g=g, cfg=json.loads(str(g["config"])),
                  sd={k[3:]: torch.from_numpy(g[k]).float() for k in g.files if k.startswith("sd.")})
    return _G["g"], _G["cfg"], _G["sd"]


def write_hf_directory(path, cfg, sd, nest=False):
    """A local Hugging Face directory: config.json (text fields at top level, or under text_config as CLIPModel writes them) +
    model.safetensors."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(dict(model_type="clip", text_config=cfg, vision_config={"hidden_size": 32}) if nest else dict(cfg, model_type="clip_text_model"), fh)
    save_file({k: v.clone().contiguous() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))
    return str(path)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_restatement_reproduces_the_four_pinned_transformers_outputs():
    g, cfg, sd = golden()
    ids, mask, ids77 = (torch.from_numpy(g[k]) for k in ("input_ids", "attention_mask", "input_ids77"))
    assert mask.sum(1).tolist() == [40, 7, 1, 33] and tuple(ids77.shape) == (2, 77)
    for act in ACTS:
        r40 = rel_l2(clip_encode(sd, cfg, ids, mask, hidden_act=act), torch.from_numpy(g["last_hidden_state." + act]))
        r77 = rel_l2(clip_encode(sd, cfg, ids77, None, hidden_act=act), torch.from_numpy(g["last_hidden_state77." + act]))
        print(f"restatement vs transformers, {act}: rel-L2 {r40:.2e} (masked, all rows), {r77:.2e} (77 tokens) (bound 1e-5)")
        assert r40 < 1e-5 and r77 < 1e-5, (act, r40, r77)
    assert not np.array_equal(g["last_hidden_state.quick_gelu"], g["last_hidden_state.gelu"])


def test_valid_rows_do_not_depend_on_the_mask():
    g, cfg, sd = golden()
    ids, mask = torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"])
    a, b = clip_encode(sd, cfg, ids, mask), clip_encode(sd, cfg, ids, None)
    for i, n in enumerate(mask.sum(1).tolist()):
        assert torch.equal(a[i, :n].view(torch.int32), b[i, :n].view(torch.int32)), i


def test_state_dict_keys_are_the_published_names_and_load_strictly():
    g, cfg, sd = golden()
    m = CLIPTextEncoder(**cfg)
    assert set(m.state_dict()) == set(PUBLISHED) == set(sd)
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert not any(p.requires_grad for p in m.parameters())
    assert m.compute_dtype == "f32" and m.set_compute_dtype("bf16").compute_dtype == "bf16"
    assert m.config.hidden_act == "quick_gelu" and m.config.max_position_embeddings == 77


def test_from_directory_round_trips(tmp_path):
    g, cfg, sd = golden()
    same = lambda m: all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert same(CLIPTextEncoder.from_directory(write_hf_directory(tmp_path / "prefixed", cfg, sd)))
    bare = {k[len("text_model."):]: v for k, v in sd.items()}                 # transformers 5.x's CLIPTextModel.state_dict()
    assert same(CLIPTextEncoder.from_directory(write_hf_directory(tmp_path / "bare", cfg, bare)))
    m = CLIPTextEncoder.from_directory(write_hf_directory(tmp_path / "nested", dict(cfg, hidden_act="gelu"), sd, nest=True))
    assert same(m) and m.config.hidden_act == "gelu" and m.config.hidden_size == 128
    extra = {"vision_model.embeddings.class_embedding": torch.randn(32), "visual_projection.weight": torch.randn(16, 32),
             "text_projection.weight": torch.randn(16, 128), "logit_scale": torch.tensor(2.6),
             "text_model.embeddings.position_ids": torch.arange(77)[None], "vision_model.embeddings.position_ids": torch.arange(5)[None]}
    assert same(CLIPTextEncoder.from_directory(write_hf_directory(tmp_path / "both_towers", cfg, dict(sd, **extra), nest=True)))
    with pytest.raises(FileNotFoundError, match="config.json"):
        CLIPTextEncoder.from_directory(str(tmp_path / "nothing"))
    short = {k: v for k, v in sd.items() if k != "text_model.final_layer_norm.bias"}
    with pytest.raises(RuntimeError, match="final_layer_norm.bias"):
        CLIPTextEncoder.from_directory(write_hf_directory(tmp_path / "short", cfg, short))
    with pytest.raises(RuntimeError, match="stray"):                          # strict: an unknown text key is an error
        CLIPTextEncoder.from_directory(write_hf_directory(tmp_path / "stray", cfg, dict(sd, **{"text_model.stray.weight": torch.ones(1)})))
    with pytest.raises(ValueError, match="hidden_size"):
        CLIPTextEncoder.from_directory(write_hf_directory(tmp_path / "nocfg", {"vocab_size": 64}, sd))


def test_constructor_refusals_name_the_option():
    _, cfg, _ = golden()
    for bad, word in ((dict(hidden_size=96, num_attention_heads=3), "hidden_size"), (dict(intermediate_size=100), "intermediate_size"),
                      (dict(num_attention_heads=16), "num_attention_heads"),            # head width 8
                      (dict(hidden_size=192, num_attention_heads=4), "num_attention_heads"),       # head width 48
                      (dict(max_position_embeddings=513), "max_position_embeddings"), (dict(hidden_act="gelu_new"), "hidden_act")):
        with pytest.raises(NotImplementedError, match=word):
            CLIPTextEncoder(**dict(cfg, **bad))
    CLIPTextEncoder(**dict(cfg, num_attention_heads=4, hidden_act="gelu", max_position_embeddings=512))     # width 32: the exact kernel


def test_forward_refusals_on_the_host():
    g, cfg, sd = golden()
    m = CLIPTextEncoder(**cfg)
    ids, mask = torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"])
    holes = mask.clone(); holes[0, 3] = 0
    for bad in (holes, mask.flip(1)):
        with pytest.raises(L.DcamdError, match="right-padded"):
            m(ids, bad)
    with pytest.raises(ValueError, match=r"\[0, 64\)"):
        m(ids + 40, mask)
    with pytest.raises(ValueError, match="max_position_embeddings = 77"):
        m(torch.zeros(1, 78, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        m(ids.to(torch.int32), mask)
    with pytest.raises(L.DcamdError, match="no CPU fallback"):
        m(ids, mask)


def test_classifier_construction_and_refusals(tmp_path):
    g, cfg, sd = golden()
    path = write_hf_directory(tmp_path / "clip", cfg, sd)
    unet = lambda **kw: dca.UNetCondition2D(**dict(dca.small_unet_kwargs(), **kw))
    conf = dict(CFG, encoder_type="clip", prompt_tokens=48, classes=3)
    with pytest.raises(NotImplementedError, match="clip_path"):
        dca.DiffusionClassifier(unet(encoder_hid_dim=128), dca.Config(**conf))
    dc = dca.DiffusionClassifier(unet(encoder_hid_dim=128), dca.Config(**dict(conf, clip_path=path)))
    assert isinstance(dc.text_encoder, CLIPTextEncoder) and dc.tokenizer is None and dc.null_token == 3 and dc._table_mode()
    assert tuple(dc.encoder.weight.shape) == (4, 48, 128) and list(dc.encoder.state_dict()) == ["weight"]
    with pytest.raises(RuntimeError, match="set_class_prompts") as e:
        dc.classify(torch.zeros(2, 3, 32, 32))
    assert "encoder_type='clip'" in str(e.value)
    with pytest.raises(RuntimeError, match="set_class_prompts"):
        dc.sample(torch.zeros(1, 3, 32, 32), text=torch.tensor([0]))
    with pytest.raises(ValueError, match="input_ids must be"):
        dc.set_class_prompts(torch.zeros(3, 40, dtype=torch.int64))      # classes + 1 rows
    with pytest.raises(ValueError, match="input_ids must be"):
        dc.set_class_prompts(torch.zeros(4, 49, dtype=torch.int64))      # L <= S
    holes = torch.from_numpy(g["attention_mask"]).clone(); holes[1, 2] = 0
    with pytest.raises(L.DcamdError, match="right-padded"):
        dc.set_class_prompts(torch.from_numpy(g["input_ids"]), holes)
    dc.save_checkpoint(str(tmp_path / "ckpt"))                            # the checkpoint holds the table, not the CLIP weights
    from safetensors.torch import load_file
    assert list(load_file(str(tmp_path / "ckpt" / "model_2.safetensors"))) == ["weight"]
    with pytest.raises(ValueError, match="encoder_hid_dim"):
        dca.DiffusionClassifier(unet(), dca.Config(**dict(conf, clip_path=path)))          # the small UNet's own width is not 128
    with pytest.raises(NotImplementedError, match="encoder_hid_dim"):
        dca.DiffusionClassifier(dca.DiT(**dict(dca.chexpert_dit_b4_kwargs(), num_layers=1)), dca.Config(**dict(conf, clip_path=path)))
    with pytest.raises(AssertionError):
        dca.DiffusionClassifier(unet(encoder_hid_dim=128), dca.Config(**dict(conf, clip_path=path, prompt_tokens=None)))


# ---- C-ABI ----------------------------------------------------------------------------------------
NEW_SYMBOLS = ("dc_attention_causal", "dc_attention_causal_variant", "dc_layernorm_rows", "dc_embed_rows_pos", "dc_act_pass")


def test_structs_match_header_field_order_and_every_symbol_is_exported():
    assert C.sizeof(L.AttentionCausalParams) == 72 and C.sizeof(L.LayernormRowsParams) == 64
    assert C.sizeof(L.EmbedRowsPosParams) == 56 and C.sizeof(L.ActPassParams) == 24
    hdr = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    for name, val in (("DC_OP_ATTENTION_CAUSAL", L.OP_ATTENTION_CAUSAL), ("DC_OP_LAYERNORM_ROWS", L.OP_LAYERNORM_ROWS),
                      ("DC_OP_EMBED_ROWS_POS", L.OP_EMBED_ROWS_POS), ("DC_OP_ACT_PASS", L.OP_ACT_PASS),
                      ("DC_PASS_QUICK_GELU", L.PASS_QUICK_GELU), ("DC_PASS_GELU_ERF", L.PASS_GELU_ERF)):
        assert f"{name} = {val}" in hdr
    assert (L.OP_ATTENTION_CAUSAL, L.OP_LAYERNORM_ROWS, L.OP_EMBED_ROWS_POS, L.OP_ACT_PASS) == (15, 16, 17, 18)
    assert f"#define DC_ATTENTION_CAUSAL_MAX_L {L.ATTENTION_CAUSAL_MAX_L}" in hdr
    assert set(NEW_SYMBOLS) <= set(L.EXPORTS)
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None and re.search(r"\b" + name + r"\(", hdr), name
    assert lib.dc_abi_version() == 5


PTR = 1 << 20


def _causal_params(**kw):
    base = dict(q=PTR, k=PTR, v=PTR, out=PTR, row_len=PTR, dtype=L.DC_BF16, n=11, L=77, heads=12, d=64, ld_qkv=2304, ld_out=768,
                scale=0.125)
    base.update(kw)
    return L.AttentionCausalParams(**base)


def test_attention_causal_validation_and_routes_need_no_gpu():
    lib = L.lib()
    variant = lambda **kw: lib.dc_attention_causal_variant(_causal_params(**kw)).decode()
    for dt in (L.DC_BF16, L.DC_F16):
        assert variant(dtype=dt) == "mfma"
        assert variant(dtype=dt, row_len=None) == "mfma"
        assert variant(dtype=dt, L=1) == "mfma" and variant(dtype=dt, L=512) == "mfma"
        assert variant(dtype=dt, ld_qkv=2308) == "fp32"               # ld_qkv % 8 != 0
        assert variant(dtype=dt, q=PTR + 2) == "fp32"                 # rows the 16-byte loads cannot take
        assert variant(dtype=dt, k=PTR + 8) == "fp32" and variant(dtype=dt, v=PTR + 4) == "fp32"
        assert variant(dtype=dt, out=PTR + 4) == "fp32" and variant(dtype=dt, ld_out=770) == "fp32"     # 8-byte output rows
        for d in (16, 32, 128):
            assert variant(dtype=dt, d=d, ld_qkv=36 * d, ld_out=12 * d) == "fp32"
    for d in (16, 32, 64, 128):
        assert variant(dtype=L.DC_F32, d=d, ld_qkv=36 * d, ld_out=12 * d) == "fp32"
    for bad, word, code in ((dict(q=None), b"null", -1), (dict(out=None), b"null", -1), (dict(scale=0.0), b"scale", -1),
                            (dict(scale=-1.0), b"scale", -1), (dict(d=24), b"head dim 24", -2), (dict(d=256), b"head dim 256", -2),
                            (dict(L=0), b"L=0", -2), (dict(L=513), b"L=513", -2), (dict(ld_qkv=64), b"ld", -2), (dict(dtype=7), b"dtype", -3),
                            (dict(row_len=PTR + 2), b"aligned", -4), (dict(q=PTR + 1), b"aligned", -4)):
        assert variant(**bad) == "invalid", bad
        assert lib.dc_attention_causal(_causal_params(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    assert lib.dc_attention_causal(None, None) == -1 and lib.dc_attention_causal_variant(None) == b"invalid"
    p = _causal_params(d=24)
    ops = (L.Op * 1)()
    ops[0].kind, ops[0].params = L.OP_ATTENTION_CAUSAL, C.cast(C.pointer(p), C.c_void_p)
    assert lib.dc_run_plan(ops, 1, None) == -2
    assert b"op 0 (kind 15)" in lib.dc_last_error() and b"head dim 24" in lib.dc_last_error()


def test_layernorm_rows_embed_pos_act_pass_validation_needs_no_gpu():
    lib = L.lib()
    ln = lambda **kw: L.LayernormRowsParams(**dict(dict(x=PTR, y=PTR, gamma=PTR, beta=PTR, dtype=L.DC_F32, out_dtype=L.DC_BF16, rows=80,
                                                        C=128, rows_per_sample=40, eps=1e-5), **kw))
    for bad, word, code in ((dict(x=None), b"null", -1), (dict(gamma=None), b"null", -1), (dict(beta=None), b"null", -1),
                            (dict(out_dtype=5), b"dtype", -3), (dict(rows=0), b"rows=0", -2), (dict(rows_per_sample=3), b"rows_per_sample=3", -2),
                            (dict(eps=-1.0), b"eps", -1), (dict(y=PTR + 1), b"aligned", -4), (dict(beta=PTR + 2), b"aligned", -4)):
        assert lib.dc_layernorm_rows(ln(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    emb = lambda **kw: L.EmbedRowsPosParams(**dict(dict(table=PTR, pos=PTR, ids=PTR, out=PTR, out_dtype=L.DC_F32, rows=80, C=128, vocab=64,
                                                        L=40), **kw))
    for bad, word, code in ((dict(ids=None), b"null", -1), (dict(pos=None), b"null", -1), (dict(out_dtype=9), b"dtype", -3),
                            (dict(vocab=0), b"vocab=0", -2), (dict(L=0), b"L=0", -2), (dict(ids=PTR + 4), b"aligned", -4)):
        assert lib.dc_embed_rows_pos(emb(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    act = lambda **kw: L.ActPassParams(**dict(dict(x=PTR, n=1024, dtype=L.DC_BF16, kind=L.PASS_QUICK_GELU), **kw))
    for bad, word, code in ((dict(x=None), b"null", -1), (dict(dtype=3), b"dtype", -3), (dict(n=0), b"n=0", -2), (dict(x=PTR + 8), b"aligned", -4),
                            (dict(kind=0), b"kind 0", -1), (dict(kind=3), b"kind 3", -1)):
        assert lib.dc_act_pass(act(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    for kind, p, code in ((L.OP_LAYERNORM_ROWS, ln(rows=0), -2), (L.OP_EMBED_ROWS_POS, emb(vocab=0), -2), (L.OP_ACT_PASS, act(kind=7), -1)):
        ops = (L.Op * 1)()
        ops[0].kind, ops[0].params = kind, C.cast(C.pointer(p), C.c_void_p)
        assert lib.dc_run_plan(ops, 1, None) == code
        assert f"op 0 (kind {kind})".encode() in lib.dc_last_error()


def test_the_plans_gemm_forms_are_served_by_dc_igemm():
    """bias + fp32 residual + fp32 out (out_proj, fc2) and bias alone (q|k|v, fc1) at the golden's and at ViT-L/14's text shape: asked of
    dc_igemm_variant on the host, as ClipPlan asks it when it builds."""
    lib = L.lib()
    for dt in (L.DC_F32, L.DC_BF16, L.DC_F16):
        for rows, D, dff in ((4 * 40, 128, 256), (11 * 77, 768, 3072), (1, 128, 256)):
            for K, N, res in ((D, 3 * D, False), (D, D, True), (D, dff, False), (dff, D, True)):
                f = dict(dtype=dt, taps=1, stride=1, upsample=0, n_img=1, Hin=1, Win=rows, Hout=1, Wout=rows, src0=PTR, C0=K, ld0=K,
                         W=PTR, Cout=N, tile_n=128, bias=PTR, out=PTR, out_dtype=L.DC_F32 if res else dt, out_ld=N)
                if res:
                    f.update(residual=PTR, res_dtype=L.DC_F32, res_ld=N)
                v = lib.dc_igemm_variant(L.IgemmParams(**f)).decode()
                assert v != "invalid", (dt, rows, K, N, res, lib.dc_last_error())
    assert EC.ACTS == {"quick_gelu": L.PASS_QUICK_GELU, "gelu": L.PASS_GELU_ERF}
