"""CPU: the T5 encoder path without a GPU — the plain-torch restatement against the pinned transformers output, the host-built
relative-position table, T5Encoder's parameter names and local loading, every refusal, and the C-ABI of dc_attention_bias / dc_rmsnorm /
dc_embed_rows / dc_relu (struct order, argument validation and routing)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine_t5 as ET
from diffusion_classifier_amd.nets.t5 import T5Encoder
from t5_oracle import relative_bucket, t5_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(pred_param="eps", schedule="cosine", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, n_stages=1,
           evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32", image_size=32, noise_d=32)
REL_KEY = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "t5_tiny.npz"))
    cfg = json.loads(str(g["config"]))
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    return g, cfg, sd


def write_hf_directory(path, cfg, sd, extra=None):
    """A local Hugging Face directory: config.json + model.safetensors."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(dict(cfg, model_type="t5", architectures=["T5EncoderModel"]), fh)
    save_file({k: v.clone().contiguous() for k, v in dict(sd, **(extra or {})).items()}, os.path.join(path, "model.safetensors"))
    return str(path)


def test_restatement_reproduces_the_pinned_transformers_output():
    g, cfg, sd = golden()
    out = t5_encode(sd, cfg, torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"]))
    err = (out - torch.from_numpy(g["last_hidden_state"])).abs().max().item()
    print(f"restatement vs transformers, all rows: max abs {err:.2e} (bound 1e-5; values of mean magnitude {out.abs().mean():.2f})")
    assert err < 1e-5, err
    assert torch.equal(relative_bucket(torch.arange(-511, 512)), torch.from_numpy(g["bucket"]))


def test_host_bias_table_equals_transformers_bit_for_bit():
    g, cfg, sd = golden()
    nb, md = cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"]
    assert torch.equal(ET.relative_bucket(torch.arange(-511, 512), nb, md), torch.from_numpy(g["bucket"]))
    pb = torch.from_numpy(g["position_bias"])                      # [1, heads, query, key]
    Lq = pb.shape[-1]
    tb = ET.bias_table(sd[REL_KEY], Lq, nb, md)
    assert tuple(tb.shape) == (cfg["num_heads"], 2 * Lq - 1) and tb.dtype == torch.float32
    q, k = torch.arange(Lq)[:, None], torch.arange(Lq)[None, :]
    assert torch.equal(tb[:, k - q + Lq - 1], pb[0])
    # the longest table: every distance of L = 512 lands in the golden's bucket
    t512 = ET.bias_table(sd[REL_KEY], 512, nb, md)
    assert torch.equal(t512, sd[REL_KEY][torch.from_numpy(g["bucket"])].t())


def test_state_dict_keys_are_transformers_and_load_strictly():
    g, cfg, sd = golden()
    m = T5Encoder(**cfg)
    assert set(m.state_dict()) == set(sd) - {"encoder.embed_tokens.weight"}
    own = {k: v for k, v in sd.items() if k != "encoder.embed_tokens.weight"}
    m.load_state_dict(own, strict=True)
    assert all(torch.equal(v, own[k]) for k, v in m.state_dict().items())
    assert not any(p.requires_grad for p in m.parameters())
    assert m.compute_dtype == "f32" and m.set_compute_dtype("bf16").compute_dtype == "bf16"
    assert m.config.d_model == 64 and m.config.num_heads * m.config.d_kv == 128


def test_from_directory_round_trip_alias_and_decoder_keys(tmp_path):
    g, cfg, sd = golden()
    own = {k: v for k, v in sd.items() if k != "encoder.embed_tokens.weight"}
    m = T5Encoder.from_directory(write_hf_directory(tmp_path / "plain", cfg, sd))
    assert all(torch.equal(v, own[k]) for k, v in m.state_dict().items())
    # a full T5 checkpoint: decoder / lm_head keys are ignored
    extra = {"decoder.block.0.layer.0.SelfAttention.q.weight": torch.randn(128, 64), "lm_head.weight": torch.randn(48, 64),
             "decoder.final_layer_norm.weight": torch.ones(64)}
    m = T5Encoder.from_directory(write_hf_directory(tmp_path / "full", cfg, sd, extra))
    assert all(torch.equal(v, own[k]) for k, v in m.state_dict().items())
    # only the alias of the embedding
    alias = {k: v for k, v in sd.items() if k != "shared.weight"}
    m = T5Encoder.from_directory(write_hf_directory(tmp_path / "alias", cfg, alias))
    assert torch.equal(m.shared.weight, sd["shared.weight"])
    with pytest.raises(FileNotFoundError, match="config.json"):
        T5Encoder.from_directory(str(tmp_path / "nothing"))
    missing = {k: v for k, v in own.items() if not k.endswith("final_layer_norm.weight")}
    with pytest.raises(RuntimeError, match="final_layer_norm"):
        T5Encoder.from_directory(write_hf_directory(tmp_path / "short", cfg, missing))


def test_constructor_refusals_name_the_option():
    _, cfg, _ = golden()
    with pytest.raises(NotImplementedError, match="feed_forward_proj"):
        T5Encoder(**dict(cfg, feed_forward_proj="gated-gelu"))
    with pytest.raises(NotImplementedError, match="d_model"):
        T5Encoder(**dict(cfg, d_model=96))
    with pytest.raises(NotImplementedError, match="d_ff"):
        T5Encoder(**dict(cfg, d_ff=100))
    with pytest.raises(NotImplementedError, match="num_heads \\* d_kv"):
        T5Encoder(**dict(cfg, num_heads=3, d_kv=32))
    with pytest.raises(NotImplementedError, match="d_kv"):
        T5Encoder(**dict(cfg, num_heads=8, d_kv=24))
    T5Encoder(**dict(cfg, num_heads=4, d_kv=32))                      # inner = 128: served on the exact attention kernel


def test_forward_refusals_on_the_host():
    g, cfg, sd = golden()
    m = T5Encoder(**cfg)
    ids = torch.from_numpy(g["input_ids"])
    mask = torch.from_numpy(g["attention_mask"])
    holes = mask.clone(); holes[0, 3] = 0
    left = mask.flip(1)
    empty = mask.clone(); empty[2] = 0
    for bad in (holes, left, empty):
        with pytest.raises(L.DcamdError, match="right-padded"):
            m(ids, bad)
    with pytest.raises(L.DcamdError, match="attention_mask must be"):
        m(ids, mask[:, :5])
    with pytest.raises(ValueError, match=r"\[0, 48\)"):
        m(ids + 40, mask)
    with pytest.raises(ValueError, match=r"\[0, 48\)"):
        m(ids - 1, mask)
    with pytest.raises(ValueError, match="512"):
        m(torch.zeros(1, 513, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        m(ids.to(torch.int32), mask)
    with pytest.raises(L.DcamdError, match="no CPU fallback"):        # valid inputs on the CPU: there is no CPU path
        m(ids, mask)
    assert ET.lengths_of_mask(mask, ids.shape).tolist() == [20, 7, 1, 13]
    assert ET.lengths_of_mask(None, ids.shape).tolist() == [20] * 4


def test_classifier_construction_and_refusals(tmp_path):
    g, cfg, sd = golden()
    path = write_hf_directory(tmp_path / "t5", cfg, sd)
    unet = lambda **kw: dca.UNetCondition2D(**dict(dca.small_unet_kwargs(), **kw))
    conf = dict(CFG, encoder_type="t5", prompt_tokens=24, classes=3)
    # without a path: today's refusal, same text
    with pytest.raises(NotImplementedError, match="prompt") as e:
        dca.DiffusionClassifier(unet(), dca.Config(**conf))
    assert "fetches t5-base over the network" in str(e.value)
    dc = dca.DiffusionClassifier(unet(), dca.Config(**dict(conf, t5_path=path)))
    assert isinstance(dc.text_encoder, T5Encoder) and dc.tokenizer is None and dc.null_token == 3
    assert tuple(dc.encoder.weight.shape) == (4, 24, 64) and list(dc.encoder.state_dict()) == ["weight"]
    assert not any(k.startswith("text_encoder") for k in dc.encoder.state_dict())
    # the table is empty until set_class_prompts: classify / sample say which method to call
    with pytest.raises(RuntimeError, match="set_class_prompts"):
        dc.classify(torch.zeros(2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="set_class_prompts"):
        dc.sample(torch.zeros(1, 3, 32, 32), text=torch.tensor([0]))
    with pytest.raises(ValueError, match="input_ids must be"):
        dc.set_class_prompts(torch.zeros(3, 20, dtype=torch.int64))      # classes + 1 rows
    with pytest.raises(ValueError, match="input_ids must be"):
        dc.set_class_prompts(torch.zeros(4, 25, dtype=torch.int64))      # L <= S
    holes = torch.from_numpy(g["attention_mask"]).clone(); holes[1, 2] = 0
    with pytest.raises(L.DcamdError, match="right-padded"):
        dc.set_class_prompts(torch.from_numpy(g["input_ids"]), holes)
    # the checkpoint holds the table, not the T5 weights
    dc.save_checkpoint(str(tmp_path / "ckpt"))
    from safetensors.torch import load_file
    assert list(load_file(str(tmp_path / "ckpt" / "model_2.safetensors"))) == ["weight"]
    assert not any("text_encoder" in k for k in load_file(str(tmp_path / "ckpt" / "model.safetensors")))
    # hid mismatch / no projected context / another encoder type
    with pytest.raises(ValueError, match="encoder_hid_dim"):
        dca.DiffusionClassifier(unet(encoder_hid_dim=128), dca.Config(**dict(conf, t5_path=path)))
    with pytest.raises(NotImplementedError, match="encoder_hid_dim"):
        dca.DiffusionClassifier(dca.DiT(**dict(dca.chexpert_dit_b4_kwargs(), num_layers=1)), dca.Config(**dict(conf, t5_path=path)))
    with pytest.raises(AssertionError):
        dca.DiffusionClassifier(unet(), dca.Config(**dict(conf, t5_path=path, prompt_tokens=None)))
    other = dca.DiffusionClassifier(unet(), dca.Config(**dict(CFG, encoder_type="prompt", prompt_tokens=4, classes=3)))
    with pytest.raises(RuntimeError, match="t5"):
        other.set_class_prompts(torch.zeros(4, 4, dtype=torch.int64))


# ---- C-ABI ----------------------------------------------------------------------------------------
def test_structs_match_header_field_order_and_ops_are_declared():
    hdr = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    for name, val in (("DC_OP_ATTENTION_BIAS", L.OP_ATTENTION_BIAS), ("DC_OP_RMSNORM", L.OP_RMSNORM), ("DC_OP_EMBED_ROWS", L.OP_EMBED_ROWS),
                      ("DC_OP_RELU", L.OP_RELU)):
        assert f"{name} = {val}" in hdr
    assert (L.OP_ATTENTION_BIAS, L.OP_RMSNORM, L.OP_EMBED_ROWS, L.OP_RELU) == (11, 12, 13, 14)
    assert f"#define DC_ATTENTION_BIAS_MAX_L {L.ATTENTION_BIAS_MAX_L}" in hdr
    assert {"dc_attention_bias", "dc_attention_bias_variant", "dc_rmsnorm", "dc_embed_rows", "dc_relu"} <= set(L.EXPORTS)
    assert L.lib().dc_abi_version() == 5


PTR = 1 << 20


def _bias_params(**kw):
    base = dict(q=PTR, k=PTR, v=PTR, out=PTR, bias=PTR, kv_len=PTR, dtype=L.DC_BF16, n=3, L=77, heads=12, d=64, ld_qkv=2304, ld_out=768,
                scale=1.0)
    base.update(kw)
    return L.AttentionBiasParams(**base)


def test_attention_bias_validation_and_routes_need_no_gpu():
    lib = L.lib()
    variant = lambda **kw: lib.dc_attention_bias_variant(_bias_params(**kw)).decode()
    for dt in (L.DC_BF16, L.DC_F16):
        assert variant(dtype=dt) == "mfma"
        assert variant(dtype=dt, kv_len=None) == "mfma"
        assert variant(dtype=dt, ld_qkv=2308) == "fp32"               # ld_qkv % 8 != 0
        assert variant(dtype=dt, q=PTR + 2) == "fp32"                 # rows the 16-byte loads cannot take
        for d in (16, 32, 128):
            assert variant(dtype=dt, d=d, ld_qkv=36 * d, ld_out=12 * d) == "fp32"
    for d in (16, 32, 64, 128):
        assert variant(dtype=L.DC_F32, d=d, ld_qkv=36 * d, ld_out=12 * d) == "fp32"
    for bad, word, code in ((dict(q=None), b"null", -1), (dict(bias=None), b"null", -1), (dict(scale=0.0), b"scale", -1),
                            (dict(scale=-1.0), b"scale", -1), (dict(d=24), b"head dim 24", -2), (dict(L=0), b"L=0", -2),
                            (dict(L=513), b"L=513", -2), (dict(ld_qkv=64), b"ld", -2), (dict(dtype=7), b"dtype", -3),
                            (dict(bias=PTR + 2), b"aligned", -4)):
        assert variant(**bad) == "invalid", bad
        assert lib.dc_attention_bias(_bias_params(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    assert lib.dc_attention_bias(None, None) == -1 and lib.dc_attention_bias_variant(None) == b"invalid"
    # the plan runner knows the op: a refused launch is reported with its index and kind
    p = _bias_params(d=24)
    ops = (L.Op * 1)()
    ops[0].kind, ops[0].params = L.OP_ATTENTION_BIAS, C.cast(C.pointer(p), C.c_void_p)
    assert lib.dc_run_plan(ops, 1, None) == -2
    assert b"op 0 (kind 11)" in lib.dc_last_error() and b"head dim 24" in lib.dc_last_error()


def test_rmsnorm_embed_relu_validation_needs_no_gpu():
    lib = L.lib()
    rms = lambda **kw: L.RmsnormParams(**dict(dict(x=PTR, y=PTR, weight=PTR, dtype=L.DC_F32, out_dtype=L.DC_BF16, rows=40, C=64,
                                                   rows_per_sample=20, eps=1e-6), **kw))
    for bad, word, code in ((dict(x=None), b"null", -1), (dict(weight=None), b"null", -1), (dict(out_dtype=5), b"dtype", -3),
                            (dict(rows=0), b"rows=0", -2), (dict(rows_per_sample=3), b"rows_per_sample=3", -2), (dict(eps=-1.0), b"eps", -1),
                            (dict(y=PTR + 1), b"aligned", -4)):
        assert lib.dc_rmsnorm(rms(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    emb = lambda **kw: L.EmbedRowsParams(**dict(dict(table=PTR, ids=PTR, out=PTR, out_dtype=L.DC_F32, rows=8, C=64, vocab=48), **kw))
    for bad, word, code in ((dict(ids=None), b"null", -1), (dict(out_dtype=9), b"dtype", -3), (dict(vocab=0), b"vocab=0", -2),
                            (dict(ids=PTR + 4), b"aligned", -4)):
        assert lib.dc_embed_rows(emb(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    relu = lambda **kw: L.ReluParams(**dict(dict(x=PTR, n=1024, dtype=L.DC_BF16), **kw))
    for bad, word, code in ((dict(x=None), b"null", -1), (dict(dtype=3), b"dtype", -3), (dict(n=0), b"n=0", -2), (dict(x=PTR + 8), b"aligned", -4)):
        assert lib.dc_relu(relu(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    for kind, p, code in ((L.OP_RMSNORM, rms(rows=0), -2), (L.OP_EMBED_ROWS, emb(vocab=0), -2), (L.OP_RELU, relu(n=0), -2)):
        ops = (L.Op * 1)()
        ops[0].kind, ops[0].params = kind, C.cast(C.pointer(p), C.c_void_p)
        assert lib.dc_run_plan(ops, 1, None) == code
        assert f"op 0 (kind {kind})".encode() in lib.dc_last_error()
