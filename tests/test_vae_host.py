"""CPU: the AutoencoderKL encoder path without a GPU — VAEEncoder's parameter names and local loading (legacy attention names, ignored
decoder, strict on strays, missing files), every refusal, the conv_out . quant_conv fold, the C-ABI of dc_attention_wide / dc_im2col_s2
(struct order, exports, argument validation, routing) and DiffusionClassifier's config.vae_path refusals."""
import ctypes as C
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine_vae as EV
from diffusion_classifier_amd.nets.vae import VAEEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(pred_param="eps", schedule="cosine", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, n_stages=1,
           evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32", image_size=16, noise_d=16,
           encoder_type="nn", classes=3)
TINY = dict(in_channels=3, latent_channels=4, block_out_channels=(64, 128), layers_per_block=1, norm_num_groups=32, scaling_factor=0.5)
PTR = 1 << 20


def published_keys(boc, layers, quant=True):
    """The encoder-side keys of a diffusers 0.31 AutoencoderKL state dict."""
    wb = lambda k: [k + ".weight", k + ".bias"]
    keys = wb("encoder.conv_in")

    def resnet(k, cin, cout):
        out = wb(k + ".norm1") + wb(k + ".conv1") + wb(k + ".norm2") + wb(k + ".conv2")
        return out + (wb(k + ".conv_shortcut") if cin != cout else [])
    c = boc[0]
    for i, co in enumerate(boc):
        for j in range(layers):
            keys += resnet(f"encoder.down_blocks.{i}.resnets.{j}", c, co)
            c = co
        if i != len(boc) - 1:
            keys += wb(f"encoder.down_blocks.{i}.downsamplers.0.conv")
    for j in range(2):
        keys += resnet(f"encoder.mid_block.resnets.{j}", c, c)
    for n in ("group_norm", "to_q", "to_k", "to_v", "to_out.0"):
        keys += wb("encoder.mid_block.attentions.0." + n)
    keys += wb("encoder.conv_norm_out") + wb("encoder.conv_out")
    return keys + (wb("quant_conv") if quant else [])


def write_directory(path, cfg, sd, extra_cfg=None):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(dict(dict(cfg, block_out_channels=list(cfg["block_out_channels"])), _class_name="AutoencoderKL", sample_size=256,
                       out_channels=3, up_block_types=["UpDecoderBlock2D"] * len(cfg["block_out_channels"]), **(extra_cfg or {})), fh)
    save_file({k: v.clone().contiguous() for k, v in sd.items()}, os.path.join(path, VAEEncoder.WEIGHTS))
    return str(path)


def test_state_dict_keys_are_the_published_names():
    for kw in (TINY, dca.sd_vae_kwargs(), dict(TINY, use_quant_conv=False, block_out_channels=(64, 64, 256), layers_per_block=2)):
        m = VAEEncoder(**kw)
        want = published_keys(tuple(kw["block_out_channels"]), kw["layers_per_block"], kw.get("use_quant_conv", True))
        assert sorted(m.state_dict().keys()) == sorted(want), set(m.state_dict()) ^ set(want)
        assert not any(p.requires_grad for p in m.parameters())
    sd = dca.sd_vae_kwargs()
    assert sd["block_out_channels"] == (128, 256, 512, 512) and sd["layers_per_block"] == 2 and sd["latent_channels"] == 4
    assert sd["scaling_factor"] == 0.18215 and VAEEncoder(**sd).downscale == 8
    m = VAEEncoder(**sd)
    assert tuple(m.encoder.down_blocks[0].downsamplers[0].conv.weight.shape) == (128, 128, 3, 3)
    assert tuple(m.encoder.mid_block.attentions[0].to_q.weight.shape) == (512, 512)
    assert tuple(m.encoder.conv_out.weight.shape) == (8, 512, 3, 3) and tuple(m.quant_conv.weight.shape) == (8, 8, 1, 1)


def test_from_directory_round_trip_legacy_names_ignored_decoder_strays_and_missing_files(tmp_path):
    torch.manual_seed(11)
    src = VAEEncoder(**TINY)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    # current names, with decoder.* / post_quant_conv.* beside them
    full = dict(sd, **{"decoder.conv_in.weight": torch.zeros(4, 4, 3, 3), "post_quant_conv.weight": torch.zeros(4, 4, 1, 1),
                       "post_quant_conv.bias": torch.zeros(4)})
    m = VAEEncoder.from_directory(write_directory(tmp_path / "new", TINY, full))
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items()) and sorted(m.state_dict()) == sorted(sd)
    assert m.config.scaling_factor == 0.5 and m.config.block_out_channels == (64, 128) and m.config.shift_factor is None
    # legacy attention names with their 1x1-conv weight shapes
    at = "encoder.mid_block.attentions.0."
    legacy = {k: v for k, v in sd.items() if not k.startswith(at) or ".group_norm." in k}
    for old, new in (("query", "to_q"), ("key", "to_k"), ("value", "to_v"), ("proj_attn", "to_out.0")):
        legacy[at + old + ".weight"] = sd[at + new + ".weight"].reshape(128, 128, 1, 1)
        legacy[at + old + ".bias"] = sd[at + new + ".bias"]
    m2 = VAEEncoder.from_directory(write_directory(tmp_path / "old", TINY, legacy, extra_cfg=dict(shift_factor=0.25, force_upcast=True)))
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in sd.items()) and m2.config.shift_factor == 0.25
    # a stray key, a missing key: strict
    with pytest.raises(RuntimeError, match="encoder.stray"):
        VAEEncoder.from_directory(write_directory(tmp_path / "stray", TINY, dict(sd, **{"encoder.stray.weight": torch.zeros(1)})))
    with pytest.raises(RuntimeError, match="quant_conv.bias"):
        VAEEncoder.from_directory(write_directory(tmp_path / "short", TINY, {k: v for k, v in sd.items() if k != "quant_conv.bias"}))
    # missing files
    with pytest.raises(FileNotFoundError, match="config.json"):
        VAEEncoder.from_directory(str(tmp_path / "nowhere"))
    os.remove(os.path.join(tmp_path / "new", VAEEncoder.WEIGHTS))
    with pytest.raises(FileNotFoundError, match="diffusion_pytorch_model.safetensors"):
        VAEEncoder.from_directory(str(tmp_path / "new"))
    os.makedirs(tmp_path / "cfg")
    with open(tmp_path / "cfg" / "config.json", "w") as fh:
        json.dump({"in_channels": 3}, fh)
    open(tmp_path / "cfg" / VAEEncoder.WEIGHTS, "wb").close()
    with pytest.raises(ValueError, match="latent_channels"):
        VAEEncoder.from_directory(str(tmp_path / "cfg"))


@pytest.mark.parametrize("bad, word", [
    (dict(act_fn="relu"), "act_fn='relu'.*'silu'"),
    (dict(down_block_types=("DownEncoderBlock2D", "AttnDownEncoderBlock2D")), "down_block_types.*DownEncoderBlock2D"),
    (dict(mid_block_add_attention=False), "mid_block_add_attention=False.*True"),
    (dict(double_z=False), "double_z=False.*True"),
    (dict(block_out_channels=(64, 192)), "192.*served widths"),
    (dict(block_out_channels=(64, 1024)), "1024.*served widths"),
    (dict(block_out_channels=(32, 64)), "32 must be a multiple of 64"),
    (dict(block_out_channels=(96, 128)), "96 must be a multiple of 64"),
    (dict(block_out_channels=(64, 128), norm_num_groups=48), "norm_num_groups=48"),
    (dict(layers_per_block=(1, 2)), "layers_per_block"),
    (dict(latent_channels=0), "latent_channels=0"),
])
def test_refusals_name_the_supported_value(bad, word):
    with pytest.raises(NotImplementedError, match=word):
        VAEEncoder(**dict(TINY, **bad))


def test_served_mid_widths_and_image_shapes():
    assert EV.MID_WIDTHS == (64, 128, 256, 512) and L.ATTENTION_WIDE_DIMS == (256, 512)
    for c in EV.MID_WIDTHS:
        VAEEncoder(**dict(TINY, block_out_channels=(64, c)))
    m = VAEEncoder(**dict(TINY, block_out_channels=(64, 64, 128)))
    assert m.downscale == 4
    m.check_image_shape((2, 3, 32, 48))
    for shape in ((2, 3, 32, 50), (2, 4, 32, 32), (2, 3, 2, 32), (3, 32, 32)):
        with pytest.raises(ValueError, match="multiples of 4"):
            m.check_image_shape(shape)
    with pytest.raises(L.DcamdError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 32, 32))


@pytest.mark.parametrize("quant", [True, False])
def test_tail_fold_equals_the_unfolded_pair_in_fp64(quant):
    torch.manual_seed(5)
    z, Cc = 4, 64
    w, b = torch.randn(2 * z, Cc, 3, 3, dtype=torch.float64), torch.randn(2 * z, dtype=torch.float64)
    qw, qb = (torch.randn(2 * z, 2 * z, 1, 1, dtype=torch.float64), torch.randn(2 * z, dtype=torch.float64)) if quant else (None, None)
    scale, shift = 0.18215, 0.3
    x = torch.randn(2, Cc, 6, 10, dtype=torch.float64)
    mom = F.conv2d(x, w, b, padding=1)
    if quant:
        mom = F.conv2d(mom, qw, qb)
    ref = (mom[:, :z] - shift) * scale
    fw, fb = EV.fold_tail(w, b, qw, qb, z, scale, shift)
    assert fw.dtype == torch.float64 and tuple(fw.shape) == (z, Cc, 3, 3) and tuple(fb.shape) == (z,)
    got = F.conv2d(x, fw, fb, padding=1)
    rel = ((got - ref).norm() / ref.norm()).item()
    worst = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"conv_out . quant_conv fold (quant_conv {quant}): rel-L2 {rel:.2e}, max / max {worst:.2e} (bound 1e-12)")
    assert rel < 1e-12 and worst < 1e-12
    fw0, fb0 = EV.fold_tail(w, b, qw, qb, z, 1.0, None)                        # no shift: None reads as 0
    assert torch.equal(fw0 * scale, fw) and torch.allclose((fb0 - shift) * scale, fb, rtol=1e-14, atol=0)


NEW_SYMBOLS = ("dc_attention_wide", "dc_attention_wide_variant", "dc_im2col_s2")


def test_structs_header_constants_and_exports():
    assert L.AttentionWideParams._fields_ == L.AttentionParams._fields_
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(L.AttentionWideParams) == C.sizeof(L.AttentionParams) == 4 * ptr + 8 * 4
    assert C.sizeof(L.Im2colS2Params) == 2 * ptr + 6 * 4
    hdr = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    assert "DC_OP_ATTENTION_WIDE = 20" in hdr and "DC_OP_IM2COL_S2 = 21" in hdr
    assert (L.OP_ATTENTION_WIDE, L.OP_IM2COL_S2) == (20, 21)
    assert "#define DC_ABI_VERSION 5" in hdr and L.ABI_VERSION == 5
    assert set(NEW_SYMBOLS) <= set(L.EXPORTS)
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None and re.search(r"\b" + name + r"\(", hdr), name
    assert lib.dc_abi_version() == 5


def _wide(**kw):
    base = dict(q=PTR, k=PTR + 1024, v=PTR + 2048, out=PTR + (1 << 16), dtype=L.DC_BF16, n=2, L=64, heads=1, d=512, ld_qkv=1536, ld_out=512,
                scale=512 ** -0.5)
    base.update(kw)
    return L.AttentionWideParams(**base)


def test_attention_wide_validation_and_routes_need_no_gpu():
    lib = L.lib()
    variant = lambda **kw: lib.dc_attention_wide_variant(_wide(**kw)).decode()
    for dt in (L.DC_BF16, L.DC_F16):
        for d in (256, 512):
            assert variant(dtype=dt, d=d, ld_qkv=3 * d, ld_out=d) == "wide"
            assert variant(dtype=dt, d=d, heads=2, ld_qkv=6 * d, ld_out=2 * d) == "wide"
            assert variant(dtype=dt, d=d, ld_qkv=d, ld_out=d) == "wide"                      # separate tensors
        assert variant(dtype=dt, L=1) == "wide" and variant(dtype=dt, L=100000) == "wide"
        assert variant(dtype=dt, ld_out=516) == "wide"                                      # 8-byte output rows are enough
        assert variant(dtype=dt, ld_qkv=1537) == "fp32" and variant(dtype=dt, ld_qkv=1540) == "fp32"     # ld_qkv % 8 != 0
        assert variant(dtype=dt, q=PTR + 2) == "fp32" and variant(dtype=dt, k=PTR + 8) == "fp32" and variant(dtype=dt, v=PTR + 4) == "fp32"
        assert variant(dtype=dt, out=PTR + 4) == "fp32" and variant(dtype=dt, ld_out=514) == "fp32"
    for d in (256, 512):
        assert variant(dtype=L.DC_F32, d=d, ld_qkv=3 * d, ld_out=d) == "fp32"
    for bad, word, code in ((dict(q=None), b"null", -1), (dict(out=None), b"null", -1), (dict(scale=0.0), b"scale", -1),
                            (dict(scale=-0.1), b"scale", -1), (dict(d=128), b"head dim 128 (256/512)", -2), (dict(d=384), b"head dim 384", -2),
                            (dict(d=1024, ld_qkv=3072, ld_out=1024), b"head dim 1024", -2), (dict(L=0), b"n/L/heads", -2),
                            (dict(n=0), b"n/L/heads", -2), (dict(heads=0), b"n/L/heads", -2), (dict(ld_qkv=256), b"ld", -2),
                            (dict(ld_out=511), b"ld", -2), (dict(dtype=7), b"dtype", -3), (dict(q=PTR + 1), b"aligned", -4),
                            (dict(dtype=L.DC_F32, out=PTR + 2), b"aligned", -4)):
        assert variant(**bad) == "invalid", bad
        assert lib.dc_attention_wide(_wide(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    assert lib.dc_attention_wide(None, None) == -1 and lib.dc_attention_wide_variant(None) == b"invalid"
    # dc_attention's own refusals are where they were
    assert lib.dc_attention_variant(L.AttentionParams(q=PTR, k=PTR, v=PTR, out=PTR, dtype=L.DC_BF16, n=2, L=64, heads=1, d=256, ld_qkv=768,
                                                      ld_out=256, scale=0.0625)) == b"invalid"
    p = _wide(d=128)
    ops = (L.Op * 1)()
    ops[0].kind, ops[0].params = L.OP_ATTENTION_WIDE, C.cast(C.pointer(p), C.c_void_p)
    assert lib.dc_run_plan(ops, 1, None) == -2
    assert b"op 0 (kind 20)" in lib.dc_last_error() and b"head dim 128" in lib.dc_last_error()


def test_im2col_s2_validation_needs_no_gpu():
    lib = L.lib()
    mk = lambda **kw: L.Im2colS2Params(**dict(dict(x=PTR, out=PTR + (1 << 16), dtype=L.DC_BF16, n=2, H=16, W=16, C=64, ld=64), **kw))
    for bad, word, code in ((dict(x=None), b"null", -1), (dict(out=None), b"null", -1), (dict(dtype=4), b"dtype", -3),
                            (dict(H=15), b"H=15 W=16 must be even", -2), (dict(W=7), b"must be even", -2), (dict(H=0), b"extents", -2),
                            (dict(C=0), b"extents", -2), (dict(n=0), b"extents", -2), (dict(ld=63), b"ld=63", -2),
                            (dict(x=PTR + 1), b"aligned", -4), (dict(dtype=L.DC_F32, out=PTR + 2), b"aligned", -4)):
        assert lib.dc_im2col_s2(mk(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    assert lib.dc_im2col_s2(None, None) == -1
    p = mk(H=3)
    ops = (L.Op * 1)()
    ops[0].kind, ops[0].params = L.OP_IM2COL_S2, C.cast(C.pointer(p), C.c_void_p)
    assert lib.dc_run_plan(ops, 1, None) == -2
    assert b"op 0 (kind 21)" in lib.dc_last_error() and b"must be even" in lib.dc_last_error()


def test_the_plans_gemm_forms_are_served_by_dc_igemm():
    """The downsampler as a 1x1 GEMM over K = 9 C, q | k | v and to_out (bias + residual in the compute type) at every published width,
    and the folded tail conv with an fp32 output: asked of dc_igemm_variant on the host, as VaePlan checks when it builds."""
    lib = L.lib()
    for dt in (L.DC_F32, L.DC_BF16, L.DC_F16):
        for rows, K, N, res in ((2 * 16 * 16, 9 * 128, 128, False), (2 * 8 * 8, 9 * 256, 256, False), (2 * 4 * 4, 9 * 512, 512, False),
                                (2 * 64, 512, 1536, False), (2 * 64, 512, 512, True), (2 * 64, 256, 768, False), (2 * 64, 256, 256, True),
                                (2 * 64, 9 * 64, 64, False)):
            f = dict(dtype=dt, taps=1, stride=1, upsample=0, n_img=2, Hin=1, Win=rows // 2, Hout=1, Wout=rows // 2, src0=PTR, C0=K, ld0=K,
                     W=PTR, Cout=N, tile_n=128, bias=PTR, out=PTR, out_dtype=dt, out_ld=N)
            if res:
                f.update(residual=PTR, res_dtype=dt, res_ld=N)
            assert lib.dc_igemm_variant(L.IgemmParams(**f)).decode() != "invalid", (dt, rows, K, N, res, lib.dc_last_error())
        for Cc in (256, 512):
            f = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=2, Hin=8, Win=8, Hout=8, Wout=8, src0=PTR, C0=Cc, ld0=Cc, W=PTR, Cout=4,
                     tile_n=32, bias=PTR, out=PTR, out_dtype=L.DC_F32, out_ld=4)
            assert lib.dc_igemm_variant(L.IgemmParams(**f)).decode() != "invalid", (dt, Cc, lib.dc_last_error())


def test_classifier_refuses_a_latent_channel_mismatch_and_a_missing_directory(tmp_path):
    torch.manual_seed(3)
    path = write_directory(tmp_path / "vae", TINY, VAEEncoder(**TINY).state_dict())
    kw = dict(dca.small_unet_kwargs(), sample_size=16)
    with pytest.raises(ValueError, match="in_channels = 3 .* latent_channels = 4"):
        dca.DiffusionClassifier(dca.UNetCondition2D(**kw), dca.Config(**dict(CFG, vae_path=path)))
    with pytest.raises(FileNotFoundError, match="nothing is fetched"):
        dca.DiffusionClassifier(dca.UNetCondition2D(**dict(kw, in_channels=4, out_channels=4)),
                                dca.Config(**dict(CFG, vae_path=str(tmp_path / "absent"))))
    dc = dca.DiffusionClassifier(dca.UNetCondition2D(**dict(kw, in_channels=4, out_channels=4)),
                                 dca.Config(**dict(CFG, vae_path=path, vae_dtype="bf16")))
    assert isinstance(dc.vae, VAEEncoder) and dc.vae.compute_dtype == "bf16"
    assert any(k.startswith("vae.encoder.conv_in") for k in dc.state_dict())
    plain = dca.DiffusionClassifier(dca.UNetCondition2D(**kw), dca.Config(**CFG))
    assert plain.vae is None
    with pytest.raises(RuntimeError, match="vae_path"):
        plain.encode_latents(torch.zeros(1, 3, 32, 32))
    assert dca.DiffusionClassifier(dca.UNetCondition2D(**dict(kw, in_channels=4, out_channels=4)),
                                   dca.Config(**dict(CFG, vae_path=path))).vae.compute_dtype == "f32"
