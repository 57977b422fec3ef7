"""CPU: the AutoencoderKL decoder path without a GPU — VAEDecoder's parameter names and shapes, local loading (legacy attention names,
ignored encoder, strict on strays, missing decoder keys named, missing files), every refusal, the lazy load behind
DiffusionClassifier.decode_latents, the ValueErrors of decode=True, and the C-ABI of dc_latent_im2col (struct order and size, export, plan
kind, argument validation)."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine_vae as EV
from diffusion_classifier_amd.nets.vae import VAEDecoder, VAEEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(pred_param="eps", schedule="cosine", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, n_stages=1,
           evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32", image_size=16, noise_d=16,
           encoder_type="nn", classes=3, sampling_steps=2)
TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(64, 128), layers_per_block=1, norm_num_groups=32, scaling_factor=0.5)
ENC_TINY = dict(in_channels=3, latent_channels=4, block_out_channels=(64, 128), layers_per_block=1, norm_num_groups=32, scaling_factor=0.5)
PTR = 1 << 20


def wb(*names):
    return [n + s for n in names for s in (".weight", ".bias")]


def resnet(k, shortcut=False):
    return wb(k + ".norm1", k + ".conv1", k + ".norm2", k + ".conv2") + (wb(k + ".conv_shortcut") if shortcut else [])


# The decoder-side keys of the published Stable Diffusion AutoencoderKL (diffusers 0.31 names), written out by hand: block_out_channels
# (128, 256, 512, 512), two layers per block, so three ResNets per up block; up blocks 2 and 3 change the width (512 -> 256 -> 128).
SD_DECODER_KEYS = (
    wb("post_quant_conv", "decoder.conv_in")
    + resnet("decoder.mid_block.resnets.0") + resnet("decoder.mid_block.resnets.1")
    + wb("decoder.mid_block.attentions.0.group_norm", "decoder.mid_block.attentions.0.to_q", "decoder.mid_block.attentions.0.to_k",
         "decoder.mid_block.attentions.0.to_v", "decoder.mid_block.attentions.0.to_out.0")
    + resnet("decoder.up_blocks.0.resnets.0") + resnet("decoder.up_blocks.0.resnets.1") + resnet("decoder.up_blocks.0.resnets.2")
    + wb("decoder.up_blocks.0.upsamplers.0.conv")
    + resnet("decoder.up_blocks.1.resnets.0") + resnet("decoder.up_blocks.1.resnets.1") + resnet("decoder.up_blocks.1.resnets.2")
    + wb("decoder.up_blocks.1.upsamplers.0.conv")
    + resnet("decoder.up_blocks.2.resnets.0", shortcut=True) + resnet("decoder.up_blocks.2.resnets.1") + resnet("decoder.up_blocks.2.resnets.2")
    + wb("decoder.up_blocks.2.upsamplers.0.conv")
    + resnet("decoder.up_blocks.3.resnets.0", shortcut=True) + resnet("decoder.up_blocks.3.resnets.1") + resnet("decoder.up_blocks.3.resnets.2")
    + wb("decoder.conv_norm_out", "decoder.conv_out"))


def write_directory(path, cfg, sd, extra_cfg=None):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(dict(dict(cfg, block_out_channels=list(cfg["block_out_channels"])), _class_name="AutoencoderKL", sample_size=256,
                       in_channels=3, down_block_types=["DownEncoderBlock2D"] * len(cfg["block_out_channels"]), **(extra_cfg or {})), fh)
    save_file({k: v.clone().contiguous() for k, v in sd.items()}, os.path.join(path, VAEDecoder.WEIGHTS))
    return str(path)


def test_state_dict_keys_are_the_published_names_and_shapes():
    # 2 x (post_quant_conv, conv_in, conv_norm_out, conv_out) + 14 ResNets x 8 + 2 shortcuts x 2 + 5 x 2 in the attention + 3 upsamplers x 2
    assert len(SD_DECODER_KEYS) == 8 + 112 + 4 + 10 + 6 == 140 and len(set(SD_DECODER_KEYS)) == 140
    m = VAEDecoder(**dca.sd_vae_kwargs())
    sd = m.state_dict()
    assert sorted(sd.keys()) == sorted(SD_DECODER_KEYS), set(sd) ^ set(SD_DECODER_KEYS)
    assert not any(p.requires_grad for p in m.parameters())
    assert m.upscale == 8 and m.config.out_channels == 3 and m.config.use_post_quant_conv
    for key, shape in (("decoder.conv_in.weight", (512, 4, 3, 3)),
                       ("decoder.up_blocks.2.resnets.0.conv_shortcut.weight", (256, 512, 1, 1)),
                       ("decoder.up_blocks.3.resnets.0.conv_shortcut.weight", (128, 256, 1, 1)),
                       ("decoder.conv_out.weight", (3, 128, 3, 3)),
                       ("post_quant_conv.weight", (4, 4, 1, 1)),
                       ("decoder.up_blocks.2.resnets.0.conv1.weight", (256, 512, 3, 3)),
                       ("decoder.up_blocks.0.upsamplers.0.conv.weight", (512, 512, 3, 3)),
                       ("decoder.mid_block.attentions.0.to_q.weight", (512, 512))):
        assert tuple(sd[key].shape) == shape, key
    no_pq = VAEDecoder(**dict(TINY, use_post_quant_conv=False, layers_per_block=2))
    assert not any(k.startswith("post_quant_conv") for k in no_pq.state_dict())
    assert "decoder.up_blocks.1.resnets.2.conv2.weight" in no_pq.state_dict() and "decoder.up_blocks.1.upsamplers.0.conv.weight" not in no_pq.state_dict()
    assert VAEEncoder.IGNORED == ("decoder.", "post_quant_conv.")                       # the encoder's loader is where it was


def test_from_directory_round_trip_legacy_names_ignored_encoder_strays_missing_keys_and_files(tmp_path):
    torch.manual_seed(12)
    src = VAEDecoder(**TINY)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    enc = {k: v.clone() for k, v in VAEEncoder(**ENC_TINY).state_dict().items()}
    # a full AutoencoderKL file: the encoder's keys beside the decoder's
    m = VAEDecoder.from_directory(write_directory(tmp_path / "new", TINY, dict(sd, **enc)))
    assert sorted(m.state_dict()) == sorted(sd) and all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    assert m.config.scaling_factor == 0.5 and m.config.block_out_channels == (64, 128) and m.config.shift_factor is None
    e = VAEEncoder.from_directory(str(tmp_path / "new"))                                # the same directory still feeds the encoder
    assert all(torch.equal(e.state_dict()[k], v) for k, v in enc.items())
    # legacy attention names with their 1x1-conv weight shapes
    at = "decoder.mid_block.attentions.0."
    legacy = {k: v for k, v in sd.items() if not k.startswith(at) or ".group_norm." in k}
    for old, new in (("query", "to_q"), ("key", "to_k"), ("value", "to_v"), ("proj_attn", "to_out.0")):
        legacy[at + old + ".weight"] = sd[at + new + ".weight"].reshape(128, 128, 1, 1)
        legacy[at + old + ".bias"] = sd[at + new + ".bias"]
    m2 = VAEDecoder.from_directory(write_directory(tmp_path / "old", TINY, legacy, extra_cfg=dict(shift_factor=0.25, force_upcast=True)))
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in sd.items()) and m2.config.shift_factor == 0.25
    # a stray key is refused; a missing one is named; an encoder-only file names the decoder's first key
    with pytest.raises(RuntimeError, match="decoder.stray"):
        VAEDecoder.from_directory(write_directory(tmp_path / "stray", TINY, dict(sd, **{"decoder.stray.weight": torch.zeros(1)})))
    with pytest.raises(RuntimeError, match="post_quant_conv.bias"):
        VAEDecoder.from_directory(write_directory(tmp_path / "short", TINY, {k: v for k, v in sd.items() if k != "post_quant_conv.bias"}))
    with pytest.raises(RuntimeError, match=r"holds no decoder\.conv_in\.weight"):
        VAEDecoder.from_directory(write_directory(tmp_path / "enc", TINY, enc))
    # missing files
    with pytest.raises(FileNotFoundError, match="config.json"):
        VAEDecoder.from_directory(str(tmp_path / "nowhere"))
    os.remove(os.path.join(tmp_path / "new", VAEDecoder.WEIGHTS))
    with pytest.raises(FileNotFoundError, match="diffusion_pytorch_model.safetensors.*nothing is fetched"):
        VAEDecoder.from_directory(str(tmp_path / "new"))
    os.makedirs(tmp_path / "cfg")
    with open(tmp_path / "cfg" / "config.json", "w") as fh:
        json.dump({"latent_channels": 4}, fh)
    open(tmp_path / "cfg" / VAEDecoder.WEIGHTS, "wb").close()
    with pytest.raises(ValueError, match="block_out_channels"):
        VAEDecoder.from_directory(str(tmp_path / "cfg"))


@pytest.mark.parametrize("bad, word", [
    (dict(act_fn="relu"), "act_fn='relu'.*'silu'"),
    (dict(up_block_types=("UpDecoderBlock2D", "AttnUpDecoderBlock2D")), "up_block_types.*UpDecoderBlock2D"),
    (dict(mid_block_add_attention=False), "mid_block_add_attention=False.*True"),
    (dict(block_out_channels=(64, 192)), "192.*served widths.*64, 128, 256, 512"),
    (dict(block_out_channels=(64, 1024)), "1024.*served widths"),
    (dict(block_out_channels=(32, 64)), "32 must be a multiple of 64"),
    (dict(block_out_channels=(96, 128)), "96 must be a multiple of 64"),
    (dict(block_out_channels=(64, 128), norm_num_groups=48), "norm_num_groups=48"),
    (dict(layers_per_block=(1, 2)), "layers_per_block.*one int >= 1"),
    (dict(latent_channels=0), "latent_channels=0.*both >= 1"),
    (dict(out_channels=0), "out_channels=0.*both >= 1"),
])
def test_refusals_name_the_supported_value(bad, word):
    with pytest.raises(NotImplementedError, match=word):
        VAEDecoder(**dict(TINY, **bad))


def test_served_mid_widths_and_latent_shapes():
    for c in EV.MID_WIDTHS:
        VAEDecoder(**dict(TINY, block_out_channels=(64, c)))
    m = VAEDecoder(**dict(TINY, block_out_channels=(64, 64, 128)))
    assert m.upscale == 4
    m.check_latent_shape((2, 4, 1, 1))
    m.check_latent_shape((1, 4, 8, 12))
    for shape in ((2, 3, 8, 8), (2, 4, 0, 8), (4, 8, 8), (0, 4, 8, 8)):
        with pytest.raises(ValueError, match=r"latents \[B, 4, h, w\]"):
            m.check_latent_shape(shape)
    with pytest.raises(L.DcamdError, match="no CPU fallback"):
        m(torch.zeros(1, 4, 8, 8))


def test_lazy_load_and_the_errors_of_decode(tmp_path):
    """A classifier on an encoder-only directory constructs as ever (and holds no decoder key); decode_latents then names the key the
    directory lacks.  decode=True is a ValueError without vae_path and together with pixel_space, before anything is drawn."""
    torch.manual_seed(3)
    enc = VAEEncoder(**ENC_TINY).state_dict()
    path = write_directory(tmp_path / "vae", TINY, enc)
    kw = dict(dca.small_unet_kwargs(), sample_size=16, in_channels=4, out_channels=4)
    dc = dca.DiffusionClassifier(dca.UNetCondition2D(**kw), dca.Config(**dict(CFG, vae_path=path)))
    keys = set(dc.state_dict())
    assert isinstance(dc.vae, VAEEncoder) and not any("decoder." in k for k in keys)
    with pytest.raises(RuntimeError, match=r"decoder\.conv_in\.weight"):
        dc.decode_latents(torch.zeros(1, 4, 4, 4))
    assert set(dc.state_dict()) == keys
    x = torch.zeros(1, 4, 4, 4)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="pixel_space"):
        dc.counterfactual(x, decode=True, pixel_space=True)
    full = write_directory(tmp_path / "full", TINY, dict(enc, **VAEDecoder(**TINY).state_dict()))
    both = dca.DiffusionClassifier(dca.UNetCondition2D(**kw), dca.Config(**dict(CFG, vae_path=full, vae_decode_batch=0)))
    with pytest.raises(ValueError, match="vae_decode_batch must be an int >= 1, got 0"):
        both.decode_latents(x)
    assert isinstance(both._vae_decoder, VAEDecoder) and not any("decoder." in k for k in both.state_dict())      # loaded, and no submodule
    plain = dca.DiffusionClassifier(dca.UNetCondition2D(**dict(dca.small_unet_kwargs(), sample_size=16)), dca.Config(**CFG))
    torch.set_rng_state(state)
    with pytest.raises(ValueError, match="decode=True needs config.vae_path"):
        plain.sample(torch.zeros(1, 3, 16, 16), torch.zeros(1, dtype=torch.long), decode=True)
    with pytest.raises(ValueError, match="decode=True needs config.vae_path"):
        plain.counterfactual(torch.zeros(1, 3, 16, 16), decode=True)
    assert torch.equal(torch.get_rng_state(), state)                                     # refused before the first draw
    with pytest.raises(RuntimeError, match="vae_path"):
        plain.decode_latents(x)


def test_latent_im2col_struct_header_constant_and_export():
    assert C.sizeof(L.LatentIm2colParams) == 4 * C.sizeof(C.c_void_p) + 8 * 4
    hdr = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    assert "DC_OP_LATENT_IM2COL = 23" in hdr and L.OP_LATENT_IM2COL == 23
    assert "#define DC_ABI_VERSION 5" in hdr and L.ABI_VERSION == 5
    assert "dc_latent_im2col" in L.EXPORTS and re.search(r"\bdc_latent_im2col\(", hdr)
    assert L.lib().dc_latent_im2col is not None


def test_latent_im2col_validation_needs_no_gpu():
    lib = L.lib()
    mk = lambda **kw: L.LatentIm2colParams(**dict(dict(z=PTR, Q=PTR + 4096, bias=PTR + 8192, out=PTR + (1 << 16), out_dtype=L.DC_BF16, n=2,
                                                       Z=4, H=8, W=8, Kpad=64, inv_scale=2.0, shift=0.0), **kw))
    for bad, word, code in ((dict(z=None), b"null", -1), (dict(Q=None), b"null", -1), (dict(bias=None), b"null", -1), (dict(out=None), b"null", -1),
                            (dict(out_dtype=5), b"out_dtype 5", -3), (dict(Z=0), b"Z=0", -2), (dict(Z=-1), b"Z=-1", -2), (dict(n=0), b"extents", -2),
                            (dict(H=0), b"extents", -2), (dict(W=0), b"extents", -2),
                            (dict(Kpad=0), b"Kpad=0 (need >= 9 Z = 36", -2), (dict(Z=8), b"Kpad=64 (need >= 9 Z = 72", -2),
                            (dict(Kpad=96), b"a multiple of 64", -2), (dict(out_dtype=L.DC_F32, Kpad=48), b"a multiple of 32", -2),
                            (dict(out_dtype=L.DC_F16, Kpad=40), b"a multiple of 64", -2),
                            (dict(z=PTR + 2), b"aligned", -4), (dict(out=PTR + 8), b"aligned", -4)):
        assert lib.dc_latent_im2col(mk(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    assert lib.dc_latent_im2col(None, None) == -1
    p = mk(Kpad=32)
    ops = (L.Op * 1)()
    ops[0].kind, ops[0].params = L.OP_LATENT_IM2COL, C.cast(C.pointer(p), C.c_void_p)
    assert lib.dc_run_plan(ops, 1, None) == -2
    assert b"op 0 (kind 23)" in lib.dc_last_error() and b"Kpad=32" in lib.dc_last_error()


@pytest.mark.parametrize("name", ["mid64", "mid128"])
def test_the_storage_rounding_table_behind_the_16_bit_bars_is_current(name):
    """tests/test_gpu_vae_decoder.py takes its bf16 / f16 bars from STORE_DISTANCE, a table measured on the restatement alone.  The two
    cheapest cases are measured again here, so that an edit of the restatement or another torch cannot leave stale bars unnoticed.
    Each distance must lie within a factor 1.5 of its entry: an evaluation that differs in the last fp32 bit (another host, another
    thread count) is another draw of the same rounding noise, and the draws of one case over its seeds span up to 1.45x in
    the table itself; 1.5 is also the factor the bars allow over the table."""
    import test_gpu_vae_decoder as G
    kw, shape = G.CASES[name]
    for dt, store in G.STORE.items():
        for seed, entry in zip(G.SEEDS, G.STORE_DISTANCE[(name, dt)]):
            m = G.random_decoder(kw, seed)
            sd, z = G.cpu_state(m), G.latents_of(seed, shape)
            d = G.per_sample_rel(G.vae_decode(sd, G.cfg_of(m), z, store=store), G.vae_decode(sd, G.cfg_of(m), z))
            print(f"storage-rounding distance {name} {dt} seed {seed}: {d:.3e} (table {entry:.3e})")
            assert entry / 1.5 < d < entry * 1.5, (name, dt, seed, d, entry)
    assert set(G.STORE_DISTANCE) == {(n, dt) for n in G.CASES for dt in G.STORE}
