"""Host: StableDiffusionUNet's envelope, loading and published geometry; the 'scaled_linear' DDPM schedule of DiffusionClassifier; the
routes of dc_cross_attention at head width 160.  No GPU."""
import contextlib
import io
import json
import math
import os

import pytest
import torch
from safetensors.torch import save_file

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd.nets.sd_unet import StableDiffusionUNet
import draws_fixture

PTR = 1 << 20
DC_ERR_SHAPE = -2
MINI = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=(128, 320), layers_per_block=1, norm_num_groups=32,
            down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
            cross_attention_dim=64, attention_head_dim=2)
MINI_LINEAR = dict(MINI, sample_size=8, cross_attention_dim=128, attention_head_dim=(2, 5), use_linear_projection=True)


# ------------------------------------------------------------------------------------------------ envelope
def test_accepted_options_construct():
    m = StableDiffusionUNet(**MINI)
    assert not hasattr(m, "encoder_hid_proj") and not any(k.startswith("encoder_hid_proj") for k in m.state_dict())
    assert m.config.encoder_hid_dim == 64 and m.config.encoder_hid_dim_type is None and m.config.attention_head_dim == (2, 2)
    assert tuple(m.down_blocks[1].attentions[0].proj_in.weight.shape) == (320, 320, 1, 1)
    lin = StableDiffusionUNet(**MINI_LINEAR)
    assert tuple(lin.down_blocks[1].attentions[0].proj_in.weight.shape) == (320, 320) and lin.config.attention_head_dim == (2, 5)
    assert tuple(lin.up_blocks[0].attentions[0].proj_out.weight.shape) == (320, 320)
    for extra in (dict(upcast_attention=True), dict(upcast_attention=False), dict(layers_per_block=(1, 2)), dict(flip_sin_to_cos=False, freq_shift=1),
                  dict(encoder_hid_dim_type=None, encoder_hid_dim=None), dict(only_cross_attention=(False, False)),
                  dict(down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D")),
                  dict(block_out_channels=(128, 640), attention_head_dim=(2, 8)),        # heads of 64 and 80 (zero-padded to 96)
                  dict(block_out_channels=(64, 128), attention_head_dim=8)):             # heads of 8 and 16
        StableDiffusionUNet(**dict(MINI, **extra))
    assert isinstance(StableDiffusionUNet(**MINI), dca.UNetCondition2D) and dca.StableDiffusionUNet is StableDiffusionUNet


@pytest.mark.parametrize("bad, word", [
    (dict(class_embed_type="timestep"), "class_embed_type"), (dict(addition_embed_type="text_time"), "addition_embed_type"),
    (dict(dual_cross_attention=True), "dual_cross_attention"), (dict(only_cross_attention=True), "only_cross_attention"),
    (dict(only_cross_attention=(False, True)), "only_cross_attention"), (dict(transformer_layers_per_block=2), "transformer_layers_per_block"),
    (dict(transformer_layers_per_block=(1, 2)), "transformer_layers_per_block"), (dict(time_cond_proj_dim=256), "time_cond_proj_dim"),
    (dict(attention_type="gated"), "attention_type"), (dict(encoder_hid_dim_type="text_proj", encoder_hid_dim=64), "encoder_hid_dim_type"),
    (dict(num_attention_heads=8), "num_attention_heads"), (dict(num_class_embeds=10), "num_class_embeds"),
    (dict(attention_head_dim=1), "320"),                                               # a head of 320 channels
    (dict(block_out_channels=(128, 384), attention_head_dim=2), "192"),                # a head of 192 channels: above 128 and not 160
    (dict(attention_head_dim=3), "attention_head_dim"),                                # 128 channels in 3 heads
])
def test_refused_options_raise_naming_the_option(bad, word):
    with pytest.raises(NotImplementedError, match=word):
        StableDiffusionUNet(**dict(MINI, **bad))


def test_controlnet_residuals_are_refused_before_anything_else():
    m = StableDiffusionUNet(**MINI)
    with pytest.raises(NotImplementedError, match="ControlNet"):
        m(torch.zeros(1, 4, 16, 16), 1.0, downblock_additional_residuals=[torch.zeros(1)], encoder_hidden_states=torch.zeros(1, 2, 64))


def test_the_refusals_of_unet_condition_2d_stay():
    with pytest.raises(NotImplementedError, match="use_linear_projection"):
        dca.UNetCondition2D(**dict(dca.small_unet_kwargs(), use_linear_projection=True))
    with pytest.raises(NotImplementedError, match="160"):
        dca.UNetCondition2D(**dict(dca.small_unet_kwargs(), block_out_channels=(64, 640), attention_head_dim=4))
    with pytest.raises(NotImplementedError, match="encoder_hid_dim_type"):
        dca.UNetCondition2D(**dict(dca.small_unet_kwargs(), encoder_hid_dim_type=None))


# ------------------------------------------------------------------------------------------------ loading
def _write(tmp_path, name, kw, sd=None, drop=None, extra_cfg=None):
    d = tmp_path / name
    d.mkdir()
    cfg = dict(kw, _class_name="UNet2DConditionModel", _diffusers_version="0.31.0", _name_or_path="somewhere", **(extra_cfg or {}))
    for k in drop or ():
        del cfg[k]
    (d / "config.json").write_text(json.dumps(cfg))
    if sd is not None:
        save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    return str(d)


@pytest.mark.parametrize("kw", [MINI, MINI_LINEAR], ids=["conv_proj", "linear_proj"])
def test_from_directory_round_trip_strays_missing_keys_and_config_fields(tmp_path, kw):
    torch.manual_seed(3)
    src = StableDiffusionUNet(**kw)
    sd = src.state_dict()
    m = StableDiffusionUNet.from_directory(_write(tmp_path, "ok", kw, sd, extra_cfg=dict(upcast_attention=True, act_fn="silu", center_input_sample=False)))
    assert list(m.state_dict()) == list(sd) and all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert all(not p.requires_grad for p in m.parameters()) and m.config.upcast_attention is True
    assert m.config.sample_size == kw["sample_size"]
    assert StableDiffusionUNet.from_directory(_write(tmp_path, "ok2", kw, sd), sample_size=32).config.sample_size == 32
    with pytest.raises(RuntimeError, match="stray.weight"):
        StableDiffusionUNet.from_directory(_write(tmp_path, "stray", kw, dict(sd, **{"stray.weight": torch.zeros(2)})))
    with pytest.raises(RuntimeError, match="encoder_hid_proj"):                      # a checkpoint of the reference's family does not fit
        StableDiffusionUNet.from_directory(_write(tmp_path, "hid", kw, dict(sd, **{"encoder_hid_proj.weight": torch.zeros(64, 64)})))
    lost = "mid_block.attentions.0.transformer_blocks.0.attn2.to_k.weight"
    with pytest.raises(RuntimeError, match=lost.replace(".", r"\.")):
        StableDiffusionUNet.from_directory(_write(tmp_path, "lost", kw, {k: v for k, v in sd.items() if k != lost}))
    with pytest.raises(ValueError, match="cross_attention_dim"):
        StableDiffusionUNet.from_directory(_write(tmp_path, "nofield", kw, sd, drop=["cross_attention_dim"]))
    with pytest.raises(NotImplementedError, match="addition_embed_type"):
        StableDiffusionUNet.from_directory(_write(tmp_path, "xl", kw, sd, extra_cfg=dict(addition_embed_type="text_time")))
    with pytest.raises(FileNotFoundError, match="diffusion_pytorch_model.safetensors"):
        StableDiffusionUNet.from_directory(_write(tmp_path, "noweights", kw))
    # the other projection style's file does not load: [C, C] against [C, C, 1, 1]
    other = StableDiffusionUNet(**dict(kw, use_linear_projection=not kw.get("use_linear_projection", False))).state_dict()
    with pytest.raises(RuntimeError, match="proj_in"):
        StableDiffusionUNet.from_directory(_write(tmp_path, "style", kw, other))


# ------------------------------------------------------------------------------------------------ published geometry
def test_published_geometry_on_the_meta_device():
    site = "down_blocks.2.attentions.1.transformer_blocks.0"
    shapes = {}
    for name, fn in (("1.5", dca.sd15_unet_kwargs), ("2.1", dca.sd21_unet_kwargs)):
        with torch.device("meta"):
            m = StableDiffusionUNet(**fn())
        sd = m.state_dict()
        shapes[name] = {k: tuple(v.shape) for k, v in sd.items()}
        assert not any(k.startswith("encoder_hid_proj") for k in sd)
        s = shapes[name]
        assert s["time_embedding.linear_1.weight"] == (1280, 320)
        assert s[site + ".ff.net.0.proj.weight"] == (10240, 1280)
        assert s["up_blocks.1.resnets.2.conv1.weight"] == (1280, 1920, 3, 3)
        assert s["up_blocks.2.resnets.2.conv1.weight"] == (640, 960, 3, 3)
        assert s["up_blocks.3.resnets.2.conv1.weight"] == (320, 640, 3, 3)
        assert s["conv_in.weight"] == (320, 4, 3, 3) and s["conv_out.weight"] == (4, 320, 3, 3)
        assert "down_blocks.3.attentions.0.proj_in.weight" not in s and "up_blocks.0.attentions.0.proj_in.weight" not in s
        # head widths per site, from the engine's own reading of the config
        from diffusion_classifier_amd import engine as E
        widths = {k[: -len(".proj_in.weight")]: v[0] // E.site_heads(m.config, k) for k, v in s.items() if k.endswith(".proj_in.weight")}
        assert len(widths) == 16                                        # 6 down, 1 mid, 9 up
        by_level = lambda prefix: {w for k, w in widths.items() if k.startswith(prefix)}
        if name == "1.5":
            assert by_level("down_blocks.0") == {40} and by_level("down_blocks.1") == {80} and by_level("down_blocks.2") == {160}
            assert by_level("mid_block") == {160} and by_level("up_blocks.1") == {160} and by_level("up_blocks.2") == {80} and by_level("up_blocks.3") == {40}
            assert [E.site_head_dim(w) for w in (40, 80, 160)] == [64, 96, 160]
        else:
            assert set(widths.values()) == {64}
    assert shapes["1.5"]["down_blocks.1.attentions.0.proj_in.weight"] == (640, 640, 1, 1)
    assert shapes["2.1"]["down_blocks.1.attentions.0.proj_in.weight"] == (640, 640)
    assert shapes["1.5"][site + ".attn2.to_k.weight"] == (1280, 768) and shapes["2.1"][site + ".attn2.to_k.weight"] == (1280, 1024)
    assert sum(math.prod(v) for v in shapes["1.5"].values()) == 859520964            # the published parameter count of the SD 1.x UNet


def test_packing_head_dims_stay_and_the_wide_head_is_the_engines():
    from diffusion_classifier_amd import engine as E, packing
    assert packing.HEAD_DIMS == (16, 32, 64, 96, 128) and E.WIDE_HEAD == 160
    with pytest.raises(NotImplementedError, match="160"):
        packing.padded_head_dim(160)
    assert E.site_head_dim(160) == 160 and E.site_head_dim(80) == 96
    with pytest.raises(NotImplementedError):
        E.site_head_dim(192)
    cfg = StableDiffusionUNet(**MINI_LINEAR).config
    assert [E.site_heads(cfg, k) for k in ("down_blocks.0.attentions.0", "down_blocks.1.attentions.0", "mid_block.attentions.0",
                                          "up_blocks.0.attentions.1", "up_blocks.1.attentions.0")] == [2, 5, 5, 5, 2]


# ------------------------------------------------------------------------------------------------ schedule
def _classifier(**over):
    return draws_fixture.classifier(over.pop("schedule", "scaled_linear"), **over)


def _ref_schedule(N=1000, b0=0.00085, b1=0.012):
    """Independent fp64 restatement: plain Python floats."""
    lam, abar = [], 1.0
    for i in range(N):
        beta = (math.sqrt(b0) + (math.sqrt(b1) - math.sqrt(b0)) * i / (N - 1)) ** 2
        abar *= 1.0 - beta
        lam.append(math.log(abar / (1.0 - abar)))
    return lam


@pytest.mark.parametrize("N, b0, b1", [(1000, 0.00085, 0.012), (50, 0.001, 0.02)])
def test_scaled_linear_schedule_against_an_fp64_restatement(N, b0, b1):
    over = {} if N == 1000 else dict(train_timesteps=N, beta_start=b0, beta_end=b1)
    dc = _classifier(**over)
    ref = _ref_schedule(N, b0, b1)
    t = torch.tensor([0.0, 1.0 / N, 0.5, 1.0 - 1e-7, 1.0], dtype=torch.float32)
    k_ref = [min(int(math.floor(float(v) * N)), N - 1) for v in t.tolist()]       # the fp32 value of t, the product in fp64
    # (fp32(1 / 50) lies just below 1 / 50 and falls into step 0; fp32(1 / 1000) just above 1 / 1000)
    assert k_ref == [0, 1 if N == 1000 else 0, N // 2, N - 1, N - 1]
    lam, lab = dc.schedule(t), dc.noise_labels(t)
    assert lam.dtype == torch.float32 and lab.dtype == torch.float32 and lab.tolist() == [float(k) for k in k_ref]
    assert torch.equal(lam, torch.tensor([ref[k] for k in k_ref], dtype=torch.float64).to(torch.float32))
    table = dc.ddpm_logsnr
    assert tuple(table.shape) == (N,) and torch.equal(table, torch.tensor(ref, dtype=torch.float64).to(torch.float32))
    assert bool((table[1:] < table[:-1]).all())                                    # strictly decreasing in k
    al, sg = torch.sqrt(torch.sigmoid(table)), torch.sqrt(torch.sigmoid(-table))
    assert float((al * al + sg * sg - 1).abs().max()) <= 4 * torch.finfo(torch.float32).eps
    # a scalar and a [T, BS] grid go through as the per-trial vectors do
    assert float(dc.schedule(torch.tensor(0.5))) == float(lam[2]) and torch.equal(dc.schedule(t.reshape(5, 1)), lam.reshape(5, 1))


def test_trial_draws_carry_the_step_as_label_and_keep_alpha_sigma_of_the_logsnr():
    dc = _classifier()
    T, BS = draws_fixture.T, draws_fixture.BS
    t = torch.linspace(0, 1, T * BS).reshape(T, BS)
    d = dc._trial_draws(torch.zeros(BS, 3, 4, 4), T, t, torch.zeros(T, BS, 3, 4, 4), "reference", 0)
    assert torch.equal(d["label"], torch.clamp(torch.floor(t.double() * 1000), max=999).float())
    assert torch.equal(d["logsnr"], dc.ddpm_logsnr[d["label"].long()])
    assert torch.equal(d["alpha"], torch.sqrt(torch.sigmoid(d["logsnr"]))) and torch.equal(d["sigma"], torch.sqrt(torch.sigmoid(-d["logsnr"])))


def test_cosine_trial_draws_are_the_recorded_bytes_and_their_label_is_the_logsnr():
    with open(draws_fixture.FIXTURE) as f:
        want = json.load(f)
    assert draws_fixture.draws() == want
    for schedule in ("cosine", "shifted_cosine"):
        dc = _classifier(schedule=schedule)
        t = torch.rand(draws_fixture.T, draws_fixture.BS)
        d = dc._trial_draws(torch.zeros(draws_fixture.BS, 3, 4, 4), draws_fixture.T, t, torch.zeros(draws_fixture.T, draws_fixture.BS, 3, 4, 4), "reference", 0)
        assert d["label"] is d["logsnr"]                                          # the control block's lam slot: the same tensor as ever
        assert torch.equal(dc.noise_labels(t[0]), dc.schedule(t[0]))


def test_scheduler_path_parsing_and_the_prediction_type_conflict(tmp_path):
    def write(name, **kw):
        p = tmp_path / name
        p.mkdir()
        (p / "scheduler_config.json").write_text(json.dumps(dict(dict(_class_name="PNDMScheduler", beta_schedule="scaled_linear", beta_start=0.001,
                                                                      beta_end=0.02, num_train_timesteps=50, prediction_type="epsilon"), **kw)))
        return str(p)
    dc = _classifier(scheduler_path=write("a"))
    assert dc.train_timesteps == 50 and torch.equal(dc.ddpm_logsnr, torch.tensor(_ref_schedule(50, 0.001, 0.02), dtype=torch.float64).float())
    assert _classifier(scheduler_path=os.path.join(write("b"), "scheduler_config.json")).train_timesteps == 50      # the file itself
    assert _classifier(scheduler_path=write("c"), train_timesteps=20).train_timesteps == 20                          # the config's own key wins
    assert _classifier(scheduler_path=write("v", prediction_type="v_prediction"), pred_param="v").train_timesteps == 50
    with pytest.raises(ValueError, match="prediction_type"):
        _classifier(scheduler_path=write("d", prediction_type="v_prediction"))
    with pytest.raises(ValueError, match="prediction_type"):
        _classifier(scheduler_path=write("e"), pred_param="v")
    with pytest.raises(ValueError, match="beta_schedule"):
        _classifier(scheduler_path=write("f", beta_schedule="linear"))


def test_generation_entry_points_refuse_the_discrete_schedule():
    dc = _classifier(sampling_steps=4)
    x = torch.zeros(2, 3, 32, 32)
    for call in (lambda: dc.sample(x, torch.tensor([0, 1])), lambda: dc.counterfactual(x), lambda: dc.invert(x), lambda: dc.invert_ddpm(x)):
        with pytest.raises(NotImplementedError, match="scaled_linear"):
            call()
    with pytest.raises(AssertionError, match="Invalid schedule"):
        _classifier(schedule="linear")


def test_classifier_takes_its_table_width_from_the_sd_unet():
    with contextlib.redirect_stdout(io.StringIO()):
        dc = dca.DiffusionClassifier(StableDiffusionUNet(**MINI), dca.Config(
            pred_param="eps", schedule="scaled_linear", noise_d=16, image_size=16, cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1,
            encoder_type="prompt", prompt_tokens=7, classes=3, n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2))
    assert tuple(dc.encoder.weight.shape) == (4, 7, 64)


# ------------------------------------------------------------------------------------------------ routes at head width 160
def _cross(**kw):
    base = dict(q=PTR, k=PTR, v=PTR, out=PTR, dtype=L.DC_BF16, n=3, Lq=33, S=7, heads=2, d=160, ld_q=320, ld_kv=320, ld_out=320, scale=160 ** -0.5)
    return dict(base, **kw)


def test_cross_attention_routes_at_160_need_no_gpu():
    lib = L.lib()
    plain = lambda **kw: lib.dc_cross_attention_variant(L.CrossAttentionParams(**_cross(**kw))).decode()
    length = lambda **kw: lib.dc_cross_attention_len_variant(L.CrossAttentionLenParams(**_cross(**kw), kv_len=PTR)).decode()
    for variant in (plain, length):
        for dt in (L.DC_BF16, L.DC_F16):
            assert variant(dtype=dt) == "mfma"
            assert variant(dtype=dt, ld_q=960, ld_kv=960, k=PTR + 640, v=PTR + 1280, Lq=64, S=64) == "mfma"      # the self form: fused QKV
            assert variant(dtype=dt, ld_kv=1280, v=PTR + 640) == "mfma"                                      # stacked K | V
            assert variant(dtype=dt, q=PTR + 2) == "fp32" and variant(dtype=dt, k=PTR + 8) == "fp32" and variant(dtype=dt, v=PTR + 4) == "fp32"
            assert variant(dtype=dt, ld_q=324) == "fp32" and variant(dtype=dt, ld_kv=322) == "fp32"          # rows that are not 16-byte aligned
            assert variant(dtype=dt, out=PTR + 4) == "fp32" and variant(dtype=dt, ld_out=322) == "fp32"
        assert variant(dtype=L.DC_F32) == "fp32"
        for dt in (L.DC_F32, L.DC_BF16, L.DC_F16):
            assert variant(dtype=dt, d=192, ld_q=384, ld_kv=384, ld_out=384) == "invalid"
            assert variant(dtype=dt, d=144, ld_q=288, ld_kv=288, ld_out=288) == "invalid"
            assert variant(dtype=dt, ld_q=319) == "invalid"                                                  # a row shorter than heads * d
    p = L.CrossAttentionParams(**_cross(d=192, ld_q=384, ld_kv=384, ld_out=384))
    assert lib.dc_cross_attention(p, None) == DC_ERR_SHAPE and "16/32/64/96/128/160" in lib.dc_last_error().decode()
    # dc_attention keeps refusing the width
    a = L.AttentionParams(q=PTR, k=PTR, v=PTR, out=PTR, dtype=L.DC_BF16, n=2, L=64, heads=2, d=160, ld_qkv=960, ld_out=320, scale=0.1)
    assert lib.dc_attention_variant(a) == b"invalid" and lib.dc_attention(a, None) == DC_ERR_SHAPE
