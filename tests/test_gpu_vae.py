"""GPU: the AutoencoderKL encoder path — dc_im2col_s2 bit for bit against unfold of the bottom/right-padded tensor, VAEEncoder.forward
against the plain-torch restatement (tests/vae_oracle.py), classify through latents, and loading from a directory.

Bars are the project's for a whole forward (tests/test_gpu_clip_model.py): 1e-4 relative L2 in f32 and 2e-2 in bf16 / f16, both against the
fp32 restatement on the CPU; 1e-4 per-cell relative error of the eps-MSE in f32.

Why the 16-bit forwards are held against the PLAIN fp32 restatement and not its storage-rounded form (vae_encode(store=...)): rounding every
stored tensor to bf16 makes two evaluations that differ in the last fp32 bit part ways — a value next to a rounding boundary lands on the
other side, the next layer turns that into more such values — until they differ like two independent draws of the rounding noise.  Measured
on the restatement alone (no kernel involved), sd_vae_kwargs() at 64x64, three seeds: storage-rounded in fp32 against storage-rounded in
fp64 arithmetic 1.1e-2 .. 1.8e-2, one CPU thread against many 1.2e-2; storage-rounded against plain fp32 1.0e-2 .. 1.6e-2 (tiny
architecture: 0.5e-2 .. 1.1e-2).  A storage-rounded reference therefore adds its own draw of that noise, which depends on the host's
thread count, and removes none of the kernel's; the plain fp32 reference is reproducible to 1e-6 on any host.  q / k weights are scaled by 2
(not more: a sharper softmax raises the same noise, 1.8e-2 .. 2.2e-2 at 4): a choice made on those restatement-only figures."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import diffusion_classifier_amd as dca
import oracle
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd.nets.vae import VAEEncoder
from vae_oracle import vae_encode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
TINY = dict(in_channels=3, latent_channels=4, block_out_channels=(64, 128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)
SENTINEL, GUARD = 7.0, 4096
_CACHE = {}


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- dc_im2col_s2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("H, W, pad", [(2, 2, 0), (6, 10, 0), (16, 16, 0), (6, 10, 8), (16, 16, 3)])
def test_im2col_s2_is_unfold_of_the_bottom_right_padded_tensor(dt, C, H, W, pad):
    """pad: ld - C, the pad columns NaN (8: rows stay 16-byte multiples, the vector form; 3: the element form)."""
    n, ld = 3, C + pad
    gen = torch.Generator().manual_seed(H * 1000 + W * 10 + C + pad)
    x = torch.randn(n, H, W, C, generator=gen).to(TD[dt])
    src = torch.full((n, H, W, ld), float("nan"), dtype=TD[dt])
    src[..., :C] = x
    nchw = F.pad(x.float().permute(0, 3, 1, 2), (0, 1, 0, 1))                          # bottom / right only
    cols = F.unfold(nchw, kernel_size=3, stride=2)                                     # [n, C * 9, Ho * Wo], row c * 9 + ky * 3 + kx
    Ho, Wo = H // 2, W // 2
    assert cols.shape[-1] == Ho * Wo
    ref = cols.view(n, C, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(n, Ho, Wo, 9 * C).to(TD[dt])
    nel = n * Ho * Wo * 9 * C
    out = torch.full((nel + GUARD,), SENTINEL, dtype=TD[dt], device=DEV)
    sd = src.to(DEV)
    p = L.Im2colS2Params(x=sd.data_ptr(), out=out.data_ptr(), dtype=dt, n=n, H=H, W=W, C=C, ld=ld)
    L.check(L.lib().dc_im2col_s2(p, L.stream_ptr()), "dc_im2col_s2")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(bits(got[nel:]), bits(torch.full((GUARD,), SENTINEL, dtype=TD[dt]))), "the guard behind the output was written"
    assert torch.equal(bits(got[:nel].view(n, Ho, Wo, 9 * C)), bits(ref))
    assert bool((ref[:, -1, :, 6 * C:] == 0).all()) and bool((ref[:, :, -1, 2 * C:3 * C] == 0).all())      # the padded taps are zeros


# ---- the encoder -------------------------------------------------------------------------------------------------------------------
def random_vae(kw, seed):
    """Default torch initialisation under a fixed seed, GroupNorm affines moved off (1, 0) and q / k scaled up so that the softmax is not
    flat."""
    torch.manual_seed(seed)
    m = VAEEncoder(**kw)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "norm" in name:
                p.add_(0.1 * torch.randn_like(p))
            elif ".to_q.weight" in name or ".to_k.weight" in name:
                p.mul_(2.0)
    return m


def cfg_of(m):
    return dict(vars(m.config))


def per_sample_rel(got, ref):
    """Largest relative L2 over the samples (the measure of tests/test_gpu_clip_model.py, a sample for a prompt)."""
    return max(((got[i].double() - ref[i].double()).norm() / ref[i].double().norm()).item() for i in range(ref.shape[0]))


def model_and_image(name, kw, seed, shape):
    key = (name, shape)
    if key not in _CACHE:
        m = random_vae(kw, seed)
        x = torch.rand(*shape, generator=torch.Generator().manual_seed(seed + 1)) * 2 - 1
        _CACHE[key] = (m, x, {}, cpu_state(m))
    return _CACHE[key]


def cpu_state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def reference(entry, store=None):
    m, x, refs, sd = entry
    if store not in refs:                                                               # computed once, shared, never modified
        refs[store] = vae_encode(sd, cfg_of(m), x, store=store)
    return refs[store]


def plan_kinds(m):
    plan = next(iter(m._plans.values()))
    return plan, [k for k, _, _ in plan.pb.ops]


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (2, 3, 32, 48)], ids=["32x32", "32x48"])
def test_tiny_encoder_against_the_restatement(dt, shape):
    """(64, 128, 256), one layer per block: 32x32 -> 8x8 latents, the mid block attends 64 tokens of 256 channels; 32x48: non-square."""
    entry = model_and_image("tiny", TINY, 21, shape)
    m = entry[0].to(DEV).set_compute_dtype(dt)
    m._plans.clear()
    got = m(entry[1].to(DEV))
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (2, 4, shape[2] // 4, shape[3] // 4)
    got = got.cpu()
    assert torch.isfinite(got).all()
    ref = reference(entry, None)
    r = per_sample_rel(got, ref)
    plan, kinds = plan_kinds(m)
    assert kinds.count(L.OP_ATTENTION_WIDE) == 1 and kinds.count(L.OP_IM2COL_S2) == 2 and kinds.count(L.OP_ATTENTION) == 0
    assert kinds[0] == L.OP_QSAMPLE and kinds[-1] == L.OP_IGEMM
    variants = {mt["variant"] for k, mt in zip(kinds, plan.pb.meta) if k == L.OP_ATTENTION_WIDE}
    assert variants == ({"fp32"} if dt == "f32" else {"wide"})
    assert not any(mt.get("pn") for mt in plan.pb.meta)                                 # the producer-side GroupNorm hand-off is never claimed
    bar = 1e-4 if dt == "f32" else 2e-2
    print(f"tiny VAE encoder {dt} {shape[2]}x{shape[3]}: largest per-sample rel-L2 {r:.2e} (bound {bar:g}), {len(kinds)} ops, attention on {variants}")
    assert r < bar, r
    m.to("cpu")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sd_encoder_against_the_restatement(dt):
    """sd_vae_kwargs() at 64x64 -> 8x8 latents: every published channel width, the mid block at d = 512."""
    entry = model_and_image("sd", dca.sd_vae_kwargs(), 31, (1, 3, 64, 64))
    m = entry[0].to(DEV).set_compute_dtype(dt)
    m._plans.clear()
    got = m(entry[1].to(DEV)).cpu()
    assert tuple(got.shape) == (1, 4, 8, 8) and torch.isfinite(got).all()
    r = per_sample_rel(got, reference(entry, None))
    plan, kinds = plan_kinds(m)
    assert kinds.count(L.OP_ATTENTION_WIDE) == 1 and kinds.count(L.OP_IM2COL_S2) == 3
    variants = {mt["variant"] for k, mt in zip(kinds, plan.pb.meta) if k == L.OP_ATTENTION_WIDE}
    assert variants == ({"fp32"} if dt == "f32" else {"wide"})
    bar = 1e-4 if dt == "f32" else 2e-2
    print(f"SD VAE encoder {dt} 64x64: rel-L2 {r:.2e} (bound {bar:g}), {len(kinds)} ops, attention on {variants}")
    assert r < bar, r
    m.to("cpu")


def test_no_quant_conv_with_a_shift_factor():
    kw = dict(TINY, use_quant_conv=False, shift_factor=0.6, scaling_factor=1.5)
    entry = model_and_image("noquant", kw, 41, (2, 3, 32, 32))
    m = entry[0].to(DEV).set_compute_dtype("f32")
    got = m(entry[1].to(DEV)).cpu()
    ref = reference(entry, None)
    r = per_sample_rel(got, ref)
    unshifted = vae_encode(entry[3], dict(cfg_of(m), shift_factor=None), entry[1])
    print(f"tiny VAE encoder f32 without quant_conv, shift 0.6: rel-L2 {r:.2e} (bound 1e-4); ignoring the shift would be {per_sample_rel(unshifted, ref):.2e}")
    assert r < 1e-4, r
    assert per_sample_rel(unshifted, ref) > 1e-2
    m.to("cpu")


def test_mid_block_of_128_channels_takes_dc_attention():
    kw = dict(TINY, block_out_channels=(64, 128))
    entry = model_and_image("mid128", kw, 51, (2, 3, 16, 16))
    m = entry[0].to(DEV).set_compute_dtype("f32")
    got = m(entry[1].to(DEV)).cpu()
    r = per_sample_rel(got, reference(entry, None))
    _, kinds = plan_kinds(m)
    assert kinds.count(L.OP_ATTENTION) == 1 and kinds.count(L.OP_ATTENTION_WIDE) == 0
    assert r < 1e-4, r
    m.to("cpu")


# ---- loading from disk, classify through latents -----------------------------------------------------------------------------------
def write_directory(path, m):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(dict(cfg_of(m), block_out_channels=list(m.config.block_out_channels), down_block_types=list(m.config.down_block_types),
                       _class_name="AutoencoderKL"), fh)
    save_file({k: v.detach().cpu().clone().contiguous() for k, v in m.state_dict().items()}, os.path.join(path, VAEEncoder.WEIGHTS))
    return str(path)


def test_from_directory_gives_the_same_latents_bit_for_bit(tmp_path):
    entry = model_and_image("tiny", TINY, 21, (2, 3, 32, 32))
    m = entry[0].to(DEV).set_compute_dtype("bf16")
    a = m(entry[1].to(DEV))
    m2 = VAEEncoder.from_directory(write_directory(tmp_path / "vae", m)).to(DEV).set_compute_dtype("bf16")
    b = m2(entry[1].to(DEV))
    assert torch.equal(bits(a), bits(b))
    m.to("cpu")


def test_classify_through_latents(tmp_path):
    """Tiny VAE + the small UNet on 4 latent channels at 16x16, 64x64 images, 3 classes, 2 trials, f32: classify(x) is
    classify(encode_latents(x), latents=True) bit for bit; labels equal, and per-cell errors within 1e-4 relative of, the oracle's loop on
    the restatement's latents."""
    vae = random_vae(TINY, 61)
    path = write_directory(tmp_path / "vae", vae)
    kw = dict(dca.small_unet_kwargs(), in_channels=4, out_channels=4, sample_size=16)
    cfg = dict(pred_param="eps", schedule="cosine", noise_d=16, image_size=16, cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1,
               encoder_type="nn", classes=3, n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32")
    torch.manual_seed(62)
    dc = dca.DiffusionClassifier(dca.UNetCondition2D(**kw), dca.Config(**dict(cfg, vae_path=path)))
    ob = oracle.OracleUNetCondition2D(**kw)
    ob.load_state_dict(dc.model.state_dict())
    oc = oracle.OracleDiffusionClassifier(ob, oracle.AttrBag(**cfg))
    oc.encoder.load_state_dict(dc.encoder.state_dict())
    BS, T = 2, 2
    x = torch.rand(BS, 3, 64, 64) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 4, 16, 16)
    lat_o = vae_encode(vae.state_dict(), cfg_of(vae), x)
    lab_o, err_o = oc.classify(lat_o, t=t, eps=eps, return_errors=True)
    dc = dc.to(DEV)
    assert dc.vae.compute_dtype == "f32" and dc.vae.encoder.conv_in.weight.is_cuda
    lat = dc.encode_latents(x.to(DEV))
    assert tuple(lat.shape) == (BS, 4, 16, 16) and lat.dtype == torch.float32 and lat.is_cuda
    lab, err = dc.classify(x.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    lab2, err2 = dc.classify(lat, t=t, eps=eps.to(DEV), return_errors=True, latents=True)
    assert torch.equal(bits(err), bits(err2)) and torch.equal(lab.cpu(), lab2.cpu())
    rl = per_sample_rel(lat.cpu(), lat_o)
    rel = ((err - err_o).abs() / err_o.abs()).max().item()
    print(f"classify through latents f32: latents rel-L2 {rl:.2e}, per-cell eps-MSE max rel err {rel:.2e} (bound 1e-4), labels {lab.tolist()}")
    assert rel < 1e-4, rel
    assert lab.cpu().tolist() == lab_o.tolist()
    dc.check_device_errors()
