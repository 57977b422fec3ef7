"""GPU: the AutoencoderKL decoder path — dc_latent_im2col against an fp64 evaluation, VAEDecoder.forward against the plain-torch
restatement (tests/vae_decoder_oracle.py), the plan's routes, chunked decode_latents, and sample / counterfactual with decode=True.

Bars of a whole forward, on the largest per-sample relative L2 against the fp32 restatement on the CPU (the measure of
tests/test_gpu_vae.py): f32 below 1e-4, the project's f32 parity bar.  The 16-bit bar is 1.5 x the largest distance, over the three
seeds SEEDS, between the fp32 restatement and the same restatement rounding every stored tensor to the type (vae_decode(store=...)):
no kernel is involved in it, and two fp32 evaluations that round their stored tensors already land that far apart.  STORE_DISTANCE holds
those distances per case and type as `PYTHONPATH=. python tests/test_gpu_vae_decoder.py`, run from the repository root, prints them (CPU
only); tests/test_vae_decoder_host.py measures the two cheapest cases again.  The first seed of a case is the model the GPU test runs.

dc_latent_im2col's f32 bound, |got - fp64| <= 1e-6 (1 + |fp64|), is met by construction of the inputs and not by luck: with scaling_factor
0.5 (1 / s = 2 exactly), shift 0.25, |z| <= 0.25 and |Q[c, j]| <= 1 / Z every v = 2 z + 0.25 has |v| <= 0.75 and sum_j |Q[c, j] v[j]| <=
0.75, so the fp32 sum of Z products, each with a rounded v, is within (Z + 2) 2^-24 0.75 <= 8.1e-7 of the exact one at Z = 16, and the
final + bias (|u| <= 1.25) adds at most 7.5e-8."""
import json
import os

import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import counterfactual as CF
from diffusion_classifier_amd.nets.vae import VAEDecoder, VAEEncoder
from vae_decoder_oracle import vae_decode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
STORE = {"bf16": torch.bfloat16, "f16": torch.float16}
TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(64, 128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)
ENC_TINY = dict(in_channels=3, latent_channels=4, block_out_channels=(64, 128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)
SENTINEL, GUARD = 7.0, 4096
SEEDS = (71, 72, 73)


def mid(c):
    return dict(TINY, block_out_channels=(64, c))


# name -> (kwargs, latent shape): the tiny architecture square and not, the mid block at every other served width, the published widths
CASES = {"tiny8x8": (TINY, (2, 4, 8, 8)), "tiny8x12": (TINY, (2, 4, 8, 12)), "mid64": (mid(64), (2, 4, 4, 4)), "mid128": (mid(128), (2, 4, 4, 4)),
         "mid512": (mid(512), (2, 4, 4, 4)), "sd8x8": (dca.sd_vae_kwargs(), (1, 4, 8, 8))}
# largest per-sample rel-L2 between vae_decode(store=None) and vae_decode(store=type) for the seeds SEEDS, in their order
STORE_DISTANCE = {
    ("tiny8x8", "bf16"): (1.309e-02, 1.309e-02, 1.326e-02),
    ("tiny8x8", "f16"): (1.587e-03, 1.602e-03, 1.612e-03),
    ("tiny8x12", "bf16"): (1.311e-02, 1.284e-02, 1.321e-02),
    ("tiny8x12", "f16"): (1.622e-03, 1.579e-03, 1.661e-03),
    ("mid64", "bf16"): (7.719e-03, 7.400e-03, 8.061e-03),
    ("mid64", "f16"): (9.624e-04, 9.380e-04, 1.103e-03),
    ("mid128", "bf16"): (7.918e-03, 8.914e-03, 9.119e-03),
    ("mid128", "f16"): (9.620e-04, 1.385e-03, 9.688e-04),
    ("mid512", "bf16"): (9.298e-03, 8.677e-03, 8.285e-03),
    ("mid512", "f16"): (1.137e-03, 1.067e-03, 1.084e-03),
    ("sd8x8", "bf16"): (1.522e-02, 1.743e-02, 1.363e-02),
    ("sd8x8", "f16"): (1.895e-03, 2.159e-03, 1.674e-03),
}
_CACHE = {}


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def random_decoder(kw, seed):
    """Default torch initialisation under a fixed seed, GroupNorm affines moved off (1, 0) and q / k scaled by 2 so that the softmax is
    not flat (tests/test_gpu_vae.py random_vae)."""
    torch.manual_seed(seed)
    m = VAEDecoder(**kw)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "norm" in name:
                p.add_(0.1 * torch.randn_like(p))
            elif ".to_q.weight" in name or ".to_k.weight" in name:
                p.mul_(2.0)
    return m


def latents_of(seed, shape):
    """Unit-variance latents, what a scaled posterior mean looks like."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 1000))


def cfg_of(m):
    return dict(vars(m.config))


def cpu_state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def per_sample_rel(got, ref):
    return max(((got[i].double() - ref[i].double()).norm() / ref[i].double().norm()).item() for i in range(ref.shape[0]))


def entry_of(name):
    """(model, latents, {store: reference}, cpu state dict) of a case under its first seed: built once, shared, never modified."""
    if name not in _CACHE:
        kw, shape = CASES[name]
        m = random_decoder(kw, SEEDS[0])
        _CACHE[name] = (m, latents_of(SEEDS[0], shape), {}, cpu_state(m))
    return _CACHE[name]


def reference(entry, store=None):
    m, z, refs, sd = entry
    if store not in refs:
        refs[store] = vae_decode(sd, cfg_of(m), z, store=store)
    return refs[store]


def run_decoder(name, dt):
    entry = entry_of(name)
    m = entry[0].to(DEV).set_compute_dtype(dt)
    m._plans.clear()
    got = m(entry[1].to(DEV))
    plan = next(iter(m._plans.values()))
    m.to("cpu")
    return entry, got, plan


# ---- dc_latent_im2col --------------------------------------------------------------------------------------------------------------
def ordered(i16):
    """int16 bit patterns of 16-bit floats -> integers in value order (+0 and -0 both 0)."""
    i = i16.to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h, w", [(1, 1), (3, 5), (8, 8), (8, 12)])
@pytest.mark.parametrize("Z", [4, 16])
def test_latent_im2col_against_fp64(Z, h, w, n, dt):
    gen = torch.Generator().manual_seed(Z * 10000 + h * 100 + w * 10 + n)
    u01 = lambda *s: torch.rand(*s, generator=gen)
    z = (u01(n, Z, h, w) - 0.5) * 0.5
    Q = (u01(Z, Z) * 2 - 1) / Z
    b = u01(Z) - 0.5
    inv_s, shift = 2.0, 0.25
    gran = 32 if dt == L.DC_F32 else 64
    Kpad = (9 * Z + gran - 1) // gran * gran
    # fp64: u, then its zero-padded 3x3 patches in (tap, c) order
    u = torch.einsum("cj,njhw->nchw", Q.double(), z.double() * inv_s + shift) + b.double().view(1, Z, 1, 1)
    up = torch.nn.functional.pad(u, (1, 1, 1, 1))
    ref = torch.zeros(n, h, w, Kpad, dtype=torch.float64)
    inside = torch.zeros(n, h, w, Kpad, dtype=torch.bool)
    ones = torch.nn.functional.pad(torch.ones(n, Z, h, w, dtype=torch.bool), (1, 1, 1, 1))
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        ref[..., tap * Z:(tap + 1) * Z] = up[:, :, ky:ky + h, kx:kx + w].permute(0, 2, 3, 1)
        inside[..., tap * Z:(tap + 1) * Z] = ones[:, :, ky:ky + h, kx:kx + w].permute(0, 2, 3, 1)
    # z sits between NaNs: a read outside the tensor poisons the output
    zbuf = torch.full((GUARD + z.numel() + GUARD,), float("nan"))
    zbuf[GUARD:GUARD + z.numel()] = z.reshape(-1)
    zd, Qd, bd = zbuf.to(DEV), Q.to(DEV), b.to(DEV)
    nel = n * h * w * Kpad
    out = torch.full((nel + GUARD,), SENTINEL, dtype=TD[dt], device=DEV)
    p = L.LatentIm2colParams(z=zd.data_ptr() + 4 * GUARD, Q=Qd.data_ptr(), bias=bd.data_ptr(), out=out.data_ptr(), out_dtype=dt, n=n, Z=Z,
                             H=h, W=w, Kpad=Kpad, inv_scale=inv_s, shift=shift)
    L.check(L.lib().dc_latent_im2col(p, L.stream_ptr()), "dc_latent_im2col")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(bits(got[nel:]), bits(torch.full((GUARD,), SENTINEL, dtype=TD[dt]))), "the guard behind the output was written"
    got = got[:nel].view(n, h, w, Kpad)
    assert bool((got[~inside] == 0).all()) and int((~inside).sum()) > 0                  # border taps and pad columns: exact zeros
    assert bool((~inside[..., 9 * Z:]).all()) and bool(inside[:, h // 2, w // 2, 4 * Z:5 * Z].all())
    assert not torch.isnan(got.float()).any()
    if dt == L.DC_F32:
        err = ((got.double() - ref).abs() / (1.0 + ref.abs())).max().item()
        print(f"dc_latent_im2col f32 Z={Z} {h}x{w} n={n}: max |got - fp64| / (1 + |fp64|) = {err:.2e} (bound 1e-6)")
        assert err <= 1e-6, err
    else:
        steps = (ordered(bits(got)) - ordered(bits(ref.to(TD[dt])))).abs().max().item()
        print(f"dc_latent_im2col 16-bit Z={Z} {h}x{w} n={n}: at most {steps} step(s) from the rounded fp64 value (bound 1)")
        assert steps <= 1, steps
    if (Z, h, w, n) == (4, 3, 5, 3):
        # sample 1's rows do not move when the other samples change
        z2 = z.clone()
        z2[0], z2[2] = z2[0] + 0.1, -z2[2]
        zbuf[GUARD:GUARD + z.numel()] = z2.reshape(-1)
        zd.copy_(zbuf)
        L.check(L.lib().dc_latent_im2col(p, L.stream_ptr()), "dc_latent_im2col")
        again = out.cpu()[:nel].view(n, h, w, Kpad)
        assert torch.equal(bits(again[1]), bits(got[1])) and not torch.equal(bits(again[0]), bits(got[0]))
        # bad arguments are refused and nothing is written
        out.fill_(SENTINEL)
        for bad, code in ((dict(Kpad=32), -2), (dict(Z=0), -2), (dict(z=None), -1), (dict(Kpad=Kpad + 8), -2)):
            q = L.LatentIm2colParams(**dict({f: getattr(p, f) for f, _ in L.LatentIm2colParams._fields_}, **bad))
            assert L.lib().dc_latent_im2col(q, L.stream_ptr()) == code, bad
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())


# ---- the decoder -------------------------------------------------------------------------------------------------------------------
def bar_of(name, dt):
    return 1e-4 if dt == "f32" else 1.5 * max(STORE_DISTANCE[(name, dt)])


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", list(CASES))
def test_decoder_against_the_restatement(name, dt):
    entry, got, plan = run_decoder(name, dt)
    z = entry[1]
    f = entry[0].upscale
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (z.shape[0], 3, f * z.shape[2], f * z.shape[3])
    got = got.cpu()
    r = per_sample_rel(got, reference(entry, None))
    bar = bar_of(name, dt)
    print(f"VAE decoder {name} {dt}: largest per-sample rel-L2 {r:.3e} (bar {bar:.3e}), {len(plan.pb.ops)} ops")
    assert torch.isfinite(got).all()
    assert r < bar, (r, bar)


@pytest.mark.parametrize("name", ["tiny8x8", "tiny8x12", "mid64", "mid128", "mid512", "sd8x8"])
def test_plan_shape(name):
    """No op is invalid; the head is dc_latent_im2col + a 1x1 GEMM, the tail an fp32 conv on the 32-wide tile; upsamplers run the
    four-phase form at the power-of-two shapes and the plain upsample route at 8x12; attention by width."""
    entry, _, plan = run_decoder(name, "bf16")
    pb = plan.pb
    kinds = [k for k, _, _ in pb.ops]
    assert not any(mt.get("variant") == "invalid" or mt["family"] == "invalid" for mt in pb.meta)
    assert kinds[0] == L.OP_LATENT_IM2COL and kinds[1] == L.OP_IGEMM and pb.ops[1][2]["taps"] == 1 and pb.ops[1][2]["C0"] == 64
    assert kinds.count(L.OP_LATENT_IM2COL) == 1 and kinds.count(L.OP_QSAMPLE) == 0 and kinds.count(L.OP_IM2COL_S2) == 0
    tail = pb.ops[-1][2]
    assert kinds[-1] == L.OP_IGEMM and kinds[-2] == L.OP_GROUPNORM and tail["taps"] == 9 and tail["out_dtype"] == L.DC_F32 and tail["tile_n"] == 32
    assert not any(mt.get("pn") for mt in pb.meta)
    ups = [f for (k, _, f), mt in zip(pb.ops, pb.meta) if k == L.OP_IGEMM and mt["name"].endswith("upsamplers.0.conv")]
    assert len(ups) == len(entry[0].config.block_out_channels) - 1 and all(f["upsample"] == 1 and f["taps"] == 9 for f in ups)
    assert [bool(f.get("up4")) for f in ups] == [name != "tiny8x12"] * len(ups), name
    wide = entry[0].config.block_out_channels[-1] > 128
    assert kinds.count(L.OP_ATTENTION_WIDE) == int(wide) and kinds.count(L.OP_ATTENTION) == int(not wide)
    if wide:
        assert {mt["variant"] for k, mt in zip(kinds, pb.meta) if k == L.OP_ATTENTION_WIDE} == {"wide"}


def test_no_post_quant_conv_with_a_shift_factor():
    kw = dict(TINY, use_post_quant_conv=False, shift_factor=0.6, scaling_factor=1.5)
    m = random_decoder(kw, 91)
    z = latents_of(91, (2, 4, 8, 8))
    ref = vae_decode(cpu_state(m), cfg_of(m), z)
    unshifted = vae_decode(cpu_state(m), dict(cfg_of(m), shift_factor=None), z)
    got = m.to(DEV).set_compute_dtype("f32")(z.to(DEV)).cpu()
    r = per_sample_rel(got, ref)
    print(f"tiny VAE decoder f32 without post_quant_conv, shift 0.6: rel-L2 {r:.2e} (bound 1e-4); ignoring the shift would be {per_sample_rel(unshifted, ref):.2e}")
    assert r < 1e-4 and per_sample_rel(unshifted, ref) > 1e-2


# ---- the classifier's surface ------------------------------------------------------------------------------------------------------
def write_directory(path, dec, enc):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    cfg = dict(cfg_of(enc), **cfg_of(dec))
    for k in ("block_out_channels", "down_block_types", "up_block_types"):
        cfg[k] = list(cfg[k])
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(dict(cfg, _class_name="AutoencoderKL"), fh)
    sd = dict(enc.state_dict(), **dec.state_dict())
    save_file({k: v.detach().cpu().clone().contiguous() for k, v in sd.items()}, os.path.join(path, VAEDecoder.WEIGHTS))
    return str(path)


@pytest.fixture(scope="module")
def latent_dc(tmp_path_factory):
    """The small UNet on 4 latent channels at 8x8 behind the tiny VAE (32x32 images), f32, 3 classes, 2 sampling steps."""
    dec = random_decoder(TINY, 81)
    torch.manual_seed(82)
    enc = VAEEncoder(**ENC_TINY)
    path = write_directory(tmp_path_factory.mktemp("vae"), dec, enc)
    kw = dict(dca.small_unet_kwargs(), in_channels=4, out_channels=4, sample_size=8)
    cfg = dict(pred_param="v", schedule="cosine", noise_d=8, image_size=8, cfg_w=1.5, ema_beta=0.999, ema_warmup=0, ema_update_freq=1,
               encoder_type="nn", classes=3, n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32",
               sampling_steps=2, vae_path=path)
    torch.manual_seed(83)
    dc = dca.DiffusionClassifier(dca.UNetCondition2D(**kw), dca.Config(**cfg)).to(DEV)
    return dc, dec


def test_decode_latents_is_deterministic_chunked_and_the_decoder(latent_dc):
    dc, dec = latent_dc
    z = latents_of(5, (3, 4, 8, 8)).to(DEV)
    keys = set(dc.state_dict())
    a = dc.decode_latents(z)
    b = dc.decode_latents(z)
    assert tuple(a.shape) == (3, 3, 32, 32) and a.dtype == torch.float32 and a.is_cuda and torch.equal(bits(a), bits(b))
    assert set(dc.state_dict()) == keys and dc._vae_decoder.compute_dtype == dc.vae.compute_dtype == "f32"
    ref = vae_decode(cpu_state(dec), cfg_of(dec), z.cpu())
    assert per_sample_rel(a.cpu(), ref) < 1e-4
    dc.config.vae_decode_batch = 2
    c = dc.decode_latents(z)
    dc.config.vae_decode_batch = None
    assert sorted(k[0] for k in dc._vae_decoder._plans) == [1, 2, 3]                    # one plan per chunk size
    r = per_sample_rel(c.cpu(), a.cpu())
    print(f"decode_latents: 3 images in chunks of 2 against one chunk of 3, rel-L2 {r:.2e} (bound 1e-4)")
    assert torch.isfinite(c).all() and r < 1e-4


def test_encode_then_decode(latent_dc):
    dc, _ = latent_dc
    x = (torch.rand(2, 3, 32, 48, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(DEV)
    lat = dc.encode_latents(x)
    img = dc.decode_latents(lat)
    assert tuple(lat.shape) == (2, 4, 8, 12) and tuple(img.shape) == (2, 3, 32, 48) and torch.isfinite(img).all()


def test_sample_decode_is_decode_latents_of_sample(latent_dc):
    dc, _ = latent_dc
    x = latents_of(6, (2, 4, 8, 8)).to(DEV)
    text = torch.tensor([2, 0]).to(DEV)
    torch.manual_seed(17)
    lat = dc.sample(x, text, from_t=0.7)
    torch.manual_seed(17)
    lat2 = dc.sample(x, text, from_t=0.7, decode=False)
    torch.manual_seed(17)
    img = dc.sample(x, text, from_t=0.7, decode=True)
    assert tuple(lat.shape) == (2, 4, 8, 8) and torch.equal(bits(lat), bits(lat2))
    assert tuple(img.shape) == (2, 3, 32, 32) and torch.equal(bits(img), bits(dc.decode_latents(lat)))


def test_counterfactual_decode(latent_dc):
    dc, _ = latent_dc
    x = latents_of(7, (2, 4, 8, 8)).to(DEV)
    cl = torch.tensor([[1, 2, 0], [0, 2, 1]])
    for against in ("input", torch.tensor([2, 1])):
        torch.manual_seed(19)
        plain = dc.counterfactual(x, cl, 0.7, against=against)
        torch.manual_seed(19)
        same = dc.counterfactual(x, cl, 0.7, against=against, decode=False)
        torch.manual_seed(19)
        cf = dc.counterfactual(x, cl, 0.7, against=against, decode=True)
        assert torch.equal(bits(plain.samples), bits(same.samples)) and torch.equal(bits(plain.maps), bits(same.maps))
        assert tuple(plain.samples.shape) == (2, 3, 4, 8, 8) and tuple(plain.maps.shape) == (2, 3, 8, 8)
        assert tuple(cf.samples.shape) == (2, 3, 3, 32, 32) and tuple(cf.maps.shape) == (2, 3, 32, 32) and torch.equal(cf.classes, plain.classes)
        flat = dc.decode_latents(plain.samples.reshape(6, 4, 8, 8))
        assert torch.equal(bits(cf.samples.reshape(6, 3, 32, 32)), bits(flat))
        if isinstance(against, str):
            base, rows = dc.decode_latents(x), torch.arange(2).repeat_interleave(3)
        else:
            base, rows = flat, CF.base_rows(against, cl)
        want = CF.abs_diff_map_torch(flat, base, rows)                                  # the ascending fp32 channel sum
        assert torch.equal(bits(cf.maps.reshape(6, 32, 32)), bits(want))
        if not isinstance(against, str):
            assert bool((cf.maps[0, 1] == 0).all()) and bool((cf.maps[1, 2] == 0).all()) and float(cf.maps[0, 0].max()) > 0


def test_one_output_channel_returns_tensors_of_their_own(tmp_path):
    """out_channels = 1 (a grayscale VAE): the plan's NHWC output permuted to NCHW already counts as contiguous, so a result that was not
    copied out of the plan would be overwritten by the next run.  Two decodes of different latents keep their values; five images in
    chunks of two (two chunks share one plan) each equal the restatement; and the decoder follows a later change of the VAE's dtype."""
    kw = dict(TINY, out_channels=1, block_out_channels=(64, 128))
    dec = random_decoder(kw, 95)
    sd, cfg = cpu_state(dec), cfg_of(dec)
    z = latents_of(95, (5, 4, 8, 8))
    ref = vae_decode(sd, cfg, z)
    m = dec.to(DEV).set_compute_dtype("f32")
    a = m(z[:2].to(DEV))
    keep = a.clone()
    b = m(z[2:4].to(DEV))                                                               # the same plan again
    assert tuple(a.shape) == (2, 1, 16, 16) and a.is_contiguous() and a.data_ptr() != b.data_ptr()
    assert torch.equal(bits(a), bits(keep)) and not torch.equal(bits(a), bits(b))
    assert per_sample_rel(a.cpu(), ref[:2]) < 1e-4 and per_sample_rel(b.cpu(), ref[2:4]) < 1e-4
    m.to("cpu")
    torch.manual_seed(96)
    enc = VAEEncoder(**dict(ENC_TINY, in_channels=1, block_out_channels=(64, 128)))
    path = write_directory(tmp_path / "gray", dec, enc)
    unet = dict(dca.small_unet_kwargs(), in_channels=4, out_channels=4, sample_size=8)
    cfg_dc = dict(pred_param="v", schedule="cosine", noise_d=8, image_size=8, cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1,
                  encoder_type="nn", classes=3, n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32",
                  sampling_steps=2, vae_path=path, vae_decode_batch=2)
    dc = dca.DiffusionClassifier(dca.UNetCondition2D(**unet), dca.Config(**cfg_dc)).to(DEV)
    img = dc.decode_latents(z.to(DEV))
    assert tuple(img.shape) == (5, 1, 16, 16) and sorted(k[0] for k in dc._vae_decoder._plans) == [1, 2]
    worst = max(per_sample_rel(img[i:i + 1].cpu(), ref[i:i + 1]) for i in range(5))
    print(f"grayscale decoder f32, 5 images in chunks of 2: largest per-sample rel-L2 {worst:.2e} (bound 1e-4)")
    assert worst < 1e-4
    # against="input" with one class per image: base and samples are two decodes through one plan, and must not be one buffer
    torch.manual_seed(97)
    cf = dc.counterfactual(z[:2].to(DEV), torch.tensor([1]), 0.7, decode=True)
    assert tuple(cf.maps.shape) == (2, 1, 16, 16) and float(cf.maps.min()) >= 0 and float(cf.maps.max()) > 0
    want = CF.abs_diff_map_torch(cf.samples.reshape(2, 1, 16, 16), dc.decode_latents(z[:2].to(DEV)), torch.arange(2))
    assert torch.equal(bits(cf.maps.reshape(2, 16, 16)), bits(want))
    # the decoder's dtype is the VAE's at every call
    dc.vae.set_compute_dtype("bf16")
    img16 = dc.decode_latents(z.to(DEV))
    assert dc._vae_decoder.compute_dtype == "bf16" and {k[-1] for k in dc._vae_decoder._plans} == {"f32", "bf16"}
    r16 = per_sample_rel(img16.cpu(), ref)
    # another type ran: above the f32 bar, and within 1.5 x the restatement's own storage-rounding distance for this model
    bar16 = 1.5 * per_sample_rel(vae_decode(sd, cfg, z, store=torch.bfloat16), ref)
    print(f"grayscale decoder bf16 after set_compute_dtype: rel-L2 {r16:.2e} (bar {bar16:.2e})")
    assert 1e-4 < r16 < bar16, (r16, bar16)
    dc.vae.set_compute_dtype("f32")
    assert torch.equal(bits(dc.decode_latents(z.to(DEV))), bits(img))


# ---- the storage-rounding distances behind the 16-bit bars (CPU; `python tests/test_gpu_vae_decoder.py`) ----------------------------
if __name__ == "__main__":
    for name, (kw, shape) in CASES.items():
        for dt, store in STORE.items():
            ds = []
            for seed in SEEDS:
                m = random_decoder(kw, seed)
                sd, z = cpu_state(m), latents_of(seed, shape)
                ds.append(per_sample_rel(vae_decode(sd, cfg_of(m), z, store=store), vae_decode(sd, cfg_of(m), z)))
            print(f'    ("{name}", "{dt}"): ({", ".join(f"{d:.3e}" for d in ds)}),', flush=True)
