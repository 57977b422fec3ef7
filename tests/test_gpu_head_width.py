"""GPU: attention heads of any width up to 128 — the flash kernel at head dim 96 (long sequences in 16-bit), zero-padded heads at the op
level (48 / 72 / 80 run at 64 / 96 / 96 with the scale of the true width), and the models that need them end to end against the
oracle: DiT at the reference constructor's defaults (16 heads x 72, DiT-XL/2), UNets with 384- / 640-channel attention levels
(8 heads of 48 / 80) and the CheXpert experiment UNet's 768-channel level beyond 128 tokens."""
import pytest
import torch

import diffusion_classifier_amd as dca
import oracle
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
LOWP = [L.DC_BF16, L.DC_F16]


def relerr(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _ref64(qkv, n, Lq, heads, dh, Cc, d):
    """float64 softmax(q k^T / sqrt(d)) v of the [n, L, ld] rows (q | k | v at columns 0, Cc, 2 Cc; heads of dh channels), on the device."""
    x = qkv.to(DEV).double()
    out = torch.empty(n, Lq, heads * dh, dtype=torch.float64, device=DEV)
    for h in range(heads):
        q, k, v = (x[..., o + h * dh:o + (h + 1) * dh] for o in (0, Cc, 2 * Cc))
        out[..., h * dh:(h + 1) * dh] = torch.softmax(q @ k.transpose(1, 2) * d ** -0.5, -1) @ v
    return out.float().cpu()


def _params(dt, qd, out, n, Lq, heads, dh, Cc, ld, d):
    es = 4 if dt == L.DC_F32 else 2
    return L.AttentionParams(q=qd.data_ptr(), k=qd.data_ptr() + Cc * es, v=qd.data_ptr() + 2 * Cc * es, out=out.data_ptr(), dtype=dt,
                             n=n, L=Lq, heads=heads, d=dh, ld_qkv=ld, ld_out=heads * dh, scale=d ** -0.5)


def _run(dt, qkv, n, Lq, heads, dh, Cc, ld, d=None):
    """dc_attention at head width dh (scale of width d, default dh); returns (output as f32 on the host, kernel name)."""
    qd = qkv.to(TD[dt]).to(DEV)
    out = torch.full((n, Lq, heads * dh), float("nan"), dtype=TD[dt], device=DEV)
    p = _params(dt, qd, out, n, Lq, heads, dh, Cc, ld, dh if d is None else d)
    L.check(L.lib().dc_attention(p, L.stream_ptr()), "attn")
    torch.cuda.synchronize()
    return out.float().cpu(), L.lib().dc_attention_variant(p).decode()


# ------------------------------------------------------------------------------------------------ dc_attention, flash kernel at d = 96
@pytest.mark.parametrize("dt", LOWP)
@pytest.mark.parametrize("Lq", [144, 256, 1000, 1024, 4096])
@pytest.mark.parametrize("heads", [8, 3])
def test_flash_head_dim_96(dt, Lq, heads):
    """L > 128 at d = 96 in 16-bit runs on the flash kernel (blocks of 64 keys, 128 queries per workgroup): 144 / 1000 tokens end in a
    ragged key block and a ragged query block."""
    d = 96
    torch.manual_seed(Lq + heads)
    n = 2 if Lq <= 1024 else 1
    Cc = heads * d
    qkv = torch.randn(n, Lq, 3 * Cc).to(TD[dt]).float()
    got, kern = _run(dt, qkv, n, Lq, heads, d, Cc, 3 * Cc)
    assert kern == "flash"
    assert torch.isfinite(got).all()
    err = (got - _ref64(qkv, n, Lq, heads, d, Cc, d)).abs().max().item()
    assert err < 1.5e-2, err


@pytest.mark.parametrize("dt", LOWP)
@pytest.mark.parametrize("Lq", [256, 1000])
def test_flash_head_dim_96_with_large_logits(dt, Lq):
    d, n, heads = 96, 2, 2
    torch.manual_seed(960 + Lq)
    Cc = heads * d
    qkv = torch.randn(n, Lq, 3 * Cc)
    qkv[..., :2 * Cc] *= 5.0
    qkv = qkv.to(TD[dt]).float()
    lg = qkv[..., :d] @ qkv[..., Cc:Cc + d].transpose(1, 2) * d ** -0.5
    assert lg.amax(-1).max().item() > 60
    got, kern = _run(dt, qkv, n, Lq, heads, d, Cc, 3 * Cc)
    assert kern == "flash" and torch.isfinite(got).all()
    assert (got - _ref64(qkv, n, Lq, heads, d, Cc, d)).abs().max().item() < {L.DC_BF16: 4e-2, L.DC_F16: 6e-3}[dt]


@pytest.mark.parametrize("dt", LOWP)
@pytest.mark.parametrize("Lq", [256, 1000])
def test_flash_head_dim_96_wide_row_stride(dt, Lq):
    """ld_qkv > 3 * heads * d with a NaN gap behind v: the kernel steps by ld and never reads the gap."""
    d, n, heads = 96, 2, 8
    torch.manual_seed(70 + Lq)
    Cc = heads * d
    ld = 3 * Cc + 64
    qkv = torch.randn(n, Lq, ld).to(TD[dt]).float()
    qkv[..., 3 * Cc:] = float("nan")
    got, kern = _run(dt, qkv, n, Lq, heads, d, Cc, ld)
    assert kern == "flash" and torch.isfinite(got).all()
    assert (got - _ref64(qkv[..., :3 * Cc], n, Lq, heads, d, Cc, d)).abs().max().item() < 1.5e-2


def test_attention_variant_routes():
    """dc_attention_variant names the kernel: d = 96 goes to the flash kernel beyond 128 tokens in 16-bit only; everything else keeps
    its route (no wave instance at 96, the whole-sequence kernel up to 128 tokens, fp32 on the exact kernel)."""
    x = torch.zeros(2, 4096, 3 * 8 * 128, device=DEV)

    def variant(dt, Lq, d, heads=8):
        Cc = heads * d
        p = L.AttentionParams(q=x.data_ptr(), k=x.data_ptr() + 2 * Cc, v=x.data_ptr() + 4 * Cc, out=x.data_ptr(), dtype=dt, n=2, L=Lq,
                              heads=heads, d=d, ld_qkv=3 * Cc, ld_out=Cc, scale=d ** -0.5)
        return L.lib().dc_attention_variant(p).decode()

    for dt in LOWP:
        for Lq in (144, 256, 1000, 1024, 4096):
            assert variant(dt, Lq, 96) == "flash"
        for Lq in (16, 32, 64, 128):
            assert variant(dt, Lq, 96) == "mfma"
        assert variant(dt, 100, 96) == "fp32"
        assert variant(dt, 64, 64) == "wave" and variant(dt, 1024, 64) == "flash" and variant(dt, 256, 16) == "fp32"
        assert variant(dt, 256, 80) == "invalid"
    for Lq in (64, 128, 256, 1024):
        assert variant(L.DC_F32, Lq, 96) == "fp32"


@pytest.mark.parametrize("dt", LOWP)
def test_flash_head_dim_96_is_deterministic(dt):
    """Two launches at 1024 tokens give the same bits (a kernel was withdrawn for launch-to-launch differences)."""
    d, n, heads, Lq = 96, 2, 8, 1024
    torch.manual_seed(5)
    Cc = heads * d
    qd = torch.randn(n, Lq, 3 * Cc, device=DEV).to(TD[dt])
    outs = []
    for _ in range(2):
        out = torch.full((n, Lq, Cc), float("nan"), dtype=TD[dt], device=DEV)
        L.check(L.lib().dc_attention(_params(dt, qd, out, n, Lq, heads, d, Cc, 3 * Cc, d), L.stream_ptr()), "attn")
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


# ------------------------------------------------------------------------------------------------ zero-padded heads, op level
@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("d", [48, 72, 80])
@pytest.mark.parametrize("Lq", [64, 256])
def test_padded_heads_equal_true_width(dt, d, Lq):
    """q/k/v of heads of width d, zero-padded per head to dp = padded_head_dim(d) as the packed weights produce them, run at dp with the
    scale d^-1/2: the real columns are the attention at width d, the pad columns exactly 0."""
    dp, heads, n = E.padded_head_dim(d), 4, 2
    torch.manual_seed(d + Lq)
    C, Cp = heads * d, heads * dp
    qkv = torch.randn(n, Lq, 3 * C).to(TD[dt]).float()
    qkv_p = E.pad_head_rows(qkv.reshape(-1, 3 * C).t(), d, dp).t().reshape(n, Lq, 3 * Cp).contiguous()
    got, _ = _run(dt, qkv_p, n, Lq, heads, dp, Cp, 3 * Cp, d=d)
    got = got.reshape(n, Lq, heads, dp)
    assert (got[..., d:] == 0).all()
    ref = _ref64(qkv, n, Lq, heads, d, C, d)
    err = (got[..., :d].reshape(n, Lq, C) - ref).abs().max().item()
    assert err < (2e-5 if dt == L.DC_F32 else 1.5e-2), err


# ------------------------------------------------------------------------------------------------ models
CFG = dict(pred_param="eps", schedule="cosine", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, n_stages=1,
           evaluation_per_stage=[4], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32")


def _randomise_vectors(m):
    """Default inits leave norm affines at (1, 0) and biases tiny: randomise them so a dropped bias or a swapped pair shows."""
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)


def _attention_ops(pb):
    return [(f, mt) for (kind, _, f), mt in zip(pb.ops, pb.meta) if kind == L.OP_ATTENTION]


DIT_XL = dict(num_attention_heads=16, attention_head_dim=72, in_channels=4, num_layers=2, sample_size=32, patch_size=2,
              num_embeds_ada_norm=10)


def _check_dit_plan(pb, lowp):
    ops = _attention_ops(pb)
    assert len(ops) == DIT_XL["num_layers"]
    for f, mt in ops:
        assert f["d"] == 96 and f["heads"] == 16 and f["scale"] == 72 ** -0.5 and f["q"].C == 16 * 96 and f["L"] == 256
        assert mt["variant"] == ("flash" if lowp else "fp32")


def test_dit_xl2_defaults_f32_forward_and_classify():
    """The reference constructor's default heads (16 x 72, D = 1152) at 256 tokens, 2 layers: forward and classify against the oracle."""
    torch.manual_seed(31)
    m = dca.DiT(**DIT_XL)
    _randomise_vectors(m)
    o = oracle.OracleDiT(**DIT_XL)
    o.load_state_dict(m.state_dict())
    N = 2
    x, lam, lab = torch.randn(N, 4, 32, 32), torch.tensor([3.0, -5.0]), torch.tensor([1, 8])
    with torch.no_grad():
        ref = o(x, lam, lab)
    md = m.to(DEV)
    got = md(x.to(DEV), lam.to(DEV), lab.to(DEV)).cpu()
    assert relerr(got, ref) < 2e-5, relerr(got, ref)
    _check_dit_plan(next(iter(md._plans.values())).pb, False)
    cfg = dict(CFG, encoder_type="DiT", classes=3, image_size=32, noise_d=32)
    dc = dca.DiffusionClassifier(m.cpu(), dca.Config(**cfg)).to(DEV)
    oc = oracle.OracleDiffusionClassifier(o, oracle.AttrBag(**cfg))
    BS, T = 2, 4
    xx = torch.rand(BS, 4, 32, 32) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 4, 32, 32)
    ref_l, ref_e = oc.classify(xx, t=t, eps=eps, return_errors=True)
    got_l, got_e = dc.classify(xx.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    assert ((got_e - ref_e).abs() / ref_e).max().item() < 1e-4
    assert got_l.cpu().tolist() == ref_l.tolist()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_dit_xl2_defaults_lowp_forward(dt):
    torch.manual_seed(32)
    m = dca.DiT(**DIT_XL)
    _randomise_vectors(m)
    o = oracle.OracleDiT(**DIT_XL, lowp=True, lowp_dtype=torch.bfloat16 if dt == "bf16" else torch.float16)
    o.load_state_dict(m.state_dict())
    x, lam, lab = torch.randn(2, 4, 32, 32), torch.tensor([2.0, -3.0]), torch.tensor([4, 7])
    with torch.no_grad():
        ref = o(x, lam, lab)
    md = m.to(DEV).set_compute_dtype(dt)
    got = md(x.to(DEV), lam.to(DEV), lab.to(DEV)).cpu()
    assert torch.isfinite(got).all()
    assert relerr(got, ref) < 5e-3, relerr(got, ref)
    _check_dit_plan(next(iter(md._plans.values())).pb, True)


def _unet_kwargs(C):
    """A two-level UNet whose second level (attention, 8 heads) has C channels: 384 -> heads of 48 (run at 64), 640 -> 80 (at 96)."""
    return dict(dca.small_unet_kwargs(), block_out_channels=(128, C), sample_size=32)


def _check_unet_plan(pb, C, dp, lowp):
    ops = _attention_ops(pb)
    assert ops
    for f, mt in ops:
        assert f["heads"] == 8 and f["d"] == dp and f["scale"] == (C // 8) ** -0.5 and f["q"].C == 8 * dp
        if lowp:
            assert mt["variant"] == "flash"        # 16 x 16 = 256 tokens
    assert not any(kind == L.OP_TBLOCK_FRONT for kind, _, _ in pb.ops)


@pytest.mark.parametrize("C,dp", [(384, 64), (640, 96)])
def test_unet_padded_heads_f32_forward_and_classify(C, dp):
    kw = _unet_kwargs(C)
    torch.manual_seed(41)
    m = dca.UNetCondition2D(**kw)
    _randomise_vectors(m)
    o = oracle.OracleUNetCondition2D(**kw)
    o.load_state_dict(m.state_dict())
    torch.manual_seed(42)
    x, lam, emb = torch.randn(1, 3, 32, 32) * 0.5, torch.tensor([0.5]), torch.randn(1, 1, kw["encoder_hid_dim"])
    with torch.no_grad():
        ref = o(x, lam, encoder_hidden_states=emb)
    got = m.to(DEV)(x.to(DEV), lam.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    assert relerr(got, ref) < 1e-4, relerr(got, ref)
    _check_unet_plan(next(iter(m._plans.values())).pb, C, dp, False)
    cfg = dict(CFG, encoder_type="nn", classes=3, image_size=32, noise_d=32, evaluation_per_stage=[1])
    dc = dca.DiffusionClassifier(m.cpu(), dca.Config(**cfg))
    with torch.no_grad():
        dc.encoder.weight.mul_(3.0)
    oc = oracle.OracleDiffusionClassifier(o, oracle.AttrBag(**cfg))
    oc.encoder.load_state_dict(dc.encoder.state_dict())
    torch.manual_seed(43)
    xs = torch.rand(1, 3, 32, 32) * 2 - 1
    t, eps = torch.rand(1, 1), torch.randn(1, 1, 3, 32, 32)
    ref_l, ref_e = oc.classify(xs, t=t, eps=eps, return_errors=True)
    dc = dc.to(DEV)
    got_l, got_e = dc.classify(xs.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    assert ((got_e - ref_e).abs() / ref_e).max().item() < 1e-4
    assert got_l.cpu().tolist() == ref_l.tolist()
    _check_unet_plan(next(iter(dc._score_plans.values()))["plan"].pb, C, dp, False)


@pytest.mark.parametrize("C,dp", [(384, 64), (640, 96)])
def test_unet_padded_heads_bf16_forward(C, dp):
    kw = _unet_kwargs(C)
    torch.manual_seed(51)
    m = dca.UNetCondition2D(**kw)
    _randomise_vectors(m)
    o = oracle.OracleUNetCondition2D(**kw, lowp=True)
    o.load_state_dict(m.state_dict())
    torch.manual_seed(52)
    x, lam, emb = torch.randn(1, 3, 32, 32) * 0.5, torch.tensor([1.0]), torch.randn(1, 1, kw["encoder_hid_dim"])
    with torch.no_grad():
        ref = o(x, lam, encoder_hidden_states=emb)
    m = m.to(DEV).set_compute_dtype("bf16")
    got = m(x.to(DEV), lam.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    assert torch.isfinite(got).all()
    assert relerr(got, ref) < 2e-2, relerr(got, ref)
    _check_unet_plan(next(iter(m._plans.values())).pb, C, dp, True)


def test_chexpert_experiment_unet_bf16_flash_level():
    """experiments/chexpert-unet's UNet (256 / 512 / 768 channels) at sample_size 64: its 768-channel level is 16 x 16 = 256 tokens,
    every attention of that level on the flash kernel at d = 96."""
    kw = dict(dca.chexpert_experiment_unet_kwargs(image_channels=1), sample_size=64)
    torch.manual_seed(61)
    m = dca.UNetCondition2D(**kw)
    _randomise_vectors(m)
    o = oracle.OracleUNetCondition2D(**kw, lowp=True)
    o.load_state_dict(m.state_dict())
    torch.manual_seed(62)
    x, lam, emb = torch.randn(1, 4, 64, 64) * 0.5, torch.tensor([1.0]), torch.randn(1, 1, kw["encoder_hid_dim"])
    with torch.no_grad():
        ref = o(x, lam, encoder_hidden_states=emb)
    m = m.to(DEV).set_compute_dtype("bf16")
    got = m(x.to(DEV), lam.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    assert torch.isfinite(got).all()
    assert relerr(got, ref) < 2e-2, relerr(got, ref)
    ops = [(f, mt) for f, mt in _attention_ops(next(iter(m._plans.values())).pb) if f["q"].C == 768]
    assert len(ops) == 2 + 1 + 3             # down block (2 layers), mid block, up block (3 layers)
    for f, mt in ops:
        assert f["d"] == 96 and f["L"] == 256 and mt["variant"] == "flash"
