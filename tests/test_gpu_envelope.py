"""GPU: the shapes of the reference's remaining UNet backbones (ipmsa-5-dwt-unet, unet-128, unet-256 and the CheXpert / IPMSA
experiment nets) that the BASELINE configurations never reach — attention head dim 96 (768 channels, 8 heads), GroupNorm groups
of 24 / 40 / 48 channels (768 / 32, the concatenated skips 1280 / 32 and 1536 / 32, two-source forms whose seam falls inside a
group), odd input / output channel counts (40 = 4 x 10, 4 = 4 x 1, 12 = 4 x 3) and GEMMs at K = 768 — op by op against a float64
reference of the same op, the gates that must refuse them, and each backbone end to end against the oracle."""
import pytest
import torch
import torch.nn.functional as F

import diffusion_classifier_amd as dca
import oracle
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E
from helpers import hip_preds, pred_rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
ALL = [L.DC_F32, L.DC_BF16, L.DC_F16]


def ptr(t):
    return None if t is None else t.data_ptr()


def maxrel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def relerr(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def nhwc(x, dt):
    return x.permute(0, 2, 3, 1).contiguous().to(TD[dt]).to(DEV)


def run_igemm(**kw):
    L.check(L.lib().dc_igemm(L.IgemmParams(**kw), L.stream_ptr()), "dc_igemm")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ attention, head dim 96
def _attn_ref64(qkv, n, Lq, heads, d, Cc):
    """float64 softmax(q k^T / sqrt(d)) v of the [n, L, ld] rows (q | k | v at columns 0, Cc, 2 Cc), on the device, head by head."""
    x = qkv.to(DEV).double()
    out = torch.empty(n, Lq, Cc, dtype=torch.float64, device=DEV)
    for h in range(heads):
        q, k, v = (x[..., o + h * d:o + (h + 1) * d] for o in (0, Cc, 2 * Cc))
        p = torch.softmax(q @ k.transpose(1, 2) * d ** -0.5, -1)
        out[..., h * d:(h + 1) * d] = p @ v
    return out.float().cpu()


def _run_attention(dt, qkv, n, Lq, heads, d, Cc, ld):
    qd = qkv.to(TD[dt]).to(DEV)
    out = torch.full((n, Lq, Cc), float("nan"), dtype=TD[dt], device=DEV)
    es = 4 if dt == L.DC_F32 else 2
    p = L.AttentionParams(q=qd.data_ptr(), k=qd.data_ptr() + Cc * es, v=qd.data_ptr() + 2 * Cc * es, out=ptr(out), dtype=dt,
                          n=n, L=Lq, heads=heads, d=d, ld_qkv=ld, ld_out=Cc, scale=d ** -0.5)
    L.check(L.lib().dc_attention(p, L.stream_ptr()), "attn")
    torch.cuda.synchronize()
    return out.float().cpu()


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("Lq", [16, 24, 64, 100, 128, 256, 1024, 4096])
@pytest.mark.parametrize("heads", [8, 3])
def test_attention_head_dim_96(dt, Lq, heads):
    """768 channels / 8 heads.  16-bit: L <= 128 with L % 16 == 0 on the whole-sequence matrix-core kernel (3 k-chunks of 32,
    6 output tiles of 16), everything else on the fp32 kernel (24-wide slices, 4 lanes per query) — K / V whole in LDS up to
    213 tokens, streamed in blocks beyond.  heads = 3: a ragged last group of (sample, head) pairs."""
    d = 96
    torch.manual_seed(Lq + heads)
    n = 2 if Lq <= 1024 else 1
    Cc = heads * d
    qkv = torch.randn(n, Lq, 3 * Cc).to(TD[dt]).float()
    ref = _attn_ref64(qkv, n, Lq, heads, d, Cc)
    got = _run_attention(dt, qkv, n, Lq, heads, d, Cc, 3 * Cc)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    assert err < (2e-5 if dt == L.DC_F32 else 1.5e-2), err


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("Lq", [16, 64, 128, 256, 1024, 100])
def test_attention_head_dim_96_with_large_logits(dt, Lq):
    """Peaked rows (logits of 60 and more) at d = 96: every route subtracts the row maximum (style of test_attention_with_large_logits)."""
    d, n, heads = 96, 2, 2
    torch.manual_seed(96 + Lq)
    Cc = heads * d
    qkv = torch.randn(n, Lq, 3 * Cc)
    qkv[..., :2 * Cc] *= 5.0
    qkv = qkv.to(TD[dt]).float()
    ref = _attn_ref64(qkv, n, Lq, heads, d, Cc)
    lg = qkv[..., :d] @ qkv[..., Cc:Cc + d].transpose(1, 2) * d ** -0.5
    assert lg.amax(-1).max().item() > 60
    got = _run_attention(dt, qkv, n, Lq, heads, d, Cc, 3 * Cc)
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() < {L.DC_F32: 2e-4, L.DC_BF16: 4e-2, L.DC_F16: 6e-3}[dt]


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("Lq", [64, 100, 256])
def test_attention_head_dim_96_wide_row_stride(dt, Lq):
    """q / k / v rows with ld_qkv > 3 * heads * d (a 64-element gap behind v): the kernels must step by ld, not by 3 C."""
    d, n, heads = 96, 2, 8
    torch.manual_seed(7 + Lq)
    Cc = heads * d
    ld = 3 * Cc + 64
    qkv = torch.randn(n, Lq, ld).to(TD[dt]).float()
    qkv[..., 3 * Cc:] = float("nan")                      # the gap is never read
    ref = _attn_ref64(qkv[..., :3 * Cc], n, Lq, heads, d, Cc)
    got = _run_attention(dt, qkv, n, Lq, heads, d, Cc, ld)
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() < (2e-5 if dt == L.DC_F32 else 1.5e-2)


def test_attention_rejects_other_head_dims():
    x = torch.zeros(1, 16, 3 * 80, device=DEV)
    for d in (48, 80, 160):
        p = L.AttentionParams(q=ptr(x), k=ptr(x), v=ptr(x), out=ptr(x), dtype=L.DC_F32, n=1, L=16, heads=1, d=d, ld_qkv=3 * 80,
                              ld_out=80, scale=1.0)
        assert L.lib().dc_attention(p, L.stream_ptr()) == -2 and b"head dim" in L.lib().dc_last_error()


# ------------------------------------------------------------------------------------------------ GroupNorm, 24 / 40 / 48 per group
GN_WIDE = {"c768_cpg24": (768, 0, 32), "c1280_cpg40": (1280, 0, 32), "c1536_cpg48": (1536, 0, 32),
           "c512+256_cpg24": (512, 256, 32), "c768+512_cpg40": (768, 512, 32), "c1024+512_cpg48": (1024, 512, 32)}


def _gn_ref64(x, groups, gamma, beta, silu, eps=1e-5):
    """x [n, HW, C] -> float64 GroupNorm (+SiLU) in the same layout."""
    n, HW, C = x.shape
    y = F.group_norm(x.double().permute(0, 2, 1), groups, gamma.double(), beta.double(), eps).permute(0, 2, 1)
    return F.silu(y) if silu else y


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16])
@pytest.mark.parametrize("hw", [8, 16, 32])
@pytest.mark.parametrize("case", list(GN_WIDE))
def test_groupnorm_wide_groups(dt, hw, case):
    """The sweep kernel at 24 / 40 / 48 channels per group, single source and two sources whose seam falls inside a group
    (512 | 256 with 24 per group: the seam splits group 21), plus the statistics-only form (per-channel scale / shift of the fused
    conv prologue) against float64."""
    C0, C1, groups = GN_WIDE[case]
    torch.manual_seed(hw + C0 + C1)
    n, HW, Cc = 3, hw * hw, C0 + C1
    q = lambda t: t.to(TD[dt]).float()
    x0 = q(torch.randn(n, HW, C0) * 2 + 0.5)
    x1 = q(torch.randn(2, HW, C1) - 0.3) if C1 else None
    m1 = torch.tensor([1, 0, 1], dtype=torch.int32)
    xcat = torch.cat([x0, x1[m1.long()]], -1) if C1 else x0
    gamma, beta = torch.randn(Cc), torch.randn(Cc)
    lib = L.lib()
    splits = lib.dc_groupnorm_splits(n, HW, Cc)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n, groups, splits), device=DEV)
    x0d, x1d, m1d = x0.to(TD[dt]).to(DEV), (x1.to(TD[dt]).to(DEV) if C1 else None), m1.to(DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    y = torch.full((n, HW, Cc), float("nan"), dtype=TD[dt], device=DEV)
    sc, sh = torch.full((n, Cc), float("nan"), device=DEV), torch.full((n, Cc), float("nan"), device=DEV)
    gk = dict(x=ptr(x0d), x1=ptr(x1d), map1=ptr(m1d) if C1 else None, dtype=dt, out_dtype=dt, n=n, HW=HW, C=C0, C1=C1, groups=groups,
              splits=splits, eps=1e-5, gamma=ptr(gd), beta=ptr(bd), ws=ptr(ws))
    # the sweep kernels: one workgroup per sample up to 4 MiB, the split sweep beyond (fp32 at 32x32 from 1280 channels on)
    sweep = "image" if HW * Cc * (4 if dt == L.DC_F32 else 2) <= 4 << 20 else "stats+apply"
    assert lib.dc_groupnorm_variant(L.GroupnormParams(y=ptr(y), silu=1, **gk)).decode() == sweep
    assert lib.dc_groupnorm_variant(L.GroupnormParams(y=None, silu=0, out_scale=ptr(sc), out_shift=ptr(sh), **gk)) == b"stats"
    L.check(lib.dc_groupnorm(L.GroupnormParams(y=ptr(y), silu=1, **gk), L.stream_ptr()), "gn")
    L.check(lib.dc_groupnorm(L.GroupnormParams(y=None, silu=0, out_scale=ptr(sc), out_shift=ptr(sh), **gk), L.stream_ptr()), "gn stats")
    torch.cuda.synchronize()
    ref = _gn_ref64(xcat, groups, gamma, beta, True)
    err = (y.float().cpu().double() - ref).abs().max().item()
    assert err < (2e-4 if dt == L.DC_F32 else 6e-2), err       # outputs are O(1..8); bf16 rounding 2^-8 relative
    # scale / shift: GroupNorm(x) = x * scale + shift per (sample, channel)
    xg = xcat.double().view(n, HW, groups, Cc // groups)
    mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
    rstd = (var + 1e-5).rsqrt().repeat_interleave(Cc // groups, 1)
    sc_ref = rstd * gamma.double()
    sh_ref = beta.double() - mean.repeat_interleave(Cc // groups, 1) * sc_ref
    assert maxrel(sc.cpu(), sc_ref) < 2e-5 and (sh.cpu().double() - sh_ref).abs().max().item() < 1e-4 * max(1.0, sh_ref.abs().max().item())


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("hw", [8, 16, 32])
@pytest.mark.parametrize("Cout", [768, 1280, 1536])
def test_groupnorm_from_quad_records_wide_groups(dt, hw, Cout):
    """The quad-record path at 6 / 10 / 12 quads per group: a 3x3 conv writes (mean, M2) per channel quad of its output, the GroupNorm
    folds them (gn_fold_rec / gn_qfold_kernel) instead of sweeping; it must match the sweep and the float64 GroupNorm of the stored
    tensor (style of test_conv3x3_quad_statistics_feed_groupnorm)."""
    torch.manual_seed(Cout + hw)
    n, H, W = 2, hw, hw
    g = E.bke(dt)
    C0 = 2 * g
    q = lambda t: t.to(TD[dt]).float()
    x0 = q(torch.randn(n, C0, H, W))
    w = q(torch.randn(Cout, C0, 3, 3) / (3 * C0 ** 0.5))
    b = (torch.randn(32, 1) + 0.5).expand(32, Cout // 32).reshape(Cout).contiguous()     # a different offset per group
    lib = L.lib()
    a0, bd, Wp = nhwc(x0, dt), b.to(DEV), E.pack_conv3x3(w, dt, DEV)
    out = torch.full((n, H, W, Cout), float("nan"), dtype=TD[dt], device=DEV)
    kw = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=C0, W=ptr(Wp),
              Cout=Cout, tile_n=128, bias=ptr(bd), out=ptr(out), out_dtype=dt, out_ld=Cout)
    parts = lib.dc_igemm_qstats_parts(L.IgemmParams(**kw))
    assert parts == max(1, H * W // 128)
    qs = torch.full((n, parts, Cout // 4, 2), float("nan"), device=DEV)
    run_igemm(qstats=ptr(qs), **kw)
    assert torch.isfinite(qs).all()
    gamma, beta = torch.randn(Cout, device=DEV), torch.randn(Cout, device=DEV)
    splits = lib.dc_groupnorm_splits(n, H * W, Cout)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n, 32, splits), device=DEV)
    ya, yb = torch.empty_like(out), torch.empty_like(out)
    gk = dict(x=ptr(out), dtype=dt, out_dtype=dt, n=n, HW=H * W, C=Cout, C1=0, groups=32, silu=1, splits=splits, eps=1e-5,
              gamma=ptr(gamma), beta=ptr(beta), ws=ptr(ws))
    # the records folded inside gn_image_kernel (gn_fold_rec) below 1 MiB per sample, by gn_qfold_kernel in front of the split apply sweep
    # from there on (96 ... 384 chunks per pixel: no span kernel, whatever DCAMD_GN_SPAN says)
    folded = "image" if H * W * Cout * (4 if dt == L.DC_F32 else 2) < 1 << 20 else "qfold+apply"
    assert lib.dc_groupnorm_variant(L.GroupnormParams(y=ptr(yb), qstats=ptr(qs), qparts=parts, **gk)).decode() == folded
    L.check(lib.dc_groupnorm(L.GroupnormParams(y=ptr(ya), **gk), L.stream_ptr()), "gn")
    L.check(lib.dc_groupnorm(L.GroupnormParams(y=ptr(yb), qstats=ptr(qs), qparts=parts, **gk), L.stream_ptr()), "gn qstats")
    torch.cuda.synchronize()
    of = out.float()
    ref = F.silu(F.group_norm(of.double().permute(0, 3, 1, 2), 32, gamma.double(), beta.double(), 1e-5)).permute(0, 2, 3, 1)
    tol = {L.DC_F32: 2e-5, L.DC_BF16: 1e-2, L.DC_F16: 2e-3}[dt]
    e_q, e_s = maxrel(yb.float(), ref), maxrel(ya.float(), ref)
    print(f"GroupNorm from quad records C={Cout} ({Cout // 128} quads/group) {hw}x{hw} dt={dt}: {e_q:.2e} (sweep {e_s:.2e}, bound {tol:.0e})")
    assert e_q < tol and e_s < tol, (e_q, e_s)
    assert maxrel(yb.float(), ya.float()) < tol


FUSED = {"cpg24": (384, 0, 16), "cpg40": (320, 0, 8), "cpg48": (384, 0, 8), "cpg24_seam": (256, 128, 16)}   # 16-bit convs: C % 64 == 0


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("hw", [8, 16, 32])
@pytest.mark.parametrize("case", list(FUSED))
def test_fused_groupnorm_prologue_wide_groups(dt, hw, case):
    """GroupNorm + SiLU -> 3x3 conv with the normalisation in the conv's loader, at 24 / 40 / 48 channels per group: the affine from
    the producer's quad records (single source) or from the statistics sweep (two sources 256 | 128, the seam inside group 10), then conv3_ws
    (Cout 128) and the thin conv3_halo form (Cout 12, the conv_out of a 3-channel DWT backbone).  The fused prologue holds at most
    512 channels: at 768 and more it must be refused (the engine then takes the GroupNorm pass), as it must below 16x16."""
    C0, C1, groups = FUSED[case]
    torch.manual_seed(hw * 7 + C0 + groups)
    n, H, W = 2, hw, hw
    Cc = C0 + C1
    g = E.bke(dt)
    q = lambda t: t.to(TD[dt]).float()
    lib = L.lib()
    splits = lib.dc_groupnorm_splits(n, H * W, Cc)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n, groups, splits), device=DEV)
    gamma, beta = (torch.randn(Cc) * 0.5 + 1), torch.randn(Cc)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    sc, sh = torch.zeros(n, Cc, device=DEV), torch.zeros(n, Cc, device=DEV)
    gk = dict(dtype=dt, out_dtype=dt, n=n, HW=H * W, C=C0, C1=C1, groups=groups, silu=0, splits=splits, eps=1e-5, gamma=ptr(gd),
              beta=ptr(bd), ws=ptr(ws), out_scale=ptr(sc), out_shift=ptr(sh))
    if C1:
        x0, x1 = q(torch.randn(n, C0, H, W) * 1.5 + 0.3), q(torch.randn(n, C1, H, W) - 0.5)
        a0, a1 = nhwc(x0, dt), nhwc(x1, dt)
        xc = torch.cat([x0, x1], 1)
        L.check(lib.dc_groupnorm(L.GroupnormParams(x=ptr(a0), x1=ptr(a1), y=None, **gk), L.stream_ptr()), "gn stats")
    else:
        # producer: a 3x3 conv (Cout 320 / 384: a ragged last N tile) that writes the quad records of its output
        xp = q(torch.randn(n, 2 * g, H, W))
        wp_ = q(torch.randn(Cc, 2 * g, 3, 3) / (3 * (2 * g) ** 0.5))
        bp_ = (torch.randn(Cc) * 0.5).to(DEV)
        a0 = torch.empty(n, H, W, Cc, dtype=TD[dt], device=DEV)
        pk = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(nhwc(xp, dt)), C0=2 * g,
                  W=ptr(E.pack_conv3x3(wp_, dt, DEV)), Cout=Cc, tile_n=128, bias=ptr(bp_), out=ptr(a0), out_dtype=dt, out_ld=Cc)
        parts = lib.dc_igemm_qstats_parts(L.IgemmParams(**pk))
        assert parts > 0
        qs = torch.zeros(n, parts, Cc // 4, 2, device=DEV)
        run_igemm(qstats=ptr(qs), **pk)
        a1 = None
        xc = a0.float().cpu().permute(0, 3, 1, 2)
        L.check(lib.dc_groupnorm(L.GroupnormParams(x=ptr(a0), y=None, qstats=ptr(qs), qparts=parts, **gk), L.stream_ptr()), "gn affine")
    hn = q(F.silu(F.group_norm(xc.double(), groups, gamma.double(), beta.double(), 1e-5)).float())
    for Co in (128, 12):
        w = q(torch.randn(Co, Cc, 3, 3) / (3 * Cc ** 0.5))
        b = torch.randn(Co)
        ref = F.conv2d(hn.double(), w.double(), b.double(), padding=1).float()
        Wo, bo = E.pack_conv3x3(w, dt, DEV, tile_n=128 if Co > 16 else 32), b.to(DEV)
        odt = dt if Co > 16 else L.DC_F32
        out = torch.full((n, H, W, Co), float("nan"), dtype=TD[odt], device=DEV)
        p = L.IgemmParams(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=C0, src1=ptr(a1), C1=C1,
                          W=ptr(Wo), Cout=Co, tile_n=128 if Co > 16 else 32, bias=ptr(bo), out=ptr(out), out_dtype=odt, out_ld=Co,
                          gn_scale=ptr(sc), gn_shift=ptr(sh), gn_silu=1)
        if hw < 16:
            assert lib.dc_igemm_gn_fusable(p) == 0
            continue
        assert lib.dc_igemm_gn_fusable(p) == 1
        v = lib.dc_igemm_variant(p).decode()
        assert v.startswith("conv3_ws") if Co > 16 else v.startswith("conv3_thin"), v
        L.check(lib.dc_igemm(p, L.stream_ptr()), "fused conv")
        torch.cuda.synchronize()
        got = out.float().cpu().permute(0, 3, 1, 2)
        assert torch.isfinite(got).all()
        e = maxrel(got, ref)
        print(f"fused GroupNorm prologue {case} {hw}x{hw} Cout={Co} ({v}) dt={dt}: {e:.2e}")
        assert e < {L.DC_F32: 3e-5, L.DC_BF16: 1.5e-2, L.DC_F16: 3e-3}[dt], e
    # the real 768 / 1280 / 1536 widths: no fused prologue (the affine table holds 512 channels)
    for Cw in (768, 1280, 1536):
        pw = L.IgemmParams(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=Cw, W=ptr(a0),
                           Cout=128, tile_n=128, out=ptr(a0), out_dtype=dt, out_ld=128, gn_scale=ptr(sc), gn_shift=ptr(sh), gn_silu=1)
        assert lib.dc_igemm_gn_fusable(pw) == 0


# ------------------------------------------------------------------------------------------------ gates that must refuse
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("hw", [8, 16, 32])
@pytest.mark.parametrize("Cout", [768, 1280, 1536])
def test_producer_groupnorm_gate_refuses_wide_groups(dt, hw, Cout):
    """dc_igemm_pn_ok: the producer-side GroupNorm (epi_pn.h) serves groups of 4 / 8 / 16 / 32 channels only — 0 for 24 / 40 / 48,
    and still 1 for the accepted widths at the same conv shape."""
    fake = 1 << 20
    lib = L.lib()
    base = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=4, Hin=hw, Win=hw, Hout=hw, Wout=hw, src0=fake, C0=256, ld0=256, W=fake,
                Cout=Cout, tile_n=128, out=fake, out_dtype=dt, out_ld=Cout, pn_eps=1e-5)
    for cpg in (24, 40, 48):
        if Cout % cpg == 0:
            assert lib.dc_igemm_pn_ok(L.IgemmParams(pn_groups=Cout // cpg, **base)) == 0, cpg
    assert Cout // 32 in (24, 40, 48)
    for cpg in (4, 8, 16, 32):
        assert lib.dc_igemm_pn_ok(L.IgemmParams(pn_groups=Cout // cpg, **base)) == 1, cpg


@pytest.mark.parametrize("dt", [L.DC_BF16, L.DC_F16])
def test_tblock_front_refuses_wide_blocks(dt):
    """dc_tblock_front serves C = 256 only: the 512- and 768-channel transformer blocks take the launch chain."""
    lib = L.lib()
    for C_, heads, ok in ((256, 8, 1), (256, 4, 1), (512, 8, 0), (768, 8, 0)):
        for Lq in (64, 256, 1024):
            p = L.TblockFrontParams(dtype=dt, n=4, L=Lq, C=C_, heads=heads, ldx=C_, ld_out=C_)
            assert lib.dc_tblock_front_ok(p) == (ok if Lq == 64 else 0), (C_, heads, Lq)


# ------------------------------------------------------------------------------------------------ odd channel counts, K = 768 GEMMs
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("Cin,Cout,hw", [(40, 128, 16), (4, 256, 32), (12, 128, 8), (40, 128, 64)])
def test_conv_in_with_odd_input_channels(dt, Cin, Cout, hw):
    """conv_in as the plan runs it: dc_qsample in im2col form (K = 9 Cin, padded to the K granule: 360 -> 384 / 36 -> 64 / 108 -> 128)
    and a 1-tap GEMM, against the float64 3x3 conv of the noised image."""
    torch.manual_seed(Cin + hw)
    n_bj, B = 3, 2
    kin = E.round_up(9 * Cin, E.bke(dt))
    x, eps = torch.rand(B, Cin, hw, hw) * 2 - 1, torch.randn(n_bj, Cin, hw, hw)
    al, sg = torch.rand(n_bj), torch.rand(n_bj)
    img = torch.tensor([1, 0, 1], dtype=torch.int32)
    z = al.view(-1, 1, 1, 1) * x[img.long()] + sg.view(-1, 1, 1, 1) * eps
    w = torch.randn(Cout, Cin, 3, 3) / (3 * Cin ** 0.5)
    b = torch.randn(Cout)
    a = torch.full((n_bj, hw, hw, kin), float("nan"), dtype=TD[dt], device=DEV)
    xd, ed, ald, sgd, imd = x.to(DEV), eps.to(DEV), al.to(DEV), sg.to(DEV), img.to(DEV)
    L.check(L.lib().dc_qsample(L.QsampleParams(x=ptr(xd), eps=ptr(ed), alpha=ptr(ald), sigma=ptr(sgd), img_of_bj=ptr(imd), out=ptr(a),
                                               out_dtype=dt, n_bj=n_bj, C=Cin, H=hw, W=hw, ld=kin, im2col=1), L.stream_ptr()), "qsample")
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all() and (a[..., 9 * Cin:] == 0).all()
    Wp, bd = E.pack_conv3x3(w, dt, DEV, kpad=kin), b.to(DEV)
    out = torch.full((n_bj, hw, hw, Cout), float("nan"), dtype=TD[dt], device=DEV)
    run_igemm(dtype=dt, taps=1, stride=1, upsample=0, n_img=n_bj, Hin=hw, Win=hw, Hout=hw, Wout=hw, src0=ptr(a), C0=kin, W=ptr(Wp),
              Cout=Cout, tile_n=128, bias=ptr(bd), out=ptr(out), out_dtype=dt, out_ld=Cout)
    q = lambda t: t.to(TD[dt]).double()
    ref = F.conv2d(q(z), q(w), b.double(), padding=1).permute(0, 2, 3, 1)
    e = maxrel(out.float().cpu(), ref)
    assert e < {L.DC_F32: 2e-5, L.DC_BF16: 1.5e-2, L.DC_F16: 3e-3}[dt], e


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("Cout,hw", [(40, 16), (40, 32), (40, 8), (4, 16), (12, 32)])
@pytest.mark.parametrize("fuse", [False, True])
def test_conv_out_with_odd_output_channels(dt, Cout, hw, fuse):
    """conv_out of the DWT backbones (128 -> 40: IPMSA-5-DWT; -> 4 / 12: the CheXpert-style nets), fp32 output, with the
    conv_norm_out + SiLU prologue fused (fuse_gn_out: affine from the statistics pass) and without (GroupNorm pass, then the conv)."""
    torch.manual_seed(Cout * hw + fuse)
    n, C0 = 2, 128
    q = lambda t: t.to(TD[dt]).float()
    x = q(torch.randn(n, C0, hw, hw) * 1.5 + 0.2)
    gamma, beta = torch.randn(C0) * 0.5 + 1, torch.randn(C0)
    w = q(torch.randn(Cout, C0, 3, 3) / (3 * C0 ** 0.5))
    b = torch.randn(Cout)
    hn = q(F.silu(F.group_norm(x.double(), 32, gamma.double(), beta.double(), 1e-5)).float())
    ref = F.conv2d(hn.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    lib = L.lib()
    a0 = nhwc(x, dt)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    splits = lib.dc_groupnorm_splits(n, hw * hw, C0)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n, 32, splits), device=DEV)
    tn = 32 if Cout <= 32 else 128
    Wp, bb = E.pack_conv3x3(w, dt, DEV, tile_n=tn), b.to(DEV)
    out = torch.full((n, hw, hw, Cout), float("nan"), device=DEV)
    ck = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=hw, Win=hw, Hout=hw, Wout=hw, C0=C0, W=ptr(Wp), Cout=Cout, tile_n=tn,
              bias=ptr(bb), out=ptr(out), out_dtype=L.DC_F32, out_ld=Cout)
    gk = dict(x=ptr(a0), dtype=dt, out_dtype=dt, n=n, HW=hw * hw, C=C0, C1=0, groups=32, splits=splits, eps=1e-5, gamma=ptr(gd),
              beta=ptr(bd), ws=ptr(ws))
    if fuse:
        sc, sh = torch.zeros(n, C0, device=DEV), torch.zeros(n, C0, device=DEV)
        L.check(lib.dc_groupnorm(L.GroupnormParams(y=None, silu=0, out_scale=ptr(sc), out_shift=ptr(sh), **gk), L.stream_ptr()), "gn stats")
        p = L.IgemmParams(src0=ptr(a0), gn_scale=ptr(sc), gn_shift=ptr(sh), gn_silu=1, **ck)
        if not lib.dc_igemm_gn_fusable(p):
            assert hw < 16, "conv_out of a >= 16x16 image must take the fused prologue"
            return
        L.check(lib.dc_igemm(p, L.stream_ptr()), "fused conv_out")
    else:
        y = torch.empty_like(a0)
        L.check(lib.dc_groupnorm(L.GroupnormParams(y=ptr(y), silu=1, **gk), L.stream_ptr()), "gn")
        L.check(lib.dc_igemm(L.IgemmParams(src0=ptr(y), **ck), L.stream_ptr()), "conv_out")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isfinite(got).all()
    e = maxrel(got, ref)
    assert e < {L.DC_F32: 3e-5, L.DC_BF16: 1.5e-2, L.DC_F16: 3e-3}[dt], e


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("which", ["proj_in", "qkv", "geglu", "geglu_ln", "ff_proj_out"])
@pytest.mark.parametrize("rows", [64, 100])
def test_transformer_gemms_at_768_channels(dt, which, rows):
    """The 1x1 / linear GEMMs of a 768-channel transformer block (3 samples x 64 or 100 tokens: a ragged M): proj_in (+ bias), q/k/v
    (N = 2304), the GEGLU projection 768 -> 2 x 3072 (plain, and behind the row LayerNorm: folded into the GEMM where dc_igemm_ln_ok
    accepts it, else the LayerNorm launch the plan then takes),
    and the feed-forward output folded with proj_out (K = 3072 + 768 over [f | h], bias, residual)."""
    torch.manual_seed(rows + len(which))
    C_, n = 768, 3
    M = n * rows
    q = lambda t: t.to(TD[dt]).float()
    lib = L.lib()
    if which == "ff_proj_out":
        f, h, res = q(torch.randn(M, 4 * C_)), q(torch.randn(M, C_)), q(torch.randn(M, C_))
        w = q(torch.randn(C_, 5 * C_) / (5 * C_) ** 0.5)
        b = torch.randn(C_)
        ref = torch.cat([f, h], 1).double() @ w.double().t() + b.double() + res.double()
        fd, hd, rd = f.to(TD[dt]).to(DEV), h.to(TD[dt]).to(DEV), res.to(TD[dt]).to(DEV)
        out = torch.full((M, C_), float("nan"), dtype=TD[dt], device=DEV)
        run_igemm(dtype=dt, taps=1, stride=1, upsample=0, n_img=n, Hin=rows, Win=1, Hout=rows, Wout=1, src0=ptr(fd), C0=4 * C_, ld0=4 * C_,
                  src1=ptr(hd), C1=C_, ld1=C_, W=ptr(E.pack_matrix(w, dt, DEV)), Cout=C_, tile_n=128, bias=ptr(b.to(DEV)),
                  residual=ptr(rd), res_dtype=dt, res_ld=C_, out=ptr(out), out_dtype=dt, out_ld=C_)
    else:
        x = q(torch.randn(M, C_) * (2.0 if which == "geglu_ln" else 1.0) + (0.3 if which == "geglu_ln" else 0.0))
        Nn = {"proj_in": C_, "qkv": 3 * C_, "geglu": 8 * C_, "geglu_ln": 8 * C_}[which]
        w = q(torch.randn(Nn, C_) / C_ ** 0.5)
        b = torch.randn(Nn) * 0.2 if which != "qkv" else None
        kw = dict(dtype=dt, taps=1, stride=1, upsample=0, n_img=n, Hin=rows, Win=1, Hout=rows, Wout=1, C0=C_, ld0=C_, Cout=Nn, tile_n=128)
        a = x.double()
        xd = x.to(TD[dt]).to(DEV)
        fold = False
        if which == "geglu_ln":
            a = q(F.layer_norm(x.double(), (C_,), eps=1e-5).float()).double()
            fold = bool(lib.dc_igemm_ln_ok(L.IgemmParams(src0=1 << 20, W=1 << 20, out=1 << 20, out_dtype=dt, out_ld=Nn // 2, act=L.ACT_GEGLU,
                                                         ln_eps=1e-5, **kw)))
            if not fold:        # the plan's fallback: a LayerNorm launch, then the plain GEGLU GEMM of the normalised rows
                ones, zeros = torch.ones(C_, device=DEV), torch.zeros(C_, device=DEV)
                xn = torch.full_like(xd, float("nan"))
                L.check(lib.dc_layernorm(L.LayernormParams(x=ptr(xd), y=ptr(xn), dtype=dt, out_dtype=dt, rows=M, C=C_, rows_per_sample=rows,
                                                           mod_ld=0, eps=1e-5, gamma=ptr(ones), beta=ptr(zeros)), L.stream_ptr()), "ln")
                xd = xn
        y = a @ w.double().t() + (b.double() if b is not None else 0)
        if which.startswith("geglu"):
            u, gg = y.chunk(2, dim=-1)
            ref = u * F.gelu(gg)
            perm = E.geglu_perm(Nn // 2)
            Wp, bp, n_out = E.pack_matrix(w[perm], dt, DEV), b[perm].contiguous().to(DEV), Nn // 2
            kw.update(act=L.ACT_GEGLU, ln_eps=1e-5 if fold else 0.0)
        else:
            ref, Wp, bp, n_out = y, E.pack_matrix(w, dt, DEV), (b.to(DEV) if b is not None else None), Nn
        out = torch.full((M, n_out), float("nan"), dtype=TD[dt], device=DEV)
        run_igemm(src0=ptr(xd), W=ptr(Wp), bias=ptr(bp), out=ptr(out), out_dtype=dt, out_ld=n_out, **kw)
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    e = maxrel(got, ref)
    print(f"K=768 GEMM {which}{' (LayerNorm folded)' if which == 'geglu_ln' and fold else ''} rows={rows} dt={dt}: {e:.2e}")
    assert e < {L.DC_F32: 2e-5, L.DC_BF16: 1.2e-2, L.DC_F16: 2e-3}[dt], e


# ------------------------------------------------------------------------------------------------ scoring ops at 10 -> 40 channels
@pytest.mark.parametrize("Cin", [10, 40])
def test_qsample_eps_mse_and_haar_at_ipmsa_channels(Cin):
    """IPMSA images (10 channels; 40 after the Haar DWT): dc_haar_dwt2 / idwt2 round trip and against the float64 Haar transform,
    dc_qsample (plain NHWC) and dc_eps_mse against float64."""
    torch.manual_seed(Cin)
    B, n_bj, H, W = 2, 3, 16, 16
    if Cin == 40:
        x10 = torch.rand(B, 10, 2 * H, 2 * W) * 2 - 1
        dec = dca.wavelet_dec_2(x10.to(DEV))
        assert tuple(dec.shape) == (B, 40, H, W)
        x64 = x10.double()
        a, b_, c, d = x64[..., 0::2, 0::2], x64[..., 0::2, 1::2], x64[..., 1::2, 0::2], x64[..., 1::2, 1::2]
        # channel 4i + (0, 1, 2, 3) = (cA, cH, cV, cD) of input channel i (pywt.dwt2 'haar', oracle/wavelet.py)
        ref = torch.stack([(a + b_ + c + d) / 2, (a + b_ - c - d) / 2, (a - b_ + c - d) / 2, (a - b_ - c + d) / 2], 2).reshape(B, 40, H, W)
        assert (dec.cpu().double() - ref).abs().max().item() < 1e-6
        rt = dca.wavelet_enc_2(dec)
        assert (rt.cpu() - x10).abs().max().item() < 1e-6
        x = dec.cpu().float()
    else:
        x = torch.rand(B, Cin, H, W) * 2 - 1
    eps = torch.randn(n_bj, Cin, H, W)
    al, sg = torch.rand(n_bj) * 0.9 + 0.05, torch.rand(n_bj) * 0.9 + 0.05
    img = torch.tensor([1, 0, 1], dtype=torch.int32)
    z = al.double().view(-1, 1, 1, 1) * x[img.long()].double() + sg.double().view(-1, 1, 1, 1) * eps.double()
    ld = E.round_up(Cin, 8)
    out = torch.full((n_bj, H, W, ld), float("nan"), device=DEV)
    xd, ed, ald, sgd, imd = x.to(DEV), eps.to(DEV), al.to(DEV), sg.to(DEV), img.to(DEV)
    L.check(L.lib().dc_qsample(L.QsampleParams(x=ptr(xd), eps=ptr(ed), alpha=ptr(ald), sigma=ptr(sgd), img_of_bj=ptr(imd), out=ptr(out),
                                               out_dtype=L.DC_F32, n_bj=n_bj, C=Cin, H=H, W=W, ld=ld, im2col=0), L.stream_ptr()), "qsample")
    torch.cuda.synchronize()
    assert (out.cpu()[..., :Cin].double() - z.permute(0, 2, 3, 1)).abs().max().item() < 1e-6
    k = 4
    U = n_bj * k
    bj = (torch.arange(U) // k).to(torch.int32)
    pred = torch.randn(U, Cin, H, W)
    for v in (0, 1):
        a4, s4 = al.double()[bj.long()].view(-1, 1, 1, 1), sg.double()[bj.long()].view(-1, 1, 1, 1)
        e = eps.double()[bj.long()]
        zz = z[bj.long()]
        eh = s4 * zz + a4 * pred.double() if v else pred.double()
        ref = ((eh - e) ** 2).flatten(1).sum(1)
        oi = torch.randperm(U).to(torch.int32)
        o = torch.full((U,), float("nan"), device=DEV)
        t = [t_.to(DEV) for t_ in (pred.permute(0, 2, 3, 1).contiguous(), eps, x, al, sg, bj, img, oi)]
        L.check(L.lib().dc_eps_mse(L.EpsMseParams(pred=ptr(t[0]), eps=ptr(t[1]), x=ptr(t[2]), alpha=ptr(t[3]), sigma=ptr(t[4]),
                                                  bj_of_unit=ptr(t[5]), img_of_bj=ptr(t[6]), out_index=ptr(t[7]), out=ptr(o), n_units=U,
                                                  C=Cin, H=H, W=W, ld=Cin, v_param=v, patch=0), L.stream_ptr()), "mse")
        got = o.cpu()[oi.long()]
        assert maxrel(got, ref) < 5e-6, maxrel(got, ref)


# ------------------------------------------------------------------------------------------------ backbones against the oracle
def _randomise_vectors(m):
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)


BACKBONES = {
    "ipmsa5_dwt": lambda size=128: dict(dca.ipmsa5_dwt_unet_kwargs(), sample_size=size),
    "unet128": lambda size=128: dict(dca.unet128_kwargs(image_channels=3), sample_size=size),
    "unet256": lambda size=128: dict(dca.unet256_kwargs(image_channels=3), sample_size=size),
    "chexpert_exp_c4": lambda size=128: dict(dca.chexpert_experiment_unet_kwargs(image_channels=1), sample_size=size),
    "chexpert_exp_c12": lambda size=128: dict(dca.chexpert_experiment_unet_kwargs(image_channels=3), sample_size=size),
    "ipmsa_exp": lambda size=128: dict(dca.ipmsa_experiment_unet_kwargs(image_channels=10), sample_size=size),
}
REDUCED = {"ipmsa5_dwt": 64, "unet128": 64, "unet256": 128, "chexpert_exp_c4": 64, "chexpert_exp_c12": 64, "ipmsa_exp": 64}
PN_WIDTHS = (4, 8, 16, 32)


def _check_plan(pb, kw):
    """Plan assertions: no producer-side GroupNorm on groups that are not 4 / 8 / 16 / 32 wide; tuple layers_per_block gives the
    expected ResNet counts; every attention of a 768-channel level ran with d = 96 (and none as dc_tblock_front)."""
    names = [mt["name"] for mt in pb.meta]
    for (kind, _, f), mt in zip(pb.ops, pb.meta):
        if mt.get("pn"):
            assert f["Cout"] // f["pn_groups"] in PN_WIDTHS, (mt["name"], f["Cout"], f["pn_groups"])
        if kind == L.OP_ATTENTION:
            assert f["heads"] * f["d"] == f["q"].C and f["heads"] == 8
            if f["q"].C == 768:
                assert f["d"] == 96
        if kind == L.OP_TBLOCK_FRONT:
            assert f["C"] == 256
    lpb = kw["layers_per_block"]
    lpb = (lpb,) * len(kw["block_out_channels"]) if isinstance(lpb, int) else lpb
    for i, nres in enumerate(lpb):
        assert f"down_blocks.{i}.resnets.{nres - 1}.conv1" in names and f"down_blocks.{i}.resnets.{nres}.conv1" not in names
    for i, nres in enumerate(lpb[::-1]):
        assert any(n.startswith(f"up_blocks.{i}.resnets.{nres}.") for n in names)
        assert not any(n.startswith(f"up_blocks.{i}.resnets.{nres + 1}.") for n in names)
    if 768 in kw["block_out_channels"]:
        assert any(k == L.OP_ATTENTION and f["d"] == 96 for k, _, f in pb.ops)


@pytest.mark.parametrize("name", list(BACKBONES))
def test_backbone_forward_bf16(name):
    """One bf16 forward at the backbone's real sample_size (128: the DWT form of a 256 image), N = 1, against the storage-rounded
    oracle and the fp32 oracle (style of test_cfg4_ipmsa_unet_forward_bf16)."""
    kw = BACKBONES[name]()
    torch.manual_seed(71)
    m = dca.UNetCondition2D(**kw)
    _randomise_vectors(m)
    o = oracle.OracleUNetCondition2D(**kw, lowp=True)
    o.load_state_dict(m.state_dict())
    torch.manual_seed(72)
    C_, S = kw["in_channels"], kw["sample_size"]
    x, lam, emb = torch.randn(1, C_, S, S) * 0.5, torch.tensor([1.0]), torch.randn(1, 1, kw["encoder_hid_dim"])
    with torch.no_grad():
        ref = o(x, lam, encoder_hidden_states=emb)
        o.lowp = False
        ref32 = o(x, lam, encoder_hidden_states=emb)
    got = m.to(DEV).set_compute_dtype("bf16")(x.to(DEV), lam.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    assert torch.isfinite(got).all()
    r, r32 = relerr(got, ref), relerr(got, ref32)
    print(f"{name} bf16 forward ({C_}x{S}x{S}) rel-L2: vs storage-rounded oracle {r:.2e}, vs fp32 oracle {r32:.2e}")
    assert r < 2e-2, r
    assert r32 < 2.5e-2, r32
    _check_plan(next(iter(m._plans.values())).pb, kw)


CFG = dict(pred_param="eps", schedule="cosine", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, encoder_type="nn",
           n_stages=1, evaluation_per_stage=[1], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32")


@pytest.mark.parametrize("name", list(BACKBONES))
def test_backbone_f32_forward_and_classify(name):
    """f32 at a reduced sample_size (every level at least 4x4): a forward within 1e-4 relative L2 of the oracle, and a 1-trial,
    3-class classify: per-cell eps-MSE within 1e-4, identical labels, each prediction within 5e-5 (relative L2)."""
    S = REDUCED[name]
    kw = BACKBONES[name](S)
    torch.manual_seed(81)
    m = dca.UNetCondition2D(**kw)
    _randomise_vectors(m)
    o = oracle.OracleUNetCondition2D(**kw)
    o.load_state_dict(m.state_dict())
    C_ = kw["in_channels"]
    torch.manual_seed(82)
    x, lam, emb = torch.randn(1, C_, S, S) * 0.5, torch.tensor([0.5]), torch.randn(1, 1, kw["encoder_hid_dim"])
    with torch.no_grad():
        ref = o(x, lam, encoder_hidden_states=emb)
    got = m.to(DEV).set_compute_dtype("f32")(x.to(DEV), lam.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    r = relerr(got, ref)
    assert r < 1e-4, r
    _check_plan(next(iter(m._plans.values())).pb, kw)
    cfg = dict(CFG, classes=3, image_size=S, noise_d=S)
    m = m.cpu()
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg))
    with torch.no_grad():
        dc.encoder.weight.mul_(3.0)
    oc = oracle.OracleDiffusionClassifier(o, oracle.AttrBag(**cfg))
    oc.encoder.load_state_dict(dc.encoder.state_dict())
    torch.manual_seed(83)
    xs = torch.rand(1, C_, S, S) * 2 - 1
    t, eps = torch.rand(1, 1), torch.randn(1, 1, C_, S, S)
    ref_l, ref_e, ref_p = oc.classify(xs, t=t, eps=eps, return_errors=True, return_preds=True)
    dc = dc.to(DEV)
    got_l, got_e = dc.classify(xs.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    rel = ((got_e - ref_e).abs() / ref_e).max().item()
    pr = pred_rel_l2(hip_preds(dc, 1, 1), ref_p)
    print(f"{name} f32 ({C_}x{S}x{S}) forward rel-L2 {r:.2e}; classify per-cell eps-MSE max rel err {rel:.2e}, predictions rel-L2 {pr:.2e}")
    assert rel < 1e-4, rel
    assert pr < 5e-5, pr
    assert got_l.cpu().tolist() == ref_l.tolist()
    _check_plan(next(iter(dc._score_plans.values()))["plan"].pb, kw)
