"""GPU: every HIP kernel of libdcamd, called through the C-ABI, against a plain PyTorch fp32
reference of the same op on the CPU (and pywt goldens for Haar).  Tolerances are written next
to each check: fp32 kernels must agree to ~1e-5 relative (different summation order only);
bf16/f16 kernels are compared with the SAME rounded inputs and fp32 accumulation, so only the
output rounding (2^-8 bf16, 2^-11 f16) remains."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
TOL = {L.DC_F32: 2e-5, L.DC_BF16: 1.2e-2, L.DC_F16: 2e-3}


def ptr(t):
    return None if t is None else t.data_ptr()


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def maxrel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def nhwc(x, dt):
    return x.permute(0, 2, 3, 1).contiguous().to(TD[dt]).to(DEV)


def run_igemm(**kw):
    p = L.IgemmParams(**kw)
    L.check(L.lib().dc_igemm(p, L.stream_ptr()), "dc_igemm")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("case", ["plain", "stride2", "stride2_tile256", "upsample", "concat", "maps", "small_n", "ragged_m", "side", "side_maps", "thin"])
def test_conv3x3(dt, case, monkeypatch):
    torch.manual_seed(1)
    g = E.bke(dt)
    N, H, W, C0, C1, Cout, stride, up = 3, 8, 8, 2 * g, 0, 128, 1, 0
    tile_n = 128
    if case == "stride2_tile256":           # the 256-row tile of igemm_pipe on a grid that does not fill the chip (the dispatcher would take the 128-row one)
        monkeypatch.setenv("DCAMD_PIPE_CHIP_TILES", "0")
    if case.startswith("stride2"):
        stride = 2
    if case == "upsample":
        up = 1
    if case == "concat":
        C1 = g
    if case == "small_n":
        Cout, tile_n = 3, 32
    if case == "thin":                      # conv_out-like: Cout <= 16 on a >= 16x16 image -> conv3_thin kernel (bias only)
        H, W, Cout, tile_n, C1 = 16, 32, 5, 32, g
    if case == "ragged_m":
        N, H, W, Cout = 5, 6, 10, 200   # M = 300 (not a tile multiple), Cout not a tile multiple
    q = lambda t: t.to(TD[dt]).float()
    x0 = q(torch.randn(N, C0, H, W))
    x1 = q(torch.randn(N, C1, H, W)) if C1 else None
    w = q(torch.randn(Cout, C0 + C1, 3, 3) / (3 * (C0 + C1) ** 0.5))
    b = torch.randn(Cout)
    xin = torch.cat([x0, x1], 1) if C1 else x0
    n_out, map0 = N, None
    if case == "maps":
        n_out = 7
        m = torch.tensor([2, 0, 1, 1, 2, 0, 0], dtype=torch.int32)
        xin = xin[m.long()]
        map0 = m.to(DEV)
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, w, b, stride=stride, padding=1)
    side = None
    if case.startswith("side"):          # 1x1 side source summed into the same output (conv_shortcut folded into conv2)
        C2 = 2 * g
        if case == "side_maps":
            n_out = 5
            m = torch.tensor([1, 1, 0, 2, 0], dtype=torch.int32)
            ref = ref[m.long()]
            map0 = m.to(DEV)
        x2 = q(torch.randn(n_out, C2, H, W))
        w2 = q(torch.randn(Cout, C2) / C2 ** 0.5)
        ref = ref + torch.einsum("nchw,oc->nohw", x2, w2)
        side = (nhwc(x2, dt), E.pack_matrix(w2, dt, DEV), C2)
    Hin, Win = xin.shape[2:]
    Ho, Wo = ref.shape[2:]
    rv = torch.randn(n_out, Cout)
    res = q(torch.randn(n_out, Cout, Ho, Wo))
    if case == "thin":
        rv, res = torch.zeros_like(rv), torch.zeros_like(res)
    ref = ref + rv[:, :, None, None] + res
    Wp = E.pack_conv3x3(w, dt, DEV, tile_n)
    out = torch.full((n_out, Ho, Wo, Cout), float("nan"), dtype=TD[dt], device=DEV)
    a0, a1 = nhwc(x0, dt), (nhwc(x1, dt) if C1 else None)
    bd, rvd, resd = b.to(DEV), rv.to(DEV).contiguous(), nhwc(res, dt)
    run_igemm(dtype=dt, taps=9, stride=stride, upsample=up, n_img=n_out, Hin=Hin, Win=Win, Hout=Ho, Wout=Wo,
              src0=ptr(a0), map0=ptr(map0), C0=C0, ld0=0, src1=ptr(a1), map1=ptr(map0) if C1 else None, C1=C1, ld1=0,
              W=ptr(Wp), Cout=Cout, tile_n=tile_n, bias=ptr(bd), rowvec=None if case == "thin" else ptr(rvd), rowvec_map=None, rowvec_ld=Cout,
              act=L.ACT_NONE, residual=None if case == "thin" else ptr(resd), res_map=None, res_dtype=dt, res_ld=Cout,
              out=ptr(out), out_dtype=dt, out_ld=Cout,
              src2=ptr(side[0]) if side else None, W2=ptr(side[1]) if side else None, C2=side[2] if side else 0, ld2=0)
    got = out.float().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    assert maxrel(got, ref) < TOL[dt], (case, maxrel(got, ref))


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("case", ["plain", "concat", "maps", "side", "ragged_patch", "deep"])
def test_conv3x3_4x4_images_on_mosaic_halo_patches(dt, case):
    """3x3 convs of 4x4 images (cfg2's deepest level: reference nets/unet.py:186-195 at block_out_channels[-1]) run on the halo
    kernel as a mosaic — 32 whole images per 512-pixel patch laid out as an 8x4 grid that shares its zero borders — so every
    input pixel is fetched once per patch instead of once per tap.  Same checks as test_conv3x3."""
    torch.manual_seed(5)
    g = E.bke(dt)
    N, C0, C1, Cout = 40, 2 * g, 0, 128          # 40 images: one full patch of 32 and a ragged one of 8
    if case == "concat":
        C1 = 3 * g
    if case == "ragged_patch":
        N, Cout = 3, 256
    if case == "deep":
        N, C0, C1, Cout = 33, 8 * g, 8 * g, 256   # K = 9 * 1024 (bf16): the up-path ResNets of the 4x4 level
    H = W = 4
    q = lambda t: t.to(TD[dt]).float()
    x0 = q(torch.randn(N, C0, H, W))
    x1 = q(torch.randn(N, C1, H, W)) if C1 else None
    w = q(torch.randn(Cout, C0 + C1, 3, 3) / (3 * (C0 + C1) ** 0.5))
    b = torch.randn(Cout)
    xin = torch.cat([x0, x1], 1) if C1 else x0
    n_out, map0 = N, None
    if case == "maps":
        m = torch.randint(0, N, (77,), dtype=torch.int32)
        n_out, xin, map0 = 77, xin[m.long()], m.to(DEV)
    ref = F.conv2d(xin, w, b, padding=1)
    side = None
    if case == "side":
        C2 = 4 * g
        x2 = q(torch.randn(n_out, C2, H, W))
        w2 = q(torch.randn(Cout, C2) / C2 ** 0.5)
        ref = ref + torch.einsum("nchw,oc->nohw", x2, w2)
        side = (nhwc(x2, dt), E.pack_matrix(w2, dt, DEV), C2)
    rv = torch.randn(n_out, Cout)
    res = q(torch.randn(n_out, Cout, H, W))
    ref = ref + rv[:, :, None, None] + res
    Wp = E.pack_conv3x3(w, dt, DEV)
    out = torch.full((n_out, H, W, Cout), float("nan"), dtype=TD[dt], device=DEV)
    a0, a1 = nhwc(x0, dt), (nhwc(x1, dt) if C1 else None)
    bd, rvd, resd = b.to(DEV), rv.to(DEV).contiguous(), nhwc(res, dt)
    kw = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n_out, Hin=H, Win=W, Hout=H, Wout=W,
              src0=ptr(a0), map0=ptr(map0), C0=C0, ld0=0, src1=ptr(a1), map1=ptr(map0) if C1 else None, C1=C1, ld1=0,
              W=ptr(Wp), Cout=Cout, tile_n=128, bias=ptr(bd), rowvec=ptr(rvd), rowvec_map=None, rowvec_ld=Cout,
              act=L.ACT_NONE, residual=ptr(resd), res_map=None, res_dtype=dt, res_ld=Cout, out=ptr(out), out_dtype=dt, out_ld=Cout,
              src2=ptr(side[0]) if side else None, W2=ptr(side[1]) if side else None, C2=side[2] if side else 0, ld2=0)
    p = L.IgemmParams(**kw)
    if os.environ.get("DCAMD_NO_MOSAIC") is None:
        assert L.lib().dc_igemm_variant(p).decode().startswith("conv3_halo<"), L.lib().dc_igemm_variant(p)
        assert L.lib().dc_igemm_qstats_parts(p) == 0          # no quad statistics from mosaic patches
    run_igemm(**kw)
    got = out.float().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    assert maxrel(got, ref) < TOL[dt], (case, maxrel(got, ref))


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16])
@pytest.mark.parametrize("act", [L.ACT_NONE, L.ACT_SILU, L.ACT_GELU_TANH, L.ACT_GEGLU])
def test_gemm_epilogues(dt, act):
    torch.manual_seed(2)
    g = E.bke(dt)
    rows_per, n, K, Nn = 20, 9, 3 * g, 256
    q = lambda t: t.to(TD[dt]).float()
    a = q(torch.randn(n * rows_per, K))
    w = q(torch.randn(Nn, K) / K ** 0.5)
    b = torch.randn(Nn)
    gate = torch.randn(4, Nn)
    gmap = torch.randint(0, 4, (n,), dtype=torch.int32)
    y = a @ w.t() + b
    if act == L.ACT_SILU:
        y = F.silu(y)
    elif act == L.ACT_GELU_TANH:
        y = F.gelu(y, approximate="tanh")
    if act == L.ACT_GEGLU:
        u, gg = y.chunk(2, dim=-1)
        y = u * F.gelu(gg)
        perm = E.geglu_perm(Nn // 2)
        Wp, bp = E.pack_matrix(w[perm], dt, DEV), b[perm].contiguous().to(DEV)
        n_out = Nn // 2
        gate_d = None
    else:
        y = y * gate[gmap.long()].repeat_interleave(rows_per, 0)
        Wp, bp, n_out = E.pack_matrix(w, dt, DEV), b.to(DEV), Nn
        gate_d = gate.to(DEV).contiguous()
    out = torch.full((n * rows_per, n_out), float("nan"), dtype=torch.float32, device=DEV)
    ad = a.to(TD[dt]).to(DEV)
    gm = gmap.to(DEV)
    run_igemm(dtype=dt, taps=1, stride=1, upsample=0, n_img=n, Hin=rows_per, Win=1, Hout=rows_per, Wout=1,
              src0=ptr(ad), C0=K, ld0=0, C1=0, W=ptr(Wp), Cout=Nn, tile_n=128, bias=ptr(bp), act=act,
              gate=ptr(gate_d), gate_map=ptr(gm) if gate_d is not None else None, gate_ld=Nn,
              out=ptr(out), out_dtype=L.DC_F32, out_ld=n_out)
    assert maxrel(out.cpu(), y) < (2e-5 if dt == L.DC_F32 else 2e-3), maxrel(out.cpu(), y)


@pytest.mark.parametrize("case", ["k256_res_rowvec", "k256_dual_maps_geglu", "k512_tail_f16_f32out", "k128_many_tiles",
                                  "tiny_images_rowvec", "k256_rowln", "k512_rowln_geglu"])
def test_gemm_activation_stationary(case):
    """igemm_xreg (K <= 512, 16-bit, >= 3 N tiles): activation rows held in registers across all N tiles.  Cases cover
    ragged M, two sources with sample maps, residual through a sample map, a row vector whose samples straddle a wave,
    GEGLU, a channel tail (Cout not a multiple of 128) and an fp32 output; the last one must NOT take the kernel."""
    torch.manual_seed(11)
    dt = L.DC_F16 if case == "k512_tail_f16_f32out" else L.DC_BF16
    td = TD[dt]
    q = lambda t: t.to(td).float()
    cfgs = {  # n_out, rows_per (H*W), C0, C1, Nn, act, residual, rowvec, maps, out f32
        "k256_res_rowvec": (7, 80, 256, 0, 512, L.ACT_NONE, True, True, False, False),
        "k256_dual_maps_geglu": (6, 64, 128, 128, 768, L.ACT_GEGLU, False, False, True, False),
        "k512_tail_f16_f32out": (5, 64, 512, 0, 648, L.ACT_NONE, True, False, False, True),
        "k128_many_tiles": (9, 50, 128, 0, 1024, L.ACT_NONE, False, True, False, False),
        "tiny_images_rowvec": (40, 16, 256, 0, 512, L.ACT_NONE, False, True, False, False),
        # ln_eps: the GEMM standardises its input rows itself (LayerNorm folded into the consumer)
        "k256_rowln": (6, 64, 256, 0, 768, L.ACT_NONE, False, False, False, False),
        "k512_rowln_geglu": (5, 16, 512, 0, 1024, L.ACT_GEGLU, False, False, False, False),
    }
    rowln = "rowln" in case
    n_out, HW, C0, C1, Nn, act, use_res, use_rv, use_maps, out32 = cfgs[case]
    n_src = 4 if use_maps else n_out
    x0 = q(torch.randn(n_src, HW, C0))
    x1 = q(torch.randn(n_src, HW, C1)) if C1 else None
    m0 = torch.randint(0, n_src, (n_out,), dtype=torch.int32) if use_maps else None
    m1 = torch.randint(0, n_src, (n_out,), dtype=torch.int32) if (use_maps and C1) else None
    w = q(torch.randn(Nn, C0 + C1) / (C0 + C1) ** 0.5)
    b = torch.randn(Nn)
    a0 = x0[m0.long()] if use_maps else x0
    a = torch.cat([a0, x1[m1.long()] if use_maps else x1], -1) if C1 else a0
    if rowln:
        x0 = q(x0 * 3.0 + 0.5)                                   # a mean and a scale for the kernel to remove
        a = q(F.layer_norm(x0, (C0,), eps=1e-5))                 # what the kernel must feed the MFMAs (rounded like a LayerNorm output)
    y = a.reshape(n_out * HW, -1) @ w.t() + b
    n_ch = Nn
    if act == L.ACT_GEGLU:
        u, gg = y.chunk(2, dim=-1)
        y = u * F.gelu(gg)
        perm = E.geglu_perm(Nn // 2)
        Wp, bp, n_ch = E.pack_matrix(w[perm], dt, DEV), b[perm].contiguous().to(DEV), Nn // 2
    else:
        Wp, bp = E.pack_matrix(w, dt, DEV), b.to(DEV)
    rv = rvm = None
    if use_rv:
        table = torch.randn(5, n_ch)
        rvm = torch.randint(0, 5, (n_out,), dtype=torch.int32)
        y = y + table[rvm.long()].repeat_interleave(HW, 0)
        rv, rvm = table.to(DEV).contiguous(), rvm.to(DEV)
    res = resm = None
    if use_res:
        rsrc = q(torch.randn(3, HW, n_ch))
        rm = torch.randint(0, 3, (n_out,), dtype=torch.int32)
        y = y + rsrc[rm.long()].reshape(n_out * HW, n_ch)
        res, resm = rsrc.to(td).to(DEV), rm.to(DEV)
    odt = L.DC_F32 if out32 else dt
    out = torch.full((n_out * HW, n_ch), float("nan"), dtype=TD[odt], device=DEV)
    d0, d1 = x0.to(td).to(DEV), (x1.to(td).to(DEV) if C1 else None)
    md0, md1 = (m0.to(DEV) if use_maps else None), (m1.to(DEV) if m1 is not None else None)
    kw = dict(dtype=dt, taps=1, stride=1, upsample=0, n_img=n_out, Hin=HW, Win=1, Hout=HW, Wout=1,
              src0=ptr(d0), map0=ptr(md0), C0=C0, ld0=0, src1=ptr(d1), map1=ptr(md1), C1=C1, ld1=0,
              W=ptr(Wp), Cout=Nn, tile_n=128, bias=ptr(bp), act=act, rowvec=ptr(rv), rowvec_map=ptr(rvm), rowvec_ld=n_ch,
              residual=ptr(res), res_map=ptr(resm), res_dtype=dt, res_ld=n_ch, out=ptr(out), out_dtype=odt, out_ld=n_ch,
              ln_eps=1e-5 if rowln else 0.0)
    variant = L.lib().dc_igemm_variant(L.IgemmParams(**kw)).decode()
    assert ("xreg" in variant) == (case != "tiny_images_rowvec"), variant
    run_igemm(**kw)
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    tol = 2e-3 if out32 else TOL[dt]        # fp32 output of 16-bit operands: only the accumulation order differs
    assert maxrel(got, y) < tol, (case, variant, maxrel(got, y))


def test_gemm_strided_source_and_rowvec_map():
    """ld0 > C0 (a column slice of a wider matrix) and an indexed per-sample vector."""
    torch.manual_seed(3)
    n, K, Kfull, Nn = 6, 64, 192, 96
    big = torch.randn(n, Kfull)
    w = torch.randn(Nn, K) / 8
    table = torch.randn(5, Nn)
    idx = torch.tensor([4, 0, 3, 3, 1, 2], dtype=torch.int32)
    ref = big[:, 64:128] @ w.t() + table[idx.long()]
    bigd, td, idd = big.to(DEV), table.to(DEV), idx.to(DEV)
    Wp = E.pack_matrix(w, L.DC_F32, DEV)
    out = torch.zeros(n, Nn, device=DEV)
    run_igemm(dtype=L.DC_F32, taps=1, stride=1, upsample=0, n_img=n, Hin=1, Win=1, Hout=1, Wout=1,
              src0=bigd.data_ptr() + 64 * 4, C0=K, ld0=Kfull, C1=0, W=ptr(Wp), Cout=Nn, tile_n=128,
              rowvec=ptr(td), rowvec_map=ptr(idd), rowvec_ld=Nn, out=ptr(out), out_dtype=L.DC_F32, out_ld=Nn)
    assert maxrel(out.cpu(), ref) < 2e-5


def test_igemm_rejects_bad_arguments():
    lib = L.lib()
    x = torch.zeros(1, 4, 4, 64, device=DEV)
    w = torch.zeros(128, 9 * 48, device=DEV)
    p = L.IgemmParams(dtype=L.DC_F32, taps=9, stride=1, upsample=0, n_img=1, Hin=4, Win=4, Hout=4, Wout=4,
                      src0=ptr(x), C0=48, W=ptr(w), Cout=128, tile_n=128, out=ptr(x), out_dtype=0, out_ld=128)
    assert lib.dc_igemm(p, L.stream_ptr()) == -2 and b"C0" in lib.dc_last_error()
    p.C0 = 64; p.Hout = 5
    assert lib.dc_igemm(p, L.stream_ptr()) == -2


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16])
@pytest.mark.parametrize("shape", [(5, 64, 128, 0, True, "wave", "wave"), (3, 16, 384, 0, False, "image", "wave"), (4, 256, 256, 128, True, "image", "image"),
                                   (2, 4096, 128, 0, True, "image", "image"), (3, 16, 1024, 1024, True, "image", "image"),
                                   # tiny samples: one wave per sample, register resident (gn_wave_kernel) — up to 64 chunks per pixel, so in
                                   # fp32 the 256- and 512-channel ones take one workgroup per sample (gn_image_kernel)
                                   (6, 16, 512, 0, True, "image", "wave"), (7, 16, 256, 256, True, "image", "wave"), (5, 64, 256, 0, False, "image", "wave"),
                                   (9, 10, 64, 0, True, "wave", "wave")])
def test_groupnorm(dt, shape):
    n, HW, C0, C1, silu, route_f32, route_bf16 = shape
    torch.manual_seed(4)
    q = lambda t: t.to(TD[dt]).float()
    Cc = C0 + C1
    x0 = q(torch.randn(n, HW, C0) * 2 + 0.5)
    x1 = q(torch.randn(2, HW, C1)) if C1 else None
    m1 = torch.randint(0, 2, (n,), dtype=torch.int32)
    xcat = torch.cat([x0, x1[m1.long()]], -1) if C1 else x0
    gamma, beta = torch.randn(Cc), torch.randn(Cc)
    ref = F.group_norm(xcat.permute(0, 2, 1).reshape(n, Cc, HW), 32, gamma, beta, 1e-5)
    if silu:
        ref = F.silu(ref)
    ref = ref.permute(0, 2, 1)
    lib = L.lib()
    splits = lib.dc_groupnorm_splits(n, HW, Cc)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n, 32, splits), device=DEV)
    x0d = x0.to(TD[dt]).to(DEV)
    x1d = x1.to(TD[dt]).to(DEV) if C1 else None
    m1d = m1.to(DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    y = torch.full((n, HW, Cc), float("nan"), dtype=TD[dt], device=DEV)
    p = L.GroupnormParams(x=ptr(x0d), map0=None, x1=ptr(x1d), map1=ptr(m1d) if C1 else None, y=ptr(y), dtype=dt, out_dtype=dt,
                          n=n, HW=HW, C=C0, C1=C1, groups=32, silu=int(silu), splits=splits, eps=1e-5,
                          gamma=ptr(gd), beta=ptr(bd), ws=ptr(ws))
    assert lib.dc_groupnorm_variant(p).decode() == (route_f32 if dt == L.DC_F32 else route_bf16)
    L.check(lib.dc_groupnorm(p, L.stream_ptr()), "gn")
    torch.cuda.synchronize()
    err = (y.float().cpu() - ref).abs().max().item()
    assert err < (2e-4 if dt == L.DC_F32 else 6e-2), err     # outputs are O(1..8); bf16 rounding 2^-8 relative


@pytest.mark.parametrize("shape", [(3, 16, 256, 0, "wave"), (2, 64, 128, 128, "image"), (3, 1024, 128, 0, "image"), (2, 4096, 128, 0, "image"),
                                   (2, 65536, 64, 0, "stats+apply")])
def test_groupnorm_with_large_offsets_f32(shape):
    """|mean| >> std: group means of ~1e3 standard deviations.  The sum / sum-of-squares
    form loses the variance to cancellation there (fp32: relative error ~1e-7 * mean^2 / var = 10 %); the (mean, M2) form with
    shifted sums must stay at torch's own accuracy.  Paths: one wave per sample, one workgroup per sample (one and two sources, up
    to 2 MiB), the split sweep on 16 MiB samples."""
    n, HW, C0, C1, route = shape
    torch.manual_seed(44)
    Cc = C0 + C1
    off = (torch.randn(1, 1, 32, 1) * 300 + 1000).expand(1, 1, 32, Cc // 32).reshape(1, 1, Cc)   # one offset of ~1e3 std per GROUP
    xcat = torch.randn(n, HW, Cc) + off
    gamma, beta = torch.randn(Cc), torch.randn(Cc)
    ref = F.silu(F.group_norm(xcat.double().permute(0, 2, 1).reshape(n, Cc, HW), 32, gamma.double(), beta.double(), 1e-5)).permute(0, 2, 1).float()
    lib = L.lib()
    splits = lib.dc_groupnorm_splits(n, HW, Cc)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n, 32, splits), device=DEV)
    x0d = xcat[..., :C0].contiguous().to(DEV)
    x1d = xcat[..., C0:].contiguous().to(DEV) if C1 else None
    gd, bd = gamma.to(DEV), beta.to(DEV)
    y = torch.full((n, HW, Cc), float("nan"), device=DEV)
    p = L.GroupnormParams(x=ptr(x0d), x1=ptr(x1d), y=ptr(y), dtype=L.DC_F32, out_dtype=L.DC_F32, n=n, HW=HW, C=C0, C1=C1, groups=32, silu=1,
                          splits=splits, eps=1e-5, gamma=ptr(gd), beta=ptr(bd), ws=ptr(ws))
    assert lib.dc_groupnorm_variant(p).decode() == route
    L.check(lib.dc_groupnorm(p, L.stream_ptr()), "gn")
    torch.cuda.synchronize()
    err = (y.cpu() - ref).abs().max().item()
    t32 = F.silu(F.group_norm(xcat.permute(0, 2, 1).reshape(n, Cc, HW), 32, gamma, beta, 1e-5)).permute(0, 2, 1)
    err_torch = (t32 - ref).abs().max().item()                       # torch's own fp32 kernel against the fp64 reference
    assert err < max(4 * err_torch, 2e-4), (err, err_torch)


def test_groupnorm_from_producer_statistics_with_large_offsets_f32():
    """The conv's channel records at a large output offset (bias ~ 1e3 x the output's spread): GroupNorm from the records must match
    the fp64 GroupNorm of the stored tensor."""
    torch.manual_seed(45)
    n, H, W, C0, Cout = 2, 32, 32, 32, 128
    x0 = torch.randn(n, C0, H, W)
    w = torch.randn(Cout, C0, 3, 3) / (3 * C0 ** 0.5) * 0.05           # small spread ...
    b = (torch.randn(32, 1) * 20 + 60).expand(32, Cout // 32).reshape(Cout).contiguous()   # ... on a large offset per GROUP
    lib = L.lib()
    a0, bd, Wp = nhwc(x0, L.DC_F32), b.to(DEV), E.pack_conv3x3(w, L.DC_F32, DEV)
    out = torch.empty(n, H, W, Cout, device=DEV)
    kw = dict(dtype=L.DC_F32, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=C0, W=ptr(Wp),
              Cout=Cout, tile_n=128, bias=ptr(bd), out=ptr(out), out_dtype=L.DC_F32, out_ld=Cout)
    parts = lib.dc_igemm_qstats_parts(L.IgemmParams(**kw))
    qs = torch.zeros(n, parts, Cout // 4, 2, device=DEV)
    run_igemm(qstats=ptr(qs), **kw)
    gamma, beta = torch.randn(Cout, device=DEV), torch.randn(Cout, device=DEV)
    splits = lib.dc_groupnorm_splits(n, H * W, Cout)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n, 32, splits), device=DEV)
    y = torch.empty_like(out)
    L.check(lib.dc_groupnorm(L.GroupnormParams(x=ptr(out), y=ptr(y), dtype=L.DC_F32, out_dtype=L.DC_F32, n=n, HW=H * W, C=Cout, C1=0, groups=32,
                                               silu=0, splits=splits, eps=1e-5, gamma=ptr(gamma), beta=ptr(beta), ws=ptr(ws), qstats=ptr(qs),
                                               qparts=parts), L.stream_ptr()), "gn")
    torch.cuda.synchronize()
    o64 = out.double().permute(0, 3, 1, 2)
    ref = F.group_norm(o64, 32, gamma.double(), beta.double(), 1e-5).permute(0, 2, 3, 1).float()
    t32 = F.group_norm(out.permute(0, 3, 1, 2), 32, gamma, beta, 1e-5).permute(0, 2, 3, 1)
    err, err_torch = (y - ref).abs().max().item(), (t32 - ref).abs().max().item()
    assert err < max(4 * err_torch, 2e-4), (err, err_torch)


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("C_", [64, 256, 768, 1024])
def test_layernorm_plain_and_adaln(dt, C_):
    torch.manual_seed(5)
    q = lambda t: t.to(TD[dt]).float()
    n, L_ = 3, 10
    x = q(torch.randn(n * L_, C_) * 3 + 1)
    gamma, beta = torch.randn(C_), torch.randn(C_)
    lib = L.lib()
    xd = x.to(TD[dt]).to(DEV)
    y = torch.empty_like(xd)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    p = L.LayernormParams(x=ptr(xd), y=ptr(y), dtype=dt, out_dtype=dt, rows=n * L_, C=C_, rows_per_sample=L_, mod_ld=0,
                          eps=1e-5, gamma=ptr(gd), beta=ptr(bd))
    chunks = C_ // (4 if dt == L.DC_F32 else 8)      # ln_route: 16-byte chunks per row, and whether two rows fit a 16-bit lane group
    route = "ln" if chunks > 128 else ("ln16" if dt == L.DC_F32 or chunks > 96 else "ln16x2")
    assert lib.dc_layernorm_variant(p).decode() == route
    L.check(lib.dc_layernorm(p, L.stream_ptr()), "ln")
    ref = F.layer_norm(x, (C_,), gamma, beta, 1e-5)
    tol = {L.DC_F32: 2e-5, L.DC_BF16: 5e-2, L.DC_F16: 8e-3}[dt]
    assert (y.float().cpu() - ref).abs().max().item() < tol
    mod = torch.randn(4, 6 * C_)
    mm = torch.tensor([3, 1, 1], dtype=torch.int32)
    modd, mmd = mod.to(DEV), mm.to(DEV)
    p = L.LayernormParams(x=ptr(xd), y=ptr(y), dtype=dt, out_dtype=dt, rows=n * L_, C=C_, rows_per_sample=L_, mod_ld=6 * C_,
                          eps=1e-6, scale=modd.data_ptr() + C_ * 4, shift=modd.data_ptr(), mod_map=ptr(mmd))
    assert lib.dc_layernorm_variant(p).decode() == route
    L.check(lib.dc_layernorm(p, L.stream_ptr()), "ln")
    sel = mod[mm.long()].repeat_interleave(L_, 0)
    ref = F.layer_norm(x, (C_,), eps=1e-6) * (1 + sel[:, C_:2 * C_]) + sel[:, :C_]
    assert (y.float().cpu() - ref).abs().max().item() < 3 * tol


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("Ld", [(64, 32), (16, 64), (256, 64), (64, 128), (100, 16), (64, 64),
                                (48, 32), (32, 64), (16, 128), (24, 32)])       # L <= 64: one wave per (sample, head) pair, masked key / query tiles
def test_attention(dt, Ld):
    Lq, d = Ld
    torch.manual_seed(6)
    n, heads = 2, (3 if Ld == (64, 64) else 4)      # (64, 64): 6 (sample, head) pairs on workgroups of 4 -> a ragged last group
    Cc = heads * d
    q = lambda t: t.to(TD[dt]).float()
    qkv = q(torch.randn(n, Lq, 3 * Cc))
    sh = lambda z: z.view(n, Lq, heads, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(sh(qkv[..., :Cc]), sh(qkv[..., Cc:2 * Cc]), sh(qkv[..., 2 * Cc:]))
    ref = ref.transpose(1, 2).reshape(n, Lq, Cc)
    qd = qkv.to(TD[dt]).to(DEV)
    out = torch.empty(n, Lq, Cc, dtype=TD[dt], device=DEV)
    es = 4 if dt == L.DC_F32 else 2
    p = L.AttentionParams(q=qd.data_ptr(), k=qd.data_ptr() + Cc * es, v=qd.data_ptr() + 2 * Cc * es, out=ptr(out), dtype=dt,
                          n=n, L=Lq, heads=heads, d=d, ld_qkv=3 * Cc, ld_out=Cc, scale=d ** -0.5)
    L.check(L.lib().dc_attention(p, L.stream_ptr()), "attn")
    assert (out.float().cpu() - ref).abs().max().item() < (2e-5 if dt == L.DC_F32 else 1.5e-2)


@pytest.mark.parametrize("dt", [L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("Ld", [(1024, 64), (300, 32), (4096, 64), (130, 128)])
def test_attention_long_sequences_flash(dt, Ld):
    """DiT token counts (1024 = DWT 128^2 / patch 4, 4096 = raw 256^2) and ragged lengths: online-softmax kernel."""
    Lq, d = Ld
    torch.manual_seed(16)
    n, heads = 2, 3
    Cc = heads * d
    qkv = (torch.randn(n, Lq, 3 * Cc) * 1.5).to(TD[dt]).float()
    sh = lambda z: z.view(n, Lq, heads, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(sh(qkv[..., :Cc]), sh(qkv[..., Cc:2 * Cc]), sh(qkv[..., 2 * Cc:]))
    ref = ref.transpose(1, 2).reshape(n, Lq, Cc)
    qd = qkv.to(TD[dt]).to(DEV)
    out = torch.full((n, Lq, Cc), float("nan"), dtype=TD[dt], device=DEV)
    p = L.AttentionParams(q=qd.data_ptr(), k=qd.data_ptr() + Cc * 2, v=qd.data_ptr() + 2 * Cc * 2, out=ptr(out), dtype=dt,
                          n=n, L=Lq, heads=heads, d=d, ld_qkv=3 * Cc, ld_out=Cc, scale=d ** -0.5)
    L.check(L.lib().dc_attention(p, L.stream_ptr()), "attn")
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() < (2e-2 if dt == L.DC_BF16 else 3e-3)   # P and O rounded to 16 bit


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("Ld", [(16, 64), (64, 32), (128, 64), (256, 64), (1024, 64), (100, 16)])
def test_attention_with_large_logits(dt, Ld):
    """Trained attention layers produce peaked rows: logits of +-60 and more after the 1/sqrt(d) scale (random weights stay near +-3).
    exp() of an unshifted logit overflows fp32 at 88 and f16 at 11: every kernel (one wave per pair, whole-sequence, flash, the
    fp32 fallback) must subtract the row maximum — the result has to be finite and equal to torch's, rows that are one-hot included."""
    Lq, d = Ld
    torch.manual_seed(26)
    n, heads = 2, 2
    Cc = heads * d
    q = lambda t: t.to(TD[dt]).float()
    qkv = torch.randn(n, Lq, 3 * Cc)
    qkv[..., :2 * Cc] *= 5.0                        # q.k / sqrt(d) ~ N(0, 25^2): row maxima of 60-100
    qkv = q(qkv)
    sh = lambda z: z.view(n, Lq, heads, d).transpose(1, 2)
    logits = sh(qkv[..., :Cc]) @ sh(qkv[..., Cc:2 * Cc]).transpose(-1, -2) * d ** -0.5
    assert logits.amax(-1).max().item() > 60
    ref = F.scaled_dot_product_attention(sh(qkv[..., :Cc]).double(), sh(qkv[..., Cc:2 * Cc]).double(), sh(qkv[..., 2 * Cc:]).double())
    ref = ref.transpose(1, 2).reshape(n, Lq, Cc).float()
    qd = qkv.to(TD[dt]).to(DEV)
    out = torch.full((n, Lq, Cc), float("nan"), dtype=TD[dt], device=DEV)
    es = 4 if dt == L.DC_F32 else 2
    p = L.AttentionParams(q=qd.data_ptr(), k=qd.data_ptr() + Cc * es, v=qd.data_ptr() + 2 * Cc * es, out=ptr(out), dtype=dt,
                          n=n, L=Lq, heads=heads, d=d, ld_qkv=3 * Cc, ld_out=Cc, scale=d ** -0.5)
    L.check(L.lib().dc_attention(p, L.stream_ptr()), "attn")
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    # a logit error of eps_T * |logit| (the q.k products are exact in fp32, the 16-bit kernels round P and O) moves a weight by that factor
    assert (got - ref).abs().max().item() < {L.DC_F32: 2e-4, L.DC_BF16: 4e-2, L.DC_F16: 6e-3}[dt]


@pytest.mark.parametrize("Ld", [(1024, 64), (4096, 64), (700, 128), (2000, 32)])
def test_attention_f32_long_sequences(Ld):
    """The fp32 parity path at DiT token counts (1024 = DWT 128^2 / patch 4, 4096 = raw 256^2) and ragged lengths: K / V no longer fit
    LDS whole, the exact fp32 kernel streams them in blocks through its online softmax."""
    Lq, d = Ld
    torch.manual_seed(17)
    n, heads = 1, 2
    Cc = heads * d
    qkv = torch.randn(n, Lq, 3 * Cc) * 1.5
    sh = lambda z: z.view(n, Lq, heads, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(sh(qkv[..., :Cc]).double(), sh(qkv[..., Cc:2 * Cc]).double(), sh(qkv[..., 2 * Cc:]).double())
    ref = ref.transpose(1, 2).reshape(n, Lq, Cc).float()
    qd = qkv.to(DEV)
    out = torch.full((n, Lq, Cc), float("nan"), device=DEV)
    p = L.AttentionParams(q=qd.data_ptr(), k=qd.data_ptr() + Cc * 4, v=qd.data_ptr() + 2 * Cc * 4, out=ptr(out), dtype=L.DC_F32,
                          n=n, L=Lq, heads=heads, d=d, ld_qkv=3 * Cc, ld_out=Cc, scale=d ** -0.5)
    L.check(L.lib().dc_attention(p, L.stream_ptr()), "attn")
    got = out.cpu()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() < 5e-5      # outputs are O(1); fp32 running sums over up to 4096 keys


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_qsample_layouts(dt, mode):
    torch.manual_seed(7)
    B, n_bj, Cc, H, W = 3, 5, 3, 8, 8
    x, eps = torch.rand(B, Cc, H, W) * 2 - 1, torch.randn(n_bj, Cc, H, W)
    al, sg = torch.rand(n_bj), torch.rand(n_bj)
    img = torch.tensor([0, 2, 1, 1, 0], dtype=torch.int32)
    z = al.view(-1, 1, 1, 1) * x[img.long()] + sg.view(-1, 1, 1, 1) * eps
    pch = 4
    if mode == 0:
        ld, ref = 64, torch.zeros(n_bj, H, W, 64)
        ref[..., :Cc] = z.permute(0, 2, 3, 1)
    elif mode == 1:
        ld = 64
        cols = F.unfold(z, 3, padding=1).view(n_bj, Cc, 9, H, W)      # [n, c, tap, H, W]
        ref = torch.zeros(n_bj, H, W, ld)
        ref[..., :27] = cols.permute(0, 3, 4, 2, 1).reshape(n_bj, H, W, 27)   # k = tap*C + c
    else:
        ld = 64
        cols = F.unfold(z, pch, stride=pch).view(n_bj, Cc * pch * pch, H // pch, W // pch)   # k = c*p*p + py*p + px
        ref = torch.zeros(n_bj, H // pch, W // pch, ld)
        ref[..., :Cc * pch * pch] = cols.permute(0, 2, 3, 1)
    out = torch.full(ref.shape, float("nan"), dtype=TD[dt], device=DEV)
    xd, ed, ald, sgd, imd = x.to(DEV), eps.to(DEV), al.to(DEV), sg.to(DEV), img.to(DEV)
    p = L.QsampleParams(x=ptr(xd), eps=ptr(ed), alpha=ptr(ald), sigma=ptr(sgd), img_of_bj=ptr(imd), out=ptr(out), out_dtype=dt,
                        n_bj=n_bj, C=Cc, H=H, W=W, ld=ld, im2col=mode, patch=pch)
    L.check(L.lib().dc_qsample(p, L.stream_ptr()), "qsample")
    got = out.float().cpu()
    assert (got - ref).abs().max().item() < (1e-6 if dt == L.DC_F32 else 2e-2)
    if dt == L.DC_F32 and mode == 0:
        assert torch.equal(got[..., :Cc], ref[..., :Cc]) or (got - ref).abs().max().item() < 3e-7


@pytest.mark.parametrize("v", [0, 1])
@pytest.mark.parametrize("patch", [0, 4])
def test_eps_mse(v, patch):
    torch.manual_seed(8)
    B, n_bj, k, Cc, H, W = 2, 3, 4, 3, 8, 8
    U = n_bj * k
    x, eps = torch.rand(B, Cc, H, W) * 2 - 1, torch.randn(n_bj, Cc, H, W)
    al, sg = torch.rand(n_bj) * 0.9 + 0.05, torch.rand(n_bj) * 0.9 + 0.05
    img = torch.tensor([1, 0, 1], dtype=torch.int32)
    bj = (torch.arange(U) // k).to(torch.int32)
    pred = torch.randn(U, Cc, H, W)
    a4, s4 = al[bj.long()].view(-1, 1, 1, 1), sg[bj.long()].view(-1, 1, 1, 1)
    e = eps[bj.long()]
    z = a4 * x[img.long()][bj.long()] + s4 * e
    eh = s4 * z + a4 * pred if v else pred
    ref = torch.norm((eh - e).view(U, -1), dim=1, p=2) ** 2
    if patch:
        g = H // patch
        pd = pred.view(U, Cc, g, patch, g, patch).permute(0, 2, 4, 3, 5, 1).reshape(U, g, g, patch * patch * Cc).contiguous()
        ld = patch * patch * Cc
    else:
        pd = pred.permute(0, 2, 3, 1).contiguous()
        ld = Cc
    oi = torch.randperm(U).to(torch.int32)
    out = torch.full((U,), float("nan"), device=DEV)
    t = [t_.to(DEV) for t_ in (pd, eps, x, al, sg, bj, img, oi)]
    p = L.EpsMseParams(pred=ptr(t[0]), eps=ptr(t[1]), x=ptr(t[2]), alpha=ptr(t[3]), sigma=ptr(t[4]), bj_of_unit=ptr(t[5]),
                       img_of_bj=ptr(t[6]), out_index=ptr(t[7]), out=ptr(out), n_units=U, C=Cc, H=H, W=W, ld=ld, v_param=v,
                       patch=patch)
    L.check(L.lib().dc_eps_mse(p, L.stream_ptr()), "mse")
    got = out.cpu()[oi.long()]
    assert maxrel(got, ref) < 5e-6        # same fp32 sum in a different (fixed) order
    out2 = torch.zeros_like(out)
    p.out = ptr(out2)
    L.check(L.lib().dc_eps_mse(p, L.stream_ptr()), "mse")
    assert torch.equal(out, out2)         # deterministic reduction: bit-identical run to run


def test_sinusoid_matches_timesteps():
    lam = torch.tensor([15.0, 1.76, 1e-7, -1.76, -14.99, 3.3])
    for dim, flip, shift in [(128, 1, 0.0), (256, 1, 1.0), (64, 0, 0.0)]:
        half = dim // 2
        ex = -np.log(10000) * torch.arange(half, dtype=torch.float32) / (half - shift)
        arg = lam[:, None] * torch.exp(ex)[None]
        ref = torch.cat([torch.cos(arg), torch.sin(arg)], -1) if flip else torch.cat([torch.sin(arg), torch.cos(arg)], -1)
        ld, out = lam.to(DEV), torch.zeros(len(lam), dim, device=DEV)
        p = L.SinusoidParams(lam=ptr(ld), out=ptr(out), n=len(lam), dim=dim, flip_sin_to_cos=flip, freq_shift=shift)
        L.check(L.lib().dc_sinusoid(p, L.stream_ptr()), "sin")
        assert (out.cpu() - ref).abs().max().item() < 2e-6


def test_haar_matches_pywt_goldens_and_roundtrips():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "dwt_pywt.npz"))
    for k in ["rand_3x64x64", "rand_10x32x48", "ramp_1x4x4"]:
        x = torch.from_numpy(g[k + ".x"])
        dec = dca.wavelet_dec_2(x.to(DEV))
        assert dec.device.type == "cuda" and tuple(dec.shape) == g[k + ".dec"].shape
        scale = max(1.0, float(np.abs(g[k + ".dec"]).max()))
        np.testing.assert_allclose(dec.cpu().numpy(), g[k + ".dec"], rtol=0, atol=2e-6 * scale)   # 1e-6 class
        rec = dca.wavelet_enc_2(torch.from_numpy(g[k + ".dec"]).to(DEV))
        np.testing.assert_allclose(rec.cpu().numpy(), g[k + ".enc_of_dec"], rtol=0, atol=2e-6 * scale)
        np.testing.assert_allclose(dca.wavelet_enc_2(dec).cpu().numpy(), g[k + ".x"], rtol=0, atol=2e-6 * scale)
    assert dca.wavelet_dec_2(torch.zeros(3, 8, 8)).device.type == "cpu"      # result lives on images.device
    big = torch.rand(4, 3, 256, 256, device=DEV) * 2 - 1                        # CheXpert-256 shape, batched
    rt = dca.wavelet_enc_2(dca.wavelet_dec_2(big))
    assert (rt - big).abs().max().item() < 1e-6
    half = dca.wavelet_dec_2(big, scale=0.5)                                    # the loaders' "/2" (dataset/chexpert.py:147)
    assert tuple(half.shape) == (4, 12, 128, 128) and (half * 2 - dca.wavelet_dec_2(big)).abs().max().item() < 1e-6
    with pytest.raises(L.DcamdError):
        dca.wavelet_dec_2(torch.zeros(1, 5, 5, device=DEV))                     # odd sizes never occur in the reference


def test_philox_normal_rows_are_keyed_by_id():
    lib = L.lib()
    rows, n = 6, 4096
    ids = torch.tensor([5, 0, 3, 3, 100, 1], dtype=torch.int64, device=DEV)
    a = torch.zeros(rows, n, device=DEV)
    L.check(lib.dc_philox_normal(ptr(a), rows, n, ptr(ids), 1234, L.stream_ptr()), "philox")
    b = torch.zeros(2, n, device=DEV)
    ids2 = torch.tensor([3, 5], dtype=torch.int64, device=DEV)
    L.check(lib.dc_philox_normal(ptr(b), 2, n, ptr(ids2), 1234, L.stream_ptr()), "philox")
    assert torch.equal(a[2], a[3]) and torch.equal(b[0], a[2]) and torch.equal(b[1], a[0])   # value depends on (seed,id) only
    assert not torch.equal(a[0], a[1])
    big = torch.zeros(64, 65536, device=DEV)
    L.check(lib.dc_philox_normal(ptr(big), 64, 65536, None, 7, L.stream_ptr()), "philox")
    assert abs(big.mean().item()) < 3e-3 and abs(big.std().item() - 1) < 3e-3
    assert abs((big ** 4).mean().item() - 3.0) < 0.05


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16])
@pytest.mark.parametrize("concat", [False, True])
def test_conv3x3_with_fused_groupnorm_prologue(dt, concat):
    """GroupNorm statistics-only pass + conv whose halo load applies scale/shift + SiLU in place (padding stays 0)."""
    torch.manual_seed(9)
    g = E.bke(dt)
    n, H, W, C0, C1, Cout = 3, 16, 16, 2 * g, (g if concat else 0), 128
    q = lambda t: t.to(TD[dt]).float()
    x0, x1 = q(torch.randn(n, C0, H, W) * 1.5 + 0.3), (q(torch.randn(n, C1, H, W)) if C1 else None)
    xc = torch.cat([x0, x1], 1) if C1 else x0
    Cc = C0 + C1
    gamma, beta = torch.randn(Cc), torch.randn(Cc)
    w = q(torch.randn(Cout, Cc, 3, 3) / (3 * Cc ** 0.5))
    b = torch.randn(Cout)
    hn = F.silu(F.group_norm(xc, 32, gamma, beta, 1e-5))
    ref = F.conv2d(q(hn), w, b, padding=1)
    lib = L.lib()
    a0, a1 = nhwc(x0, dt), (nhwc(x1, dt) if C1 else None)
    splits = lib.dc_groupnorm_splits(n, H * W, Cc)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n, 32, splits), device=DEV)
    sc, sh = torch.zeros(n, Cc, device=DEV), torch.zeros(n, Cc, device=DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    gp = L.GroupnormParams(x=ptr(a0), x1=ptr(a1), y=None, dtype=dt, out_dtype=dt, n=n, HW=H * W, C=C0, C1=C1, groups=32, silu=0,
                           splits=splits, eps=1e-5, gamma=ptr(gd), beta=ptr(bd), ws=ptr(ws), out_scale=ptr(sc), out_shift=ptr(sh))
    L.check(lib.dc_groupnorm(gp, L.stream_ptr()), "gn stats")
    Wp, bb = E.pack_conv3x3(w, dt, DEV), b.to(DEV)
    out = torch.full((n, H, W, Cout), float("nan"), dtype=TD[dt], device=DEV)
    p = L.IgemmParams(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=C0,
                      src1=ptr(a1), C1=C1, W=ptr(Wp), Cout=Cout, tile_n=128, bias=ptr(bb), out=ptr(out), out_dtype=dt, out_ld=Cout,
                      gn_scale=ptr(sc), gn_shift=ptr(sh), gn_silu=1)
    assert lib.dc_igemm_gn_fusable(p) == 1
    L.check(lib.dc_igemm(p, L.stream_ptr()), "fused conv")
    got = out.float().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    assert maxrel(got, ref) < (3e-5 if dt == L.DC_F32 else 1.5e-2), maxrel(got, ref)
    p.Hin = p.Win = p.Hout = p.Wout = 4                       # 4x4 images are not on the halo kernel: fusion must be refused
    assert lib.dc_igemm_gn_fusable(p) == 0 and lib.dc_igemm(p, L.stream_ptr()) == -6


def _merge_quad_records(qs, nq):
    """(mean, M2) records [n, parts, C/4, 2], each over nq values -> per-quad mean and M2 over the whole sample (Chan's merge)."""
    mean = qs[..., 0].double().mean(1)
    m2 = qs[..., 1].double().sum(1) + nq * ((qs[..., 0].double() - mean[:, None]) ** 2).sum(1)
    return mean, m2


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("shape", [(3, 32, 32, 128, 3), (2, 16, 16, 256, 12), (2, 64, 32, 128, 4)])
def test_thin_conv_with_groupnorm_from_quad_statistics(dt, shape):
    """conv_norm_out + conv_out as ONE launch: the producer conv's quad records -> statistics-only GroupNorm (no sweep of the tensor)
    -> thin-output conv normalising its halo chunks in place.  Must equal GroupNorm kernel + thin conv BIT FOR BIT (same affine,
    same rounding points), and torch within the dtype's tolerance."""
    torch.manual_seed(33)
    n, H, W, C, Co = shape
    g = E.bke(dt)
    q = lambda t: t.to(TD[dt]).float()
    lib = L.lib()
    # producer: a 3x3 conv that also writes the quad statistics of its output
    x0 = q(torch.randn(n, 2 * g, H, W))
    wp_ = q(torch.randn(C, 2 * g, 3, 3) / (3 * (2 * g) ** 0.5))
    a0, Wpp = nhwc(x0, dt), E.pack_conv3x3(wp_, dt, DEV)
    h = torch.empty(n, H, W, C, dtype=TD[dt], device=DEV)
    kw = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=2 * g, W=ptr(Wpp), Cout=C,
              tile_n=128, out=ptr(h), out_dtype=dt, out_ld=C)
    parts = lib.dc_igemm_qstats_parts(L.IgemmParams(**kw))
    assert parts > 0
    qs = torch.zeros(n, parts, C // 4, 2, device=DEV)
    run_igemm(qstats=ptr(qs), **kw)
    gamma, beta = (torch.randn(C) * 0.5 + 1).to(DEV), torch.randn(C).to(DEV)
    splits = lib.dc_groupnorm_splits(n, H * W, C)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n, 32, splits), device=DEV)
    gk = dict(x=ptr(h), dtype=dt, out_dtype=dt, n=n, HW=H * W, C=C, C1=0, groups=32, splits=splits, eps=1e-5, gamma=ptr(gamma), beta=ptr(beta),
              ws=ptr(ws), qstats=ptr(qs), qparts=parts)
    # unfused: GroupNorm(+SiLU) kernel, then the thin conv
    y = torch.empty_like(h)
    L.check(lib.dc_groupnorm(L.GroupnormParams(y=ptr(y), silu=1, **gk), L.stream_ptr()), "gn")
    w = q(torch.randn(Co, C, 3, 3) / (3 * C ** 0.5))
    b = torch.randn(Co).to(DEV)
    Wo = E.pack_conv3x3(w, dt, DEV, tile_n=32)
    o_ref = torch.full((n, H, W, Co), float("nan"), device=DEV)
    ck = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, C0=C, W=ptr(Wo), Cout=Co, tile_n=32,
              bias=ptr(b), out_dtype=L.DC_F32, out_ld=Co)
    pu = L.IgemmParams(src0=ptr(y), out=ptr(o_ref), **ck)
    assert lib.dc_igemm_variant(pu).decode().startswith("conv3_thin")
    L.check(lib.dc_igemm(pu, L.stream_ptr()), "thin conv")
    # fused: affine from the quad records only, normalised inside the conv
    sc, sh = torch.zeros(n, C, device=DEV), torch.zeros(n, C, device=DEV)
    L.check(lib.dc_groupnorm(L.GroupnormParams(y=None, silu=0, out_scale=ptr(sc), out_shift=ptr(sh), **gk), L.stream_ptr()), "gn affine")
    o = torch.full((n, H, W, Co), float("nan"), device=DEV)
    pf = L.IgemmParams(src0=ptr(h), out=ptr(o), gn_scale=ptr(sc), gn_shift=ptr(sh), gn_silu=1, **ck)
    assert lib.dc_igemm_gn_fusable(pf) == 1 and lib.dc_igemm_variant(pf).decode().startswith("conv3_thin")
    L.check(lib.dc_igemm(pf, L.stream_ptr()), "fused thin conv")
    torch.cuda.synchronize()
    assert torch.isfinite(o).all()
    if H * W * C * (4 if dt == L.DC_F32 else 2) < (1 << 20):
        assert torch.equal(o, o_ref)
    else:       # samples of 1 MiB and more: the GroupNorm kernel folds the quad records in gn_qfold_kernel's order, the affine in gn_image_kernel's
        assert maxrel(o, o_ref) < (1e-5 if dt == L.DC_F32 else 4e-3), maxrel(o, o_ref)
    hn = F.silu(F.group_norm(h.float().permute(0, 3, 1, 2), 32, gamma, beta, 1e-5))
    ref = F.conv2d(q(hn), w.to(DEV), b, padding=1).permute(0, 2, 3, 1)
    assert maxrel(o, ref) < {L.DC_F32: 3e-5, L.DC_BF16: 1.5e-2, L.DC_F16: 3e-3}[dt], maxrel(o, ref)


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("case", ["c128_32x32_res", "c128_32x32_side", "c256to128_16x16", "two_ntiles_64x32", "maps_plain"])
def test_wave_specialised_conv_with_fused_groupnorm_is_bit_identical(dt, case):
    """GroupNorm + SiLU -> 3x3 conv as ONE launch (conv3_ws.hip: loader waves normalise each landed halo chunk in place from the
    producer's quad records, MFMA waves only multiply) against the two launches it replaces (dc_groupnorm with the same quad records,
    then conv3_halo): outputs AND the output's own quad records bit for bit, with a bias, a per-sample row vector, a residual read
    through a map, the folded 1x1 side source, several N tiles, sample maps; and torch within the dtype's tolerance."""
    torch.manual_seed(35)
    n, H, W, C, Co, side, res, maps = {"c128_32x32_res": (5, 32, 32, 128, 128, 0, True, False),
                                       "c128_32x32_side": (3, 32, 32, 128, 128, 128, True, False),
                                       "c256to128_16x16": (6, 16, 16, 256, 128, 0, False, False),
                                       "two_ntiles_64x32": (2, 64, 32, 128, 256, 64, True, False),
                                       "maps_plain": (7, 16, 16, 128, 128, 0, True, True)}[case]
    g = E.bke(dt)
    q = lambda t: t.to(TD[dt]).float()
    lib = L.lib()
    n_src = 3 if maps else n                  # sample maps: 7 output samples read 3 source samples (class-shared trunk -> per-unit layer)
    # producer: a 3x3 conv that also writes the quad statistics of its output h
    x0 = q(torch.randn(n_src, 2 * g, H, W))
    wp_ = q(torch.randn(C, 2 * g, 3, 3) / (3 * (2 * g) ** 0.5))
    a0, Wpp = nhwc(x0, dt), E.pack_conv3x3(wp_, dt, DEV)
    h = torch.empty(n_src, H, W, C, dtype=TD[dt], device=DEV)
    kw = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n_src, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=2 * g, W=ptr(Wpp), Cout=C,
              tile_n=128, out=ptr(h), out_dtype=dt, out_ld=C)
    parts = lib.dc_igemm_qstats_parts(L.IgemmParams(**kw))
    assert parts > 0
    qs = torch.zeros(n_src, parts, C // 4, 2, device=DEV)
    run_igemm(qstats=ptr(qs), **kw)
    gamma, beta = (torch.randn(C) * 0.5 + 1).to(DEV), torch.randn(C).to(DEV)
    splits = lib.dc_groupnorm_splits(n_src, H * W, C)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n_src, 32, splits), device=DEV)
    gk = dict(x=ptr(h), dtype=dt, out_dtype=dt, n=n_src, HW=H * W, C=C, C1=0, groups=32, splits=splits, eps=1e-5, gamma=ptr(gamma), beta=ptr(beta),
              ws=ptr(ws), qstats=ptr(qs), qparts=parts)
    y = torch.empty_like(h)
    L.check(lib.dc_groupnorm(L.GroupnormParams(y=ptr(y), silu=1, **gk), L.stream_ptr()), "gn")
    sc, sh = torch.zeros(n_src, C, device=DEV), torch.zeros(n_src, C, device=DEV)
    L.check(lib.dc_groupnorm(L.GroupnormParams(y=None, silu=0, out_scale=ptr(sc), out_shift=ptr(sh), **gk), L.stream_ptr()), "gn affine")
    # the consumer conv
    w = q(torch.randn(Co, C, 3, 3) / (3 * C ** 0.5))
    b, rv = torch.randn(Co).to(DEV), torch.randn(n, Co).to(DEV)
    Wo = E.pack_conv3x3(w, dt, DEV)
    smap = torch.tensor([i % n_src for i in range(n)], dtype=torch.int32, device=DEV) if maps else None
    r = torch.randn(n_src if maps else n, H, W, Co, device=DEV).to(TD[dt]) if res else None
    xs = q(torch.randn(n_src if maps else n, side, H, W)) if side else None
    ws2 = q(torch.randn(Co, side) / side ** 0.5) if side else None
    ck = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, C0=C, map0=ptr(smap), W=ptr(Wo), Cout=Co, tile_n=128,
              bias=ptr(b), rowvec=ptr(rv), rowvec_ld=Co, out_dtype=dt, out_ld=Co)
    keep = []
    if res:
        ck.update(residual=ptr(r), res_map=ptr(smap), res_dtype=dt, res_ld=Co)
    if side:
        a2, W2 = nhwc(xs, dt), E.pack_matrix(ws2, dt, DEV)
        keep += [a2, W2]
        ck.update(src2=ptr(a2), map2=ptr(smap), W2=ptr(W2), C2=side, ld2=side)
    parts_o = lib.dc_igemm_qstats_parts(L.IgemmParams(src0=ptr(y), out=ptr(y), **ck))
    assert parts_o > 0
    o_ref = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt])
    q_ref = torch.full((n, parts_o, Co // 4, 2), float("nan"), device=DEV)
    pu = L.IgemmParams(src0=ptr(y), out=ptr(o_ref), qstats=ptr(q_ref), **ck)
    assert lib.dc_igemm_variant(pu).decode().startswith("conv3_halo")
    L.check(lib.dc_igemm(pu, L.stream_ptr()), "GroupNorm kernel + halo conv")
    # the affine of a mapped source sample lives in the conv's own sample index space: gather it like the engine's domains do
    scn, shn = (sc[smap.long()].contiguous(), sh[smap.long()].contiguous()) if maps else (sc, sh)
    o = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt])
    q_o = torch.full((n, parts_o, Co // 4, 2), float("nan"), device=DEV)
    pf = L.IgemmParams(src0=ptr(h), out=ptr(o), qstats=ptr(q_o), gn_scale=ptr(scn), gn_shift=ptr(shn), gn_silu=1, **ck)
    assert lib.dc_igemm_gn_fusable(pf) == 1 and lib.dc_igemm_variant(pf).decode() == "conv3_ws<%s,gn>" % {L.DC_F32: "f32", L.DC_BF16: "bf16", L.DC_F16: "f16"}[dt]
    L.check(lib.dc_igemm(pf, L.stream_ptr()), "wave-specialised conv with fused GroupNorm")
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all() and torch.isfinite(q_o).all()
    if H * W * C * (4 if dt == L.DC_F32 else 2) < (1 << 20):
        assert torch.equal(o, o_ref) and torch.equal(q_o, q_ref)
    else:       # samples of 1 MiB and more: the GroupNorm kernel folds the quad records in gn_qfold_kernel's order, the affine in gn_image_kernel's
        assert maxrel(o, o_ref) < (1e-5 if dt == L.DC_F32 else 4e-3), maxrel(o, o_ref)
    idx = smap.long().cpu() if maps else torch.arange(n)
    hn = q(F.silu(F.group_norm(h.float().permute(0, 3, 1, 2), 32, gamma, beta, 1e-5))).cpu()[idx]
    ref = F.conv2d(hn, w, b.cpu(), padding=1) + rv.cpu()[:, :, None, None]
    if side:
        ref = ref + torch.einsum("nchw,oc->nohw", xs[idx], ws2)
    if res:
        ref = ref + r.float().cpu()[idx].permute(0, 3, 1, 2)
    assert maxrel(o.float().cpu(), ref.permute(0, 2, 3, 1)) < {L.DC_F32: 3e-5, L.DC_BF16: 1.5e-2, L.DC_F16: 3e-3}[dt]


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("case", ["c128_32x32_res_side_maps", "c256_16x16_one_tile", "c128_64x64_cpg8_raw_dropped", "two_ntiles_32x32_nosilu",
                                  "c512_16x16_cpg16", "c1024_16x16_cpg32", "c128_32x32_many_samples"])
def test_conv3x3_normalises_its_own_output_for_the_next_groupnorm(dt, case):
    """Producer-side GroupNorm (dc_igemm pn_*; csrc/epi_pn.h): the conv stores act(gn(v)) of its output v — the workgroups of a sample
    exchange their (mean, M2) quad records through memory — next to (or instead of) the raw v.  Checks: the raw output and the quad
    records equal the plain launch's bit for bit; the normalised output equals dc_groupnorm of those records applied to the fp32
    values (f32: to rounding noise; 16-bit: within one rounding of the output type, because the producer normalises its fp32
    accumulators where the GroupNorm kernel reads the rounded tensor) and torch's group_norm + silu; no wait timed out.  One tile per
    sample (16x16), four (32x32), sixteen (64x64); 4 / 8 / 16 / 32 channels per group; several N tiles; bias, per-sample row
    vector, residual and 1x1 side source read through sample maps."""
    torch.manual_seed(77)
    n, H, W, Ci, Co, groups, side, res, maps, silu, raw = {
        "c128_32x32_res_side_maps": (7, 32, 32, 128, 128, 32, 128, True, True, True, True),
        "c256_16x16_one_tile": (6, 16, 16, 128, 256, 32, 0, False, False, True, True),
        "c128_64x64_cpg8_raw_dropped": (3, 64, 64, 128, 128, 16, 0, True, False, True, False),
        "two_ntiles_32x32_nosilu": (5, 32, 32, 128, 256, 32, 64, True, False, False, True),
        "c512_16x16_cpg16": (4, 16, 16, 128, 512, 32, 0, False, False, True, True),
        "c1024_16x16_cpg32": (2, 16, 16, 64, 1024, 32, 0, False, False, True, False),
        "c128_32x32_many_samples": (300, 32, 32, 64, 128, 32, 0, False, False, True, True)}[case]
    q = lambda t: t.to(TD[dt]).float()
    lib = L.lib()
    eps = 1e-5 if silu else 1e-6
    n_src = 3 if maps else n
    smap = torch.tensor([i % n_src for i in range(n)], dtype=torch.int32, device=DEV) if maps else None
    x = q(torch.randn(n_src, Ci, H, W))
    w = q(torch.randn(Co, Ci, 3, 3) / (3 * Ci ** 0.5))
    b, rv = torch.randn(Co).to(DEV), (torch.randn(n, Co) * 2).to(DEV)
    a0, Wp = nhwc(x, dt), E.pack_conv3x3(w, dt, DEV)
    r = torch.randn(n_src if maps else n, H, W, Co, device=DEV).to(TD[dt]) if res else None
    xs = q(torch.randn(n_src if maps else n, side, H, W)) if side else None
    ws2 = q(torch.randn(Co, side) / side ** 0.5) if side else None
    ck = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=Ci, map0=ptr(smap), W=ptr(Wp), Cout=Co,
              tile_n=128, bias=ptr(b), rowvec=ptr(rv), rowvec_ld=Co, out_dtype=dt, out_ld=Co)
    keep = []
    if res:
        ck.update(residual=ptr(r), res_map=ptr(smap), res_dtype=dt, res_ld=Co)
    if side:
        a2, W2 = nhwc(xs, dt), E.pack_matrix(ws2, dt, DEV)
        keep += [a2, W2]
        ck.update(src2=ptr(a2), map2=ptr(smap), W2=ptr(W2), C2=side, ld2=side)
    # the plain launch: raw output + quad records
    o_ref = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt])
    parts = lib.dc_igemm_qstats_parts(L.IgemmParams(out=ptr(o_ref), **ck))
    assert parts == H * W // 128
    q_ref = torch.full((n, parts, Co // 4, 2), float("nan"), device=DEV)
    run_igemm(out=ptr(o_ref), qstats=ptr(q_ref), **ck)
    # the GroupNorm kernel on the raw tensor with those records
    gamma, beta = (torch.randn(Co) * 0.5 + 1).to(DEV), torch.randn(Co).to(DEV)
    splits = lib.dc_groupnorm_splits(n, H * W, Co)
    wsb = torch.zeros(lib.dc_groupnorm_ws_floats(n, groups, splits), device=DEV)
    y_ref = torch.empty_like(o_ref)
    L.check(lib.dc_groupnorm(L.GroupnormParams(x=ptr(o_ref), y=ptr(y_ref), dtype=dt, out_dtype=dt, n=n, HW=H * W, C=Co, C1=0, groups=groups, silu=int(silu),
                                               splits=splits, eps=eps, gamma=ptr(gamma), beta=ptr(beta), ws=ptr(wsb), qstats=ptr(q_ref), qparts=parts),
                             L.stream_ptr()), "gn")
    # the producer-normalising launch
    o = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt]) if raw else None
    y = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt])
    q_o = torch.full((n, parts, Co // 4, 2), float("nan"), device=DEV)
    cnt = torch.zeros(n * ((Co + 127) // 128), dtype=torch.int32, device=DEV)      # zeroed ONCE: the counters are monotonic
    pp = L.IgemmParams(out=ptr(o), qstats=ptr(q_o), pn_out=ptr(y), pn_gamma=ptr(gamma), pn_beta=ptr(beta), pn_cnt=ptr(cnt), pn_ld=Co, pn_groups=groups,
                       pn_silu=int(silu), pn_eps=eps, **ck)
    assert lib.dc_igemm_pn_ok(pp) == 1
    assert lib.dc_igemm_variant(pp).decode() == "conv3_halo<%s,4w,pn>" % {L.DC_F32: "f32", L.DC_BF16: "bf16", L.DC_F16: "f16"}[dt]
    for _ in range(2):                                     # twice: nothing is reset between launches
        L.check(lib.dc_igemm(pp, L.stream_ptr()), "conv with producer-side GroupNorm")
    torch.cuda.synchronize()
    assert lib.dc_pn_timeouts() == 0
    assert torch.equal(cnt, torch.full_like(cnt, 2 * (H * W // 256) if H * W > 256 else 0))     # (one tile per sample: nothing crosses a workgroup)
    assert torch.equal(q_o, q_ref)
    if raw:
        assert torch.equal(o, o_ref)
    assert torch.isfinite(y.float()).all()
    # against the GroupNorm kernel: same records, same fold; the 16-bit kernel normalises the ROUNDED tensor, the producer its fp32 values
    tol_k = {L.DC_F32: 5e-6, L.DC_BF16: 1.6e-2, L.DC_F16: 2e-3}[dt]
    assert maxrel(y, y_ref) < tol_k, maxrel(y, y_ref)
    # against torch, from the same rounded operands
    idx = smap.long().cpu() if maps else torch.arange(n)
    ref = F.conv2d(x[idx], w, b.cpu(), padding=1) + rv.cpu()[:, :, None, None]
    if side:
        ref = ref + torch.einsum("nchw,oc->nohw", xs[idx], ws2)
    if res:
        ref = ref + r.float().cpu()[idx].permute(0, 3, 1, 2)
    yn = F.group_norm(ref, groups, gamma.cpu(), beta.cpu(), eps)
    if silu:
        yn = F.silu(yn)
    assert maxrel(y.float().cpu(), yn.permute(0, 2, 3, 1)) < {L.DC_F32: 3e-5, L.DC_BF16: 8e-3, L.DC_F16: 1.5e-3}[dt]
    assert rel(y.float().cpu(), yn.permute(0, 2, 3, 1)) < {L.DC_F32: 1e-5, L.DC_BF16: 4e-3, L.DC_F16: 6e-4}[dt]


@pytest.mark.parametrize("n", [700, 3])
def test_producer_normalised_conv_never_reads_a_previous_launch_s_records(n):
    """The hand-off inside a producer-normalising conv (csrc/epi_pn.h: records -> agent-scope release -> counter -> acquire -> fold)
    replayed on the SAME buffers with alternating inputs, as a plan replays it per micro-batch: a wave that folded a record of the
    previous launch (a stale L2 / L1 line) would store a slightly different tensor.  Every element of every replay must equal the
    first-touch result of its input; uneven load comes from a second stream streaming a large copy beside half of the replays.  n = 3 is the
    case that failed once (round 4): so little traffic that the previous replay's lines survive in L2 between launches."""
    torch.manual_seed(78)
    dt, H, W, Ci, Co = L.DC_BF16, 32, 32, 64, 128
    lib = L.lib()
    xs = [nhwc(torch.randn(n, Ci, H, W) * (1.0 + 0.5 * i), dt) for i in range(2)]
    Wp = E.pack_conv3x3(torch.randn(Co, Ci, 3, 3) / (3 * Ci ** 0.5), dt, DEV)
    b = torch.randn(Co).to(DEV)
    gamma, beta = (torch.randn(Co) * 0.5 + 1).to(DEV), torch.randn(Co).to(DEV)
    parts = H * W // 128

    def launch(x, y, qs, cnt):
        p = L.IgemmParams(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(x), C0=Ci, W=ptr(Wp), Cout=Co, tile_n=128,
                          bias=ptr(b), out=None, out_dtype=dt, out_ld=Co, qstats=ptr(qs), pn_out=ptr(y), pn_gamma=ptr(gamma), pn_beta=ptr(beta),
                          pn_cnt=ptr(cnt), pn_ld=Co, pn_groups=32, pn_silu=1, pn_eps=1e-5)
        L.check(lib.dc_igemm(p, L.stream_ptr()), "pn conv")
    want = []
    for x in xs:                               # first touch: fresh buffers
        y, qs, cnt = torch.empty(n, H, W, Co, dtype=TD[dt], device=DEV), torch.zeros(n, parts, Co // 4, 2, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
        launch(x, y, qs, cnt)
        torch.cuda.synchronize()
        want.append(y)
    assert not torch.equal(want[0], want[1])
    y, qs, cnt = torch.empty_like(want[0]), torch.zeros(n, parts, Co // 4, 2, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    big_a, big_b = torch.empty(1 << 28, dtype=torch.uint8, device=DEV), torch.empty(1 << 28, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    bad = 0
    for it in range(24):
        if it % 4 >= 2:
            with torch.cuda.stream(side):
                big_b.copy_(big_a)
        launch(xs[it & 1], y, qs, cnt)
        bad += int((y != want[it & 1]).sum().item())
    torch.cuda.synchronize()
    assert lib.dc_pn_timeouts() == 0
    assert bad == 0, bad


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("case", ["c256_cpg8_res_maps_raw", "c512_cpg16_nosilu_raw", "c128_cpg4", "c1024_cpg32", "c256_ragged_patch_side"])
def test_conv3x3_on_8x8_images_normalises_its_own_output_inside_the_wave(dt, case):
    """Producer-side GroupNorm on 8x8 images (the staggered 8-wave halo kernel: two whole images per wave): the group statistics come
    from the quad records the epilogue forms anyway and never leave the wave (groups wider than a lane's 8-channel run are merged
    with the lanes 16 / 32 apart).  Raw output and records equal the plain launch's bit for bit; the normalised output equals
    dc_groupnorm on those records / torch; sample counts that leave a patch (8 images) ragged."""
    torch.manual_seed(91)
    n, Ci, Co, groups, res, maps, silu, raw, side = {
        "c256_cpg8_res_maps_raw": (21, 128, 256, 32, True, True, True, True, 0),
        "c512_cpg16_nosilu_raw": (9, 128, 512, 32, False, False, False, True, 0),
        "c128_cpg4": (16, 128, 128, 32, False, False, True, False, 0),
        "c1024_cpg32": (5, 64, 1024, 32, False, False, True, False, 0),
        "c256_ragged_patch_side": (11, 128, 256, 16, True, False, True, True, 128)}[case]
    H = W = 8
    q = lambda t: t.to(TD[dt]).float()
    lib = L.lib()
    eps = 1e-5 if silu else 1e-6
    n_src = 4 if maps else n
    smap = torch.tensor([i % n_src for i in range(n)], dtype=torch.int32, device=DEV) if maps else None
    x = q(torch.randn(n_src, Ci, H, W))
    w = q(torch.randn(Co, Ci, 3, 3) / (3 * Ci ** 0.5))
    b, rv = torch.randn(Co).to(DEV), (torch.randn(n, Co) * 2).to(DEV)
    a0, Wp = nhwc(x, dt), E.pack_conv3x3(w, dt, DEV)
    r = torch.randn(n_src if maps else n, H, W, Co, device=DEV).to(TD[dt]) if res else None
    xs = q(torch.randn(n_src if maps else n, side, H, W)) if side else None
    ws2 = q(torch.randn(Co, side) / side ** 0.5) if side else None
    ck = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=Ci, map0=ptr(smap), W=ptr(Wp), Cout=Co,
              tile_n=128, bias=ptr(b), rowvec=ptr(rv), rowvec_ld=Co, out_dtype=dt, out_ld=Co)
    keep = []
    if res:
        ck.update(residual=ptr(r), res_map=ptr(smap), res_dtype=dt, res_ld=Co)
    if side:
        a2, W2 = nhwc(xs, dt), E.pack_matrix(ws2, dt, DEV)
        keep += [a2, W2]
        ck.update(src2=ptr(a2), map2=ptr(smap), W2=ptr(W2), C2=side, ld2=side)
    o_ref = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt])
    parts = lib.dc_igemm_qstats_parts(L.IgemmParams(out=ptr(o_ref), **ck))
    assert parts == 1
    q_ref = torch.full((n, parts, Co // 4, 2), float("nan"), device=DEV)
    run_igemm(out=ptr(o_ref), qstats=ptr(q_ref), **ck)
    gamma, beta = (torch.randn(Co) * 0.5 + 1).to(DEV), torch.randn(Co).to(DEV)
    splits = lib.dc_groupnorm_splits(n, H * W, Co)
    wsb = torch.zeros(lib.dc_groupnorm_ws_floats(n, groups, splits), device=DEV)
    y_ref = torch.empty_like(o_ref)
    L.check(lib.dc_groupnorm(L.GroupnormParams(x=ptr(o_ref), y=ptr(y_ref), dtype=dt, out_dtype=dt, n=n, HW=H * W, C=Co, C1=0, groups=groups, silu=int(silu),
                                               splits=splits, eps=eps, gamma=ptr(gamma), beta=ptr(beta), ws=ptr(wsb), qstats=ptr(q_ref), qparts=parts),
                             L.stream_ptr()), "gn")
    o = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt]) if raw else None
    y = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt])
    q_o = torch.full((n, parts, Co // 4, 2), float("nan"), device=DEV)
    cnt = torch.zeros(n * ((Co + 127) // 128), dtype=torch.int32, device=DEV)
    pp = L.IgemmParams(out=ptr(o), qstats=ptr(q_o), pn_out=ptr(y), pn_gamma=ptr(gamma), pn_beta=ptr(beta), pn_cnt=ptr(cnt), pn_ld=Co, pn_groups=groups,
                       pn_silu=int(silu), pn_eps=eps, **ck)
    assert lib.dc_igemm_pn_ok(pp) == 1
    assert lib.dc_igemm_variant(pp).decode() == "conv3_halo<%s,8w,pn>" % {L.DC_F32: "f32", L.DC_BF16: "bf16", L.DC_F16: "f16"}[dt]
    L.check(lib.dc_igemm(pp, L.stream_ptr()), "8x8 conv with wave-local GroupNorm")
    torch.cuda.synchronize()
    assert torch.equal(q_o, q_ref)
    if raw:
        assert torch.equal(o, o_ref)
    assert torch.isfinite(y.float()).all()
    assert maxrel(y, y_ref) < {L.DC_F32: 5e-6, L.DC_BF16: 1.6e-2, L.DC_F16: 2e-3}[dt], maxrel(y, y_ref)
    idx = smap.long().cpu() if maps else torch.arange(n)
    ref = F.conv2d(x[idx], w, b.cpu(), padding=1) + rv.cpu()[:, :, None, None]
    if side:
        ref = ref + torch.einsum("nchw,oc->nohw", xs[idx], ws2)
    if res:
        ref = ref + r.float().cpu()[idx].permute(0, 3, 1, 2)
    yn = F.group_norm(ref, groups, gamma.cpu(), beta.cpu(), eps)
    if silu:
        yn = F.silu(yn)
    assert maxrel(y.float().cpu(), yn.permute(0, 2, 3, 1)) < {L.DC_F32: 3e-5, L.DC_BF16: 1.0e-2, L.DC_F16: 1.5e-3}[dt]


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("case", ["c512_cpg16_res_raw", "c256_cpg8_nosilu_side_maps", "c1024_cpg32", "c128_cpg4_ragged"])
def test_conv3x3_on_4x4_images_normalises_its_own_output_inside_the_wave(dt, case):
    """Producer-side GroupNorm on 4x4 images (mosaic halo patches: 32 images per workgroup, one per 16-pixel MFMA fragment): the
    statistics of an image are the sums over ONE fragment row of the wave — formed in the epilogue, no quad records exist for these
    patches — merged over the group's quads like the 8x8 form.  Raw output equals the plain launch's bit for bit; the normalised
    output equals dc_groupnorm of the raw fp32 / rounded tensor and torch within the dtype's rounding."""
    torch.manual_seed(92)
    n, Ci, Co, groups, res, maps, silu, raw, side = {
        "c512_cpg16_res_raw": (70, 128, 512, 32, True, False, True, True, 0),
        "c256_cpg8_nosilu_side_maps": (45, 128, 256, 32, True, True, False, True, 128),
        "c1024_cpg32": (33, 64, 1024, 32, False, False, True, False, 0),
        "c128_cpg4_ragged": (37, 128, 128, 32, False, False, True, False, 0)}[case]
    H = W = 4
    q = lambda t: t.to(TD[dt]).float()
    lib = L.lib()
    eps = 1e-5 if silu else 1e-6
    n_src = 7 if maps else n
    smap = torch.tensor([i % n_src for i in range(n)], dtype=torch.int32, device=DEV) if maps else None
    x = q(torch.randn(n_src, Ci, H, W))
    w = q(torch.randn(Co, Ci, 3, 3) / (3 * Ci ** 0.5))
    b, rv = torch.randn(Co).to(DEV), (torch.randn(n, Co) * 2).to(DEV)
    a0, Wp = nhwc(x, dt), E.pack_conv3x3(w, dt, DEV)
    r = torch.randn(n_src if maps else n, H, W, Co, device=DEV).to(TD[dt]) if res else None
    xs = q(torch.randn(n_src if maps else n, side, H, W)) if side else None
    ws2 = q(torch.randn(Co, side) / side ** 0.5) if side else None
    ck = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=Ci, map0=ptr(smap), W=ptr(Wp), Cout=Co,
              tile_n=128, bias=ptr(b), rowvec=ptr(rv), rowvec_ld=Co, out_dtype=dt, out_ld=Co)
    keep = []
    if res:
        ck.update(residual=ptr(r), res_map=ptr(smap), res_dtype=dt, res_ld=Co)
    if side:
        a2, W2 = nhwc(xs, dt), E.pack_matrix(ws2, dt, DEV)
        keep += [a2, W2]
        ck.update(src2=ptr(a2), map2=ptr(smap), W2=ptr(W2), C2=side, ld2=side)
    o_ref = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt])
    assert lib.dc_igemm_qstats_parts(L.IgemmParams(out=ptr(o_ref), **ck)) == 0          # mosaic patches write no quad records
    run_igemm(out=ptr(o_ref), **ck)
    gamma, beta = (torch.randn(Co) * 0.5 + 1).to(DEV), torch.randn(Co).to(DEV)
    o = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt]) if raw else None
    y = torch.full((n, H, W, Co), float("nan"), device=DEV).to(TD[dt])
    cnt = torch.zeros(n * ((Co + 127) // 128), dtype=torch.int32, device=DEV)
    pp = L.IgemmParams(out=ptr(o), pn_out=ptr(y), pn_gamma=ptr(gamma), pn_beta=ptr(beta), pn_cnt=ptr(cnt), pn_ld=Co, pn_groups=groups,
                       pn_silu=int(silu), pn_eps=eps, **ck)
    assert lib.dc_igemm_pn_ok(pp) == 1
    assert lib.dc_igemm_variant(pp).decode() == "conv3_halo<%s,8w,pn>" % {L.DC_F32: "f32", L.DC_BF16: "bf16", L.DC_F16: "f16"}[dt]
    L.check(lib.dc_igemm(pp, L.stream_ptr()), "4x4 conv with wave-local GroupNorm")
    torch.cuda.synchronize()
    if raw:
        assert torch.equal(o, o_ref)
    assert torch.isfinite(y.float()).all()
    idx = smap.long().cpu() if maps else torch.arange(n)
    ref = F.conv2d(x[idx], w, b.cpu(), padding=1) + rv.cpu()[:, :, None, None]
    if side:
        ref = ref + torch.einsum("nchw,oc->nohw", xs[idx], ws2)
    if res:
        ref = ref + r.float().cpu()[idx].permute(0, 3, 1, 2)
    yn = F.group_norm(ref, groups, gamma.cpu(), beta.cpu(), eps)
    if silu:
        yn = F.silu(yn)
    assert maxrel(y.float().cpu(), yn.permute(0, 2, 3, 1)) < {L.DC_F32: 3e-5, L.DC_BF16: 1.0e-2, L.DC_F16: 1.5e-3}[dt]
    assert rel(y.float().cpu(), yn.permute(0, 2, 3, 1)) < {L.DC_F32: 1e-5, L.DC_BF16: 4e-3, L.DC_F16: 6e-4}[dt]


def test_a_wait_that_cannot_complete_times_out_counts_and_poisons_its_outputs():
    """The bounded wait of csrc/epi_pn.h: a counter that can never reach its target (here: sample 1's arrival counter preset to
    0xFFFFFFFF, so three of its four workgroups take tickets whose target is one arrival more than the launch delivers) must end in a
    timeout — the launch returns after PN_TIMEOUT_TICKS (30 ms), `dc_pn_timeouts()` reports the waves (and clears the count), the
    affected sample is NaN-poisoned and every other sample is untouched.  Never a hang."""
    torch.manual_seed(79)
    dt, n, H, W, Ci, Co = L.DC_BF16, 6, 32, 32, 64, 128
    lib = L.lib()
    x = nhwc(torch.randn(n, Ci, H, W), dt)
    Wp = E.pack_conv3x3(torch.randn(Co, Ci, 3, 3) / (3 * Ci ** 0.5), dt, DEV)
    b = torch.randn(Co).to(DEV)
    gamma, beta = (torch.randn(Co) * 0.5 + 1).to(DEV), torch.randn(Co).to(DEV)

    def launch(cnt):
        y = torch.zeros(n, H, W, Co, dtype=TD[dt], device=DEV)
        qs = torch.zeros(n, H * W // 128, Co // 4, 2, device=DEV)
        p = L.IgemmParams(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(x), C0=Ci, W=ptr(Wp), Cout=Co, tile_n=128,
                          bias=ptr(b), out=None, out_dtype=dt, out_ld=Co, qstats=ptr(qs), pn_out=ptr(y), pn_gamma=ptr(gamma), pn_beta=ptr(beta),
                          pn_cnt=ptr(cnt), pn_ld=Co, pn_groups=32, pn_silu=1, pn_eps=1e-5)
        L.check(lib.dc_igemm(p, L.stream_ptr()), "pn conv")
        torch.cuda.synchronize()
        return y
    assert lib.dc_pn_timeouts() == 0
    good = launch(torch.zeros(n, dtype=torch.int32, device=DEV))
    assert lib.dc_pn_timeouts() == 0 and torch.isfinite(good.float()).all()
    cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
    cnt[1] = -1
    bad = launch(cnt)
    assert lib.dc_pn_timeouts() >= 3          # three workgroups x (one polling wave each)
    assert lib.dc_pn_timeouts() == 0          # reading clears the count
    assert torch.isnan(bad[1].float()).any()
    keep = [0, 2, 3, 4, 5]
    assert torch.equal(bad[keep], good[keep])


def test_groupnorm_span_kernel_opt_in():
    """DCAMD_GN_SPAN=1 (read once per process): the short-span normalise sweep must pass the same quad-statistics GroupNorm
    test in ONE child interpreter — spans of 16 KiB, statistics folded from the records or from gn_qfold_kernel's output (that test
    asserts the "span" / "qfold+span" route there)."""
    import subprocess
    import sys
    if os.environ.get("DCAMD_GN_SPAN") is not None:
        pytest.skip("already running with the span kernel")
    env = dict(os.environ, DCAMD_GN_SPAN="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-k", "quad_statistics_feed_groupnorm",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("shape", [(3, 8, 8, 128), (5, 16, 16, 256), (3, 32, 32, 128),
                                   (2, 64, 32, 384),          # >= 1 MiB per sample, 48 / 96 chunks per pixel: quad records folded by gn_qfold_kernel, split apply sweep
                                   (3, 8, 16, 128),
                                   (2, 256, 128, 128)])       # > 4 MiB per sample: quad records folded by gn_qfold_kernel, span sweep; without them the split GroupNorm
def test_conv3x3_quad_statistics_feed_groupnorm(dt, shape):
    """dc_igemm qstats: per (sample, part, channel quad) sum / sumsq of the STORED output; a GroupNorm given them skips its
    statistics sweep and must match the GroupNorm that sweeps the tensor itself."""
    torch.manual_seed(21)
    n, H, W, Cout = shape
    g = E.bke(dt)
    C0 = 2 * g
    q = lambda t: t.to(TD[dt]).float()
    x0 = q(torch.randn(n, C0, H, W))
    w = q(torch.randn(Cout, C0, 3, 3) / (3 * C0 ** 0.5))
    b = torch.randn(Cout) + 0.5
    res = q(torch.randn(n, Cout, H, W))
    lib = L.lib()
    a0, resd, bd, Wp = nhwc(x0, dt), nhwc(res, dt), b.to(DEV), E.pack_conv3x3(w, dt, DEV)
    out = torch.full((n, H, W, Cout), float("nan"), dtype=TD[dt], device=DEV)
    kw = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(a0), C0=C0, W=ptr(Wp),
              Cout=Cout, tile_n=128, bias=ptr(bd), residual=ptr(resd), res_dtype=dt, res_ld=Cout, out=ptr(out), out_dtype=dt, out_ld=Cout)
    parts = lib.dc_igemm_qstats_parts(L.IgemmParams(**kw))
    assert parts == max(1, H * W // 128)
    qs = torch.full((n, parts, Cout // 4, 2), float("nan"), device=DEV)
    run_igemm(qstats=ptr(qs), **kw)
    out2 = torch.empty_like(out)
    run_igemm(**dict(kw, out=ptr(out2)))
    assert torch.equal(out, out2)                                   # the statistics do not touch the output
    of = out.float()
    assert torch.isfinite(qs).all() and (qs[..., 1] >= 0).all()
    # records: per (sample, part, quad) mean and M2 = sum (v - mean)^2 of the quad's 4 * HW / parts values; merged over the parts they
    # must be the quad's mean and centred second moment over the sample.  They are formed from the fp32 accumulators BEFORE the
    # rounding to the storage type: for 16-bit outputs they differ from the stored tensor's by the (zero-mean) rounding errors
    m_got, m2_got = _merge_quad_records(qs, 4 * H * W // parts)
    px = of.double().reshape(n, H * W, Cout // 4, 4)
    m_ref = px.mean((1, 3))
    m2_ref = ((px - m_ref[:, None, :, None]) ** 2).sum((1, 3))
    assert (m_got - m_ref).abs().max().item() < (1e-5 if dt == L.DC_F32 else 2e-3) * max(1.0, m_ref.abs().max().item())
    assert ((m2_got - m2_ref).abs() / m2_ref).max().item() < (1e-4 if dt == L.DC_F32 else 1e-2)
    # GroupNorm(+SiLU) from the quad statistics == GroupNorm that sweeps the tensor
    gamma, beta = torch.randn(Cout, device=DEV), torch.randn(Cout, device=DEV)
    splits = lib.dc_groupnorm_splits(n, H * W, Cout)
    ws = torch.zeros(lib.dc_groupnorm_ws_floats(n, 32, splits), device=DEV)
    ya, yb = torch.empty_like(out), torch.empty_like(out)
    gk = dict(x=ptr(out), dtype=dt, out_dtype=dt, n=n, HW=H * W, C=Cout, C1=0, groups=32, silu=1, splits=splits, eps=1e-5,
              gamma=ptr(gamma), beta=ptr(beta), ws=ptr(ws))
    route = lib.dc_groupnorm_variant(L.GroupnormParams(y=ptr(yb), qstats=ptr(qs), qparts=parts, **gk)).decode()
    if shape == (2, 64, 32, 384):
        assert route == "qfold+apply"
    elif shape == (2, 256, 128, 128):
        assert route == "qfold+span" and lib.dc_groupnorm_variant(L.GroupnormParams(y=ptr(ya), **gk)) == b"stats+apply"
    else:       # below 1 MiB per sample: one workgroup per sample, or the span kernel where DCAMD_GN_SPAN asks for it
        assert route == ("span" if os.environ.get("DCAMD_GN_SPAN") is not None else "image")
    L.check(lib.dc_groupnorm(L.GroupnormParams(y=ptr(ya), **gk), L.stream_ptr()), "gn")
    L.check(lib.dc_groupnorm(L.GroupnormParams(y=ptr(yb), qstats=ptr(qs), qparts=parts, **gk), L.stream_ptr()), "gn qstats")
    torch.cuda.synchronize()
    ref = F.silu(F.group_norm(of.permute(0, 3, 1, 2), 32, gamma, beta, 1e-5)).permute(0, 2, 3, 1)
    tol = {L.DC_F32: 2e-5, L.DC_BF16: 1e-2, L.DC_F16: 2e-3}[dt]
    assert maxrel(yb.float(), ref) < tol, maxrel(yb.float(), ref)
    assert maxrel(yb.float(), ya.float()) < tol
    # refused where the halo kernel does not run (stride 2), for a GroupNorm whose groups are not whole quads, and for a part count
    # that does not divide the sample
    p2 = L.IgemmParams(**dict(kw, stride=2, Hout=H // 2, Wout=W // 2, residual=None, qstats=ptr(qs)))
    assert lib.dc_igemm_qstats_parts(p2) == 0 and lib.dc_igemm(p2, L.stream_ptr()) == -6
    assert lib.dc_groupnorm(L.GroupnormParams(y=ptr(yb), qstats=ptr(qs), qparts=parts, **dict(gk, groups=Cout // 2)), L.stream_ptr()) != 0
    assert lib.dc_groupnorm(L.GroupnormParams(y=ptr(yb), qstats=ptr(qs), qparts=7, **gk), L.stream_ptr()) != 0


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("shape", [(3, 8, 8, 128), (2, 16, 16, 256), (2, 32, 32, 128), (5, 8, 16, 128), (3, 16, 8, 384), (9, 8, 8, 256),
                                   (21, 4, 4, 256), (3, 4, 4, 128), (70, 4, 4, 128), (5, 2, 2, 128)])   # 4x4: mosaic halo patches; 2x2: tap-gather kernel
def test_upsample_conv_as_four_phases(dt, shape):
    """dc_igemm up4: nearest-2x upsample + 3x3 conv == four 2x2-tap convs of the low-resolution tensor with phase-summed
    weights (engine.pack_up4).  Checked against F.conv2d(F.interpolate(x)), together with the quad statistics."""
    torch.manual_seed(31)
    n, H, W, Cout = shape
    g = E.bke(dt)
    C0 = 3 * g
    q = lambda t: t.to(TD[dt]).float()
    x0 = q(torch.randn(n, C0, H, W))
    w = q(torch.randn(Cout, C0, 3, 3) / (3 * C0 ** 0.5))
    b = torch.randn(Cout)
    ref = F.conv2d(F.interpolate(x0, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    lib = L.lib()
    a0, bd = nhwc(x0, dt), b.to(DEV)
    W4 = E.pack_up4(w, dt, DEV)
    assert tuple(W4.shape) == (4, lib.dc_igemm_cout_pad(Cout, 128), 4 * C0)
    out = torch.full((n, 2 * H, 2 * W, Cout), float("nan"), dtype=TD[dt], device=DEV)
    kw = dict(dtype=dt, taps=9, stride=1, upsample=1, n_img=n, Hin=2 * H, Win=2 * W, Hout=2 * H, Wout=2 * W, src0=ptr(a0), C0=C0,
              W=ptr(W4), Cout=Cout, tile_n=128, bias=ptr(bd), out=ptr(out), out_dtype=dt, out_ld=Cout, up4=1)
    p = L.IgemmParams(**kw)
    halo = H >= 8 and W >= 8          # quad statistics come from >= 8x8 halo patches only
    on_halo = halo or (H == 4 and W == 4 and os.environ.get("DCAMD_NO_MOSAIC") is None)    # 4x4 sources: mosaic patches of 32 images
    assert lib.dc_igemm_up4_ok(p) == 1
    assert lib.dc_igemm_variant(p).decode().startswith("conv3_up4<" if on_halo else "igemm_pipe_up4<")
    parts = lib.dc_igemm_qstats_parts(p)
    assert parts == (4 * max(1, H * W // 128) if halo else 0)     # the tap-gather kernel and the mosaic form no quad statistics
    qs = torch.full((n, max(parts, 1), Cout // 4, 2), float("nan"), device=DEV)
    run_igemm(**(dict(kw, qstats=ptr(qs)) if halo else kw))
    got = out.float().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    assert maxrel(got, ref) < TOL[dt], maxrel(got, ref)
    # a residual is refused (the upsample convs of the UNets carry a bias only)
    p2 = L.IgemmParams(**dict(kw, residual=ptr(out), res_dtype=dt, res_ld=Cout))
    assert lib.dc_igemm_up4_ok(p2) == 0 and lib.dc_igemm(p2, L.stream_ptr()) == -6
    if not halo:
        return
    assert torch.isfinite(qs).all()
    m_got, m2_got = _merge_quad_records(qs, 4 * 4 * H * W // parts)
    px = out.double().reshape(n, 4 * H * W, Cout // 4, 4)
    m_ref = px.mean((1, 3))
    m2_ref = ((px - m_ref[:, None, :, None]) ** 2).sum((1, 3))
    assert (m_got - m_ref).abs().max().item() < (1e-5 if dt == L.DC_F32 else 2e-3) * max(1.0, m_ref.abs().max().item())
    assert ((m2_got - m2_ref).abs() / m2_ref).max().item() < (1e-4 if dt == L.DC_F32 else 1e-2)


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("shape", [(9, 16, 16, 128, 128, 16), (3, 32, 32, 64, 256, 32), (40, 16, 16, 128, 128, 32)])
def test_upsample_conv_normalises_its_own_output(dt, shape):
    """Producer-side GroupNorm on the four-phase upsample conv (dc_igemm up4 + pn_*): the output sample is written by the four phases
    of every low-resolution tile, which exchange their quad records like the tiles of a plain conv do.  Raw output and records equal
    the plain up4 launch bit for bit; the normalised output equals dc_groupnorm on those records / torch within the dtype's rounding."""
    torch.manual_seed(88)
    n, H, W, Ci, Co, groups = shape
    lib = L.lib()
    q = lambda t: t.to(TD[dt]).float()
    x0 = q(torch.randn(n, Ci, H, W))
    w = q(torch.randn(Co, Ci, 3, 3) / (3 * Ci ** 0.5))
    b = torch.randn(Co).to(DEV)
    a0, W4 = nhwc(x0, dt), E.pack_up4(w, dt, DEV)
    Ho, Wo = 2 * H, 2 * W
    kw = dict(dtype=dt, taps=9, stride=1, upsample=1, n_img=n, Hin=Ho, Win=Wo, Hout=Ho, Wout=Wo, src0=ptr(a0), C0=Ci, W=ptr(W4), Cout=Co, tile_n=128,
              bias=ptr(b), out_dtype=dt, out_ld=Co, up4=1)
    o_ref = torch.full((n, Ho, Wo, Co), float("nan"), device=DEV).to(TD[dt])
    parts = lib.dc_igemm_qstats_parts(L.IgemmParams(out=ptr(o_ref), **kw))
    assert parts == Ho * Wo // 128
    q_ref = torch.full((n, parts, Co // 4, 2), float("nan"), device=DEV)
    run_igemm(out=ptr(o_ref), qstats=ptr(q_ref), **kw)
    gamma, beta = (torch.randn(Co) * 0.5 + 1).to(DEV), torch.randn(Co).to(DEV)
    splits = lib.dc_groupnorm_splits(n, Ho * Wo, Co)
    wsb = torch.zeros(lib.dc_groupnorm_ws_floats(n, groups, splits), device=DEV)
    y_ref = torch.empty_like(o_ref)
    L.check(lib.dc_groupnorm(L.GroupnormParams(x=ptr(o_ref), y=ptr(y_ref), dtype=dt, out_dtype=dt, n=n, HW=Ho * Wo, C=Co, C1=0, groups=groups, silu=1,
                                               splits=splits, eps=1e-5, gamma=ptr(gamma), beta=ptr(beta), ws=ptr(wsb), qstats=ptr(q_ref), qparts=parts),
                             L.stream_ptr()), "gn")
    o = torch.full((n, Ho, Wo, Co), float("nan"), device=DEV).to(TD[dt])
    y = torch.full((n, Ho, Wo, Co), float("nan"), device=DEV).to(TD[dt])
    q_o = torch.full((n, parts, Co // 4, 2), float("nan"), device=DEV)
    cnt = torch.zeros(n * ((Co + 127) // 128), dtype=torch.int32, device=DEV)
    pp = L.IgemmParams(out=ptr(o), qstats=ptr(q_o), pn_out=ptr(y), pn_gamma=ptr(gamma), pn_beta=ptr(beta), pn_cnt=ptr(cnt), pn_ld=Co, pn_groups=groups,
                       pn_silu=1, pn_eps=1e-5, **kw)
    assert lib.dc_igemm_pn_ok(pp) == 1
    assert lib.dc_igemm_variant(pp).decode() == "conv3_up4<%s,4w,pn>" % {L.DC_F32: "f32", L.DC_BF16: "bf16", L.DC_F16: "f16"}[dt]
    for _ in range(2):
        L.check(lib.dc_igemm(pp, L.stream_ptr()), "upsample conv with producer-side GroupNorm")
    torch.cuda.synchronize()
    assert lib.dc_pn_timeouts() == 0
    assert torch.equal(cnt, torch.full_like(cnt, 2 * 4 * (H * W // 256)))
    assert torch.equal(q_o, q_ref) and torch.equal(o, o_ref)
    assert torch.isfinite(y.float()).all()
    assert maxrel(y, y_ref) < {L.DC_F32: 5e-6, L.DC_BF16: 1.6e-2, L.DC_F16: 2e-3}[dt], maxrel(y, y_ref)
    ref = F.conv2d(F.interpolate(x0, scale_factor=2.0, mode="nearest"), w, b.cpu(), padding=1)
    yn = F.silu(F.group_norm(ref, groups, gamma.cpu(), beta.cpu(), 1e-5))
    assert maxrel(y.float().cpu(), yn.permute(0, 2, 3, 1)) < {L.DC_F32: 3e-5, L.DC_BF16: 1.2e-2, L.DC_F16: 2e-3}[dt]
    # a source below 16x16 runs on the 8-wave patch, which does not exchange statistics: refused
    small = L.IgemmParams(**dict(kw, n_img=n, Hin=16, Win=16, Hout=16, Wout=16), out=ptr(o), qstats=ptr(q_o), pn_out=ptr(y), pn_gamma=ptr(gamma),
                          pn_beta=ptr(beta), pn_cnt=ptr(cnt), pn_ld=Co, pn_groups=groups, pn_silu=1, pn_eps=1e-5)
    assert lib.dc_igemm_pn_ok(small) == 0


@pytest.mark.parametrize("shape", [(5, 10, 50, 50, 3), (3, 6, 7, 3, 2), (2, 100, 9, 9, 1), (4, 1000, 4, 2, 7)])
def test_stage_topk_and_argmin_match_torch(shape):
    """dc_stage_topk / dc_reduce_argmin: mean over the evaluated trials + k smallest classes per image (reference
    diffusion_classifier.py:718-721), unevaluated (+inf) classes never kept."""
    BS, Cn, T, t_end, k = shape
    torch.manual_seed(41)
    err = torch.rand(BS, Cn, T) * 100 + 1000
    dead = torch.rand(BS, Cn) < 0.3
    dead[:, : k + 1] = False                                   # at least k + 1 live classes per image
    err[dead] = float("inf")
    lib = L.lib()
    e = err.to(DEV)
    keep = torch.full((BS, k), -1, dtype=torch.int32, device=DEV)
    means = torch.zeros(BS, Cn, device=DEV)
    L.check(lib.dc_stage_topk(ptr(e), BS, Cn, T, t_end, k, ptr(keep), ptr(means), L.stream_ptr()), "dc_stage_topk")
    ref_mean = err[:, :, :t_end].mean(2)
    ref_keep = torch.topk(ref_mean, k, dim=1, largest=False).indices
    fin = torch.isfinite(ref_mean)
    assert torch.equal(torch.isfinite(means.cpu()), fin)
    assert ((means.cpu()[fin] - ref_mean[fin]).abs() / ref_mean[fin]).max().item() < 1e-6
    assert torch.equal(keep.cpu().long(), ref_keep)
    lab = torch.full((BS,), -1, dtype=torch.int64, device=DEV)
    L.check(lib.dc_reduce_argmin(ptr(e), BS, Cn, T, t_end, ptr(lab), None, L.stream_ptr()), "dc_reduce_argmin")
    assert torch.equal(lab.cpu(), ref_mean.argmin(1))
    # exact ties go to the lower class id
    e2 = torch.full((2, 5, 3), 7.0, device=DEV)
    k2 = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    L.check(lib.dc_stage_topk(ptr(e2), 2, 5, 3, 3, 3, ptr(k2), None, L.stream_ptr()), "dc_stage_topk")
    assert k2.cpu().tolist() == [[0, 1, 2], [0, 1, 2]]
    assert lib.dc_stage_topk(ptr(e), BS, Cn, T, t_end, Cn + 1, ptr(keep), None, L.stream_ptr()) == -2     # k > classes
    # NaN means (an overflowed f16 forward: inf - inf) sort LAST, after +inf, as in torch.topk(largest=False); every round still
    # yields a valid class id — also when fewer than k classes are not NaN, and when every class is NaN
    e3 = torch.tensor([[[5.0], [float("nan")], [float("inf")], [3.0], [float("nan")], [-0.0], [0.0]],
                       [[float("nan")]] * 7,
                       [[float("nan")], [2.0], [float("nan")], [float("nan")], [float("nan")], [float("nan")], [float("nan")]]]).to(DEV)
    for k3 in (1, 4, 7):
        k3t = torch.full((3, k3), -1, dtype=torch.int32, device=DEV)
        L.check(lib.dc_stage_topk(ptr(e3), 3, 7, 1, 1, k3, ptr(k3t), None, L.stream_ptr()), "dc_stage_topk")
        got = k3t.cpu().long()
        assert int(got.min()) >= 0 and int(got.max()) < 7
        assert all(len(set(r)) == k3 for r in got.tolist())                       # k distinct classes per image
        assert got[0].tolist() == [5, 6, 3, 0, 2, 1, 4][:k3]                       # -0 == +0 (lower id first), ..., inf, then the NaNs by id
        assert got[1].tolist() == list(range(k3)) and got[2].tolist() == [1, 0, 2, 3, 4, 5, 6][:k3]
    lab3 = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    L.check(lib.dc_reduce_argmin(ptr(e3), 3, 7, 1, 1, ptr(lab3), None, L.stream_ptr()), "dc_reduce_argmin")
    assert lab3.cpu().tolist() == [5, 0, 1]
    # a class list that is not a class list (a foreign caller) must not index out of errors[]: dc_stage_maps clamps it
    bad = torch.tensor([[0x7fffffff, -3]], dtype=torch.int32, device=DEV)
    mp = torch.full((1, 4), -7, dtype=torch.int32, device=DEV)
    L.check(lib.dc_stage_maps(ptr(bad), 1, 7, 2, 2, 1, 1, 0, 1, 1, 1, 14, ptr(mp), L.stream_ptr()), "dc_stage_maps")
    assert mp.cpu().tolist() == [[6, 0, (0 * 7 + 6) * 2 + 1, (0 * 7 + 0) * 2 + 1]]


@pytest.mark.parametrize("w", [1.5, 0.1, 0.7000000000000001, 1e-8, 2.2, -1.0])
def test_ddpm_step_equals_the_torch_expressions(w):
    """dc_ddpm_step (reference ddpm_sampler_step :175-208 + the update :262-266 as one pass): bit-equal to the reference's torch
    expressions for the same fp32 scalars — eps and v parameterisation, image-shaped and DiT-patch prediction layouts, the noise
    update and the clipped mean of the last pass; several guidance weights (1 + w is formed as a Python double and rounded to fp32 once,
    as torch does: for w = 1e-8 or 0.1 that is not 1.f + (float)w)."""
    torch.manual_seed(44)
    N, Cc, H, W = 3, 4, 8, 8
    z, noise = torch.randn(N, Cc, H, W), torch.randn(N, Cc, H, W)
    pc, pu = torch.randn(N, Cc, H, W) * 2, torch.randn(N, Cc, H, W) * 2
    lt, ls = torch.tensor(-1.25), torch.tensor(0.75)
    c = -torch.special.expm1(lt - ls)
    a_t, a_s = torch.sqrt(torch.sigmoid(lt)), torch.sqrt(torch.sigmoid(ls))
    s_t, s_s = torch.sqrt(torch.sigmoid(-lt)), torch.sqrt(torch.sigmoid(-ls))
    sd = torch.sqrt((s_s ** 2) * c)
    for v_param in (0, 1):
        pred = (1 + w) * pc - w * pu
        xp = a_t * z - s_t * pred if v_param else (z - s_t * pred) / a_t
        mu = a_s * (z * (1 - c) / a_t + c * torch.clamp(xp, -1, 1))
        for patch, ld in ((0, 8), (2, 16)):
            pair = torch.zeros(2 * N, H, W, ld) if not patch else torch.zeros(2 * N, H // patch, W // patch, ld)
            for b in range(N):
                for u, src in ((2 * b, pc[b]), (2 * b + 1, pu[b])):
                    if not patch:
                        pair[u, :, :, :Cc] = src.permute(1, 2, 0)
                    else:      # token (ty, tx), k = (py * p + px) * C + c
                        pair[u] = src.reshape(Cc, H // patch, patch, W // patch, patch).permute(1, 3, 2, 4, 0).reshape(H // patch, W // patch, ld)
            zd, nd, pd = z.to(DEV), noise.to(DEV), pair.to(DEV)
            for nz, want in ((nd, mu + noise * sd), (None, torch.clamp(mu, -1, 1))):
                out = torch.full((N, Cc, H, W), 9.0, device=DEV)
                p = L.DdpmStepParams(z=ptr(zd), pred=ptr(pd), noise=ptr(nz), out=ptr(out), n=N, C=Cc, H=H, W=W, ld=ld, patch=patch,
                                     v_param=v_param, w=w, one_plus_w=float(1.0 + w), alpha_t=float(a_t), sigma_t=float(s_t), alpha_s=float(a_s), c=float(c), sd=float(sd))
                L.check(L.lib().dc_ddpm_step(p, L.stream_ptr()), "dc_ddpm_step")
                assert torch.equal(out.cpu(), want), (v_param, patch, (out.cpu() - want).abs().max())


@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
def test_stage_maps_match_the_host_built_control_blocks(world, rank):
    """dc_stage_maps: next stage's (pair, class) -> work-unit maps from the surviving classes, against the index arithmetic
    classify does on the host for stage 0 (scoring.py `index_blocks`, from _HipRunner.run_stage)."""
    from diffusion_classifier_amd import dist as D
    from helpers import expected_unit_maps
    BS, Cn, T, k, t0, t1, n_bj = 5, 9, 12, 3, 4, 12, 7
    torch.manual_seed(43)
    keep = torch.stack([torch.randperm(Cn)[:k] for _ in range(BS)]).to(torch.int32)
    pairs = D.local_pairs(t0, t1, BS, rank, world)
    n_mb = -(-len(pairs) // n_bj)
    U, dump = n_bj * k, BS * Cn * T
    maps = torch.full((n_mb, 2 * U), -7, dtype=torch.int32, device=DEV)
    kd = keep.to(DEV)
    L.check(L.lib().dc_stage_maps(ptr(kd), BS, Cn, T, k, t0, len(pairs), rank, world, n_bj, n_mb, dump, ptr(maps), L.stream_ptr()), "dc_stage_maps")
    got = maps.cpu()
    cl, oi = expected_unit_maps(pairs, keep, n_bj, Cn, T, dump)
    for m in range(n_mb):
        assert torch.equal(got[m, :U].long(), cl[m]) and torch.equal(got[m, U:].long(), oi[m])


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
def test_weight_packers_match_their_documented_layouts(dt):
    """dc_pack_weights_{matrix,conv3x3,up4,geglu} / dc_fold_layernorm_bias (include/dcamd.h "weight packing") against the same
    layouts written out in torch: bit-exact (the only arithmetic is the fp32 tap sums of up4 and the LayerNorm folds)."""
    torch.manual_seed(61)
    td = TD[dt]
    lib = L.lib()
    # matrix: row padding to the N tile, column padding, gamma folded into the columns
    w = torch.randn(200, 72)
    got = E.pack_matrix(w, dt, DEV, kpad=96).cpu()
    ref = torch.zeros(256, 96)
    ref[:200, :72] = w
    assert got.shape == (256, 96) and torch.equal(got, ref.to(td))
    assert lib.dc_packed_bytes(200, 96, dt, 128) == got.numel() * got.element_size()
    gam = torch.randn(72)
    assert torch.equal(E.pack_matrix(w, dt, DEV, col_scale=gam).cpu()[:200], (w * gam[None, :]).to(td))
    assert tuple(E.pack_matrix(w[:5], dt, DEV, tile_n=32).shape) == (32, 72)
    # conv3x3: k = tap * C + c, channel slices for split skip-connection convs
    wc = torch.randn(40, 24, 3, 3)
    full = wc.permute(0, 2, 3, 1).reshape(40, 9 * 24)
    g3 = E.pack_conv3x3(wc, dt, DEV, kpad=256).cpu()
    assert g3.shape == (128, 256) and torch.equal(g3[:40, :216], full.to(td)) and not g3[40:].any() and not g3[:, 216:].any()
    lo = E.pack_conv3x3(wc, dt, DEV, c_lo=0, c_hi=8).cpu()
    hi = E.pack_conv3x3(wc, dt, DEV, c_lo=8).cpu()
    assert torch.equal(lo[:40], wc[:, :8].permute(0, 2, 3, 1).reshape(40, 72).to(td))
    assert torch.equal(hi[:40], wc[:, 8:].permute(0, 2, 3, 1).reshape(40, 144).to(td))
    # up4: phase-summed 2x2 taps, summed in fp32 before rounding
    sets = (((0,), (1, 2)), ((0, 1), (2,)))
    phases = []
    for a in range(2):
        for b in range(2):
            taps = []
            for dy in range(2):
                for dx in range(2):
                    acc = 0
                    for ky in sets[a][dy]:
                        for kx in sets[b][dx]:
                            acc = acc + wc[:, :, ky, kx]
                    taps.append(acc)
            phases.append(torch.cat(taps, 1))
    g4 = E.pack_up4(wc, dt, DEV).cpu()
    assert g4.shape == (4, 128, 96) and torch.equal(g4[:, :40], torch.stack(phases).to(td)) and not g4[:, 40:].any()
    # GEGLU: value / gate rows interleaved in 16-row blocks, with and without the LayerNorm fold
    nh, K = 48, 64
    wg, bg = torch.randn(2 * nh, K), torch.randn(2 * nh)
    perm = E.geglu_perm(nh)
    pw, pb = E.pack_geglu(wg, bg, dt, DEV)
    assert torch.equal(pw.cpu()[:2 * nh], wg[perm].to(td)) and torch.equal(pb.cpu(), bg[perm])
    gam, bet = torch.randn(K), torch.randn(K)
    pwf, pbf = E.pack_geglu(wg, bg, dt, DEV, ln_gamma=gam, ln_beta=bet)
    assert torch.equal(pwf.cpu()[:2 * nh], (wg * gam[None, :])[perm].to(td))
    assert (pbf.cpu() - (bg + wg @ bet)[perm]).abs().max().item() < 1e-4
    fb = E.fold_layernorm_bias(wg, None, bet, DEV).cpu()
    assert (fb - wg @ bet).abs().max().item() < 1e-4
    # workspace queries
    gp = L.GroupnormParams(n=3, HW=64, C=128, C1=0, groups=32, splits=0)
    assert lib.dc_workspace_bytes_groupnorm(gp) == 4 * lib.dc_groupnorm_ws_floats(3, 32, lib.dc_groupnorm_splits(3, 64, 128))
    assert lib.dc_workspace_bytes_igemm(L.IgemmParams()) == 0 and lib.dc_workspace_bytes_attention(L.AttentionParams()) == 0


@pytest.mark.parametrize("dt", [L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("n,heads", [(1, 8), (5, 4), (300, 8)])
def test_tblock_front_matches_the_separate_launches(dt, n, heads):
    """The attention half of a transformer block in one launch (dc_tblock_front: proj_in -> LayerNorm -> q/k/v -> attention -> to_out +
    class vector + residual, 64 tokens x 256 channels) against (a) the chain of separate C-ABI launches it replaces and (b) a plain
    PyTorch fp32 reference with the same 16-bit rounding points.  The fused kernel rounds where the chain stores, so only accumulation
    order differs: bound = a few output ulps (bf16 2^-8, f16 2^-11 relative) on values of order 1."""
    torch.manual_seed(40 + n)
    lib = L.lib()
    Lq, Cc, ncls = 64, 256, 3
    td = TD[dt]
    q = lambda t: t.to(td).float()
    x = q(torch.randn(n, Lq, Cc))
    Wp, Wqkv, Wo = (q(torch.randn(r, Cc) / Cc ** 0.5) for r in (Cc, 3 * Cc, Cc))
    bp, bo = 0.1 * torch.randn(Cc), 0.1 * torch.randn(Cc)
    g, b = 1 + 0.2 * torch.randn(Cc), 0.1 * torch.randn(Cc)
    cvec = torch.randn(ncls, Cc)
    cmap = torch.randint(0, ncls, (n,), dtype=torch.int32)
    # (b) fp32 reference, rounding where the chain stores
    h = q(x @ Wp.T + bp)
    hn = q(F.layer_norm(h, (Cc,), g, b, 1e-5))
    qkv = q(hn @ Wqkv.T)
    sh = lambda z: z.view(n, Lq, heads, Cc // heads).transpose(1, 2)
    sc = (sh(qkv[..., :Cc]) @ sh(qkv[..., Cc:2 * Cc]).transpose(-1, -2)) * (Cc // heads) ** -0.5
    p_ = torch.softmax(sc, -1)
    o = q((p_ @ sh(qkv[..., 2 * Cc:])).transpose(1, 2).reshape(n, Lq, Cc))
    ref = ((o @ Wo.T + bo) + cvec[cmap.long()][:, None, :]) + h
    # device operands
    xd = x.to(td).to(DEV)
    Wpd, Wqd, Wod = (E.pack_matrix(w, dt, DEV) for w in (Wp, Wqkv, Wo))
    f32 = lambda t: t.float().contiguous().to(DEV)
    bpd, bod, gd, bd, cvd, cmd = f32(bp), f32(bo), f32(g), f32(b), f32(cvec), cmap.to(DEV)
    out = torch.full((n, Lq, Cc), float("nan"), dtype=td, device=DEV)
    tp = L.TblockFrontParams(x=ptr(xd), Wp=ptr(Wpd), bp=ptr(bpd), ln_g=ptr(gd), ln_b=ptr(bd), Wqkv=ptr(Wqd), Wo=ptr(Wod), bo=ptr(bod),
                             rowvec=ptr(cvd), rowvec_map=ptr(cmd), out=ptr(out), dtype=dt, n=n, L=Lq, C=Cc, heads=heads, ldx=Cc, ld_out=Cc,
                             rowvec_ld=Cc, ln_eps=1e-5, scale=(Cc // heads) ** -0.5)
    assert lib.dc_tblock_front_ok(tp) == 1
    L.check(lib.dc_tblock_front(tp, L.stream_ptr()), "dc_tblock_front")
    torch.cuda.synchronize()
    # (a) the chain of separate launches
    M = n * Lq
    gemm = lambda src, W, Cout, **kw: run_igemm(dtype=dt, taps=1, stride=1, upsample=0, n_img=n, Hin=8, Win=8, Hout=8, Wout=8, src0=ptr(src), C0=Cc,
                                                ld0=Cc, W=ptr(W), Cout=Cout, tile_n=128, out_dtype=dt, out_ld=Cout, **kw)
    hd = torch.empty(M, Cc, dtype=td, device=DEV)
    gemm(xd, Wpd, Cc, bias=ptr(bpd), out=ptr(hd))
    hnd = torch.empty_like(hd)
    L.check(lib.dc_layernorm(L.LayernormParams(x=ptr(hd), y=ptr(hnd), dtype=dt, out_dtype=dt, rows=M, C=Cc, rows_per_sample=Lq, eps=1e-5,
                                               gamma=ptr(gd), beta=ptr(bd)), L.stream_ptr()), "ln")
    qkvd = torch.empty(M, 3 * Cc, dtype=td, device=DEV)
    gemm(hnd, Wqd, 3 * Cc, out=ptr(qkvd))
    od = torch.empty_like(hd)
    L.check(lib.dc_attention(L.AttentionParams(q=qkvd.data_ptr(), k=qkvd.data_ptr() + 2 * Cc, v=qkvd.data_ptr() + 4 * Cc, out=ptr(od), dtype=dt, n=n,
                                               L=Lq, heads=heads, d=Cc // heads, ld_qkv=3 * Cc, ld_out=Cc, scale=(Cc // heads) ** -0.5), L.stream_ptr()), "attn")
    chain = torch.empty_like(hd)
    gemm(od, Wod, Cc, bias=ptr(bod), rowvec=ptr(cvd), rowvec_map=ptr(cmd), rowvec_ld=Cc, residual=ptr(hd), res_dtype=dt, res_ld=Cc, out=ptr(chain))
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    ulp = 2.0 ** -8 if dt == L.DC_BF16 else 2.0 ** -11
    scale_ = ref.abs().max().item()
    e_ref = (got - ref).abs().max().item() / scale_
    e_chain = (got - chain.float().cpu().view(n, Lq, Cc)).abs().max().item() / scale_
    print(f"dc_tblock_front n={n} heads={heads} dt={dt}: max err / max|ref| vs fp32 reference {e_ref:.2e}, vs the chain of launches {e_chain:.2e} (bound {3 * ulp:.2e})")
    assert e_ref < 3 * ulp and e_chain < 3 * ulp
    # shapes it does not serve are refused, not mis-computed
    bad = L.TblockFrontParams(dtype=dt, n=n, L=16, C=512, heads=8, ldx=512, ld_out=512)
    assert lib.dc_tblock_front_ok(bad) == 0


@pytest.mark.parametrize("dt", [L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("M,K,NH,rowln", [(96 * 5, 256, 256, True), (1000, 256, 1024, False), (96 * 3 + 7, 256, 384, True), (64 * 3 + 7, 512, 384, True), (4096, 512, 2048, True)])
def test_geglu_projection_kernel(dt, M, K, NH, rowln):
    """The GEGLU projection of the UNet transformer blocks (activation-stationary kernel, K = 256 / 512) against PyTorch fp32 on the same rounded
    operands — plain and with the row LayerNorm folded in, M ragged against the 96- / 64-row workgroups (rows past M are fetched as duplicates
    and never stored: the elements behind the output stay untouched) — and launched twice: the two results must be bit-identical (a trimmed
    variant of this kernel, round 4, computed the right values within tolerance and different ones on every launch once two workgroups shared
    a CU; only the model-level repeat test caught it)."""
    torch.manual_seed(M + K)
    td = TD[dt]
    q = lambda t: t.to(td).float()
    x = q(torch.randn(M, K) * (2.0 if rowln else 1.0) + (0.3 if rowln else 0.0))
    w, b = q(torch.randn(2 * NH, K) / K ** 0.5), 0.2 * torch.randn(2 * NH)
    a = q(F.layer_norm(x, (K,), eps=1e-5)) if rowln else x
    u, g = (a @ w.t() + b).chunk(2, dim=-1)
    ref = u * F.gelu(g)
    perm = E.geglu_perm(NH)
    Wp, bp = E.pack_matrix(w[perm], dt, DEV), b[perm].contiguous().to(DEV)
    xd = x.to(td).to(DEV)
    guard = 4096                                       # elements behind the output that must stay untouched
    buf = torch.full((M * NH + guard,), 7.0, dtype=td, device=DEV)
    kw = dict(dtype=dt, taps=1, stride=1, upsample=0, n_img=1, Hin=M, Win=1, Hout=M, Wout=1, src0=ptr(xd), C0=K, ld0=K, W=ptr(Wp), Cout=2 * NH,
              tile_n=128, bias=ptr(bp), act=L.ACT_GEGLU, out=ptr(buf), out_dtype=dt, out_ld=NH, ln_eps=1e-5 if rowln else 0.0)
    assert "xreg" in L.lib().dc_igemm_variant(L.IgemmParams(**kw)).decode()
    run_igemm(**kw)
    got = buf[: M * NH].float().cpu().view(M, NH)
    assert torch.isfinite(got).all() and bool((buf[M * NH:] == 7.0).all()), "rows past M must not be stored"
    err = maxrel(got, ref)
    print(f"GEGLU projection M={M} K={K} hidden={NH} dt={dt} rowln={rowln}: max err / max|ref| {err:.2e} (bound {TOL[dt]:.1e})")
    assert err < TOL[dt], err
    first = buf.clone()
    run_igemm(**kw)
    assert torch.equal(first.view(torch.int16), buf.view(torch.int16)), "a repeated launch must give the same bits"


@pytest.mark.parametrize("which", ["geglu_k256", "geglu_k512", "tblock_front"])
def test_transformer_kernels_are_deterministic_at_bench_size(which):
    """Launch-to-launch bit-identity at the size the bench runs (8000 samples x 64 tokens: more workgroups than the chip holds at once, two per
    CU), other traffic in between: dc_tblock_front and the GEGLU projections."""
    torch.manual_seed(77)
    lib, dt, td = L.lib(), L.DC_BF16, torch.bfloat16
    outs = []
    if which == "tblock_front":
        n, Lq, Cc, heads = 8000, 64, 256, 8
        x = torch.randn(n, Lq, Cc, device=DEV).to(td)
        Wp, Wq, Wo = (E.pack_matrix(torch.randn(r, Cc) / Cc ** 0.5, dt, DEV) for r in (Cc, 3 * Cc, Cc))
        bp, bo, g, b = (torch.randn(Cc, device=DEV) * 0.1 for _ in range(4))
        cv = torch.randn(10, Cc, device=DEV)
        cm = (torch.arange(n, device=DEV, dtype=torch.int32) % 10).contiguous()
        for _ in range(3):
            out = torch.empty(n, Lq, Cc, dtype=td, device=DEV)
            tp = L.TblockFrontParams(x=ptr(x), Wp=ptr(Wp), bp=ptr(bp), ln_g=ptr(g), ln_b=ptr(b), Wqkv=ptr(Wq), Wo=ptr(Wo), bo=ptr(bo), rowvec=ptr(cv),
                                     rowvec_map=ptr(cm), out=ptr(out), dtype=dt, n=n, L=Lq, C=Cc, heads=heads, ldx=Cc, ld_out=Cc, rowvec_ld=Cc,
                                     ln_eps=1e-5, scale=(Cc // heads) ** -0.5)
            torch.randn(1 << 22, device=DEV).sum()
            L.check(lib.dc_tblock_front(tp, L.stream_ptr()), "dc_tblock_front")
            outs.append(out)
    else:
        M, K, NH = (512000, 256, 1024) if which == "geglu_k256" else (128000, 512, 2048)
        x = (torch.randn(M, K, device=DEV) * 1.5 + 0.2).to(td)
        Wp, bp = E.pack_geglu(torch.randn(2 * NH, K) / K ** 0.5, torch.randn(2 * NH) * 0.1, dt, DEV, ln_gamma=torch.ones(K), ln_beta=torch.zeros(K))
        for _ in range(3):
            out = torch.empty(M, NH, dtype=td, device=DEV)
            torch.randn(1 << 22, device=DEV).sum()
            run_igemm(dtype=dt, taps=1, stride=1, upsample=0, n_img=1, Hin=M, Win=1, Hout=M, Wout=1, src0=ptr(x), C0=K, ld0=K, W=ptr(Wp), Cout=2 * NH,
                      tile_n=128, bias=ptr(bp), act=L.ACT_GEGLU, out=ptr(out), out_dtype=dt, out_ld=NH, ln_eps=1e-5)
            outs.append(out)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), f"{which}: a repeated launch differs in {(o.view(torch.int16) != outs[0].view(torch.int16)).sum().item()} elements"
