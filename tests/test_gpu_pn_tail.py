"""GPU: the tail fold (dc_conv3_pn_tail; csrc/epi_pn.h) at op level — the last ResNet conv of a UNet with conv_norm_out + SiLU and
conv_out folded into its epilogue — against torch fp32 on the CPU of

    conv3x3 (+ bias, per-sample row vector, mapped residual, 1x1 side source) -> GroupNorm -> SiLU -> round to T -> conv_out in fp32

from the same rounded operands.  Bound: the error of the two-launch route (producer-normalising conv + conv3_thin) against that same
reference on the same inputs, times two — the folded route feeds the MFMA the very bits the normalised store holds, so only the order
of the fp32 sums differs (channels inside the MFMA, then the two channel halves, then the nine taps, then the neighbouring tiles).
Both figures are printed."""
import pytest
import torch
import torch.nn.functional as F

from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
C, GROUPS, CO, SIDE, EPS = 128, 32, 3, 128, 1e-5
# 3 x 32x32: four tiles per sample, the grid padded to 8 groups (surplus workgroups leave), pixels on a seam get two or three sums;
# 2 x 16x16: a sample is one tile, the ring is empty; 1 x 64x64: 16 tiles (2 x 8), interior tiles with 8 neighbours, seam crossings with 4 sums
SHAPES = {"3x32x32": (3, 32, 32), "2x16x16": (2, 16, 16), "1x64x64": (1, 64, 64)}


def ptr(t):
    return None if t is None else t.data_ptr()


def maxrel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def nhwc(x, dt):
    return x.permute(0, 2, 3, 1).contiguous().to(TD[dt]).to(DEV)


class Problem:
    """Operands of one case on the device, the conv's dc_igemm_params fields, and the CPU reference (computed once)."""

    def __init__(self, dt, n, H, W, Cout=C, Co=CO, seed=91):
        torch.manual_seed(seed)
        q = lambda t: t.to(TD[dt]).float()
        self.dt, self.n, self.H, self.W, self.Cout, self.Co = dt, n, H, W, Cout, Co
        n_src = 2
        smap = torch.tensor([i % n_src for i in range(n)], dtype=torch.int32)
        x = q(torch.randn(n_src, C, H, W))
        w = q(torch.randn(Cout, C, 3, 3) / (3 * C ** 0.5))
        b, rv = torch.randn(Cout), torch.randn(n, Cout) * 2
        r = q(torch.randn(n_src, Cout, H, W))
        xs = q(torch.randn(n_src, SIDE, H, W))
        ws2 = q(torch.randn(Cout, SIDE) / SIDE ** 0.5)
        gamma, beta = torch.randn(Cout) * 0.5 + 1, torch.randn(Cout)
        wo = q(torch.randn(Co, Cout, 3, 3) / (3 * Cout ** 0.5))
        bo = torch.randn(Co)
        self.t = dict(smap=smap.to(DEV), a0=nhwc(x, dt), Wp=E.pack_conv3x3(w, dt, DEV), b=b.to(DEV), rv=rv.to(DEV), r=nhwc(r, dt), a2=nhwc(xs, dt),
                      W2=E.pack_matrix(ws2, dt, DEV), gamma=gamma.to(DEV), beta=beta.to(DEV), bo=bo.to(DEV),
                      Wo=E.pack_conv3x3(wo, dt, DEV, 32), Wt=E.pack_tail(wo, dt, DEV) if Cout == 128 and Co <= 3 else torch.zeros(32, 128, dtype=TD[dt], device=DEV))
        t = self.t
        self.parts = H * W // 128
        self.qs = torch.zeros(n, self.parts, Cout // 4, 2, device=DEV)
        self.conv = dict(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(t["a0"]), C0=C, map0=ptr(t["smap"]),
                         W=ptr(t["Wp"]), Cout=Cout, tile_n=128, bias=ptr(t["b"]), rowvec=ptr(t["rv"]), rowvec_ld=Cout, out_dtype=dt, out_ld=Cout,
                         residual=ptr(t["r"]), res_map=ptr(t["smap"]), res_dtype=dt, res_ld=Cout,
                         src2=ptr(t["a2"]), map2=ptr(t["smap"]), W2=ptr(t["W2"]), C2=SIDE, ld2=SIDE, qstats=ptr(self.qs))
        idx = smap.long()
        v = F.conv2d(x[idx], w, b, padding=1) + rv[:, :, None, None] + torch.einsum("nchw,oc->nohw", xs[idx], ws2) + r[idx]
        y = q(F.silu(F.group_norm(v, GROUPS, gamma, beta, EPS)))
        self.ref = F.conv2d(y, wo, bo, padding=1).permute(0, 2, 3, 1).contiguous()

    def tail(self, pred, ring, cnt, **over):
        t = self.t
        return L.PnTailParams(**dict(dict(Wt=ptr(t["Wt"]), bias=ptr(t["bo"]), pred=ptr(pred), ring=ptr(ring), gamma=ptr(t["gamma"]), beta=ptr(t["beta"]),
                                          cnt=ptr(cnt), Co=self.Co, pred_ld=self.Co, groups=GROUPS, silu=1, eps=EPS), **over))

    def two_launch(self):
        """The separate route: producer-normalising conv, then the thin conv (whatever dc_igemm picks for it)."""
        t, dt, n, H, W = self.t, self.dt, self.n, self.H, self.W
        y = torch.full((n, H, W, self.Cout), float("nan"), device=DEV).to(TD[dt])
        cnt = torch.zeros(n * (self.Cout // 128), dtype=torch.int32, device=DEV)
        L.check(L.lib().dc_igemm(L.IgemmParams(out=None, pn_out=ptr(y), pn_gamma=ptr(t["gamma"]), pn_beta=ptr(t["beta"]), pn_cnt=ptr(cnt), pn_ld=self.Cout,
                                               pn_groups=GROUPS, pn_silu=1, pn_eps=EPS, **self.conv), L.stream_ptr()), "pn conv")
        pred = torch.full((n, H, W, self.Co), float("nan"), device=DEV)
        thin = L.IgemmParams(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=ptr(y), C0=self.Cout, W=ptr(t["Wo"]), Cout=self.Co,
                             tile_n=32, bias=ptr(t["bo"]), out=ptr(pred), out_dtype=L.DC_F32, out_ld=self.Co)
        name = L.lib().dc_igemm_variant(thin).decode()
        L.check(L.lib().dc_igemm(thin, L.stream_ptr()), "thin conv")
        torch.cuda.synchronize()
        return pred, name


@pytest.mark.parametrize("dt", [L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tail_fold_matches_reference_within_twice_the_two_launch_error(dt, shape):
    n, H, W = SHAPES[shape]
    lib = L.lib()
    p = Problem(dt, n, H, W)
    conv = L.IgemmParams(**p.conv)
    pred0, thin_name = p.two_launch()
    assert thin_name.startswith("conv3_thin")
    assert lib.dc_pn_timeouts() == 0
    e_two = maxrel(pred0.cpu(), p.ref)
    probe = p.tail(None, None, None)
    assert lib.dc_conv3_pn_tail_ok(conv, probe) == 1
    assert lib.dc_conv3_pn_tail_variant(conv, probe).decode() == "conv3_halo<%s,4w,pn,tail>" % ("bf16" if dt == L.DC_BF16 else "f16")
    tiles, tw, th = H * W // 256, min(W, 32), 256 // min(W, 32)
    ring_floats = lib.dc_conv3_pn_tail_ring_floats(conv, probe)
    assert ring_floats == n * tiles * (2 * (tw + 2) + 2 * th) * CO
    outs = []
    cnt = torch.zeros(n, dtype=torch.int32, device=DEV)                  # zeroed once: the counters only grow
    for _ in range(2):
        pred = torch.full((n, H, W, CO), float("nan"), device=DEV)
        ring = torch.full((ring_floats,), float("nan"), device=DEV)      # a slot the combine reads without its tile having written it would show
        L.check(lib.dc_conv3_pn_tail(conv, p.tail(pred, ring, cnt), L.stream_ptr()), "dc_conv3_pn_tail")
        torch.cuda.synchronize()
        outs.append(pred)
    assert lib.dc_pn_timeouts() == 0
    assert torch.equal(cnt, torch.full_like(cnt, 2 * tiles if tiles > 1 else 0))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])                                 # bit-identical from launch to launch
    e_tail = maxrel(outs[0].cpu(), p.ref)
    print(f"\npn_tail {shape} {'bf16' if dt == L.DC_BF16 else 'f16'}: max error / max |ref| two-launch {e_two:.3e}  folded {e_tail:.3e}  "
          f"folded vs two-launch {maxrel(outs[0], pred0):.3e}")
    assert e_tail <= 2 * e_two, (e_tail, e_two)


@pytest.mark.parametrize("case", ["f32", "cout256", "co4", "8x8", "raw_output"])
def test_tail_fold_refuses_what_it_does_not_serve_and_the_thin_conv_still_runs(case):
    dt, n, H, W, Cout, Co = L.DC_BF16, 2, 32, 32, 128, 3
    if case == "f32":
        dt = L.DC_F32
    if case == "cout256":
        Cout = 256
    if case == "co4":
        Co = 4
    if case == "8x8":
        H = W = 8
    lib = L.lib()
    if case == "8x8":      # (the probes touch no memory: any aligned pointer stands for the operands; conv3_thin starts at 16x16, so nothing else to run)
        d = ptr(torch.zeros(64, device=DEV))
        conv = L.IgemmParams(dtype=dt, taps=9, stride=1, upsample=0, n_img=n, Hin=H, Win=W, Hout=H, Wout=W, src0=d, C0=C, W=d, Cout=Cout, tile_n=128,
                             out_dtype=dt, out_ld=Cout, qstats=d)
        tail = L.PnTailParams(Co=Co, pred_ld=Co, groups=GROUPS, silu=1, eps=EPS)
        assert lib.dc_conv3_pn_tail_ok(conv, tail) == 0
        return
    p = Problem(dt, n, H, W, Cout=Cout, Co=Co)
    kw = dict(p.conv)
    raw = torch.empty(n, H, W, Cout, dtype=TD[dt], device=DEV)
    if case == "raw_output":
        kw["out"] = ptr(raw)
    conv = L.IgemmParams(**kw)
    pred, ring, cnt = torch.zeros(n, H, W, Co, device=DEV), torch.zeros(1 << 16, device=DEV), torch.zeros(n * (Cout // 128), dtype=torch.int32, device=DEV)
    tail = p.tail(pred, ring, cnt)
    assert lib.dc_conv3_pn_tail_ok(conv, tail) == 0
    assert not lib.dc_conv3_pn_tail_variant(conv, tail).decode().startswith("conv3_halo")
    assert lib.dc_conv3_pn_tail(conv, tail, L.stream_ptr()) != 0
    # the separate route still serves the case
    got, name = p.two_launch()
    assert name.startswith("conv3_thin")
    tol = {L.DC_F32: 1e-4, L.DC_BF16: 1.2e-2}[dt]      # two chained fp32 convs with K = 1152 / one rounding of y to bf16 (2^-8)
    assert maxrel(got.cpu(), p.ref) < tol, maxrel(got.cpu(), p.ref)
    assert lib.dc_pn_timeouts() == 0
