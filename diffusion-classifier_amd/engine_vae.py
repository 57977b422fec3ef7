"""AutoencoderKL encoder and decoder, each as ONE launch plan for libdcamd — see plan.py for the plan model.

Restated: the encoder half of diffusers' `AutoencoderKL` (0.31 layout) and the mean of its posterior, scaled:
    conv_in -> per level [layers_per_block x ResNet, then (all but the last level) pad (0, 1, 0, 1) + 3x3 stride-2 conv]
            -> mid block [ResNet, single-head attention over the H x W tokens, ResNet] -> GroupNorm + SiLU -> conv_out -> quant_conv
    latent = (mean - shift_factor) * scaling_factor,    mean = the first latent_channels of the 2 x latent_channels moments
A ResNet is GroupNorm(eps 1e-6) + SiLU -> conv3x3 -> GroupNorm + SiLU -> conv3x3, plus the input (through a 1x1 conv_shortcut when the
channel count changes); there is no time embedding.  The attention is GroupNorm -> to_q | to_k | to_v (with bias) -> softmax(q k^T C^-1/2) v
over ONE head as wide as the level -> to_out.0 + bias + the block input.

What runs where:
  conv_in          the im2col GEMM, its operand written by dc_qsample (alpha = 1, sigma = 0, im2col = 1) as in UNetCondition2D.forward
  3x3 convs        dc_igemm taps = 9 behind a dc_groupnorm pass: the plain route.  The producer-side GroupNorm hand-off (pn_claim) is the
                   UNet plan's business and is never claimed here; the convs do write the quad statistics (qstats) the GroupNorm pass
                   behind them reads, where dc_igemm offers them
  downsampler      dc_im2col_s2 + a 1x1 dc_igemm over K = 9 C: dc_igemm's stride-2 conv pads every side and reads other pixels
  mid attention    dc_attention_wide (C = 256 / 512), dc_attention where C <= 128
  tail             quant_conv's mean rows, scaling_factor and shift_factor are folded into conv_out on the host in fp64 (fold_tail): the
                   plan's last conv writes latent_channels fp32 channels and nothing of the log-variance half is computed
The residual stream is in the compute dtype, as in the UNet plan.

The decoder half (`VaeDecoderWeights`, `VaeDecoderPlan`), `AutoencoderKL.decode(z / scaling_factor + shift_factor).sample`:
    post_quant_conv -> conv_in -> mid block [ResNet, attention, ResNet]
            -> per level [(layers_per_block + 1) x ResNet, then (all but the last level) nearest 2x + 3x3 conv] -> GroupNorm + SiLU -> conv_out
  head             dc_latent_im2col: u = Q (z / scaling_factor + shift_factor) + b per pixel in fp32 (Q, b: post_quant_conv), written as the
                   3x3 patches conv_in reads, then a 1x1 dc_igemm over Kpad.  No host fold: a biased 1x1 conv in front of a zero-padded
                   3x3 conv is not a 3x3 conv at the border, and folding Q / s into 16-bit weights rounds products the reference never rounds
  ResNet, attention  the encoder's builders (resnet_ops, attention_ops)
  upsampler        dc_igemm upsample = 1: the four-phase form (pack_up4, up4) where dc_igemm_up4_ok says so, else the plain upsample route
  tail             dc_groupnorm (+ SiLU) -> dc_igemm taps = 9 with an fp32 output, on the 32-wide tile when out_channels <= 32
The producer-side GroupNorm hand-off, the fused GroupNorm prologue and the tail fold are not claimed here either.
"""
import torch

from . import _lib as L
from .packing import LazyPacks, f32c, pack_conv3x3, pack_matrix
from .plan import DT_SIZE, Plan, PlanBuilder, bke, round_up, switches

GN_EPS = 1e-6
MID_WIDTHS = (64, 128) + L.ATTENTION_WIDE_DIMS      # dc_attention / dc_attention_wide, and a multiple of the GEMMs' K granule
CHANNEL_GRANULE = 64                                # K granule of the 16-bit GEMMs (128-byte LDS rows)


def fold_tail(conv_out_w, conv_out_b, quant_w, quant_b, latent_channels, scaling_factor, shift_factor):
    """conv_out [2z, C, 3, 3] followed by the mean rows of quant_conv [2z, 2z, 1, 1] (None: no quant_conv) and by
    (mean - shift) * scaling, as ONE 3x3 conv [z, C, 3, 3] with bias [z]: a 1x1 conv after a 3x3 conv is a 3x3 conv.  fp64 on the host."""
    z = latent_channels
    w, b = conv_out_w.detach().double().cpu(), conv_out_b.detach().double().cpu()
    if quant_w is not None:
        q = quant_w.detach().double().cpu().reshape(quant_w.shape[0], -1)[:z]          # [z, 2z]: the rows that give the mean
        w = torch.einsum("om,mckl->ockl", q, w)
        b = q @ b + quant_b.detach().double().cpu()[:z]
    else:
        w, b = w[:z], b[:z]
    s = float(scaling_factor)
    return (w * s).contiguous(), ((b - float(shift_factor or 0.0)) * s).contiguous()


def pack_down(w, dt, device):
    """Conv2d weight [Cout, Cin, 3, 3] of a downsampler -> packed [Cout_pad, 9 Cin] in the (ky, kx, c) order dc_im2col_s2 writes."""
    return pack_matrix(w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1), dt, device)


class _Packer:
    """The packing steps the two halves share: fills P with the packed form of the state-dict entries of a 3x3 conv, a GroupNorm, a ResNet
    and the mid block's attention under the plans' key names."""

    def __init__(self, sd, dt, device):
        self.sd, self.dt, self.dev, self.P = sd, dt, device, {}

    def conv3(self, key, **kw):
        self.P[key + ".w"] = pack_conv3x3(self.sd[key + ".weight"], self.dt, self.dev, **kw)
        self.P[key + ".b"] = f32c(self.sd[key + ".bias"], self.dev)

    def norm(self, key):
        self.P[key + ".g"], self.P[key + ".b"] = f32c(self.sd[key + ".weight"], self.dev), f32c(self.sd[key + ".bias"], self.dev)

    def resnet(self, key):
        sd, P = self.sd, self.P
        self.norm(key + ".norm1"); self.conv3(key + ".conv1"); self.norm(key + ".norm2"); self.conv3(key + ".conv2")
        if key + ".conv_shortcut.weight" in sd:
            P[key + ".conv_shortcut.w"] = pack_matrix(sd[key + ".conv_shortcut.weight"], self.dt, self.dev)
            P[key + ".conv_shortcut.b"] = f32c(sd[key + ".conv_shortcut.bias"], self.dev)

    def attention(self, a):
        sd, P = self.sd, self.P
        self.norm(a + "group_norm")
        # q | k | v as one [3 C, C] GEMM with the stacked bias
        P[a + "qkv.w"] = pack_matrix(torch.cat([sd[a + f"to_{n}.weight"] for n in "qkv"], 0), self.dt, self.dev)
        P[a + "qkv.b"] = f32c(torch.cat([sd[a + f"to_{n}.bias"] for n in "qkv"], 0), self.dev)
        P[a + "to_out.0.w"] = pack_matrix(sd[a + "to_out.0.weight"], self.dt, self.dev)
        P[a + "to_out.0.b"] = f32c(sd[a + "to_out.0.bias"], self.dev)


class VaeWeights:
    """Device-resident packed weights of a VAEEncoder for one compute dtype."""

    def __init__(self, model, dt, device):
        self.dt, self.dev = dt, device
        cfg = model.config
        sd = model.state_dict()
        self.kin = round_up(9 * cfg.in_channels, bke(dt))
        pk = _Packer(sd, dt, device)
        P = pk.P
        pk.conv3("encoder.conv_in", kpad=self.kin)
        nb = len(cfg.block_out_channels)
        for i in range(nb):
            for j in range(cfg.layers_per_block):
                pk.resnet(f"encoder.down_blocks.{i}.resnets.{j}")
            if i != nb - 1:
                key = f"encoder.down_blocks.{i}.downsamplers.0.conv"
                P[key + ".w"] = pack_down(sd[key + ".weight"], dt, device)
                P[key + ".b"] = f32c(sd[key + ".bias"], device)
        pk.resnet("encoder.mid_block.resnets.0")
        pk.resnet("encoder.mid_block.resnets.1")
        pk.attention("encoder.mid_block.attentions.0.")
        pk.norm("encoder.conv_norm_out")
        qc = cfg.use_quant_conv
        w, b = fold_tail(sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"], sd["quant_conv.weight"] if qc else None,
                         sd["quant_conv.bias"] if qc else None, cfg.latent_channels, cfg.scaling_factor, cfg.shift_factor)
        self.tail_tile_n = 32 if cfg.latent_channels <= 32 else 128
        P["tail.w"] = pack_conv3x3(w.float(), dt, device, tile_n=self.tail_tile_n)
        P["tail.b"] = f32c(b.float(), device)
        self.P = P


# ---- the op builders the two plans share: P holds the packed weights under the keys _Packer writes, G the GroupNorm group count -----------
def gn_ops(pb, P, G, name, x, key, silu):
    return pb.groupnorm(name, x, pb.const(P[key + ".g"]), pb.const(P[key + ".b"]), G, GN_EPS, silu)


def resnet_ops(pb, P, G, use_qs, key, x):
    Cout = P[key + ".conv1.b"].shape[0]
    h = gn_ops(pb, P, G, key + ".gn1", x, key + ".norm1", True)
    h = pb.igemm(key + ".conv1", h, pb.const(P[key + ".conv1.w"]), Cout, taps=9, bias=pb.const(P[key + ".conv1.b"]), qstats=use_qs)
    h = gn_ops(pb, P, G, key + ".gn2", h, key + ".norm2", True)
    sc = x
    if key + ".conv_shortcut.w" in P:
        sc = pb.igemm(key + ".short", x, pb.const(P[key + ".conv_shortcut.w"]), Cout, bias=pb.const(P[key + ".conv_shortcut.b"]))
    return pb.igemm(key + ".conv2", h, pb.const(P[key + ".conv2.w"]), Cout, taps=9, bias=pb.const(P[key + ".conv2.b"]),
                    residual=sc, qstats=use_qs)


def attention_ops(pb, P, G, key, x):
    """One head as wide as the level over the H W tokens, with the residual: dc_attention up to 128 channels, dc_attention_wide above."""
    Cc, Lq, B, dt = x.C, x.H * x.W, pb.n[x.dom], x.dt
    es = DT_SIZE[dt]
    hn = gn_ops(pb, P, G, key + "gn", x, key + "group_norm", False)
    qkv = pb.igemm(key + "qkv", hn, pb.const(P[key + "qkv.w"]), 3 * Cc, bias=pb.const(P[key + "qkv.b"]))
    q, k, v = qkv.view(0, Cc), qkv.view(Cc, Cc), qkv.view(2 * Cc, Cc)
    if Cc <= 128:
        o = pb.attention(key + "attn", q, k, v, 1, Cc)
    else:
        o = pb.tensor(key + "attn", "bj", x.H, x.W, Cc, dt)
        pb.emit(L.OP_ATTENTION_WIDE,
                dict(q=q, k=k, v=v, out=o, dtype=dt, n=B, L=Lq, heads=1, d=Cc, ld_qkv=qkv.ld, ld_out=o.ld, scale=float(Cc) ** -0.5),
                [q, k, v], [o], dict(name=key + "attn", family="attention_wide", flops=4.0 * B * Lq * Lq * Cc, bytes=4.0 * B * Lq * Cc * es))
    return pb.igemm(key + "to_out", o, pb.const(P[key + "to_out.0.w"]), Cc, bias=pb.const(P[key + "to_out.0.b"]), residual=x)


class VaePlan(Plan):
    """input: x [B, in_channels, H, W] fp32 (a device buffer of the plan: copy into it, then run()).
    output: latents [B, H / f, W / f, latent_channels] fp32 NHWC (out_view), f = 2^(levels - 1)."""

    def __init__(self, model, weights, B, H, W):
        cfg = model.config
        dev, dt, P = weights.dev, weights.dt, weights.P
        boc, G = cfg.block_out_channels, cfg.norm_num_groups
        use_qs = switches().qstats
        self.B, self.H, self.W, self.dt = B, H, W, dt
        pb = self.pb = PlanBuilder(dev, B, 1, 1)
        f32 = dict(dtype=torch.float32, device=dev)
        self.x = torch.zeros(B, cfg.in_channels, H, W, **f32)
        xt = pb.external("x", self.x, "bj", 1, 1, 1, L.DC_F32)
        one = pb.external("alpha", torch.ones(B, **f32), "bj", 1, 1, 1, L.DC_F32)
        zero = pb.external("sigma", torch.zeros(B, **f32), "bj", 1, 1, 1, L.DC_F32)
        # z = 1 * x + 0 * x as 3x3 patches: the A operand of conv_in as a GEMM
        a0 = pb.qsample("a0", pb.const(self.x), xt, one, zero, None, cfg.in_channels, H, W, weights.kin, dt, im2col=True)
        es = DT_SIZE[dt]

        def downsample(key, x):
            col = pb.tensor(key + ".col", "bj", x.H // 2, x.W // 2, 9 * x.C, dt)
            pb.emit(L.OP_IM2COL_S2, dict(x=x, out=col, dtype=dt, n=B, H=x.H, W=x.W, C=x.C, ld=x.ld), [x], [col],
                    dict(name=key + ".col", family="im2col_s2", flops=0.0, bytes=float(B * x.H * x.W * x.C * es + B * col.H * col.W * col.C * es)))
            return pb.igemm(key, col, pb.const(P[key + ".w"]), x.C, bias=pb.const(P[key + ".b"]))

        h = pb.igemm("encoder.conv_in", a0, pb.const(P["encoder.conv_in.w"]), boc[0], bias=pb.const(P["encoder.conv_in.b"]),
                     k_real=9 * cfg.in_channels)
        for i in range(len(boc)):
            for j in range(cfg.layers_per_block):
                h = resnet_ops(pb, P, G, use_qs, f"encoder.down_blocks.{i}.resnets.{j}", h)
            if i != len(boc) - 1:
                h = downsample(f"encoder.down_blocks.{i}.downsamplers.0.conv", h)
        h = resnet_ops(pb, P, G, use_qs, "encoder.mid_block.resnets.0", h)
        h = attention_ops(pb, P, G, "encoder.mid_block.attentions.0.", h)
        h = resnet_ops(pb, P, G, use_qs, "encoder.mid_block.resnets.1", h)
        h = gn_ops(pb, P, G, "encoder.conv_norm_out", h, "encoder.conv_norm_out", True)
        self.out = pb.igemm("encoder.conv_out", h, pb.const(P["tail.w"]), cfg.latent_channels, taps=9, bias=pb.const(P["tail.b"]),
                            out_dt=L.DC_F32, tile_n=weights.tail_tile_n)
        pb.finalize(keep_alive=[self.out])
        pb.check_served("VaePlan", f"{B} x {H} x {W} in {model.compute_dtype}")


class VaeDecoderWeights(LazyPacks):
    """Device-resident packed weights of a VAEDecoder for one compute dtype."""

    def __init__(self, model, dt, device):
        self.dt, self.dev = dt, device
        cfg = model.config
        sd = self._sd = model.state_dict()
        Z = cfg.latent_channels
        self.kin = round_up(9 * Z, bke(dt))
        pk = _Packer(sd, dt, device)
        P = pk.P
        # post_quant_conv stays fp32: dc_latent_im2col applies it (the identity and zeros when the VAE has none)
        if cfg.use_post_quant_conv:
            P["head.Q"], P["head.b"] = f32c(sd["post_quant_conv.weight"].reshape(Z, Z), device), f32c(sd["post_quant_conv.bias"], device)
        else:
            P["head.Q"], P["head.b"] = torch.eye(Z, dtype=torch.float32, device=device), torch.zeros(Z, dtype=torch.float32, device=device)
        pk.conv3("decoder.conv_in", kpad=self.kin)
        pk.resnet("decoder.mid_block.resnets.0")
        pk.resnet("decoder.mid_block.resnets.1")
        pk.attention("decoder.mid_block.attentions.0.")
        nb = len(cfg.block_out_channels)
        for i in range(nb):
            for j in range(cfg.layers_per_block + 1):
                pk.resnet(f"decoder.up_blocks.{i}.resnets.{j}")
            if i != nb - 1:
                pk.conv3(f"decoder.up_blocks.{i}.upsamplers.0.conv")        # the four-phase form is packed when a plan takes it
        pk.norm("decoder.conv_norm_out")
        self.tail_tile_n = 32 if cfg.out_channels <= 32 else 128
        pk.conv3("decoder.conv_out", tile_n=self.tail_tile_n)
        self.P = P


class VaeDecoderPlan(Plan):
    """input: z [B, latent_channels, h, w] fp32, scaled latents (a device buffer of the plan: copy into it, then run()).
    output: images [B, f h, f w, out_channels] fp32 NHWC (out_view), f = 2^(levels - 1)."""

    def __init__(self, model, weights, B, h, w):
        cfg = model.config
        dev, dt, P = weights.dev, weights.dt, weights.P
        boc, G, Z = cfg.block_out_channels, cfg.norm_num_groups, cfg.latent_channels
        sw = switches()
        use_qs = sw.qstats
        self.B, self.h, self.w, self.dt = B, h, w, dt
        pb = self.pb = PlanBuilder(dev, B, 1, 1)
        self.z = torch.zeros(B, Z, h, w, dtype=torch.float32, device=dev)
        zt = pb.external("z", self.z, "bj", 1, 1, 1, L.DC_F32)
        es = DT_SIZE[dt]
        a0 = pb.tensor("a0", "bj", h, w, weights.kin, dt)
        pb.emit(L.OP_LATENT_IM2COL,
                dict(z=zt, Q=pb.const(P["head.Q"]), bias=pb.const(P["head.b"]), out=a0, out_dtype=dt, n=B, Z=Z, H=h, W=w, Kpad=weights.kin,
                     inv_scale=1.0 / cfg.scaling_factor, shift=float(cfg.shift_factor or 0.0)), [zt], [a0],
                dict(name="a0", family="latent_im2col", flops=2.0 * B * h * w * 9 * Z * Z, bytes=float(B * h * w * (Z * 4 + weights.kin * es))))
        rev = boc[::-1]
        x = pb.igemm("decoder.conv_in", a0, pb.const(P["decoder.conv_in.w"]), rev[0], bias=pb.const(P["decoder.conv_in.b"]), k_real=9 * Z)
        x = resnet_ops(pb, P, G, use_qs, "decoder.mid_block.resnets.0", x)
        x = attention_ops(pb, P, G, "decoder.mid_block.attentions.0.", x)
        x = resnet_ops(pb, P, G, use_qs, "decoder.mid_block.resnets.1", x)
        for i in range(len(boc)):
            for j in range(cfg.layers_per_block + 1):
                x = resnet_ops(pb, P, G, use_qs, f"decoder.up_blocks.{i}.resnets.{j}", x)
            if i != len(boc) - 1:
                x = pb.upsample_conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", x, weights, sw.up4, use_qs)
        x = gn_ops(pb, P, G, "decoder.conv_norm_out", x, "decoder.conv_norm_out", True)
        self.out = pb.igemm("decoder.conv_out", x, pb.const(P["decoder.conv_out.w"]), cfg.out_channels, taps=9,
                            bias=pb.const(P["decoder.conv_out.b"]), out_dt=L.DC_F32, tile_n=weights.tail_tile_n)
        pb.finalize(keep_alive=[self.out])
        pb.check_served("VaeDecoderPlan", f"{B} x {h} x {w} latents in {model.compute_dtype}")
