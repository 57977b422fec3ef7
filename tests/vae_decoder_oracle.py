"""Test-side restatement of the DECODER of diffusers' AutoencoderKL (0.31 layout) in plain torch, and of
`AutoencoderKL.decode(z / scaling_factor + shift_factor).sample`; the product never imports it.  Written from the published architecture
and UNPINNED, like tests/vae_oracle.py: diffusers is not installed where these tests run, so it is held to the architecture as published:

    u = z / scaling_factor + shift_factor -> post_quant_conv (1x1, when use_post_quant_conv) -> conv_in (3x3, pad 1)
    mid block: ResNet, attention, ResNet
    per level i over rev = block_out_channels[::-1]: (layers_per_block + 1) x ResNet, the first rev[max(i - 1, 0)] -> rev[i];
             all but the last level: nearest-neighbour 2x, then a 3x3 conv with pad 1
    GroupNorm -> SiLU -> conv_out (3x3, out_channels)
  ResNet and attention as in tests/vae_oracle.py: GroupNorm eps 1e-6, no time embedding, one head as wide as the level with a residual.

`sd` carries the published key names.  fp32 on the CPU by default.  `store`: a 16-bit torch dtype rounds every tensor the HIP path STORES in
that type to it (the GEMM / conv weights, the patches conv_in reads — that is, post_quant_conv's output, which itself stays fp32 —, every
conv and GroupNorm output, q | k | v, the attention output); the arithmetic in between stays in `dtype`, and the image comes out unrounded."""
import torch
import torch.nn.functional as F

from vae_oracle import GN_EPS


def vae_decode(sd, cfg, z, *, store=None, dtype=torch.float32):
    """cfg: dict with block_out_channels, layers_per_block, norm_num_groups, scaling_factor, shift_factor (None: 0),
    use_post_quant_conv.  z [B, latent_channels, h, w] scaled latents -> images [B, out_channels, f h, f w]."""
    rnd = (lambda t: t.to(store).to(dtype)) if store is not None else (lambda t: t)
    Wt = lambda k: rnd(sd[k + ".weight"].to(dtype))
    V = lambda k: sd[k].to(dtype)
    G = cfg["norm_num_groups"]
    nb = len(tuple(cfg["block_out_channels"]))

    def gn(h, k, silu):
        y = F.group_norm(h, G, V(k + ".weight"), V(k + ".bias"), GN_EPS)
        return rnd(F.silu(y) if silu else y)

    def resnet(h, k):
        y = rnd(F.conv2d(gn(h, k + ".norm1", True), Wt(k + ".conv1"), V(k + ".conv1.bias"), padding=1))
        y = F.conv2d(gn(y, k + ".norm2", True), Wt(k + ".conv2"), V(k + ".conv2.bias"), padding=1)
        if k + ".conv_shortcut.weight" in sd:
            h = rnd(F.conv2d(h, Wt(k + ".conv_shortcut"), V(k + ".conv_shortcut.bias")))
        return rnd(h + y)

    def attention(h, k):
        B, C, H, W = h.shape
        t = gn(h, k + ".group_norm", False).permute(0, 2, 3, 1).reshape(B, H * W, C)
        q, kk, v = (rnd(t @ Wt(k + f".to_{n}").T + V(k + f".to_{n}.bias")) for n in "qkv")
        a = rnd(torch.softmax(q @ kk.transpose(-1, -2) * C ** -0.5, dim=-1) @ v)
        o = a @ Wt(k + ".to_out.0").T + V(k + ".to_out.0.bias")
        return rnd(h + o.reshape(B, H, W, C).permute(0, 3, 1, 2))

    u = z.to(dtype) / float(cfg["scaling_factor"]) + float(cfg.get("shift_factor") or 0.0)
    if cfg.get("use_post_quant_conv", True):
        u = F.conv2d(u, V("post_quant_conv.weight"), V("post_quant_conv.bias"))            # fp32 in the HIP path: never rounded
    h = rnd(F.conv2d(rnd(u), Wt("decoder.conv_in"), V("decoder.conv_in.bias"), padding=1))
    h = resnet(h, "decoder.mid_block.resnets.0")
    h = attention(h, "decoder.mid_block.attentions.0")
    h = resnet(h, "decoder.mid_block.resnets.1")
    for i in range(nb):
        for j in range(cfg["layers_per_block"] + 1):
            h = resnet(h, f"decoder.up_blocks.{i}.resnets.{j}")
        if i != nb - 1:
            k = f"decoder.up_blocks.{i}.upsamplers.0.conv"
            h = rnd(F.conv2d(F.interpolate(h, scale_factor=2.0, mode="nearest"), Wt(k), V(k + ".bias"), padding=1))
    h = gn(h, "decoder.conv_norm_out", True)
    return F.conv2d(h, Wt("decoder.conv_out"), V("decoder.conv_out.bias"), padding=1)
