"""Test-side restatement of the ENCODER of diffusers' AutoencoderKL (0.31 layout) in plain torch, and of the scaled posterior mean
`(mean - shift_factor) * scaling_factor`; the product never imports it.  Written from the published architecture and UNPINNED, like the
UNet / DiT oracle under oracle/: diffusers is not installed where these tests run, so no output of the published implementation is
recorded here — what it is held to is the architecture as published, layer by layer:

    conv_in (3x3, pad 1)
    per level i: layers_per_block x ResNet; all but the last level: F.pad(x, (0, 1, 0, 1)) then a 3x3 stride-2 conv without padding
    mid block: ResNet, attention, ResNet
    GroupNorm -> SiLU -> conv_out (3x3, 2 z channels) -> quant_conv (1x1, when use_quant_conv) -> the first z channels are the mean
  ResNet:    GroupNorm(eps 1e-6) -> SiLU -> conv1 -> GroupNorm -> SiLU -> conv2, plus the input (through the 1x1 conv_shortcut when the
             channel count changes); no time embedding
  attention: GroupNorm -> to_q / to_k / to_v (Linear with bias) over the H W tokens -> softmax(q k^T C^-1/2) v, ONE head of C channels ->
             to_out.0 (Linear with bias) -> plus the block input

`sd` carries the published key names.  fp32 on the CPU by default.  `store`: a 16-bit torch dtype rounds every tensor the HIP path STORES
in that type to it (the GEMM / conv weights, the image patches conv_in reads, every conv and GroupNorm output, q | k | v, the attention
output), as tests/clip_oracle.py does; the arithmetic in between stays in `dtype`, and the latents come out unrounded."""
import torch
import torch.nn.functional as F

GN_EPS = 1e-6


def vae_encode(sd, cfg, x, *, store=None, dtype=torch.float32):
    """cfg: dict with block_out_channels, layers_per_block, norm_num_groups, latent_channels, scaling_factor, shift_factor (None: 0),
    use_quant_conv.  x [B, in_channels, H, W] -> latents [B, latent_channels, H / f, W / f]."""
    rnd = (lambda t: t.to(store).to(dtype)) if store is not None else (lambda t: t)
    Wt = lambda k: rnd(sd[k + ".weight"].to(dtype))        # a GEMM / conv weight, as packed
    V = lambda k: sd[k].to(dtype)                          # biases and GroupNorm parameters stay fp32
    G = cfg["norm_num_groups"]
    boc = tuple(cfg["block_out_channels"])

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

    h = rnd(F.conv2d(rnd(x.to(dtype)), Wt("encoder.conv_in"), V("encoder.conv_in.bias"), padding=1))
    for i in range(len(boc)):
        for j in range(cfg["layers_per_block"]):
            h = resnet(h, f"encoder.down_blocks.{i}.resnets.{j}")
        if i != len(boc) - 1:
            k = f"encoder.down_blocks.{i}.downsamplers.0.conv"
            h = rnd(F.conv2d(F.pad(h, (0, 1, 0, 1)), Wt(k), V(k + ".bias"), stride=2))
    h = resnet(h, "encoder.mid_block.resnets.0")
    h = attention(h, "encoder.mid_block.attentions.0")
    h = resnet(h, "encoder.mid_block.resnets.1")
    h = gn(h, "encoder.conv_norm_out", True)
    mom = F.conv2d(h, Wt("encoder.conv_out"), V("encoder.conv_out.bias"), padding=1)
    if cfg.get("use_quant_conv", True):
        mom = F.conv2d(mom, Wt("quant_conv"), V("quant_conv.bias"))
    mean = mom[:, : cfg["latent_channels"]]
    return (mean - float(cfg.get("shift_factor") or 0.0)) * float(cfg["scaling_factor"])
