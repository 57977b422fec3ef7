"""Test-side oracle of the Stable Diffusion UNet (diffusers `UNet2DConditionModel` as SD 1.x / 2.x configure it), PyTorch eager.  Test
infrastructure only: the package never imports it.

Built from the blocks of oracle/unet.py (`_Resnet`, `_Transformer2D`, `_Sampler`, `_TimestepEmbedding`, `sinusoid` and the rounding hooks
`_conv` / `_lin` / `_resnet` of `OracleUNetCondition2D`), which is imported and not edited.  What differs from that oracle:
  no `encoder_hid_proj`      the prompt states [N, S, cross_attention_dim] are attn2's keys and values as they are
  heads per level            `attention_head_dim` is the NUMBER of heads (diffusers' quirk), an int or one entry per down block; up
                             blocks read it reversed, the mid block takes the last
  use_linear_projection      proj_in / proj_out are nn.Linear [C, C] on the token rows instead of 1x1 convs: the same arithmetic
  attn2                      real attention over the S tokens (as tests/prompt_oracle.py), with `encoder_lengths` [N] masking the keys at
                             or past a prompt's length
`noise_labels` is the DDPM step as a float.  `lowp=True` rounds where the kernels store (bf16 / f16 weights and stored activations,
fp32 accumulation, norms, softmax and side path), as `OracleUNetCondition2D` does.
`zero_rows_are_padding=True` (for a classifier that drives this module as a foreign backbone, whose call carries no lengths): the
trailing all-zero rows of a prompt are padding — what `PromptTable.set_prompt` leaves behind a short prompt.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

import oracle
from oracle.unet import _Block, _Resnet, _Sampler, _TimestepEmbedding, _Transformer2D, sinusoid


class SDOracleUNet(oracle.OracleUNetCondition2D):
    def __init__(self, sample_size=None, in_channels=4, out_channels=4,
                 down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",), mid_block_type="UNetMidBlock2DCrossAttn",
                 up_block_types=("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3, block_out_channels=(320, 640, 1280, 1280),
                 layers_per_block=2, norm_num_groups=32, norm_eps=1e-5, cross_attention_dim=1280, attention_head_dim=8,
                 use_linear_projection=False, flip_sin_to_cos=True, freq_shift=0, lowp=False, lowp_dtype=torch.bfloat16,
                 zero_rows_are_padding=False, **unused):
        nn.Module.__init__(self)
        assert mid_block_type == "UNetMidBlock2DCrossAttn"
        boc = tuple(block_out_channels)
        nb = len(boc)
        lpb = (layers_per_block,) * nb if isinstance(layers_per_block, int) else tuple(layers_per_block)
        ahd = (attention_head_dim,) * nb if isinstance(attention_head_dim, int) else tuple(attention_head_dim)
        G, eps, xdim = norm_num_groups, norm_eps, cross_attention_dim
        self.config = SimpleNamespace(
            sample_size=sample_size, in_channels=in_channels, out_channels=out_channels, down_block_types=tuple(down_block_types),
            up_block_types=tuple(up_block_types), block_out_channels=boc, layers_per_block=lpb, norm_num_groups=G, norm_eps=eps,
            cross_attention_dim=xdim, encoder_hid_dim=xdim, attention_head_dim=ahd, flip_sin_to_cos=flip_sin_to_cos, freq_shift=freq_shift)
        self.lowp, self.lowp_dtype, self.linear, self.zero_rows_are_padding = lowp, lowp_dtype, bool(use_linear_projection), zero_rows_are_padding
        self.seen_labels = []                 # every noise_labels tensor forward was called with (the classify test reads it)

        def transformer(ch, heads):
            t = _Transformer2D(ch, heads, xdim, G)
            if self.linear:
                t.proj_in, t.proj_out = nn.Linear(ch, ch), nn.Linear(ch, ch)
            return t
        temb = boc[0] * 4
        self.conv_in = nn.Conv2d(in_channels, boc[0], 3, padding=1)
        self.time_embedding = _TimestepEmbedding(boc[0], temb)
        self.down_blocks = nn.ModuleList()
        out = boc[0]
        for i, kind in enumerate(down_block_types):
            cin, out = out, boc[i]
            blk = _Block()
            blk.resnets = nn.ModuleList([_Resnet(cin if j == 0 else out, out, temb, G, eps) for j in range(lpb[i])])
            if kind == "CrossAttnDownBlock2D":
                blk.attentions = nn.ModuleList([transformer(out, ahd[i]) for _ in range(lpb[i])])
            else:
                assert kind == "DownBlock2D", kind
            if i != nb - 1:
                blk.downsamplers = nn.ModuleList([_Sampler(out, 2)])
            self.down_blocks.append(blk)
        self.mid_block = _Block()
        self.mid_block.resnets = nn.ModuleList([_Resnet(boc[-1], boc[-1], temb, G, eps) for _ in range(2)])
        self.mid_block.attentions = nn.ModuleList([transformer(boc[-1], ahd[-1])])
        self.up_blocks = nn.ModuleList()
        rboc, rlpb, rahd = boc[::-1], lpb[::-1], ahd[::-1]
        out = rboc[0]
        for i, kind in enumerate(up_block_types):
            prev, out = out, rboc[i]
            cin = rboc[min(i + 1, nb - 1)]
            n = rlpb[i] + 1
            blk = _Block()
            blk.resnets = nn.ModuleList([_Resnet((prev if j == 0 else out) + (cin if j == n - 1 else out), out, temb, G, eps) for j in range(n)])
            if kind == "CrossAttnUpBlock2D":
                blk.attentions = nn.ModuleList([transformer(out, rahd[i]) for _ in range(n)])
            else:
                assert kind == "UpBlock2D", kind
            if i != nb - 1:
                blk.upsamplers = nn.ModuleList([_Sampler(out, 1)])
            self.up_blocks.append(blk)
        self.conv_norm_out = nn.GroupNorm(G, boc[0], eps=eps)
        self.conv_out = nn.Conv2d(boc[0], out_channels, 3, padding=1)

    def _q(self, x):
        return x.to(self.lowp_dtype).to(torch.float32) if self.lowp else x

    def _proj(self, m, h_tokens):
        """proj_in / proj_out on token rows [N, L, C]: nn.Linear, or the 1x1 conv's [C, C, 1, 1] weight read as one."""
        w = m.weight.reshape(m.weight.shape[0], -1)
        return F.linear(h_tokens, self._q(w), None) + m.bias

    def _transformer(self, t, x, ctx, lengths):
        q = self._q
        N, C, H, W = x.shape
        res = x.permute(0, 2, 3, 1).reshape(N, H * W, C)
        h = q(t.norm(x)).permute(0, 2, 3, 1).reshape(N, H * W, C)
        h = q(self._proj(t.proj_in, h))
        b = t.transformer_blocks[0]
        a = b.attn1
        d = C // a.heads
        sh = lambda z: z.view(N, -1, a.heads, d).transpose(1, 2)
        hn = q(b.norm1(h))
        qq, kk, vv = q(self._lin(a.to_q, hn)), q(self._lin(a.to_k, hn)), q(self._lin(a.to_v, hn))
        s = torch.matmul(sh(qq), sh(kk).transpose(-1, -2)) * (d ** -0.5)
        o = q(torch.matmul(q(torch.softmax(s, dim=-1)), sh(vv)).transpose(1, 2).reshape(N, -1, C))
        h = q(self._lin(a.to_out[0], o) + a.to_out[0].bias + h)
        a2 = b.attn2
        hn = q(b.norm2(h))
        qq = q(self._lin(a2.to_q, hn))
        kk, vv = q(F.linear(ctx, a2.to_k.weight)), q(F.linear(ctx, a2.to_v.weight))       # K / V: fp32 side path, stored rounded
        s = torch.matmul(sh(qq), sh(kk).transpose(-1, -2)) * (d ** -0.5)
        if lengths is not None:
            pad = torch.arange(ctx.shape[1])[None, :] >= lengths.reshape(-1, 1)             # [N, S]
            s = s.masked_fill(pad[:, None, None, :], float("-inf"))
        o = q(torch.matmul(q(torch.softmax(s, dim=-1)), sh(vv)).transpose(1, 2).reshape(N, -1, C))
        h = q(self._lin(a2.to_out[0], o) + a2.to_out[0].bias + h)
        hn = q(b.norm3(h))
        pr = self._lin(b.ff.net[0].proj, hn) + b.ff.net[0].proj.bias
        u, g = pr.chunk(2, dim=-1)
        f = q(u * F.gelu(g))
        h = q(self._lin(b.ff.net[2], f) + b.ff.net[2].bias + h)
        h = q(self._proj(t.proj_out, h) + res)
        return h.reshape(N, H, W, C).permute(0, 3, 1, 2)

    def forward(self, x, noise_labels, encoder_hidden_states=None, encoder_lengths=None):
        q = self._q
        N = x.shape[0]
        lam = noise_labels if torch.is_tensor(noise_labels) else torch.tensor([noise_labels], dtype=torch.float32)
        lam = lam.reshape(-1).expand(N) if lam.numel() == 1 else lam.reshape(-1)
        self.seen_labels.append(lam.detach().clone())
        c = self.config
        ctx = encoder_hidden_states.to(torch.float32)
        lengths = None if encoder_lengths is None else torch.as_tensor(encoder_lengths)
        if lengths is None and self.zero_rows_are_padding:
            real = (ctx != 0).any(dim=2)                                                    # [N, S]
            lengths = (real.to(torch.int64) * torch.arange(1, ctx.shape[1] + 1)[None, :]).max(dim=1).values.clamp(min=1)   # last real row + 1
        te = self.time_embedding
        temb = te.linear_2(F.silu(te.linear_1(sinusoid(lam, c.block_out_channels[0], c.flip_sin_to_cos, c.freq_shift))))
        temb_act = F.silu(temb)
        h = q(self._conv(self.conv_in, q(x)) + self.conv_in.bias[None, :, None, None])
        skips = [h]
        for blk in self.down_blocks:
            for j, r in enumerate(blk.resnets):
                h = self._resnet(r, h, temb_act)
                if hasattr(blk, "attentions"):
                    h = self._transformer(blk.attentions[j], h, ctx, lengths)
                skips.append(h)
            if hasattr(blk, "downsamplers"):
                d = blk.downsamplers[0].conv
                h = q(self._conv(d, h, stride=2) + d.bias[None, :, None, None])
                skips.append(h)
        m = self.mid_block
        h = self._resnet(m.resnets[0], h, temb_act)
        h = self._transformer(m.attentions[0], h, ctx, lengths)
        h = self._resnet(m.resnets[1], h, temb_act)
        for blk in self.up_blocks:
            for j, r in enumerate(blk.resnets):
                h = self._resnet(r, torch.cat([h, skips.pop()], dim=1), temb_act)
                if hasattr(blk, "attentions"):
                    h = self._transformer(blk.attentions[j], h, ctx, lengths)
            if hasattr(blk, "upsamplers"):
                u = blk.upsamplers[0].conv
                h = q(self._conv(u, F.interpolate(h, scale_factor=2.0, mode="nearest")) + u.bias[None, :, None, None])
        h = q(F.silu(self.conv_norm_out(h)))
        return (self._conv(self.conv_out, h) + self.conv_out.bias[None, :, None, None]).contiguous()
