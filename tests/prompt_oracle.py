"""Test-side oracle for contexts of several tokens.  Test infrastructure only.

`oracle.OracleUNetCondition2D._transformer` restates the one-token shortcut (softmax over one key is 1) and asserts one token.  The
subclass here overrides that one method with the full block of diffusers' BasicTransformerBlock: attn1 + residual WITHOUT a class
vector, then `h = attn2(norm2(h), ctx) + h` as real attention over the S projected context tokens (no mask: the reference passes
none), from the parameters the oracle already owns — `OracleUNetCondition2D.cross_attn_exact` is the fp32 statement of that term.
`lowp=True` rounds where the kernels store: the LayerNorm output, q, k, v, p, the attention output and the block output
(`lowp_dtype`: bf16 or f16).  The classifier subclass indexes a [classes + 1, S, hid] prompt table.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import oracle


class PromptOracleUNet(oracle.OracleUNetCondition2D):
    def __init__(self, *a, lowp_dtype=torch.bfloat16, **kw):
        super().__init__(*a, **kw)
        self.lowp_dtype = lowp_dtype

    def _q(self, x):
        return x.to(self.lowp_dtype).to(torch.float32) if self.lowp else x

    def _transformer(self, t, x, ctx):
        q = self._q
        N, C, H, W = x.shape
        res = x
        h = q(t.norm(x))
        h = q(self._conv(t.proj_in, h) + t.proj_in.bias[None, :, None, None])
        h = h.permute(0, 2, 3, 1).reshape(N, H * W, C)
        b = t.transformer_blocks[0]
        a = b.attn1
        d = C // a.heads
        sh = lambda z: z.view(N, -1, a.heads, d).transpose(1, 2)
        # self-attention + residual, no class vector
        hn = q(b.norm1(h))
        qq, kk, vv = q(self._lin(a.to_q, hn)), q(self._lin(a.to_k, hn)), q(self._lin(a.to_v, hn))
        s = torch.matmul(sh(qq), sh(kk).transpose(-1, -2)) * (d ** -0.5)
        o = q(torch.matmul(torch.softmax(s, dim=-1), sh(vv)).transpose(1, 2).reshape(N, -1, C))
        h = q(self._lin(a.to_out[0], o) + a.to_out[0].bias + h)
        # cross-attention over the S context tokens (K / V: fp32 side path, stored rounded)
        a2 = b.attn2
        hn = q(b.norm2(h))
        qq = q(self._lin(a2.to_q, hn))
        kk, vv = q(F.linear(ctx, a2.to_k.weight)), q(F.linear(ctx, a2.to_v.weight))
        s = torch.matmul(sh(qq), sh(kk).transpose(-1, -2)) * (d ** -0.5)
        p = torch.softmax(s, dim=-1)
        o = q(torch.matmul(q(p), sh(vv)).transpose(1, 2).reshape(N, -1, C))
        h = q(self._lin(a2.to_out[0], o) + a2.to_out[0].bias + h)
        # feed forward (GEGLU, erf gelu)
        hn = q(b.norm3(h))
        pr = self._lin(b.ff.net[0].proj, hn) + b.ff.net[0].proj.bias
        u, g = pr.chunk(2, dim=-1)
        f = q(u * F.gelu(g))
        h = q(self._lin(b.ff.net[2], f) + b.ff.net[2].bias + h)
        h = h.reshape(N, H, W, C).permute(0, 3, 1, 2)
        return q(self._conv(t.proj_out, h) + t.proj_out.bias[None, :, None, None] + res)


class _Table(nn.Module):
    def __init__(self, rows, tokens, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(rows, tokens, dim))


class PromptOracleClassifier(oracle.OracleDiffusionClassifier):
    """The reference loop with `encode_text_prompt` returning [BS, S, hid] rows of a per-class prompt table."""

    def __init__(self, backbone, config):
        tokens = config.prompt_tokens
        config.encoder_type = "nn"                  # the parent's constructor knows 'nn' / 'DiT' only
        super().__init__(backbone, config)
        config.encoder_type = "prompt"
        self.encoder_type = "prompt"
        self.encoder = _Table(config.classes + 1, tokens, backbone.config.encoder_hid_dim)

    def encode_text_prompt(self, text):
        return self.encoder.weight[text]
