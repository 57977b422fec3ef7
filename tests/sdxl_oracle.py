"""Test-side oracles of what Stable Diffusion XL adds, PyTorch eager.  Test infrastructure only: the package never imports this.

`SDXLOracleUNet(SDOracleUNet)`: diffusers' `UNet2DConditionModel` as SDXL-base configures it.  diffusers is not installed where these
tests run: the two additions are written from the published definition, restated here —
  transformer depth   `transformer_layers_per_block`, an int or one entry per down block (up blocks read it reversed, the mid block takes
                      the last): the `transformer_blocks.{k}` of a site run in sequence between one proj_in and one proj_out
  text_time           `addition_embed_type="text_time"`: time_ids [N, 6] are flattened, each number goes through the sinusoid of width
                      `addition_time_embed_dim` (the model's flip_sin_to_cos / freq_shift), the result is reshaped to [N, 6 * dim] and
                      concatenated BEHIND text_embeds [N, P]; aug = add_embedding.linear_2(SiLU(add_embedding.linear_1(.))); every
                      ResNet reads time_emb_proj(SiLU(time_embedding(t) + aug))
`lowp` rounds where the HIP plan stores: the output of every block of a site (ff.net.2 + residual) as SDOracleUNet rounds its one block;
the side path (time embedding, aug, time_emb_proj) is fp32 in the plan and is not rounded.  With depth 1 and no text_time the
arithmetic is SDOracleUNet's, statement for statement (the bits agree; tests/test_sdxl_host.py).
The call takes `added_cond_kwargs = {"text_embeds", "time_ids"}`, diffusers' names, as a foreign backbone of DiffusionClassifier under
encoder_type='clip_dual' is called.

`clip_encode_ext`: tests/clip_oracle.py's `clip_encode` extended by `layer` (-1: last_hidden_state; -2: transformers'
hidden_states[-2], the residual stream after num_hidden_layers - 1 layers without the final LayerNorm) and `pooled` (text_embeds: the
final-LayerNorm row at the EOS position times text_projection.weight^T; eos_token_id 2: argmax of the ids, else the first position
holding the id).  It restates, it does not call: `clip_encode` returns only the last state.
"""
import torch
import torch.nn.functional as F

from oracle.unet import _TBlock, _TimestepEmbedding, sinusoid
from sd_unet_oracle import SDOracleUNet


class SDXLOracleUNet(SDOracleUNet):
    def __init__(self, *, transformer_layers_per_block=1, addition_embed_type=None, addition_time_embed_dim=None,
                 projection_class_embeddings_input_dim=None, **kw):
        super().__init__(**kw)
        c = self.config
        nb = len(c.block_out_channels)
        tl = (transformer_layers_per_block,) * nb if isinstance(transformer_layers_per_block, int) else tuple(transformer_layers_per_block)
        assert len(tl) == nb and addition_embed_type in (None, "text_time")
        c.transformer_layers_per_block, c.addition_embed_type, c.addition_time_embed_dim = tl, addition_embed_type, addition_time_embed_dim
        c.projection_class_embeddings_input_dim = projection_class_embeddings_input_dim
        xdim = c.cross_attention_dim

        def deepen(blk, depth):
            for t in getattr(blk, "attentions", []):
                b0 = t.transformer_blocks[0]
                ch = b0.norm1.weight.shape[0]
                for _ in range(depth - 1):
                    t.transformer_blocks.append(_TBlock(ch, b0.attn1.heads, ch // b0.attn1.heads, xdim))
        for i, blk in enumerate(self.down_blocks):
            deepen(blk, tl[i])
        deepen(self.mid_block, tl[-1])
        for i, blk in enumerate(self.up_blocks):
            deepen(blk, tl[::-1][i])
        if addition_embed_type == "text_time":
            self.add_embedding = _TimestepEmbedding(projection_class_embeddings_input_dim, c.block_out_channels[0] * 4)

    def _transformer(self, t, x, ctx, lengths):
        q = self._q
        N, C, H, W = x.shape
        res = x.permute(0, 2, 3, 1).reshape(N, H * W, C)
        h = q(t.norm(x)).permute(0, 2, 3, 1).reshape(N, H * W, C)
        h = q(self._proj(t.proj_in, h))
        for b in t.transformer_blocks:
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

    def augment(self, added_cond_kwargs, N):
        """aug [N, 4 * C0] fp32 of the text_time side path."""
        c = self.config
        if added_cond_kwargs is None or "text_embeds" not in added_cond_kwargs or "time_ids" not in added_cond_kwargs:
            raise ValueError("added_cond_kwargs must hold text_embeds and time_ids")
        te, ti = added_cond_kwargs["text_embeds"].to(torch.float32), added_cond_kwargs["time_ids"].to(torch.float32)
        sin = sinusoid(ti.reshape(-1), c.addition_time_embed_dim, c.flip_sin_to_cos, c.freq_shift).reshape(N, -1)
        a = self.add_embedding
        return a.linear_2(F.silu(a.linear_1(torch.cat([te, sin], dim=-1))))

    def forward(self, x, noise_labels, encoder_hidden_states=None, added_cond_kwargs=None, encoder_lengths=None):
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
        if c.addition_embed_type == "text_time":
            temb = temb + self.augment(added_cond_kwargs, N)
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


P = "text_model."


def eos_positions(ids, eos_token_id):
    """transformers' two rules: 2 (the legacy config) -> argmax of the ids; else the first position that holds the id."""
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).to(torch.int64).argmax(dim=-1)


def clip_encode_ext(sd, cfg, ids, mask=None, *, layer=-1, pooled=False, store=None, dtype=torch.float32, hidden_act=None, eos_token_id=None):
    """-> hidden [B, L, D] (layer -1 / -2, all rows as transformers returns them), or (hidden, text_embeds [B, projection_dim])."""
    rnd = (lambda t: t.to(store).to(dtype)) if store is not None else (lambda t: t)
    W = lambda k: rnd(sd[k].to(dtype))
    V = lambda k: sd[k].to(dtype)
    heads, D, eps, n = cfg["num_attention_heads"], cfg["hidden_size"], cfg["layer_norm_eps"], cfg["num_hidden_layers"]
    act = hidden_act or cfg["hidden_act"]
    d = D // heads
    B, L = ids.shape

    def ln(x, k):
        return F.layer_norm(x, (D,), V(k + ".weight"), V(k + ".bias"), eps)
    h = V(P + "embeddings.token_embedding.weight")[ids] + V(P + "embeddings.position_embedding.weight")[:L]
    pos = torch.arange(L)
    bias = torch.zeros(L, L, dtype=dtype).masked_fill(pos[None, :] > pos[:, None], float("-inf"))[None, None]
    if mask is not None:
        bias = bias + (1.0 - mask[:, None, None, :].to(dtype)) * torch.finfo(dtype).min
    states = [h]
    for i in range(n):
        p = f"{P}encoder.layers.{i}."
        hn = rnd(ln(h, p + "layer_norm1"))
        q, k, v = (rnd(hn @ W(p + f"self_attn.{m}_proj.weight").T + V(p + f"self_attn.{m}_proj.bias")).view(B, L, heads, d).transpose(1, 2)
                   for m in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + bias, dim=-1) @ v
        a = rnd(a.transpose(1, 2).reshape(B, L, D))
        h = h + a @ W(p + "self_attn.out_proj.weight").T + V(p + "self_attn.out_proj.bias")
        hn = rnd(ln(h, p + "layer_norm2"))
        f = rnd(hn @ W(p + "mlp.fc1.weight").T + V(p + "mlp.fc1.bias"))
        f = rnd(f * torch.sigmoid(1.702 * f) if act == "quick_gelu" else F.gelu(f))
        h = h + f @ W(p + "mlp.fc2.weight").T + V(p + "mlp.fc2.bias")
        states.append(h)
    last = ln(h, P + "final_layer_norm")
    out = last if layer == -1 else states[layer]
    if not pooled:
        return out
    e = eos_positions(ids, cfg["eos_token_id"] if eos_token_id is None else eos_token_id)
    return out, last[torch.arange(B), e] @ sd["text_projection.weight"].to(dtype).T          # the projection is an fp32 GEMM in the plan
