"""Test-side restatement of transformers' T5EncoderModel (T5 v1.0: ReLU feed-forward) in plain torch; the product never imports it.

`t5_encode(sd, cfg, ids, mask)` computes, in order: the token embedding; per block RMS norm (no mean subtraction) -> q / k / v / o without
bias around UNSCALED scores + the relative-position bias of block 0 (shared by every layer) + a key-padding mask -> residual; RMS norm ->
wi -> ReLU -> wo -> residual; the final RMS norm.  Pad queries still attend the valid keys, as in transformers (the HIP path writes
zeros there instead: compare rows below each length).

`store`: a 16-bit torch dtype rounds every tensor the HIP path STORES in that type to it (the packed weights, each norm's output, q | k | v,
the attention output, the feed-forward's hidden tensor) and keeps the fp32 residual stream, as the project's storage-rounded oracles do;
the arithmetic in between stays in `dtype` (float32 or float64)."""
import math

import torch


def relative_bucket(rel, num_buckets=32, max_distance=128):
    """The bidirectional bucket of relative distances `rel` (key position - query position), transformers' expression in fp32."""
    nb = num_buckets // 2
    ret = (rel > 0).to(torch.long) * nb
    n = rel.abs()
    max_exact = nb // 2
    is_small = n < max_exact
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return ret + torch.where(is_small, n, large)


def position_bias(table, L, num_buckets=32, max_distance=128):
    """[1, heads, L, L] from block 0's relative_attention_bias.weight [num_buckets, heads]."""
    pos = torch.arange(L)
    rel = pos[None, :] - pos[:, None]                       # [query, key] = key - query
    return table[relative_bucket(rel, num_buckets, max_distance)].permute(2, 0, 1).unsqueeze(0)


def t5_encode(sd, cfg, ids, mask=None, *, store=None, dtype=torch.float32):
    rnd = (lambda t: t.to(store).to(dtype)) if store is not None else (lambda t: t)
    W = lambda k: rnd(sd[k].to(dtype))                      # a GEMM weight, as packed
    heads, dkv, eps = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"]
    B, L = ids.shape
    if mask is None:
        mask = torch.ones_like(ids)

    def rms(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w.to(dtype)
    h = sd["shared.weight"].to(dtype)[ids]
    bias = position_bias(sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], L,
                         cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"]).to(dtype)
    bias = bias + (1.0 - mask[:, None, None, :].to(dtype)) * torch.finfo(dtype).min
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}.layer."
        hn = rnd(rms(h, sd[p + "0.layer_norm.weight"]))
        q, k, v = (rnd(hn @ W(p + f"0.SelfAttention.{n}.weight").T).view(B, L, heads, dkv).transpose(1, 2) for n in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) + bias, dim=-1) @ v
        a = rnd(a.transpose(1, 2).reshape(B, L, heads * dkv))
        h = h + a @ W(p + "0.SelfAttention.o.weight").T
        hn = rnd(rms(h, sd[p + "1.layer_norm.weight"]))
        f = rnd(torch.relu(rnd(hn @ W(p + "1.DenseReluDense.wi.weight").T)))
        h = h + f @ W(p + "1.DenseReluDense.wo.weight").T
    return rms(h, sd["encoder.final_layer_norm.weight"])
