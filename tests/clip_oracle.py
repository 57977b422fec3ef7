"""Test-side restatement of transformers' CLIPTextModel (`last_hidden_state`) in plain torch; the product never imports it.

`clip_encode(sd, cfg, ids, mask)` computes, in order: token + position embedding; per layer LayerNorm1 -> q / k / v Linear with bias ->
softmax(q k^T d^-1/2 + causal [+ key padding]) v -> out_proj + bias + residual; LayerNorm2 -> fc1 + bias -> quick-GELU (x sigmoid(1.702 x))
or erf-GELU -> fc2 + bias + residual; the final LayerNorm.  `sd` carries the published key names (with the `text_model.` prefix).
Pad queries still attend, as in transformers (the HIP path writes zeros there instead: compare rows below each length).

`store`: a 16-bit torch dtype rounds every tensor the HIP path STORES in that type to it (the packed weights, each norm's output, q | k | v,
the attention output, the feed-forward's hidden tensor before and after the activation) and keeps the fp32 residual stream, as
tests/t5_oracle.py does; the arithmetic in between stays in `dtype` (float32 or float64)."""
import torch
import torch.nn.functional as F

P = "text_model."


def clip_encode(sd, cfg, ids, mask=None, *, store=None, dtype=torch.float32, hidden_act=None):
    rnd = (lambda t: t.to(store).to(dtype)) if store is not None else (lambda t: t)
    W = lambda k: rnd(sd[k].to(dtype))                      # a GEMM weight, as packed
    V = lambda k: sd[k].to(dtype)                           # biases and LayerNorm parameters stay fp32
    heads, D, eps = cfg["num_attention_heads"], cfg["hidden_size"], cfg["layer_norm_eps"]
    act = hidden_act or cfg["hidden_act"]
    d = D // heads
    B, L = ids.shape

    def ln(x, k):
        return F.layer_norm(x, (D,), V(k + ".weight"), V(k + ".bias"), eps)
    h = V(P + "embeddings.token_embedding.weight")[ids] + V(P + "embeddings.position_embedding.weight")[:L]
    pos = torch.arange(L)
    bias = torch.zeros(L, L, dtype=dtype).masked_fill(pos[None, :] > pos[:, None], float("-inf"))[None, None]      # [query, key]
    if mask is not None:
        bias = bias + (1.0 - mask[:, None, None, :].to(dtype)) * torch.finfo(dtype).min
    for i in range(cfg["num_hidden_layers"]):
        p = f"{P}encoder.layers.{i}."
        hn = rnd(ln(h, p + "layer_norm1"))
        q, k, v = (rnd(hn @ W(p + f"self_attn.{n}_proj.weight").T + V(p + f"self_attn.{n}_proj.bias")).view(B, L, heads, d).transpose(1, 2)
                   for n in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + bias, dim=-1) @ v
        a = rnd(a.transpose(1, 2).reshape(B, L, D))
        h = h + a @ W(p + "self_attn.out_proj.weight").T + V(p + "self_attn.out_proj.bias")
        hn = rnd(ln(h, p + "layer_norm2"))
        f = rnd(hn @ W(p + "mlp.fc1.weight").T + V(p + "mlp.fc1.bias"))
        f = rnd(f * torch.sigmoid(1.702 * f) if act == "quick_gelu" else F.gelu(f))
        h = h + f @ W(p + "mlp.fc2.weight").T + V(p + "mlp.fc2.bias")
    return ln(h, P + "final_layer_norm")
