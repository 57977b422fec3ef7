"""T5 (v1.0) encoder stack as ONE launch plan for libdcamd — see plan.py for the plan model.

Restated: transformers' `T5EncoderModel` behind the reference's `encoder_type='t5'` (diffusion/diffusion_classifier.py:59-74, :93-98):
token embedding -> per block [RMS norm -> q | k | v (no bias) -> softmax(q k^T + relative-position bias, keys below the prompt's length)
v -> o + residual; RMS norm -> wi -> ReLU -> wo + residual] -> final RMS norm.  The residual stream is fp32; what the GEMMs read is the
compute dtype.  The relative-position bias is block 0's, shared by every layer, as a table over the 2L - 1 relative distances built on
the host (a device logarithm could land on the other side of a bucket boundary).  The attention mask must be right-padded, so it is a
token count per prompt: dc_attention_bias's kv_len, the per-context key count dc_cross_attention_len takes downstream.
"""
import math

import torch

from . import _lib as L
from .packing import f32c, pack_matrix
from .plan import Plan, PlanBuilder

MAX_LENGTH = L.ATTENTION_BIAS_MAX_L      # the reference tokenises with max_length=512 (:95)
HEAD_DIMS = (16, 32, 64, 128)            # dc_attention_bias


def relative_bucket(rel, num_buckets=32, max_distance=128):
    """Bidirectional bucket of the relative distances `rel` (int64: key position - query position) — the fp32 torch expression of
    transformers' T5Attention._relative_position_bucket, operation for operation, so that every boundary falls where it does there."""
    nb = num_buckets // 2
    buckets = (rel > 0).to(torch.long) * nb
    n = torch.abs(rel)
    max_exact = nb // 2
    is_small = n < max_exact
    if_large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, nb - 1))
    return buckets + torch.where(is_small, n, if_large)


def bias_table(weight, Lq, num_buckets=32, max_distance=128):
    """relative_attention_bias.weight [num_buckets, heads] -> [heads, 2L - 1] fp32 on the CPU, entry k - q + L - 1 (dc_attention_bias)."""
    rel = torch.arange(-(Lq - 1), Lq, dtype=torch.long)
    w = weight.detach().to("cpu", torch.float32)
    return w[relative_bucket(rel, num_buckets, max_distance)].t().contiguous()


def lengths_of_mask(mask, shape):
    """Token counts [B] (CPU int64) of a right-padded attention mask [B, L]: each row a prefix of ones with at least one.  Holes and
    left padding are refused — the kernels take a count, not a mask."""
    if mask is None:
        return torch.full((shape[0],), shape[1], dtype=torch.int64)
    m = torch.as_tensor(mask).detach().cpu()
    if tuple(m.shape) != tuple(shape):
        raise L.DcamdError(f"attention_mask must be {tuple(shape)} like input_ids, got {tuple(m.shape)}")
    m = m != 0
    ln = m.sum(1).to(torch.int64)
    prefix = torch.arange(shape[1])[None, :] < ln[:, None]
    if bool((ln < 1).any()) or not bool((m == prefix).all()):
        bad = [i for i in range(shape[0]) if ln[i] < 1 or not bool((m[i] == prefix[i]).all())]
        raise L.DcamdError(f"attention_mask must be right-padded (a prefix of ones with at least one per prompt; no holes, no left "
                           f"padding): prompts {bad} are not")
    return ln


def check_ids(ids, vocab):
    """input_ids [B, L <= 512] int64 with every id in [0, vocab): validated on the host where they enter (the kernel only clamps)."""
    if ids.dim() != 2 or ids.dtype != torch.int64:
        raise ValueError(f"input_ids must be [B, L] int64, got {ids.dtype} {tuple(ids.shape)}")
    if not 1 <= ids.shape[1] <= MAX_LENGTH or ids.shape[0] < 1:
        raise ValueError(f"input_ids must hold at least one prompt of 1 <= L <= {MAX_LENGTH} tokens, got {tuple(ids.shape)}")
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= vocab:
        raise ValueError(f"input_ids must lie in [0, {vocab}), got [{lo}, {hi}]")


class T5Weights:
    def __init__(self, model, dt, device):
        self.dt, self.dev = dt, device
        cfg = model.config
        sd = model.state_dict()
        P = {"shared": f32c(sd["shared.weight"], device)}
        for i in range(cfg.num_layers):
            a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
            # q | k | v as one [3 * inner, d_model] GEMM; inner = num_heads * d_kv need not equal d_model
            P[a + "qkv"] = pack_matrix(torch.cat([sd[a + f"SelfAttention.{n}.weight"] for n in "qkv"], 0), dt, device)
            P[a + "o"] = pack_matrix(sd[a + "SelfAttention.o.weight"], dt, device)
            P[a + "ln"] = f32c(sd[a + "layer_norm.weight"], device)
            P[f + "wi"] = pack_matrix(sd[f + "DenseReluDense.wi.weight"], dt, device)
            P[f + "wo"] = pack_matrix(sd[f + "DenseReluDense.wo.weight"], dt, device)
            P[f + "ln"] = f32c(sd[f + "layer_norm.weight"], device)
        P["final.ln"] = f32c(sd["encoder.final_layer_norm.weight"], device)
        self.rel = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"].detach().to("cpu", torch.float32)
        self.P = P


class T5Plan(Plan):
    """inputs: ids [B, L] int64 and lens [B] int32 (device buffers of the plan: copy into them, then run()).
    output: out [B, L, d_model] fp32, rows at or past a prompt's length zero."""

    def __init__(self, model, weights, B, Lq):
        cfg = model.config
        dev, dt, P = weights.dev, weights.dt, weights.P
        D, heads, dkv, dff = cfg.d_model, cfg.num_heads, cfg.d_kv, cfg.d_ff
        inner = heads * dkv
        eps = float(cfg.layer_norm_epsilon)
        self.B, self.L, self.dt = B, Lq, dt
        pb = self.pb = PlanBuilder(dev, B, 1, 1)
        self.ids = torch.zeros(B, Lq, dtype=torch.int64, device=dev)
        self.lens = torch.full((B,), Lq, dtype=torch.int32, device=dev)
        self.bias = bias_table(weights.rel, Lq, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance).to(dev)
        ids, lens, bias = pb.const(self.ids), pb.const(self.lens), pb.const(self.bias)
        rows = B * Lq

        def rmsnorm(name, x, w, out_dt):
            y = pb.tensor(name, "bj", 1, Lq, D, out_dt)
            pb.emit(L.OP_RMSNORM,
                    dict(x=x, y=y, weight=pb.const(w), row_len=lens, dtype=x.dt, out_dtype=out_dt, rows=rows, C=D, rows_per_sample=Lq, eps=eps),
                    [x], [y], dict(name=name, family="rmsnorm", flops=0.0, bytes=float(rows * D * (4 + (4 if out_dt == L.DC_F32 else 2)))))
            return y

        h = pb.tensor("embed", "bj", 1, Lq, D, L.DC_F32)
        pb.emit(L.OP_EMBED_ROWS,
                dict(table=pb.const(P["shared"]), ids=ids, out=h, out_dtype=L.DC_F32, rows=rows, C=D, vocab=cfg.vocab_size),
                [], [h], dict(name="embed", family="embed_rows", flops=0.0, bytes=8.0 * rows * D))
        for i in range(cfg.num_layers):
            a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
            hn = rmsnorm(a + "ln", h, P[a + "ln"], dt)
            qkv = pb.igemm(a + "qkv", hn, pb.const(P[a + "qkv"]), 3 * inner)
            o = pb.tensor(a + "attn", "bj", 1, Lq, inner, dt)
            q, k, v = qkv.view(0, inner), qkv.view(inner, inner), qkv.view(2 * inner, inner)
            pb.emit(L.OP_ATTENTION_BIAS,
                    dict(q=q, k=k, v=v, out=o, bias=bias, kv_len=lens, dtype=dt, n=B, L=Lq, heads=heads, d=dkv, ld_qkv=qkv.ld, ld_out=o.ld,
                         scale=1.0),       # T5 does not scale its scores: the factor lives in the initialisation of q
                    [q, k, v], [o], dict(name=a + "attn", family="attention_bias", flops=4.0 * B * heads * Lq * Lq * dkv,
                                         bytes=4.0 * rows * inner * (4 if dt == L.DC_F32 else 2)))
            # fp32 residual stream: the GEMM reads the old stream as its residual and writes a new one (never in place)
            h = pb.igemm(a + "o", o, pb.const(P[a + "o"]), D, residual=h, out_dt=L.DC_F32)
            hn = rmsnorm(f + "ln", h, P[f + "ln"], dt)
            ff = pb.igemm(f + "wi", hn, pb.const(P[f + "wi"]), dff)
            pb.emit(L.OP_RELU, dict(x=ff, n=rows * dff, dtype=dt), [ff], [ff],
                    dict(name=f + "relu", family="relu", flops=0.0, bytes=2.0 * rows * dff * (4 if dt == L.DC_F32 else 2)))
            h = pb.igemm(f + "wo", ff, pb.const(P[f + "wo"]), D, residual=h, out_dt=L.DC_F32)
        self.out = rmsnorm("final.ln", h, P["final.ln"], L.DC_F32)
        pb.finalize(keep_alive=[self.out])

    def out_view(self):
        return super().out_view().view(self.B, self.L, -1)
