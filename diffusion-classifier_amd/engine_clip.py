"""CLIP text transformer as ONE launch plan for libdcamd — see plan.py for the plan model and engine_t5.py for the sibling encoder.

Restated: transformers' `CLIPTextModel.last_hidden_state`: token + position embedding -> per layer [LayerNorm -> q | k | v (with bias)
-> softmax(q k^T d^-1/2 over keys k <= q) v -> out_proj + bias + residual; LayerNorm -> fc1 + bias -> quick-GELU or erf-GELU -> fc2 +
bias + residual] -> final LayerNorm.  The residual stream is fp32; what the GEMMs read is the compute dtype.  The attention mask must be
right-padded, so it is a token count per prompt; causality already hides every pad key from every valid query, so the count only decides
which rows are computed (dc_attention_causal's / dc_layernorm_rows' row_len) and how many keys the UNet's cross-attention sees downstream.
On request the same plan also keeps the penultimate residual stream (`hidden_states[-2]`) and computes the projected pooled row
(`CLIPTextModelWithProjection.text_embeds`) with ops the library already has: DC_OP_EMBED_ROWS over the stream as a table,
DC_OP_LAYERNORM_ROWS over the B gathered rows and an fp32 dc_igemm.
"""
import torch

from . import _lib as L
from .packing import f32c, pack_matrix
from .plan import Plan, PlanBuilder

MAX_LENGTH = L.ATTENTION_CAUSAL_MAX_L
HEAD_DIMS = (16, 32, 64, 128)            # dc_attention_causal
ACTS = {"quick_gelu": L.PASS_QUICK_GELU, "gelu": L.PASS_GELU_ERF}

PREFIX = "text_model."


class ClipWeights:
    def __init__(self, model, dt, device):
        self.dt, self.dev = dt, device
        cfg = model.config
        sd = model.state_dict()
        P = {"tok": f32c(sd[PREFIX + "embeddings.token_embedding.weight"], device),
             "pos": f32c(sd[PREFIX + "embeddings.position_embedding.weight"], device)}
        for i in range(cfg.num_hidden_layers):
            k = f"{PREFIX}encoder.layers.{i}."
            # q | k | v as one [3 * hidden, hidden] GEMM with the stacked bias
            P[k + "qkv.w"] = pack_matrix(torch.cat([sd[k + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0), dt, device)
            P[k + "qkv.b"] = f32c(torch.cat([sd[k + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0), device)
            P[k + "out.w"] = pack_matrix(sd[k + "self_attn.out_proj.weight"], dt, device)
            P[k + "out.b"] = f32c(sd[k + "self_attn.out_proj.bias"], device)
            for n in ("fc1", "fc2"):
                P[k + n + ".w"] = pack_matrix(sd[k + f"mlp.{n}.weight"], dt, device)
                P[k + n + ".b"] = f32c(sd[k + f"mlp.{n}.bias"], device)
            for n in ("layer_norm1", "layer_norm2"):
                P[k + n + ".g"], P[k + n + ".b"] = f32c(sd[k + n + ".weight"], device), f32c(sd[k + n + ".bias"], device)
        P["final.g"] = f32c(sd[PREFIX + "final_layer_norm.weight"], device)
        P["final.b"] = f32c(sd[PREFIX + "final_layer_norm.bias"], device)
        if "text_projection.weight" in sd:        # CLIPTextEncoderWithProjection: the pooled row's fp32 GEMM (no bias)
            P["proj.w"] = pack_matrix(sd["text_projection.weight"], L.DC_F32, device)
        self.P = P


class ClipPlan(Plan):
    """inputs: ids [B, L] int64 and lens [B] int32 (device buffers of the plan: copy into them, then run()).
    output: out [B, L, hidden] fp32, rows at or past a prompt's length zero.  8 * layers + 2 ops.
    penultimate: `hs2`, the fp32 residual stream after layers - 1 layers (transformers' hidden_states[-2], no final LayerNorm), is kept
    alive to the end of the plan; its rows at or past a prompt's length are whatever the residual adds left there (the caller zeroes
    them).  pooled: three more ops — DC_OP_EMBED_ROWS gathers row `eos[b]` (int64 [B], b * L + the EOS position, a device buffer of the
    plan) of the last stream read as a table of B * L rows, DC_OP_LAYERNORM_ROWS applies the final LayerNorm to those B rows, and an
    fp32 dc_igemm multiplies them by text_projection -> `pooled` [B, projection_dim] fp32.  One run yields all of them."""

    def __init__(self, model, weights, B, Lq, penultimate=False, pooled=False):
        cfg = model.config
        dev, dt, P = weights.dev, weights.dt, weights.P
        D, heads, dff = cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size
        dh = D // heads
        eps = float(cfg.layer_norm_eps)
        kind = ACTS[cfg.hidden_act]
        self.B, self.L, self.dt = B, Lq, dt
        pb = self.pb = PlanBuilder(dev, B, 1, 1)
        self.ids = torch.zeros(B, Lq, dtype=torch.int64, device=dev)
        self.lens = torch.full((B,), Lq, dtype=torch.int32, device=dev)
        ids, lens = pb.const(self.ids), pb.const(self.lens)
        rows = B * Lq
        es = 4 if dt == L.DC_F32 else 2

        def layernorm(name, x, g, b, out_dt):
            y = pb.tensor(name, "bj", 1, Lq, D, out_dt)
            pb.emit(L.OP_LAYERNORM_ROWS,
                    dict(x=x, y=y, gamma=pb.const(g), beta=pb.const(b), row_len=lens, dtype=x.dt, out_dtype=out_dt, rows=rows, C=D,
                         rows_per_sample=Lq, eps=eps),
                    [x], [y], dict(name=name, family="layernorm_rows", flops=0.0, bytes=float(rows * D * (4 + (4 if out_dt == L.DC_F32 else 2)))))
            return y

        def gemm(name, x, w, b, cout, **kw):
            y = pb.igemm(name, x, pb.const(P[w]), cout, bias=pb.const(P[b]), **kw)
            v = L.lib().dc_igemm_variant(pb.probe(**pb.ops[-1][2])).decode()
            if v == "invalid":
                raise L.DcamdError(f"ClipPlan: dc_igemm refuses {name} ({rows} x {x.C} -> {cout})")
            pb.meta[-1]["variant"] = v
            return y

        h = pb.tensor("embed", "bj", 1, Lq, D, L.DC_F32)
        pb.emit(L.OP_EMBED_ROWS_POS,
                dict(table=pb.const(P["tok"]), pos=pb.const(P["pos"]), ids=ids, out=h, out_dtype=L.DC_F32, rows=rows, C=D,
                     vocab=cfg.vocab_size, L=Lq),
                [], [h], dict(name="embed", family="embed_rows_pos", flops=0.0, bytes=12.0 * rows * D))
        for i in range(cfg.num_hidden_layers):
            k = f"{PREFIX}encoder.layers.{i}."
            hn = layernorm(k + "ln1", h, P[k + "layer_norm1.g"], P[k + "layer_norm1.b"], dt)
            qkv = gemm(k + "qkv", hn, k + "qkv.w", k + "qkv.b", 3 * D)
            o = pb.tensor(k + "attn", "bj", 1, Lq, D, dt)
            q, kk, v = qkv.view(0, D), qkv.view(D, D), qkv.view(2 * D, D)
            pb.emit(L.OP_ATTENTION_CAUSAL,
                    dict(q=q, k=kk, v=v, out=o, row_len=lens, dtype=dt, n=B, L=Lq, heads=heads, d=dh, ld_qkv=qkv.ld, ld_out=o.ld,
                         scale=float(dh) ** -0.5),
                    [q, kk, v], [o], dict(name=k + "attn", family="attention_causal", flops=2.0 * B * heads * Lq * (Lq + 1) * dh,
                                          bytes=4.0 * rows * D * es))
            # fp32 residual stream: the GEMM reads the old stream as its residual and writes a new one (never in place)
            h = gemm(k + "out", o, k + "out.w", k + "out.b", D, residual=h, out_dt=L.DC_F32)
            hn = layernorm(k + "ln2", h, P[k + "layer_norm2.g"], P[k + "layer_norm2.b"], dt)
            ff = gemm(k + "fc1", hn, k + "fc1.w", k + "fc1.b", dff)
            pb.emit(L.OP_ACT_PASS, dict(x=ff, n=rows * dff, dtype=dt, kind=kind), [ff], [ff],
                    dict(name=k + "act", family="act_pass", flops=0.0, bytes=2.0 * rows * dff * es))
            h = gemm(k + "fc2", ff, k + "fc2.w", k + "fc2.b", D, residual=h, out_dt=L.DC_F32)
            if penultimate and i == cfg.num_hidden_layers - 2:
                self.hs2 = h
        self.out = layernorm("final.ln", h, P["final.g"], P["final.b"], L.DC_F32)
        keep = [self.out] + ([self.hs2] if penultimate else [])
        if pooled:
            self.eos = torch.zeros(B, dtype=torch.int64, device=dev)
            row = pb.tensor("pooled.row", "bj", 1, 1, D, L.DC_F32)
            pb.emit(L.OP_EMBED_ROWS, dict(table=h, ids=pb.const(self.eos), out=row, out_dtype=L.DC_F32, rows=B, C=D, vocab=rows),
                    [h], [row], dict(name="pooled.row", family="embed_rows", flops=0.0, bytes=8.0 * B * D))
            pn = pb.tensor("pooled.ln", "bj", 1, 1, D, L.DC_F32)
            pb.emit(L.OP_LAYERNORM_ROWS,
                    dict(x=row, y=pn, gamma=pb.const(P["final.g"]), beta=pb.const(P["final.b"]), row_len=None, dtype=L.DC_F32,
                         out_dtype=L.DC_F32, rows=B, C=D, rows_per_sample=1, eps=eps),
                    [row], [pn], dict(name="pooled.ln", family="layernorm_rows", flops=0.0, bytes=8.0 * B * D))
            self.pooled = pb.igemm("text_projection", pn, pb.const(P["proj.w"]), cfg.projection_dim)
            keep.append(self.pooled)
        pb.finalize(keep_alive=keep)
        if pooled:
            pb.check_served(type(model).__name__, f"the pooled output of {B} prompts of {Lq} tokens")

    def out_view(self):
        return super().out_view().view(self.B, self.L, -1)

    def hs2_view(self):
        return self.pb.tensor_view(self.hs2).view(self.B, self.L, -1)

    def pooled_view(self):
        return self.pb.tensor_view(self.pooled).view(self.B, -1)
