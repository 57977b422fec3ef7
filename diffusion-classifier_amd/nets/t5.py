"""MI355X-native T5 (v1.0) text encoder: the `T5EncoderModel` the reference builds for `encoder_type='t5'`
(diffusion/diffusion_classifier.py:59-74) and calls in encode_text_prompt (:93-98), loaded from a LOCAL Hugging Face directory.

Parameters carry the state-dict key names of `transformers.T5EncoderModel` (shared.weight, encoder.block.{i}.layer.0.SelfAttention.
{q,k,v,o}.weight, ...), so a t5-small / base / large / 3b checkpoint loads strictly.  Modules only hold parameters; arithmetic runs in
libdcamd (engine_t5.py).  Nothing here imports `transformers` or opens a socket; tokenising is the caller's job.

bf16 is the recommended 16-bit compute type: T5's feed-forward activations are known to leave fp16's range with trained weights.
"""
import json
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import _lib as L
from .. import engine as E
from .. import engine_t5 as ET
from .unet import _Bag, _HipBackbone


class _Weight(nn.Module):
    """T5LayerNorm's parameter holder: `weight` [dim], ones."""

    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))


class T5Encoder(_HipBackbone):
    def __init__(self, vocab_size, d_model, d_kv, d_ff, num_layers, num_heads, relative_attention_num_buckets=32,
                 relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="relu"):
        super().__init__()
        if feed_forward_proj != "relu":
            raise NotImplementedError(f"T5Encoder(feed_forward_proj={feed_forward_proj!r}) is not supported: only the ReLU feed-forward of "
                                      "T5 v1.0 is built (the gated-GELU of T5 v1.1 / flan is a different activation from the GEGLU kernel here)")
        inner = num_heads * d_kv
        for name, val in (("d_model", d_model), ("num_heads * d_kv", inner), ("d_ff", d_ff)):
            if val < 64 or val % 64:
                raise NotImplementedError(f"T5Encoder({name}={val}) is not supported: it must be a multiple of 64 (the K granule of the "
                                          "16-bit token GEMMs)")
        if d_kv not in ET.HEAD_DIMS:
            raise NotImplementedError(f"T5Encoder(d_kv={d_kv}) is not supported: head widths {ET.HEAD_DIMS} only")
        self.config = SimpleNamespace(vocab_size=vocab_size, d_model=d_model, d_kv=d_kv, d_ff=d_ff, num_layers=num_layers,
                                      num_heads=num_heads, relative_attention_num_buckets=relative_attention_num_buckets,
                                      relative_attention_max_distance=relative_attention_max_distance,
                                      layer_norm_epsilon=layer_norm_epsilon, feed_forward_proj=feed_forward_proj)
        self.shared = nn.Embedding(vocab_size, d_model)
        self.encoder = _Bag()
        self.encoder.block = nn.ModuleList()
        for i in range(num_layers):
            att = _Bag()
            att.SelfAttention = _Bag()
            att.SelfAttention.q = nn.Linear(d_model, inner, bias=False)
            att.SelfAttention.k = nn.Linear(d_model, inner, bias=False)
            att.SelfAttention.v = nn.Linear(d_model, inner, bias=False)
            att.SelfAttention.o = nn.Linear(inner, d_model, bias=False)
            if i == 0:
                att.SelfAttention.relative_attention_bias = nn.Embedding(relative_attention_num_buckets, num_heads)
            att.layer_norm = _Weight(d_model)
            ff = _Bag()
            ff.DenseReluDense = _Bag()
            ff.DenseReluDense.wi = nn.Linear(d_model, d_ff, bias=False)
            ff.DenseReluDense.wo = nn.Linear(d_ff, d_model, bias=False)
            ff.layer_norm = _Weight(d_model)
            blk = _Bag()
            blk.layer = nn.ModuleList([att, ff])
            self.encoder.block.append(blk)
        self.encoder.final_layer_norm = _Weight(d_model)
        self._init_engine()
        self.requires_grad_(False)         # frozen, as in the reference (:77-78)

    # ---- loading --------------------------------------------------------------------------------
    CONFIG_KEYS = ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads", "relative_attention_num_buckets",
                   "relative_attention_max_distance", "layer_norm_epsilon", "feed_forward_proj")

    @classmethod
    def from_directory(cls, path):
        """A local Hugging Face T5 directory (config.json + model.safetensors).  Keeps shared.* / encoder.*, ignores decoder.* / lm_head.*,
        takes encoder.embed_tokens.weight as an alias of shared.weight.  Never touches the network."""
        cfg_path, st_path = os.path.join(path, "config.json"), os.path.join(path, "model.safetensors")
        for p in (cfg_path, st_path):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"{p} is missing: T5Encoder.from_directory needs a local Hugging Face directory with "
                                        "config.json and model.safetensors (nothing is fetched)")
        with open(cfg_path) as fh:
            raw = json.load(fh)
        missing = [k for k in ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads") if k not in raw]
        if missing:
            raise ValueError(f"{cfg_path} lacks {missing}")
        model = cls(**{k: raw[k] for k in cls.CONFIG_KEYS if k in raw})
        from safetensors.torch import load_file
        sd = load_file(st_path)
        alias = sd.pop("encoder.embed_tokens.weight", None)
        if "shared.weight" not in sd and alias is not None:
            sd["shared.weight"] = alias
        sd = {k: v for k, v in sd.items() if k.startswith(("shared.", "encoder."))}
        model.load_state_dict(sd, strict=True)
        return model

    # ---- engine ---------------------------------------------------------------------------------
    weights_class = ET.T5Weights

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None):
        """input_ids [B, L <= 512] int64, attention_mask [B, L] right-padded (None: all ones) -> [B, L, d_model] fp32 on the device, rows at
        or past a prompt's length zero.  HIP tensors and the library are required: there is no CPU path."""
        ids = torch.as_tensor(input_ids)
        ET.check_ids(ids, self.config.vocab_size)
        lens = ET.lengths_of_mask(attention_mask, ids.shape)
        if not ids.is_cuda or self.shared.weight.device != ids.device:
            raise L.DcamdError("T5Encoder.forward needs CUDA/HIP tensors and the module on the same device (no CPU fallback)")
        L.require_gpu()
        dev = ids.device
        B, Lq = ids.shape
        key = (B, Lq, str(dev), self.compute_dtype)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = ET.T5Plan(self, self.packed_weights(E.DT[self.compute_dtype], dev), B, Lq)
        plan.ids.copy_(ids)
        plan.lens.copy_(lens.to(torch.int32))
        plan.run()
        return plan.out_view().clone()
