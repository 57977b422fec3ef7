"""MI355X-native CLIP text encoder: `transformers.CLIPTextModel`'s `last_hidden_state`, loaded from a LOCAL Hugging Face directory
(Stable Diffusion's `text_encoder/`, or an `openai/clip-vit-*` / OpenCLIP export with both towers).

Parameters carry the PUBLISHED state-dict key names (`text_model.embeddings.token_embedding.weight`, `text_model.encoder.layers.{i}.
self_attn.{q,k,v,out}_proj.{weight,bias}`, ...); transformers 5.x's own `CLIPTextModel.state_dict()` drops the `text_model.` prefix, so
`from_directory` takes keys with or without it.  Modules only hold parameters; arithmetic runs in libdcamd (engine_clip.py).  Nothing
here imports `transformers` or opens a socket; BPE tokenising is the caller's job.  Out of scope: the pooled / EOS output,
`text_projection`, `clip_skip` / penultimate-layer variants, the vision tower.
"""
import json
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import _lib as L
from .. import engine as E
from .. import engine_clip as EC
from .. import engine_t5 as ET
from .unet import _Bag, _HipBackbone


class CLIPTextEncoder(_HipBackbone):
    def __init__(self, vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads,
                 max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5):
        super().__init__()
        if hidden_act not in EC.ACTS:
            raise NotImplementedError(f"CLIPTextEncoder(hidden_act={hidden_act!r}) is not supported: {sorted(EC.ACTS)} only "
                                      "(quick_gelu: OpenAI CLIP; gelu: the erf form of OpenCLIP)")
        for name, val in (("hidden_size", hidden_size), ("intermediate_size", intermediate_size)):
            if val < 64 or val % 64:
                raise NotImplementedError(f"CLIPTextEncoder({name}={val}) is not supported: it must be a multiple of 64 (the K granule of "
                                          "the 16-bit token GEMMs)")
        if num_attention_heads < 1 or hidden_size % num_attention_heads or hidden_size // num_attention_heads not in EC.HEAD_DIMS:
            raise NotImplementedError(f"CLIPTextEncoder(num_attention_heads={num_attention_heads}) is not supported with hidden_size="
                                      f"{hidden_size}: head widths {EC.HEAD_DIMS} only")
        if not 1 <= max_position_embeddings <= EC.MAX_LENGTH:
            raise NotImplementedError(f"CLIPTextEncoder(max_position_embeddings={max_position_embeddings}) is not supported: at most "
                                      f"{EC.MAX_LENGTH} positions (dc_attention_causal)")
        self.config = SimpleNamespace(vocab_size=vocab_size, hidden_size=hidden_size, intermediate_size=intermediate_size,
                                      num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
                                      max_position_embeddings=max_position_embeddings, hidden_act=hidden_act,
                                      layer_norm_eps=layer_norm_eps)
        tm = self.text_model = _Bag()
        tm.embeddings = _Bag()
        tm.embeddings.token_embedding = nn.Embedding(vocab_size, hidden_size)
        tm.embeddings.position_embedding = nn.Embedding(max_position_embeddings, hidden_size)
        tm.encoder = _Bag()
        tm.encoder.layers = nn.ModuleList()
        for _ in range(num_hidden_layers):
            lay = _Bag()
            lay.self_attn = _Bag()
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                setattr(lay.self_attn, n, nn.Linear(hidden_size, hidden_size))
            lay.layer_norm1 = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
            lay.mlp = _Bag()
            lay.mlp.fc1 = nn.Linear(hidden_size, intermediate_size)
            lay.mlp.fc2 = nn.Linear(intermediate_size, hidden_size)
            lay.layer_norm2 = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
            tm.encoder.layers.append(lay)
        tm.final_layer_norm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
        self._init_engine()
        self.requires_grad_(False)         # frozen: an encoder of prompts, not a trained part

    # ---- loading --------------------------------------------------------------------------------
    REQUIRED_KEYS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads")
    CONFIG_KEYS = REQUIRED_KEYS + ("max_position_embeddings", "hidden_act", "layer_norm_eps")
    IGNORED = ("vision_model.", "visual_projection.", "text_projection.", "logit_scale")

    @classmethod
    def from_directory(cls, path):
        """A local Hugging Face CLIP directory (config.json + model.safetensors).  The text fields of the config may sit at top level
        (CLIPTextModel, Stable Diffusion's text_encoder/) or under "text_config" (CLIPModel).  Keys are taken with or without the
        `text_model.` prefix; vision_model.* / visual_projection.* / text_projection.* / logit_scale / *.position_ids are ignored;
        what is left loads strictly.  Never touches the network."""
        cfg_path, st_path = os.path.join(path, "config.json"), os.path.join(path, "model.safetensors")
        for p in (cfg_path, st_path):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"{p} is missing: CLIPTextEncoder.from_directory needs a local Hugging Face directory with "
                                        "config.json and model.safetensors (nothing is fetched)")
        with open(cfg_path) as fh:
            raw = json.load(fh)
        if not all(k in raw for k in cls.REQUIRED_KEYS) and isinstance(raw.get("text_config"), dict):
            raw = raw["text_config"]
        missing = [k for k in cls.REQUIRED_KEYS if k not in raw]
        if missing:
            raise ValueError(f"{cfg_path} lacks {missing} (at top level and under text_config)")
        model = cls(**{k: raw[k] for k in cls.CONFIG_KEYS if k in raw})
        from safetensors.torch import load_file
        sd = {}
        for k, v in load_file(st_path).items():
            if k.startswith(cls.IGNORED) or k.endswith(".position_ids"):
                continue
            sd[k if k.startswith(EC.PREFIX) else EC.PREFIX + k] = v
        model.load_state_dict(sd, strict=True)
        return model

    # ---- engine ---------------------------------------------------------------------------------
    weights_class = EC.ClipWeights

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None):
        """input_ids [B, L <= max_position_embeddings] int64, attention_mask [B, L] right-padded (None: all ones) -> last_hidden_state
        [B, L, hidden_size] fp32 on the device, rows at or past a prompt's length zero (the rows below it do not depend on the mask:
        causality hides the pad keys).  HIP tensors and the library are required: there is no CPU path."""
        ids = torch.as_tensor(input_ids)
        ET.check_ids(ids, self.config.vocab_size)
        if ids.shape[1] > self.config.max_position_embeddings:
            raise ValueError(f"input_ids holds {ids.shape[1]} tokens per prompt but the encoder has max_position_embeddings = "
                             f"{self.config.max_position_embeddings}")
        lens = ET.lengths_of_mask(attention_mask, ids.shape)
        tok = self.text_model.embeddings.token_embedding.weight
        if not ids.is_cuda or tok.device != ids.device:
            raise L.DcamdError("CLIPTextEncoder.forward needs CUDA/HIP tensors and the module on the same device (no CPU fallback)")
        L.require_gpu()
        dev = ids.device
        B, Lq = ids.shape
        key = (B, Lq, str(dev), self.compute_dtype)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = EC.ClipPlan(self, self.packed_weights(E.DT[self.compute_dtype], dev), B, Lq)
        plan.ids.copy_(ids)
        plan.lens.copy_(lens.to(torch.int32))
        plan.run()
        return plan.out_view().clone()
