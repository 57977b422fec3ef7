"""MI355X-native CLIP text encoder: `transformers.CLIPTextModel`'s `last_hidden_state`, loaded from a LOCAL Hugging Face directory
(Stable Diffusion's `text_encoder/`, or an `openai/clip-vit-*` / OpenCLIP export with both towers).

Parameters carry the PUBLISHED state-dict key names (`text_model.embeddings.token_embedding.weight`, `text_model.encoder.layers.{i}.
self_attn.{q,k,v,out}_proj.{weight,bias}`, ...); transformers 5.x's own `CLIPTextModel.state_dict()` drops the `text_model.` prefix, so
`from_directory` takes keys with or without it.  Modules only hold parameters; arithmetic runs in libdcamd (engine_clip.py).  Nothing
here imports `transformers` or opens a socket; BPE tokenising is the caller's job.

`CLIPTextEncoder.hidden_state(..., layer=-2)` is transformers' `hidden_states[-2]` (what `clip_skip` / Stable Diffusion XL read), and
`CLIPTextEncoderWithProjection` (`transformers.CLIPTextModelWithProjection`, SDXL's `text_encoder_2/`) adds `text_projection` and the
pooled / EOS output `text_embeds`; both come out of the same plan run as the last state.  Out of scope: other layers than the last two,
the vision tower, `logit_scale`.
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

    BARE = ()      # keys that carry no `text_model.` prefix in a published file

    @classmethod
    def from_directory(cls, path):
        """A local Hugging Face CLIP directory (config.json + model.safetensors).  The text fields of the config may sit at top level
        (CLIPTextModel, Stable Diffusion's text_encoder/) or under "text_config" (CLIPModel).  Keys are taken with or without the
        `text_model.` prefix; vision_model.* / visual_projection.* / text_projection.* / logit_scale / *.position_ids are ignored;
        what is left loads strictly.  Never touches the network."""
        return cls._load_directory(path, "model.safetensors")

    @classmethod
    def _load_directory(cls, path, weights):
        cfg_path, st_path = os.path.join(path, "config.json"), os.path.join(path, weights)
        for p in (cfg_path, st_path):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"{p} is missing: {cls.__name__}.from_directory needs a local Hugging Face directory with "
                                        f"config.json and {weights} (nothing is fetched)")
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
            sd[k if k.startswith(EC.PREFIX) or k in cls.BARE else EC.PREFIX + k] = v
        model.load_state_dict(sd, strict=True)
        return model

    # ---- engine ---------------------------------------------------------------------------------
    weights_class = EC.ClipWeights

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None):
        """input_ids [B, L <= max_position_embeddings] int64, attention_mask [B, L] right-padded (None: all ones) -> last_hidden_state
        [B, L, hidden_size] fp32 on the device, rows at or past a prompt's length zero (the rows below it do not depend on the mask:
        causality hides the pad keys).  HIP tensors and the library are required: there is no CPU path."""
        return self._encode(input_ids, attention_mask, -1, False)

    @torch.no_grad()
    def hidden_state(self, input_ids, attention_mask=None, layer=-1):
        """`forward` at layer=-1; layer=-2: transformers' `hidden_states[-2]`, the fp32 residual stream after num_hidden_layers - 1
        layers WITHOUT the final LayerNorm (what Stable Diffusion XL conditions on), rows at or past a prompt's length zero."""
        return self._encode(input_ids, attention_mask, layer, False)

    def _eos_positions(self, ids, lens):
        raise NotImplementedError(f"{type(self).__name__} has no pooled output: CLIPTextEncoderWithProjection has")

    def _encode(self, input_ids, attention_mask, layer, pooled):
        """What `forward` and `hidden_state` share (and CLIPTextEncoderWithProjection.forward): one plan run per call.  The default
        (layer=-1, no pooled output) is the plan this class has always built, under the cache key it has always had."""
        if layer not in (-1, -2):
            raise ValueError(f"layer must be -1 (last_hidden_state) or -2 (hidden_states[-2]), got {layer!r}")
        if layer == -2 and self.config.num_hidden_layers < 2:
            raise ValueError(f"layer=-2 needs at least 2 layers, the encoder has {self.config.num_hidden_layers}")
        ids = torch.as_tensor(input_ids)
        ET.check_ids(ids, self.config.vocab_size)
        if ids.shape[1] > self.config.max_position_embeddings:
            raise ValueError(f"input_ids holds {ids.shape[1]} tokens per prompt but the encoder has max_position_embeddings = "
                             f"{self.config.max_position_embeddings}")
        lens = ET.lengths_of_mask(attention_mask, ids.shape)
        eos = self._eos_positions(ids.detach().cpu(), lens) if pooled else None      # host ids: refusals come before any launch
        tok = self.text_model.embeddings.token_embedding.weight
        if not ids.is_cuda or tok.device != ids.device:
            raise L.DcamdError("CLIPTextEncoder.forward needs CUDA/HIP tensors and the module on the same device (no CPU fallback)")
        L.require_gpu()
        dev = ids.device
        B, Lq = ids.shape
        key = (B, Lq, str(dev), self.compute_dtype)
        extra = dict(penultimate=True) if layer == -2 else {}
        if pooled:
            extra["pooled"] = True
        if extra:
            key += tuple(sorted(extra))
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = EC.ClipPlan(self, self.packed_weights(E.DT[self.compute_dtype], dev), B, Lq, **extra)
        plan.ids.copy_(ids)
        plan.lens.copy_(lens.to(torch.int32))
        if pooled:
            plan.eos.copy_(torch.arange(B, dtype=torch.int64) * Lq + eos)
        plan.run()
        if layer == -1:
            out = plan.out_view().clone()
        else:
            # the stream's rows past a prompt's length hold what the residual adds left there: zero them, as every output's pad rows are
            pad = torch.arange(Lq, device=dev)[None, :] >= lens.to(dev)[:, None]
            out = plan.hs2_view().masked_fill(pad[:, :, None], 0.0)
        return (out, plan.pooled_view().clone()) if pooled else out


class CLIPTextEncoderWithProjection(CLIPTextEncoder):
    """`transformers.CLIPTextModelWithProjection` (Stable Diffusion XL's `text_encoder_2/`): the text transformer of the parent plus
    `text_projection.weight` [projection_dim, hidden_size] (the published key; no bias) applied to the final-LayerNorm row at the EOS
    position -> `text_embeds`.  `eos_token_id` picks the position by transformers' two rules: 2 is the legacy config (SDXL's
    text_encoder_2 carries it) and means argmax(input_ids[b]); any other value means the first position that holds it."""

    def __init__(self, vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, max_position_embeddings=77,
                 hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=512, eos_token_id=2):
        super().__init__(vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, max_position_embeddings,
                         hidden_act, layer_norm_eps)
        if not isinstance(projection_dim, int) or projection_dim < 1:
            raise ValueError(f"CLIPTextEncoderWithProjection(projection_dim={projection_dim!r}) must be a positive int")
        if not isinstance(eos_token_id, int) or not 0 <= eos_token_id < vocab_size:
            raise ValueError(f"CLIPTextEncoderWithProjection(eos_token_id={eos_token_id!r}) must be a token id in [0, {vocab_size})")
        self.config.projection_dim, self.config.eos_token_id = projection_dim, eos_token_id
        self.text_projection = nn.Linear(hidden_size, projection_dim, bias=False)
        self.requires_grad_(False)

    CONFIG_KEYS = CLIPTextEncoder.CONFIG_KEYS + ("projection_dim", "eos_token_id")
    IGNORED = tuple(p for p in CLIPTextEncoder.IGNORED if p != "text_projection.")
    BARE = ("text_projection.weight",)

    @classmethod
    def from_directory(cls, path, variant=None):
        """As the parent's, with `text_projection.weight` loaded (strictly: a file without it is refused by that name) and
        variant="fp16" reading `model.fp16.safetensors`, the file most Stable Diffusion XL downloads hold."""
        return cls._load_directory(path, "model.safetensors" if variant is None else f"model.{variant}.safetensors")

    def _eos_positions(self, ids, lens):
        """[B] int64 on the host, transformers' two rules; a prompt without an EOS, or with it in its padding, is refused by row."""
        eos = self.config.eos_token_id
        if eos == 2:
            pos = ids.argmax(dim=1)
        else:
            hit = ids == eos
            none = (~hit.any(dim=1)).nonzero().reshape(-1).tolist()
            if none:
                raise ValueError(f"input_ids row {none[0]} holds no EOS token (eos_token_id = {eos}): the pooled output has no position")
            pos = hit.to(torch.int64).argmax(dim=1)
        late = (pos >= lens.to(torch.int64)).nonzero().reshape(-1).tolist()
        if late:
            raise ValueError(f"input_ids row {late[0]}: the EOS position {int(pos[late[0]])} lies at or past the prompt's length "
                             f"{int(lens[late[0]])} (attention_mask)")
        return pos.to(torch.int64)

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, *, layer=-1, pooled=False):
        """layer=-1: what the parent returns; layer=-2: `hidden_states[-2]` (see `hidden_state`).  pooled=True: returns (that tensor,
        text_embeds [B, projection_dim] fp32) with text_embeds = final_layer_norm(last stream)[b, eos_b] @ text_projection.weight.T;
        both come out of one plan run.  The ids are read on the host to find eos_b."""
        return self._encode(input_ids, attention_mask, layer, pooled)
