"""The Stable Diffusion UNet (diffusers `UNet2DConditionModel` as SD 1.x / 2.x publish it) as a HIP backbone.

`StableDiffusionUNet` is a class of its own next to `UNetCondition2D`, with its own envelope: what the reference's family never needs
and every published SD UNet does —
  encoder_hid_dim_type=None   no `encoder_hid_proj`: the prompt states [N, S, cross_attention_dim] are attn2's keys and values as they are
  use_linear_projection       proj_in / proj_out stored as [C, C] (SD 2.x) or [C, C, 1, 1] (SD 1.x); the same arithmetic
  attention_head_dim          an int or one entry per down block, with diffusers' quirk kept: the value is the NUMBER OF HEADS of the level
                              (up blocks read the tuple reversed, the mid block its last entry)
  head widths                 C // heads: every width the plan serves zero-padded (at most 128), and exactly 160 (SD 1.x: 1280 channels in 8
                              heads), which runs unpadded through dc_cross_attention for attn1 and attn2 alike (engine.py)
`noise_labels` is the DDPM step as a float (DiffusionClassifier's schedule='scaled_linear' feeds it).  Parameters sit under the
published key names, so a published state dict loads strictly.  As for UNetCondition2D there is no eager / CPU path.

`StableDiffusionXLUNet`, at the end of this file, is the same for SDXL base: transformer depth per level and the text_time embedding.
"""
import json
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import _lib as L
from .. import engine as E
from .unet import UNetCondition2D, _Bag


class StableDiffusionUNet(UNetCondition2D):
    def __init__(self, sample_size=None, in_channels=4, out_channels=4, center_input_sample=False, flip_sin_to_cos=True, freq_shift=0,
                 down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
                 mid_block_type="UNetMidBlock2DCrossAttn",
                 up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
                 only_cross_attention=False, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, downsample_padding=1,
                 mid_block_scale_factor=1, dropout=0.0, act_fn="silu", norm_num_groups=32, norm_eps=1e-5, cross_attention_dim=1280,
                 transformer_layers_per_block=1, reverse_transformer_layers_per_block=None, encoder_hid_dim=None, encoder_hid_dim_type=None,
                 attention_head_dim=8, num_attention_heads=None, dual_cross_attention=False, use_linear_projection=False,
                 class_embed_type=None, addition_embed_type=None, addition_time_embed_dim=None, num_class_embeds=None,
                 upcast_attention=False, resnet_time_scale_shift="default", resnet_skip_time_act=False, resnet_out_scale_factor=1.0,
                 time_embedding_type="positional", time_embedding_dim=None, time_embedding_act_fn=None, timestep_post_act=None,
                 time_cond_proj_dim=None, conv_in_kernel=3, conv_out_kernel=3, projection_class_embeddings_input_dim=None,
                 attention_type="default", class_embeddings_concat=False, mid_block_only_cross_attention=None, cross_attention_norm=None,
                 addition_embed_type_num_heads=64):
        super(UNetCondition2D, self).__init__()
        who = type(self).__name__
        unsupported = dict(
            class_embed_type=(class_embed_type, None), addition_embed_type=(addition_embed_type, None),
            dual_cross_attention=(dual_cross_attention, False), only_cross_attention=(only_cross_attention, False),
            transformer_layers_per_block=(transformer_layers_per_block, 1), time_cond_proj_dim=(time_cond_proj_dim, None),
            attention_type=(attention_type, "default"), encoder_hid_dim_type=(encoder_hid_dim_type, None),
            encoder_hid_dim=(encoder_hid_dim, None), num_attention_heads=(num_attention_heads, None),
            center_input_sample=(center_input_sample, False), downsample_padding=(downsample_padding, 1),
            mid_block_scale_factor=(mid_block_scale_factor, 1), dropout=(dropout, 0.0), act_fn=(act_fn, "silu"),
            num_class_embeds=(num_class_embeds, None), resnet_time_scale_shift=(resnet_time_scale_shift, "default"),
            resnet_skip_time_act=(resnet_skip_time_act, False), resnet_out_scale_factor=(resnet_out_scale_factor, 1.0),
            time_embedding_type=(time_embedding_type, "positional"), time_embedding_dim=(time_embedding_dim, None),
            conv_in_kernel=(conv_in_kernel, 3), conv_out_kernel=(conv_out_kernel, 3),
            mid_block_type=(mid_block_type, "UNetMidBlock2DCrossAttn"), cross_attention_norm=(cross_attention_norm, None),
            timestep_post_act=(timestep_post_act, None), time_embedding_act_fn=(time_embedding_act_fn, None),
            reverse_transformer_layers_per_block=(reverse_transformer_layers_per_block, None),
            mid_block_only_cross_attention=(mid_block_only_cross_attention, None), class_embeddings_concat=(class_embeddings_concat, False))
        for k, (got, want) in unsupported.items():
            if k in self.OPEN:                                             # a subclass judges these itself (_open_options)
                continue
            if isinstance(got, (list, tuple)) and len(set(got)) == 1:      # (False, False, False, False) is False
                got = got[0]
            if got != want:
                raise NotImplementedError(f"{who}({k}={got!r}) is outside the {self.ENVELOPE} envelope built here (supported: {want!r})")
        if not isinstance(cross_attention_dim, int):
            raise NotImplementedError(f"{who}(cross_attention_dim={cross_attention_dim!r}): one context width for every level only")
        boc = tuple(block_out_channels)
        nb = len(boc)
        lpb = (layers_per_block,) * nb if isinstance(layers_per_block, int) else tuple(layers_per_block)
        ahd = (attention_head_dim,) * nb if isinstance(attention_head_dim, int) else tuple(attention_head_dim)
        if len(down_block_types) != nb or len(up_block_types) != nb or len(lpb) != nb or len(ahd) != nb:
            raise ValueError(f"{who}: block_out_channels, down_block_types, up_block_types, layers_per_block and attention_head_dim must "
                             f"name the same number of levels ({nb})")
        # the value is the number of heads of its level (diffusers' naming quirk, kept); up blocks read the tuple reversed
        rboc, rahd = boc[::-1], ahd[::-1]
        sites = {(boc[-1], ahd[-1])} | {(boc[i], ahd[i]) for i, k in enumerate(down_block_types) if k == "CrossAttnDownBlock2D"} \
            | {(rboc[i], rahd[i]) for i, k in enumerate(up_block_types) if k == "CrossAttnUpBlock2D"}
        for C, heads in sorted(sites):
            if not isinstance(heads, int) or heads < 1 or C % heads:
                raise NotImplementedError(f"{who}(attention_head_dim={attention_head_dim!r}): a {C}-channel level cannot be cut into {heads!r} heads")
            try:
                E.site_head_dim(C // heads)
            except NotImplementedError:
                raise NotImplementedError(f"{who}(attention_head_dim={attention_head_dim!r}): a {C}-channel attention level in {heads} heads has a "
                                          f"head width of {C // heads}: at most {E.HEAD_DIMS[-1]}, or exactly {E.WIDE_HEAD}") from None
        self.config = SimpleNamespace(
            sample_size=sample_size, in_channels=in_channels, out_channels=out_channels,
            down_block_types=tuple(down_block_types), up_block_types=tuple(up_block_types), mid_block_type=mid_block_type,
            block_out_channels=boc, layers_per_block=lpb, norm_num_groups=norm_num_groups, norm_eps=norm_eps,
            cross_attention_dim=cross_attention_dim,
            # no projection of the context: what DiffusionClassifier sizes its prompt table (and checks a text encoder's width) by is
            # the width attn2 reads
            encoder_hid_dim=cross_attention_dim, encoder_hid_dim_type=None,
            attention_head_dim=ahd, use_linear_projection=bool(use_linear_projection), upcast_attention=bool(upcast_attention),
            flip_sin_to_cos=flip_sin_to_cos, freq_shift=freq_shift)
        self._open_options(nb, transformer_layers_per_block=transformer_layers_per_block, addition_embed_type=addition_embed_type,
                           addition_time_embed_dim=addition_time_embed_dim,
                           projection_class_embeddings_input_dim=projection_class_embeddings_input_dim)
        self._build_modules(in_channels, out_channels, None, linear=bool(use_linear_projection))
        self._init_engine()

    ENVELOPE = "Stable Diffusion 1.x / 2.x"
    OPEN = ()          # constructor options whose refusal above a subclass lifts and checks in _open_options

    def _open_options(self, nb, **options):
        """Hook between the envelope check and the modules: a subclass validates its OPEN options and writes them into self.config."""

    # ---- loading --------------------------------------------------------------------------------
    REQUIRED_KEYS = ("sample_size", "in_channels", "out_channels", "down_block_types", "up_block_types", "block_out_channels",
                     "layers_per_block", "cross_attention_dim", "attention_head_dim")
    WEIGHTS = "diffusion_pytorch_model.safetensors"

    @classmethod
    def from_directory(cls, path, **overrides):
        """A local diffusers `unet/` directory (config.json + diffusion_pytorch_model.safetensors).  Config keys that start with `_` are
        ignored, every other key goes to the constructor (which refuses what is outside the envelope, by name), `overrides` replace
        keys of the file (`sample_size=32` to score 256-pixel images with a model published at 512).  The weights load strictly and the
        model is frozen.  Never touches the network."""
        return cls._load_directory(path, cls.WEIGHTS, overrides)

    @classmethod
    def _load_directory(cls, path, weights, overrides):
        cfg_path, st_path = os.path.join(path, "config.json"), os.path.join(path, weights)
        for p in (cfg_path, st_path):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"{p} is missing: {cls.__name__}.from_directory needs a local diffusers UNet2DConditionModel directory "
                                        f"with config.json and {weights} (nothing is fetched)")
        with open(cfg_path) as fh:
            raw = json.load(fh)
        missing = [k for k in cls.REQUIRED_KEYS if k not in raw]
        if missing:
            raise ValueError(f"{cfg_path} lacks {missing}")
        kw = {k: v for k, v in raw.items() if not k.startswith("_")}
        kw.update(overrides)
        try:
            model = cls(**kw)
        except TypeError as e:
            raise NotImplementedError(f"{cfg_path}: {e} (a config key this envelope does not know)") from None
        from safetensors.torch import load_file
        model.load_state_dict(load_file(st_path), strict=True)
        model.requires_grad_(False)
        return model


class StableDiffusionXLUNet(StableDiffusionUNet):
    """The UNet of Stable Diffusion XL base: a class of its own next to StableDiffusionUNet, whose envelope and refusals do not move.
    What it accepts on top:
      addition_embed_type="text_time"   `add_embedding.linear_1 / linear_2` over [text_embeds | sinusoid(time_ids)]: with
                                        `addition_time_embed_dim` (the width of each of the six size numbers' sinusoid) and
                                        `projection_class_embeddings_input_dim` (= pooled width + 6 * addition_time_embed_dim).  Every
                                        ResNet reads time_emb_proj(SiLU(time_embedding(t) + aug)), and aug differs per class: the time
                                        vector is per UNIT here, every ResNet is a per-unit layer and `share_trunk` shares conv_in alone
      transformer_layers_per_block      an int or one entry per down block (up blocks read it reversed, the mid block takes the last, as
                                        attention_head_dim): `transformer_blocks.{k}` of a site run in sequence between one proj_in and
                                        one proj_out
    Anything else StableDiffusionUNet refuses stays refused, by name.  Scoring only: `forward`, and `classify` under
    DiffusionClassifier's encoder_type='clip_dual'; `forward_pair` / `pair_session` (generation) raise NotImplementedError.  A context of
    one token is refused when a plan is built: SDXL is always a prompt plan."""
    ENVELOPE = "Stable Diffusion XL"
    OPEN = ("addition_embed_type", "transformer_layers_per_block")

    def _open_options(self, nb, *, transformer_layers_per_block, addition_embed_type, addition_time_embed_dim,
                      projection_class_embeddings_input_dim):
        who, cfg = type(self).__name__, self.config
        if addition_embed_type != "text_time":
            raise NotImplementedError(f"{who}(addition_embed_type={addition_embed_type!r}) is outside the {self.ENVELOPE} envelope built here "
                                      "(supported: 'text_time'; without it the model is a StableDiffusionUNet)")
        tl = transformer_layers_per_block
        tl = (tl,) * nb if isinstance(tl, int) and not isinstance(tl, bool) else tuple(tl) if isinstance(tl, (list, tuple)) else None
        if tl is None or len(tl) != nb or not all(isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in tl):
            raise NotImplementedError(f"{who}(transformer_layers_per_block={transformer_layers_per_block!r}) is not supported: an int >= 1 or "
                                      f"one per down block ({nb})")
        dim, pcid = addition_time_embed_dim, projection_class_embeddings_input_dim
        # the fp32 side-path GEMM reads [text_embeds | sinusoids] as two K ranges: each a multiple of its K granule (32)
        if not isinstance(dim, int) or isinstance(dim, bool) or dim < 2 or dim % 2 or (6 * dim) % 32:
            raise NotImplementedError(f"{who}(addition_time_embed_dim={dim!r}) is not supported: an even int with 6 * dim a multiple of 32")
        if not isinstance(pcid, int) or isinstance(pcid, bool) or pcid <= 6 * dim or (pcid - 6 * dim) % 32:
            raise NotImplementedError(f"{who}(projection_class_embeddings_input_dim={pcid!r}) is not supported: 6 * addition_time_embed_dim "
                                      f"(= {6 * dim}) plus a pooled text width that is a positive multiple of 32")
        cfg.transformer_layers_per_block, cfg.addition_embed_type = tl, addition_embed_type
        cfg.addition_time_embed_dim, cfg.projection_class_embeddings_input_dim = dim, pcid
        cfg.pooled_dim = pcid - 6 * dim                   # the width of text_embeds

    def _build_modules(self, in_channels, out_channels, hid_proj_dim, linear=False):
        super()._build_modules(in_channels, out_channels, hid_proj_dim, linear=linear)
        temb = self.config.block_out_channels[0] * 4
        self.add_embedding = _Bag()
        self.add_embedding.linear_1 = nn.Linear(self.config.projection_class_embeddings_input_dim, temb)
        self.add_embedding.linear_2 = nn.Linear(temb, temb)

    @classmethod
    def from_directory(cls, path, variant=None, **overrides):
        """As StableDiffusionUNet.from_directory; variant="fp16" reads `diffusion_pytorch_model.fp16.safetensors`, the file most Stable
        Diffusion XL downloads hold (the parameters are kept in fp32 either way; the compute dtype is the classifier's)."""
        return cls._load_directory(path, cls.WEIGHTS if variant is None else f"diffusion_pytorch_model.{variant}.safetensors", overrides)

    def _added(self, added_cond_kwargs, N):
        """(text_embeds [N, pooled_dim], time_ids [N, 6]) of diffusers' added_cond_kwargs, validated on the host."""
        kw = added_cond_kwargs or {}
        missing = [k for k in ("text_embeds", "time_ids") if k not in kw]
        if missing:
            raise ValueError(f"{type(self).__name__}.forward: added_cond_kwargs lacks {missing} (diffusers' names: text_embeds [N, "
                             f"{self.config.pooled_dim}], time_ids [N, 6])")
        te, ti = kw["text_embeds"], kw["time_ids"]
        if tuple(te.shape) != (N, self.config.pooled_dim) or tuple(ti.shape) != (N, 6):
            raise ValueError(f"added_cond_kwargs: text_embeds must be [{N}, {self.config.pooled_dim}] and time_ids [{N}, 6], got "
                             f"{tuple(te.shape)} and {tuple(ti.shape)}")
        return te, ti

    @torch.no_grad()
    def forward(self, x, noise_labels, encoder_hidden_states=None, added_cond_kwargs=None, encoder_lengths=None):
        """added_cond_kwargs = {"text_embeds": [N, pooled width], "time_ids": [N, 6]} (diffusers' names; a missing key: ValueError);
        encoder_lengths as StableDiffusionUNet.forward's."""
        te, ti = self._added(added_cond_kwargs, x.shape[0])
        L.require_gpu()
        if not x.is_cuda:
            raise L.DcamdError(f"{type(self).__name__}.forward needs CUDA/HIP tensors (no CPU fallback)")
        S = self._context_tokens(encoder_hidden_states)

        def fill(plan):
            plan.pooled.copy_(te.to(x.device, torch.float32))
            plan.time_ids.copy_(ti.to(x.device, torch.float32))
        plan = self._ctx_plan(("fwd",), x.shape[0], x.device, S, (encoder_hidden_states,), (encoder_lengths,), fill=fill)
        self._feed(plan, x, noise_labels)
        plan.run()
        return plan.pred_view().permute(0, 3, 1, 2).contiguous().to(x.dtype)

    def forward_pair(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__}.forward_pair: generation with an SDXL backbone is not built (scoring only)")

    def pair_session(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__}.pair_session: generation with an SDXL backbone is not built (scoring only)")
