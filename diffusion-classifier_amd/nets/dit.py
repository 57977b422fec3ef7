"""MI355X-native drop-in for reference `nets/dit.py`.

`DiT(**kwargs)` keeps the reference constructor keywords (nets/dit.py:9-27) and
`forward(x, noise_labels, encoder_hidden_states=None)` (nets/dit.py:49-51), where — exactly as
in the reference, which passes its third argument positionally into diffusers'
`class_labels` slot — `encoder_hidden_states` carries the int64 class labels
(`encoder_type='DiT'`, diffusion_classifier.py:90-92).  Parameter names are diffusers'
`DiTTransformer2DModel`'s.  Modules only hold parameters; arithmetic runs in libdcamd.
"""
import json
import os
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L
from .. import engine as E
from .. import engine_dit as ED
from ..packing import eps_rows
from .unet import PairSession, _Bag, _HipBackbone


def _sincos_1d(dim, pos):
    omega = 1.0 / 10000 ** (np.arange(dim // 2, dtype=np.float64) / (dim / 2.0))
    out = np.einsum("m,d->md", pos.reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def sincos_pos_embed(dim, grid, base_size, interpolation_scale=1.0):
    """Fixed 2-D sin-cos table of diffusers' PatchEmbed (meshgrid puts the W coordinate first)."""
    c = np.arange(grid, dtype=np.float32) / (grid / base_size) / interpolation_scale
    g = np.stack(np.meshgrid(c, c), axis=0).reshape(2, 1, grid, grid)
    return np.concatenate([_sincos_1d(dim // 2, g[0]), _sincos_1d(dim // 2, g[1])], axis=1)


class DiT(_HipBackbone):
    def __init__(
        self,
        num_attention_heads: int = 16,
        attention_head_dim: int = 72,
        in_channels: int = 4,
        out_channels: Optional[int] = None,
        num_layers: int = 28,
        dropout: float = 0.0,
        norm_num_groups: int = 32,
        attention_bias: bool = True,
        sample_size: int = 32,
        patch_size: int = 2,
        activation_fn: str = "gelu-approximate",
        num_embeds_ada_norm: Optional[int] = 1000,
        upcast_attention: bool = False,
        norm_type: str = "ada_norm_zero",
        norm_elementwise_affine: bool = False,
        norm_eps: float = 1e-5,
    ):
        super().__init__()
        for k, (got, want) in dict(dropout=(dropout, 0.0), attention_bias=(attention_bias, True),
                                   activation_fn=(activation_fn, "gelu-approximate"), norm_type=(norm_type, "ada_norm_zero"),
                                   norm_elementwise_affine=(norm_elementwise_affine, False)).items():
            if got != want:
                raise NotImplementedError(f"DiT({k}={got!r}) is outside the scoring path built here (supported: {want!r})")
        E.padded_head_dim(attention_head_dim)      # heads wider than 128 are refused here; narrower ones run zero-padded (packing.py)
        D = num_attention_heads * attention_head_dim
        out_channels = in_channels if out_channels is None else out_channels
        self.D = D
        self.config = SimpleNamespace(
            num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim, in_channels=in_channels,
            out_channels=out_channels, num_layers=num_layers, sample_size=sample_size, patch_size=patch_size,
            num_embeds_ada_norm=num_embeds_ada_norm, norm_eps=norm_eps, encoder_hid_dim=None)
        self.pos_embed = _Bag()
        self.pos_embed.proj = nn.Conv2d(in_channels, D, patch_size, stride=patch_size)
        g = sample_size // patch_size
        self.pos_embed.register_buffer(
            "pos_embed", torch.from_numpy(sincos_pos_embed(D, g, base_size=g)).float().unsqueeze(0), persistent=False)
        self.transformer_blocks = nn.ModuleList()
        for _ in range(num_layers):
            b = _Bag()
            b.norm1 = _Bag()
            b.norm1.emb = _Bag()
            b.norm1.emb.timestep_embedder = _Bag()
            b.norm1.emb.timestep_embedder.linear_1 = nn.Linear(256, D)
            b.norm1.emb.timestep_embedder.linear_2 = nn.Linear(D, D)
            b.norm1.emb.class_embedder = _Bag()
            b.norm1.emb.class_embedder.embedding_table = nn.Embedding(num_embeds_ada_norm + 1, D)
            b.norm1.linear = nn.Linear(D, 6 * D)
            a = _Bag()
            a.to_q, a.to_k, a.to_v = nn.Linear(D, D), nn.Linear(D, D), nn.Linear(D, D)
            a.to_out = nn.ModuleList([nn.Linear(D, D), nn.Identity()])
            b.attn1 = a
            b.ff = _Bag()
            pr = _Bag()
            pr.proj = nn.Linear(D, 4 * D)
            b.ff.net = nn.ModuleList([pr, nn.Identity(), nn.Linear(4 * D, D)])
            self.transformer_blocks.append(b)
        self.proj_out_1 = nn.Linear(D, 2 * D)
        self.proj_out_2 = nn.Linear(D, patch_size * patch_size * out_channels)
        self.patch = patch_size
        self._init_engine()

    weights_class, im2col = ED.DiTWeights, 2                   # `patch` is the instance's patch_size

    eps_rows_only = True       # trajectory.step_fields: forward_pair / a pair session hand out eps alone, at feature stride in_channels
    variance_pair_plans = True      # ... and with variance=True all out_channels, at feature stride out_channels (the learned-range step)

    def make_plan(self, n_bj, n_cls, n_ctx, device, score=None, share_trunk=None, eps_only=False):
        """eps_only (implied by a score): the plan's prediction holds eps alone, [U, g, g, p*p*in_channels] — with learned-variance
        outputs (out_channels == 2 * in_channels) proj_out_2 is cut to its eps rows; another out_channels != in_channels is refused
        here, before anything is packed (engine_dit.DiTPlan)."""
        if eps_only or score is not None:
            eps_rows(self.patch, self.config.in_channels, self.config.out_channels, type(self).__name__)
        dt = E.DT[self.compute_dtype]
        return ED.DiTPlan(self, self.packed_weights(dt, device), n_bj, n_cls, n_ctx, score=score, device=device, eps_only=eps_only)

    def _label_plan(self, kind, N, dev, labels):
        """What `forward`, `forward_pair` and `pair_session` share: the plan cached under kind + (N, device, dtype) (built on first use)
        with the labels — one int tensor of N per unit of an image, unit n_cls * b + u = labels[u][b] — copied into its `ctx_of_unit`.
        `forward`'s plan predicts all out_channels, the pair plans eps alone — but the "pair_var" / "pair_session_var" kinds of
        `variance=True`, plans of their own that run the full proj_out_2."""
        key = kind + (N, str(dev), self.compute_dtype)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self.make_plan(N, len(labels), None, dev, eps_only=kind[0] in ("pair", "pair_session"))
        plan.ctx_of_unit.copy_(torch.stack([lab.reshape(-1) for lab in labels], dim=1).reshape(-1).to(dev, torch.int32))
        return plan

    def _pair_kind(self, kind, variance):
        """The plan-key kind of a pair plan: `kind`, or kind + "_var" for the plans that keep the variance features."""
        if not variance:
            return kind
        C, oc = self.config.in_channels, self.config.out_channels
        if oc != 2 * C:
            raise L.DcamdError(f"variance=True needs learned-variance outputs, out_channels == 2 * in_channels (got {oc} vs 2 * {C} = {2 * C})")
        return kind + "_var"

    @torch.no_grad()
    def forward_pair(self, x, noise_labels, cond, null, variance=False):
        """Classifier-free-guidance pair as ONE batch-2 plan launch: unit 2b = image b under label `cond[b]`, unit 2b+1 under the
        null label `null[b]` (reference `sample`, :255-266, calls the backbone twice per step).  Returns the plan's patch-major
        projection [2N, H/p, W/p, p*p*in_channels] fp32, eps alone — a learned variance (out_channels == 2 * in_channels) is dropped, as
        the fixed-variance samplers never read it (the layout `dc_ddpm_step` reads with patch = p) — a view the next call overwrites.
        variance=True (out_channels == 2 * in_channels only): a plan of its own with the full proj_out_2, the prediction
        [2N, H/p, W/p, p*p*out_channels] — per pixel eps then the variance interpolation, feature stride out_channels, the layout
        `dc_ddpm_step_shared` reads in DC_STEP_LEARNED_RANGE."""
        L.require_gpu()
        if not x.is_cuda:
            raise L.DcamdError("DiT.forward_pair needs CUDA/HIP tensors (no CPU fallback)")
        plan = self._label_plan((self._pair_kind("pair", variance),), x.shape[0], x.device, (cond, null))
        self._feed(plan, x, noise_labels)
        plan.run()
        return plan.pred_view()

    @torch.no_grad()
    def pair_session(self, N, device, cond, null, slot=0, variance=False):
        """The once-per-call half of `forward_pair` for N images on `device`: the label pairs copied into the `ctx_of_unit` of a plan that
        belongs to `slot`.  Returns a `PairSession` (nets/unet.py) whose `step(x, lam)` gives what `forward_pair(x, lam, cond, null)`
        gives.  variance: as `forward_pair`'s, a plan of its own per slot."""
        L.require_gpu()
        if cond.numel() != N or null.numel() != N:
            raise L.DcamdError(f"a pair session of {N} images needs {N} labels per side, got {cond.numel()} and {null.numel()}")
        return PairSession(self, self._label_plan((self._pair_kind("pair_session", variance), slot), N, torch.device(device), (cond, null)), N)

    @torch.no_grad()
    def forward(self, x, noise_labels, encoder_hidden_states=None):
        L.require_gpu()
        if not x.is_cuda:
            raise L.DcamdError("DiT.forward needs CUDA/HIP tensors (no CPU fallback)")
        N, Cin, H, W = x.shape
        p, oc = self.patch, self.config.out_channels
        plan = self._label_plan(("fwd",), N, x.device, (encoder_hidden_states,))
        self._feed(plan, x, noise_labels)
        plan.run()
        g = H // p
        out = plan.pred_view().reshape(N, g, g, p, p, oc)          # un-patchify: nhwpqc -> nchpwq
        return out.permute(0, 5, 1, 3, 2, 4).reshape(N, oc, g * p, g * p).contiguous().to(x.dtype)

    # ---- loading --------------------------------------------------------------------------------
    REQUIRED_KEYS = ("num_attention_heads", "attention_head_dim", "in_channels", "num_layers", "sample_size", "patch_size",
                     "num_embeds_ada_norm")
    # keys of diffusers' Transformer2DModel / DiTTransformer2DModel config that the constructor does not take: accepted at the value the
    # published DiT checkpoints carry (the class-conditional adaLN-Zero transformer on continuous latents), refused by name at another
    FIXED_KEYS = dict(cross_attention_dim=None, num_vector_embeds=None, only_cross_attention=False, use_linear_projection=False,
                      double_self_attention=False, attention_type="default", caption_channels=None, interpolation_scale=None)
    WEIGHTS = "diffusion_pytorch_model.safetensors"

    @classmethod
    def from_directory(cls, path, **overrides):
        """A local diffusers `transformer/` directory (config.json + diffusion_pytorch_model.safetensors) of a published DiT.  Config keys
        that start with `_` are ignored; `overrides` replace keys of the file; the keys of FIXED_KEYS must carry the value given there;
        every other key goes to the constructor, which refuses what is outside the envelope by name — as is a key neither knows.  The
        weights load strictly (the parameter names are diffusers') and the model is frozen.  Never touches the network."""
        cfg_path, st_path = os.path.join(path, "config.json"), os.path.join(path, cls.WEIGHTS)
        for f in (cfg_path, st_path):
            if not os.path.isfile(f):
                raise FileNotFoundError(f"{f} is missing: {cls.__name__}.from_directory needs a local diffusers DiTTransformer2DModel / "
                                        f"Transformer2DModel directory with config.json and {cls.WEIGHTS} (nothing is fetched)")
        with open(cfg_path) as fh:
            raw = json.load(fh)
        missing = [k for k in cls.REQUIRED_KEYS if k not in raw]
        if missing:
            raise ValueError(f"{cfg_path} lacks {missing}")
        kw = {k: v for k, v in raw.items() if not k.startswith("_")}
        kw.update(overrides)
        for k, want in cls.FIXED_KEYS.items():
            got = kw.pop(k, want)
            if got != want:
                raise NotImplementedError(f"{cls.__name__}({k}={got!r}) is outside the scoring path built here (supported: {want!r})")
        try:
            model = cls(**kw)
        except TypeError as e:
            raise NotImplementedError(f"{cfg_path}: {e} (a config key this envelope does not know)") from None
        from safetensors.torch import load_file
        model.load_state_dict(load_file(st_path), strict=True)
        model.requires_grad_(False)
        return model
