"""MI355X-native AutoencoderKL, ENCODER and DECODER: the step from an image to the latents a Stable-Diffusion-style UNet or a DiT on
`sd-vae-ft` latents is trained on, and the step back from latents to an image, each loaded from a LOCAL diffusers directory (Stable
Diffusion's `vae/`, `stabilityai/sd-vae-ft-mse`).

`forward(x)` returns `(mean - shift_factor) * scaling_factor`, the mean of the posterior `AutoencoderKL.encode(x).latent_dist`, scaled as
the pipelines scale it.  Parameters carry the PUBLISHED state-dict key names (`encoder.conv_in.weight`, `encoder.down_blocks.{i}.resnets.
{j}.conv1.weight`, `encoder.mid_block.attentions.0.to_q.weight`, `quant_conv.weight`, ...).  Modules only hold parameters; arithmetic runs
in libdcamd (engine_vae.py).  Nothing here imports `diffusers` or opens a socket.  `VAEEncoder` ignores `decoder.*` and
`post_quant_conv.*` when loading; `VAEDecoder` (below) is the other half and ignores `encoder.*` and `quant_conv.*`.  Out of scope:
sampling from the posterior, tiling and slicing.
"""
import json
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import _lib as L
from .. import engine as E
from .. import engine_vae as EV
from .unet import _Bag, _HipBackbone


def _resnet(cin, cout, groups):
    r = _Bag()
    r.norm1 = nn.GroupNorm(groups, cin, eps=EV.GN_EPS)
    r.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
    r.norm2 = nn.GroupNorm(groups, cout, eps=EV.GN_EPS)
    r.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
    if cin != cout:
        r.conv_shortcut = nn.Conv2d(cin, cout, 1)
    return r


class VAEEncoder(_HipBackbone):
    def __init__(self, in_channels=3, latent_channels=4, block_out_channels=(64,), layers_per_block=1, norm_num_groups=32,
                 down_block_types=None, act_fn="silu", scaling_factor=0.18215, shift_factor=None, use_quant_conv=True,
                 mid_block_add_attention=True, double_z=True):
        super().__init__()
        boc = tuple(int(c) for c in block_out_channels)
        nb = len(boc)
        kinds = ("DownEncoderBlock2D",) * nb if down_block_types is None else tuple(down_block_types)
        unsupported = dict(act_fn=(act_fn, "silu"), down_block_types=(kinds, ("DownEncoderBlock2D",) * nb),
                           mid_block_add_attention=(bool(mid_block_add_attention), True), double_z=(bool(double_z), True))
        for k, (got, want) in unsupported.items():
            if got != want:
                raise NotImplementedError(f"VAEEncoder({k}={got!r}) is outside the encoder built here (supported: {want!r})")
        if not isinstance(layers_per_block, int) or layers_per_block < 1:
            raise NotImplementedError(f"VAEEncoder(layers_per_block={layers_per_block!r}) is not supported: one int >= 1")
        if in_channels < 1 or latent_channels < 1:
            raise NotImplementedError(f"VAEEncoder(in_channels={in_channels}, latent_channels={latent_channels}) is not supported: both >= 1")
        for c in boc:
            if c < EV.CHANNEL_GRANULE or c % EV.CHANNEL_GRANULE or c % norm_num_groups:
                raise NotImplementedError(f"VAEEncoder(block_out_channels={boc}) is not supported: {c} must be a multiple of "
                                          f"{EV.CHANNEL_GRANULE} (the K granule of the 16-bit GEMMs) and of norm_num_groups={norm_num_groups}")
        if boc[-1] not in EV.MID_WIDTHS:
            raise NotImplementedError(f"VAEEncoder(block_out_channels={boc}) is not supported: the mid block attends over one head of "
                                      f"{boc[-1]} channels, served widths are {EV.MID_WIDTHS} (dc_attention / dc_attention_wide)")
        self.config = SimpleNamespace(in_channels=in_channels, latent_channels=latent_channels, block_out_channels=boc,
                                      layers_per_block=layers_per_block, norm_num_groups=norm_num_groups, down_block_types=kinds,
                                      act_fn=act_fn, scaling_factor=float(scaling_factor),
                                      shift_factor=None if shift_factor is None else float(shift_factor),
                                      use_quant_conv=bool(use_quant_conv), mid_block_add_attention=True, double_z=True)
        G = norm_num_groups
        enc = self.encoder = _Bag()
        enc.conv_in = nn.Conv2d(in_channels, boc[0], 3, padding=1)
        enc.down_blocks = nn.ModuleList()
        out = boc[0]
        for i in range(nb):
            cin, out = out, boc[i]
            blk = _Bag()
            blk.resnets = nn.ModuleList([_resnet(cin if j == 0 else out, out, G) for j in range(layers_per_block)])
            if i != nb - 1:
                ds = _Bag()
                ds.conv = nn.Conv2d(out, out, 3, stride=2, padding=0)      # behind F.pad(x, (0, 1, 0, 1)): bottom / right only
                blk.downsamplers = nn.ModuleList([ds])
            enc.down_blocks.append(blk)
        mid = enc.mid_block = _Bag()
        at = _Bag()
        at.group_norm = nn.GroupNorm(G, out, eps=EV.GN_EPS)
        at.to_q, at.to_k, at.to_v = nn.Linear(out, out), nn.Linear(out, out), nn.Linear(out, out)
        at.to_out = nn.ModuleList([nn.Linear(out, out), nn.Identity()])
        mid.attentions = nn.ModuleList([at])
        mid.resnets = nn.ModuleList([_resnet(out, out, G) for _ in range(2)])
        enc.conv_norm_out = nn.GroupNorm(G, out, eps=EV.GN_EPS)
        enc.conv_out = nn.Conv2d(out, 2 * latent_channels, 3, padding=1)
        if use_quant_conv:
            self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)
        self._init_engine()
        self.requires_grad_(False)         # frozen: an encoder of images, not a trained part

    @property
    def downscale(self):
        """Image pixels per latent pixel along each axis."""
        return 2 ** (len(self.config.block_out_channels) - 1)

    # ---- loading --------------------------------------------------------------------------------
    CONFIG_KEYS = ("in_channels", "latent_channels", "block_out_channels", "layers_per_block", "norm_num_groups", "down_block_types",
                   "act_fn", "scaling_factor", "shift_factor", "use_quant_conv", "mid_block_add_attention", "double_z")
    REQUIRED_KEYS = ("in_channels", "latent_channels", "block_out_channels", "layers_per_block")
    IGNORED = ("decoder.", "post_quant_conv.")
    LEGACY = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}
    WEIGHTS = "diffusion_pytorch_model.safetensors"

    @classmethod
    def from_directory(cls, path):
        """A local diffusers AutoencoderKL directory (config.json + diffusion_pytorch_model.safetensors).  decoder.* and
        post_quant_conv.* are ignored; the legacy attention names query / key / value / proj_attn (with their 1x1-conv weight
        shapes [C, C, 1, 1]) are mapped onto to_q / to_k / to_v / to_out.0; what is left loads strictly.  Never touches the network."""
        cfg_path, st_path = os.path.join(path, "config.json"), os.path.join(path, cls.WEIGHTS)
        for p in (cfg_path, st_path):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"{p} is missing: VAEEncoder.from_directory needs a local diffusers AutoencoderKL directory with "
                                        f"config.json and {cls.WEIGHTS} (nothing is fetched)")
        with open(cfg_path) as fh:
            raw = json.load(fh)
        missing = [k for k in cls.REQUIRED_KEYS if k not in raw]
        if missing:
            raise ValueError(f"{cfg_path} lacks {missing}")
        model = cls(**{k: raw[k] for k in cls.CONFIG_KEYS if k in raw})
        from safetensors.torch import load_file
        at = "encoder.mid_block.attentions.0."
        sd = {}
        for k, v in load_file(st_path).items():
            if k.startswith(cls.IGNORED):
                continue
            if k.startswith(at):
                name, leaf = k[len(at):].rsplit(".", 1)
                if name in cls.LEGACY:
                    k = at + cls.LEGACY[name] + "." + leaf
                if leaf == "weight" and v.dim() == 4 and v.shape[2:] == (1, 1):
                    v = v.reshape(v.shape[0], v.shape[1])
            sd[k] = v
        model.load_state_dict(sd, strict=True)
        return model

    # ---- engine ---------------------------------------------------------------------------------
    weights_class = EV.VaeWeights

    def check_image_shape(self, shape):
        f = self.downscale
        if len(shape) != 4 or shape[1] != self.config.in_channels or shape[2] < f or shape[3] < f or shape[2] % f or shape[3] % f:
            raise ValueError(f"VAEEncoder takes images [B, {self.config.in_channels}, H, W] with H and W multiples of {f}, got {tuple(shape)}")

    def make_plan(self, B, H, W, device):
        return EV.VaePlan(self, self.packed_weights(E.DT[self.compute_dtype], device), B, H, W)

    @torch.no_grad()
    def forward(self, x):
        """x [B, in_channels, H, W] (H and W multiples of 2^(levels - 1), any aspect) -> latents [B, latent_channels, H / f, W / f] fp32 on
        the device: (mean - shift_factor) * scaling_factor.  HIP tensors and the library are required: there is no CPU path."""
        self.check_image_shape(x.shape)
        if not x.is_cuda or self.encoder.conv_in.weight.device != x.device:
            raise L.DcamdError("VAEEncoder.forward needs a CUDA/HIP tensor and the module on the same device (no CPU fallback)")
        L.require_gpu()
        B, _, H, W = x.shape
        key = (B, H, W, str(x.device), self.compute_dtype)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self.make_plan(B, H, W, x.device)
        plan.x.copy_(x)
        plan.run()
        return plan.out_view().permute(0, 3, 1, 2).contiguous()


class VAEDecoder(_HipBackbone):
    """The DECODER half of the same AutoencoderKL: scaled latents (what `VAEEncoder.forward` returns) -> images,
    `AutoencoderKL.decode(z / scaling_factor + shift_factor).sample`.  Published key names (`post_quant_conv.weight`,
    `decoder.conv_in.weight`, `decoder.up_blocks.{i}.resnets.{j}.conv1.weight`, `decoder.up_blocks.{i}.upsamplers.0.conv.weight`, ...);
    arithmetic in libdcamd (engine_vae.py VaeDecoderPlan).  Out of scope: tiling and slicing, uint8 output.
    Published fp16 VAE weights are known to overflow in the decoder (upstream's `force_upcast`): run it in bf16 (the default) or f32."""

    def __init__(self, latent_channels=4, out_channels=3, block_out_channels=(64,), layers_per_block=1, norm_num_groups=32,
                 up_block_types=None, act_fn="silu", scaling_factor=0.18215, shift_factor=None, use_post_quant_conv=True,
                 mid_block_add_attention=True, in_channels=None):
        """in_channels is the encoder's and is not read: one kwargs dict (`sd_vae_kwargs()`) builds both halves."""
        super().__init__()
        boc = tuple(int(c) for c in block_out_channels)
        nb = len(boc)
        kinds = ("UpDecoderBlock2D",) * nb if up_block_types is None else tuple(up_block_types)
        unsupported = dict(act_fn=(act_fn, "silu"), up_block_types=(kinds, ("UpDecoderBlock2D",) * nb),
                           mid_block_add_attention=(bool(mid_block_add_attention), True))
        for k, (got, want) in unsupported.items():
            if got != want:
                raise NotImplementedError(f"VAEDecoder({k}={got!r}) is outside the decoder built here (supported: {want!r})")
        if not isinstance(layers_per_block, int) or layers_per_block < 1:
            raise NotImplementedError(f"VAEDecoder(layers_per_block={layers_per_block!r}) is not supported: one int >= 1")
        if out_channels < 1 or latent_channels < 1:
            raise NotImplementedError(f"VAEDecoder(out_channels={out_channels}, latent_channels={latent_channels}) is not supported: both >= 1")
        for c in boc:
            if c < EV.CHANNEL_GRANULE or c % EV.CHANNEL_GRANULE or c % norm_num_groups:
                raise NotImplementedError(f"VAEDecoder(block_out_channels={boc}) is not supported: {c} must be a multiple of "
                                          f"{EV.CHANNEL_GRANULE} (the K granule of the 16-bit GEMMs) and of norm_num_groups={norm_num_groups}")
        if boc[-1] not in EV.MID_WIDTHS:
            raise NotImplementedError(f"VAEDecoder(block_out_channels={boc}) is not supported: the mid block attends over one head of "
                                      f"{boc[-1]} channels, served widths are {EV.MID_WIDTHS} (dc_attention / dc_attention_wide)")
        self.config = SimpleNamespace(latent_channels=latent_channels, out_channels=out_channels, block_out_channels=boc,
                                      layers_per_block=layers_per_block, norm_num_groups=norm_num_groups, up_block_types=kinds,
                                      act_fn=act_fn, scaling_factor=float(scaling_factor),
                                      shift_factor=None if shift_factor is None else float(shift_factor),
                                      use_post_quant_conv=bool(use_post_quant_conv), mid_block_add_attention=True)
        G = norm_num_groups
        rev = boc[::-1]
        dec = self.decoder = _Bag()
        dec.conv_in = nn.Conv2d(latent_channels, rev[0], 3, padding=1)
        mid = dec.mid_block = _Bag()
        at = _Bag()
        at.group_norm = nn.GroupNorm(G, rev[0], eps=EV.GN_EPS)
        at.to_q, at.to_k, at.to_v = nn.Linear(rev[0], rev[0]), nn.Linear(rev[0], rev[0]), nn.Linear(rev[0], rev[0])
        at.to_out = nn.ModuleList([nn.Linear(rev[0], rev[0]), nn.Identity()])
        mid.attentions = nn.ModuleList([at])
        mid.resnets = nn.ModuleList([_resnet(rev[0], rev[0], G) for _ in range(2)])
        dec.up_blocks = nn.ModuleList()
        for i in range(nb):
            cin, out = rev[max(i - 1, 0)], rev[i]
            blk = _Bag()
            blk.resnets = nn.ModuleList([_resnet(cin if j == 0 else out, out, G) for j in range(layers_per_block + 1)])
            if i != nb - 1:
                us = _Bag()
                us.conv = nn.Conv2d(out, out, 3, padding=1)                 # behind a nearest-neighbour 2x upsample
                blk.upsamplers = nn.ModuleList([us])
            dec.up_blocks.append(blk)
        dec.conv_norm_out = nn.GroupNorm(G, rev[-1], eps=EV.GN_EPS)
        dec.conv_out = nn.Conv2d(rev[-1], out_channels, 3, padding=1)
        if use_post_quant_conv:
            self.post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1)
        self._init_engine()
        self.requires_grad_(False)

    @property
    def upscale(self):
        """Image pixels per latent pixel along each axis."""
        return 2 ** (len(self.config.block_out_channels) - 1)

    # ---- loading --------------------------------------------------------------------------------
    CONFIG_KEYS = ("latent_channels", "out_channels", "block_out_channels", "layers_per_block", "norm_num_groups", "up_block_types",
                   "act_fn", "scaling_factor", "shift_factor", "use_post_quant_conv", "mid_block_add_attention")
    REQUIRED_KEYS = ("latent_channels", "block_out_channels", "layers_per_block")
    IGNORED = ("encoder.", "quant_conv.")
    LEGACY = VAEEncoder.LEGACY
    WEIGHTS = VAEEncoder.WEIGHTS

    @classmethod
    def from_directory(cls, path):
        """The directory `VAEEncoder.from_directory` reads.  encoder.* and quant_conv.* are ignored; the legacy attention names are mapped
        as there; what is left loads strictly, and a file without the decoder's weights is refused by the name of the first key it
        lacks.  Never touches the network."""
        cfg_path, st_path = os.path.join(path, "config.json"), os.path.join(path, cls.WEIGHTS)
        for p in (cfg_path, st_path):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"{p} is missing: VAEDecoder.from_directory needs a local diffusers AutoencoderKL directory with "
                                        f"config.json and {cls.WEIGHTS} (nothing is fetched)")
        with open(cfg_path) as fh:
            raw = json.load(fh)
        missing = [k for k in cls.REQUIRED_KEYS if k not in raw]
        if missing:
            raise ValueError(f"{cfg_path} lacks {missing}")
        model = cls(**{k: raw[k] for k in cls.CONFIG_KEYS if k in raw})
        from safetensors.torch import load_file
        at = "decoder.mid_block.attentions.0."
        sd = {}
        for k, v in load_file(st_path).items():
            if k.startswith(cls.IGNORED):
                continue
            if k.startswith(at):
                name, leaf = k[len(at):].rsplit(".", 1)
                if name in cls.LEGACY:
                    k = at + cls.LEGACY[name] + "." + leaf
                if leaf == "weight" and v.dim() == 4 and v.shape[2:] == (1, 1):
                    v = v.reshape(v.shape[0], v.shape[1])
            sd[k] = v
        for k in model.state_dict():
            if k not in sd:
                raise RuntimeError(f"{st_path} holds no {k}: the AutoencoderKL under {path} has no (complete) decoder")
        model.load_state_dict(sd, strict=True)
        return model

    # ---- engine ---------------------------------------------------------------------------------
    weights_class = EV.VaeDecoderWeights

    def check_latent_shape(self, shape):
        if len(shape) != 4 or shape[0] < 1 or shape[1] != self.config.latent_channels or shape[2] < 1 or shape[3] < 1:
            raise ValueError(f"VAEDecoder takes latents [B, {self.config.latent_channels}, h, w] with h, w >= 1, got {tuple(shape)}")

    def make_plan(self, B, h, w, device):
        return EV.VaeDecoderPlan(self, self.packed_weights(E.DT[self.compute_dtype], device), B, h, w)

    @torch.no_grad()
    def forward(self, z):
        """z [B, latent_channels, h, w], scaled latents (any aspect) -> images [B, out_channels, f h, f w] fp32 on the device, unclamped.
        HIP tensors and the library are required: there is no CPU path."""
        self.check_latent_shape(z.shape)
        if not z.is_cuda or self.decoder.conv_in.weight.device != z.device:
            raise L.DcamdError("VAEDecoder.forward needs a CUDA/HIP tensor and the module on the same device (no CPU fallback)")
        L.require_gpu()
        B, _, h, w = z.shape
        key = (B, h, w, str(z.device), self.compute_dtype)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self.make_plan(B, h, w, z.device)
        plan.z.copy_(z)
        plan.run()
        # always a copy: with out_channels = 1 the permuted view already counts as contiguous, and `.contiguous()` would hand out the
        # plan's own buffer, which the next run overwrites
        return plan.out_view().permute(0, 3, 1, 2).clone(memory_format=torch.contiguous_format)
