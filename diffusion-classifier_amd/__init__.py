"""diffusion-classifier_amd — MI355X (gfx950) native scoring path of faverogian/diffusion-classifier.

Import as `diffusion_classifier_amd` (the repo-root shim maps that name onto this directory,
whose on-disk name carries the reference's hyphen).  Layout mirrors the reference so that
    from nets.unet import UNetCondition2D            ->  from diffusion_classifier_amd.nets.unet import UNetCondition2D
    from nets.dit import DiT                         ->  from diffusion_classifier_amd.nets.dit import DiT
    from diffusion.diffusion_classifier import DiffusionClassifier
                                                     ->  from diffusion_classifier_amd.diffusion.diffusion_classifier import DiffusionClassifier
    from utils.wavelet import wavelet_dec_2          ->  from diffusion_classifier_amd.utils.wavelet import wavelet_dec_2
All arithmetic of the scoring path runs in `libdcamd.so` (HIP kernels + C-ABI, csrc/, include/dcamd.h).
"""
from . import _lib  # noqa: F401
from .nets.unet import UNetCondition2D, UNet2D  # noqa: F401
from .nets.sd_unet import StableDiffusionUNet, StableDiffusionXLUNet  # noqa: F401
from .nets.dit import DiT  # noqa: F401
from .nets.vae import VAEEncoder, VAEDecoder  # noqa: F401
from .diffusion.diffusion_classifier import DiffusionClassifier  # noqa: F401
from .utils.wavelet import wavelet_dec_2, wavelet_enc_2  # noqa: F401
from .posterior import ClassPosterior  # noqa: F401
from .evidence import ClassEvidence  # noqa: F401
from .counterfactual import Counterfactuals  # noqa: F401
from .ddpm_invert import DdpmInversion  # noqa: F401


class Config:
    """Attribute bag whose missing keys read as None (reference experiments/cifar10/inference.py:24-38)."""

    def __init__(self, **kw):
        self.__dict__["_d"] = dict(kw)

    def __getattr__(self, k):
        return self.__dict__["_d"].get(k)

    def __setattr__(self, k, v):
        self.__dict__["_d"][k] = v


# architectures BASELINE.json names (reference file:line in each comment)
def cifar10_unet_kwargs():
    # experiments/cifar10/inference.py:94-116
    return dict(sample_size=32, in_channels=3, out_channels=3, layers_per_block=2, block_out_channels=(128, 128, 256, 512),
                down_block_types=("DownBlock2D", "DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D", "UpBlock2D"),
                mid_block_type="UNetMidBlock2DCrossAttn", encoder_hid_dim=128, encoder_hid_dim_type="text_proj",
                cross_attention_dim=128)


def small_unet_kwargs():
    # BASELINE config 1 "small": not defined by the reference; channel counts are multiples of 64 so
    # the bf16 MFMA path (K granule 64) accepts it as well as the f32 one.
    return dict(sample_size=32, in_channels=3, out_channels=3, layers_per_block=1, block_out_channels=(64, 128),
                down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"),
                mid_block_type="UNetMidBlock2DCrossAttn", encoder_hid_dim=64, encoder_hid_dim_type="text_proj",
                cross_attention_dim=64)


def chexpert_dwt_unet_kwargs():
    # models/chexpert-256-unet-dwt-healthysick.py:4-28
    return dict(sample_size=128, in_channels=12, out_channels=12, layers_per_block=2,
                block_out_channels=(128, 128, 256, 512, 1024),
                down_block_types=("DownBlock2D", "DownBlock2D", "DownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
                up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D", "UpBlock2D", "UpBlock2D"),
                mid_block_type="UNetMidBlock2DCrossAttn", encoder_hid_dim=512, encoder_hid_dim_type="text_proj",
                cross_attention_dim=512)


def ipmsa5_unet_kwargs():
    # models/ipmsa-5-unet.py:4-30
    return dict(sample_size=256, in_channels=10, out_channels=10, layers_per_block=(2, 2, 2, 2, 4, 2),
                block_out_channels=(128, 128, 256, 512, 512, 1024),
                down_block_types=("DownBlock2D",) * 4 + ("CrossAttnDownBlock2D",) * 2,
                up_block_types=("CrossAttnUpBlock2D",) * 2 + ("UpBlock2D",) * 4,
                mid_block_type="UNetMidBlock2DCrossAttn", encoder_hid_dim=512, encoder_hid_dim_type="text_proj",
                cross_attention_dim=512)


# The reference's other UNet backbones: 768-channel levels (attention head dim 96 with 8 heads), GroupNorm groups of 24 / 40 / 48
# channels, odd input / output channel counts.  image_channels / image_size come from experiment configs the reference does not
# ship: the DWT form (4 x image_channels at image_size / 2) is restated here.
def ipmsa5_dwt_unet_kwargs():
    # models/ipmsa-5-dwt-unet.py:4-27
    return dict(sample_size=128, in_channels=40, out_channels=40, layers_per_block=(2, 2, 2, 4, 2),
                block_out_channels=(128, 128, 256, 512, 768),
                down_block_types=("DownBlock2D", "DownBlock2D", "DownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
                up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D", "UpBlock2D", "UpBlock2D"),
                mid_block_type="UNetMidBlock2DCrossAttn", encoder_hid_dim=512, encoder_hid_dim_type="text_proj",
                cross_attention_dim=512)


def unet128_kwargs(image_channels=3, image_size=256, wavelet_transform=True):
    # models/unet-128.py:4-27
    ch, size = (4 * image_channels, image_size // 2) if wavelet_transform else (image_channels, image_size)
    return dict(sample_size=size, in_channels=ch, out_channels=ch, layers_per_block=2,
                block_out_channels=(128, 128, 256, 512, 1024),
                down_block_types=("DownBlock2D", "DownBlock2D", "DownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
                up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D", "UpBlock2D", "UpBlock2D"),
                mid_block_type="UNetMidBlock2DCrossAttn", encoder_hid_dim=512, encoder_hid_dim_type="text_proj",
                cross_attention_dim=512)


def unet256_kwargs(image_channels=3, image_size=256, wavelet_transform=True):
    # models/unet-256.py:4-29
    ch, size = (4 * image_channels, image_size // 2) if wavelet_transform else (image_channels, image_size)
    return dict(sample_size=size, in_channels=ch, out_channels=ch, layers_per_block=2,
                block_out_channels=(128, 128, 256, 256, 512, 1024),
                down_block_types=("DownBlock2D",) * 4 + ("CrossAttnDownBlock2D", "DownBlock2D"),
                up_block_types=("UpBlock2D", "CrossAttnUpBlock2D") + ("UpBlock2D",) * 4,
                mid_block_type="UNetMidBlock2DCrossAttn", encoder_hid_dim=512, encoder_hid_dim_type="text_proj",
                cross_attention_dim=512)


def chexpert_experiment_unet_kwargs(image_channels=1, image_size=256, wavelet_transform=True):
    # experiments/chexpert-unet/inference.py:118-138
    ch, size = (4 * image_channels, image_size // 2) if wavelet_transform else (image_channels, image_size)
    return dict(sample_size=size, in_channels=ch, out_channels=ch, layers_per_block=2, block_out_channels=(256, 512, 768),
                down_block_types=("DownBlock2D", "DownBlock2D", "CrossAttnDownBlock2D"),
                up_block_types=("CrossAttnUpBlock2D", "UpBlock2D", "UpBlock2D"),
                mid_block_type="UNetMidBlock2DCrossAttn", encoder_hid_dim=256, encoder_hid_dim_type="text_proj",
                cross_attention_dim=256)


def ipmsa_experiment_unet_kwargs(image_channels=10, image_size=256, wavelet_transform=True):
    # experiments/ipmsa/inference.py:187-211
    ch, size = (4 * image_channels, image_size // 2) if wavelet_transform else (image_channels, image_size)
    return dict(sample_size=size, in_channels=ch, out_channels=ch, layers_per_block=(2, 2, 4, 4, 4),
                block_out_channels=(128, 256, 256, 512, 768),
                down_block_types=("DownBlock2D",) * 3 + ("CrossAttnDownBlock2D",) * 2,
                up_block_types=("CrossAttnUpBlock2D",) * 2 + ("UpBlock2D",) * 3,
                mid_block_type="UNetMidBlock2DCrossAttn", encoder_hid_dim=256, encoder_hid_dim_type="text_proj",
                cross_attention_dim=256)


def sd_vae_kwargs():
    # the published Stable Diffusion AutoencoderKL (sd-vae-ft-mse / -ema, the `vae/` of SD 1.x), 8x downsampling; VAEEncoder and VAEDecoder both take it
    return dict(in_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512), layers_per_block=2, norm_num_groups=32,
                scaling_factor=0.18215)


def sd15_unet_kwargs():
    # the published Stable Diffusion 1.x UNet (the `unet/config.json` of v1-4 / v1-5): 64x64 latents, 8 heads at every level (head widths
    # 40 / 80 / 160 / 160), the CLIP ViT-L/14 context of 768 channels, 1x1-conv projections; StableDiffusionUNet takes it
    return dict(sample_size=64, in_channels=4, out_channels=4, layers_per_block=2, block_out_channels=(320, 640, 1280, 1280),
                down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
                up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
                mid_block_type="UNetMidBlock2DCrossAttn", norm_num_groups=32, cross_attention_dim=768, attention_head_dim=8,
                use_linear_projection=False)


def sd21_unet_kwargs():
    # the published Stable Diffusion 2.1 UNet (2.1-base: 64x64 latents; the 768-pixel model differs in sample_size = 96 alone): heads
    # (5, 10, 20, 20), i.e. 64 channels per head everywhere, the OpenCLIP ViT-H context of 1024 channels, linear projections
    return dict(sd15_unet_kwargs(), cross_attention_dim=1024, attention_head_dim=(5, 10, 20, 20), use_linear_projection=True)


def sdxl_unet_kwargs():
    # the published Stable Diffusion XL base UNet (`unet/config.json` of stable-diffusion-xl-base-1.0): 128x128 latents, three levels,
    # 1 / 2 / 10 transformer blocks per site (none at the first level), 64 channels per head everywhere, the 768 + 1280 context of its two
    # CLIP text encoders, linear projections, the text_time embedding over a 1280-wide pooled row and six size numbers at 256 each;
    # StableDiffusionXLUNet takes it
    return dict(sample_size=128, in_channels=4, out_channels=4, layers_per_block=2, block_out_channels=(320, 640, 1280),
                down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"),
                mid_block_type="UNetMidBlock2DCrossAttn", norm_num_groups=32, cross_attention_dim=2048, attention_head_dim=(5, 10, 20),
                transformer_layers_per_block=(1, 2, 10), use_linear_projection=True, addition_embed_type="text_time",
                addition_time_embed_dim=256, projection_class_embeddings_input_dim=2816)


def chexpert_dit_b4_kwargs(wavelet_transform=True):
    # models/chexpert-256-dit-b4.py:4-21 (image_size 256, 3 channels, patch 4)
    ch, size = (12, 128) if wavelet_transform else (3, 256)
    return dict(num_attention_heads=12, attention_head_dim=64, in_channels=ch, out_channels=ch, num_layers=12,
                sample_size=size, patch_size=4, num_embeds_ada_norm=1000, norm_eps=1e-5)
