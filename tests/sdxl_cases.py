"""What tests/test_sdxl_host.py and tests/test_gpu_sdxl.py share: the tiny geometries, the golden of the projected CLIP, and the writers
of local directories (a diffusers `unet/`, Hugging Face `text_encoder/` and `text_encoder_2/`, a `scheduler/`)."""
import contextlib
import io
import json
import os

import numpy as np
import torch
from safetensors.torch import save_file

import diffusion_classifier_amd as dca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# two levels, depth (1, 2): the first level has no attention, so the four sites (down 1, mid, up 0 x 2) all hold two blocks
TINY = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=(64, 128),
            down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"),
            layers_per_block=1, transformer_layers_per_block=(1, 2), attention_head_dim=(2, 4), cross_attention_dim=128,
            use_linear_projection=True, addition_embed_type="text_time", addition_time_embed_dim=32,
            projection_class_embeddings_input_dim=256, norm_num_groups=32)
# three levels, the depth as an int, two layers per block: the int form, the reversed read of the up path (heads (2, 2, 4): a wrong
# order changes the head counts and with them the output) and the proj_out fold on the last block only
TINY3 = dict(TINY, block_out_channels=(64, 64, 128), layers_per_block=2, transformer_layers_per_block=2,
             down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
             up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"), attention_head_dim=(2, 2, 4))
S, CLASSES, POOLED = 8, 3, 64
CFG = dict(pred_param="eps", schedule="scaled_linear", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, classes=CLASSES,
           n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32", prompt_tokens=S)
_G = {}


def relerr(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def golden():
    """(npz, config dict, state dict under the published names) of tests/golden/clip_proj_tiny.npz."""
    if not _G:
        g = np.load(os.path.join(ROOT, "tests", "golden", "clip_proj_tiny.npz"))
        _G.update(g=g, cfg=json.loads(str(g["config"])), sd={k[3:]: torch.from_numpy(g[k]).float() for k in g.files if k.startswith("sd.")})
    return _G["g"], _G["cfg"], _G["sd"]


def randomise(m, seed):
    """Random weights with no zero or default-initialised layer: norm affines and biases moved off (1, 0)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
    return m


def write_clip(path, cfg, sd, weights="model.safetensors"):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(dict(cfg, model_type="clip_text_model"), fh)
    save_file({k: v.clone().contiguous() for k, v in sd.items()}, os.path.join(path, weights))
    return str(path)


def write_unet(path, kw, sd, weights="diffusion_pytorch_model.safetensors", **extra_cfg):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(dict(kw, _class_name="UNet2DConditionModel", _diffusers_version="0.31.0", **extra_cfg), fh)
    save_file({k: v.detach().clone().contiguous() for k, v in sd.items()}, os.path.join(path, weights))
    return str(path)


def clip_pair(seed=5):
    """Two tiny CLIP text models of hidden 64 (the golden's configuration): (cfg1, sd1) without and (cfg2, sd2) with a projection, the
    second under the legacy eos_token_id = 2.  Encoder 1 takes the golden's weights, encoder 2 a perturbed copy."""
    _, cfg, sd = golden()
    g = torch.Generator().manual_seed(seed)
    cfg1 = {k: v for k, v in cfg.items() if k not in ("projection_dim", "eos_token_id")}
    sd1 = {k: v for k, v in sd.items() if k != "text_projection.weight"}
    sd2 = {k: (v + 0.05 * torch.randn(v.shape, generator=g)).half().float() for k, v in sd.items()}
    return (cfg1, sd1), (dict(cfg, hidden_act="gelu"), sd2)


def write_tree(root, unet_kw, unet_sd, fp16_names=False):
    """A tiny Stable Diffusion XL shaped tree: unet/, text_encoder/, text_encoder_2/, scheduler/."""
    (cfg1, sd1), (cfg2, sd2) = clip_pair()
    if fp16_names:          # the files most people have: half precision under the variant's names
        unet_sd, sd2 = {k: v.half() for k, v in unet_sd.items()}, {k: v.half() for k, v in sd2.items()}
    write_unet(os.path.join(root, "unet"), unet_kw, unet_sd,
               "diffusion_pytorch_model.fp16.safetensors" if fp16_names else "diffusion_pytorch_model.safetensors")
    write_clip(os.path.join(root, "text_encoder"), cfg1, sd1)
    write_clip(os.path.join(root, "text_encoder_2"), cfg2, sd2, "model.fp16.safetensors" if fp16_names else "model.safetensors")
    os.makedirs(os.path.join(root, "scheduler"), exist_ok=True)
    with open(os.path.join(root, "scheduler", "scheduler_config.json"), "w") as fh:
        json.dump(dict(_class_name="EulerDiscreteScheduler", beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012,
                       num_train_timesteps=1000, prediction_type="epsilon"), fh)
    return str(root)


def classifier(backbone, root, **over):
    kw = dict(CFG, encoder_type="clip_dual", clip_path=os.path.join(root, "text_encoder"), clip2_path=os.path.join(root, "text_encoder_2"),
              noise_d=16, image_size=16)
    kw.update(over)
    with contextlib.redirect_stdout(io.StringIO()):
        return dca.DiffusionClassifier(backbone, dca.Config(**kw))


def prompt_ids(lengths, seed=3):
    """Token ids for both tiny encoders, [rows, S]: the same token count per row; encoder 2's EOS is the largest id (the argmax rule);
    the pad ids differ between the two, as SDXL's tokenizers' do."""
    _, cfg, _ = golden()
    g = torch.Generator().manual_seed(seed)
    rows, V = len(lengths), cfg["vocab_size"]
    lens = torch.tensor(lengths)
    mask = (torch.arange(S)[None, :] < lens[:, None]).long()
    ids1 = torch.randint(3, V - 1, (rows, S), generator=g)
    ids2 = torch.randint(3, V - 1, (rows, S), generator=g)
    for b, n in enumerate(lengths):
        ids1[b, n - 1] = ids2[b, n - 1] = V - 1
    return ids1 * mask + (1 - mask) * (V - 1), ids2 * mask, mask
