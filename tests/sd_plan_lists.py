"""The launch lists of a few StableDiffusionUNet plans, as the fixture tests/golden/sd_unet_plan_lists.json records them: per plan the
(name, family, variant) of every op of the context plan and of the main plan, in order (tests/plan_lists.py does the same for
UNetCondition2D).  The fixture was written by `record()` on the commit before StableDiffusionXLUNet existed, when a transformer site
held exactly one block and the ResNet time vector was class-independent; tests/test_gpu_sdxl.py rebuilds the lists and compares.
Building a plan packs weights on the device, so this needs a GPU."""
import json
import os

import torch

from diffusion_classifier_amd.nets.sd_unet import StableDiffusionUNet

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sd_unet_plan_lists.json")

MINI = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=(128, 320), layers_per_block=1, norm_num_groups=32,
            down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
            cross_attention_dim=64, attention_head_dim=2)
MINI_LINEAR = dict(MINI, sample_size=8, cross_attention_dim=128, attention_head_dim=(2, 5), use_linear_projection=True)

# name -> (constructor keywords, compute dtype, n_bj, n_cls, tokens per context, varlen)
CASES = {
    "mini_f32_prompt": (MINI, "f32", 2, 3, 5, False),
    "mini_bf16_prompt_varlen": (MINI, "bf16", 2, 3, 7, True),
    "mini_bf16_token": (MINI, "bf16", 2, 3, 1, False),
    "linear_bf16_prompt": (MINI_LINEAR, "bf16", 3, 2, 6, False),
    "linear_f16_prompt_varlen": (MINI_LINEAR, "f16", 2, 3, 5, True),
}


def _ops(pb):
    return [[m["name"], m["family"], m.get("variant", "")] for m in pb.meta]


def plan_lists(device="cuda:0"):
    out = {}
    for name, (kw, dt, n_bj, n_cls, S, varlen) in CASES.items():
        torch.manual_seed(0)
        m = StableDiffusionUNet(**kw).set_compute_dtype(dt)
        plan = m.make_plan(n_bj, n_cls, n_cls, torch.device(device), S=S, varlen=varlen)
        out[name] = dict(ctx=_ops(plan.ctx_pb), main=_ops(plan.pb))
    return out


def record(path):
    with open(path, "w") as f:
        json.dump(plan_lists(), f, indent=0, sort_keys=True)
        f.write("\n")
