"""The launch lists of a few UNetCondition2D plans, as the fixture tests/golden/unet_plan_lists.json records them: per plan the
(name, family, variant) of every op of the context plan and of the main plan, in order.  The fixture was written by `record()`
on the commit before StableDiffusionUNet existed; tests/test_gpu_sd_unet.py rebuilds the lists and compares.  Building a plan packs
weights on the device, so this needs a GPU."""
import json
import os

import torch

import diffusion_classifier_amd as dca

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_plan_lists.json")

# name -> (kwargs function, compute dtype, n_bj, n_cls, tokens per context, varlen)
CASES = {
    "small_f32_cls": ("small_unet_kwargs", "f32", 2, 3, 1, False),
    "small_bf16_cls": ("small_unet_kwargs", "bf16", 2, 3, 1, False),
    "small_bf16_prompt": ("small_unet_kwargs", "bf16", 2, 3, 5, False),
    "small_f16_prompt_varlen": ("small_unet_kwargs", "f16", 2, 3, 5, True),
    "cifar10_bf16_cls": ("cifar10_unet_kwargs", "bf16", 16, 10, 1, False),      # the benchmark's headline shape: 16 pairs x 10 classes
    "cifar10_f32_cls": ("cifar10_unet_kwargs", "f32", 4, 10, 1, False),
    "cifar10_bf16_prompt": ("cifar10_unet_kwargs", "bf16", 4, 10, 7, False),
}


def _ops(pb):
    return [[m["name"], m["family"], m.get("variant", "")] for m in pb.meta]


def plan_lists(device="cuda:0"):
    out = {}
    for name, (fn, dt, n_bj, n_cls, S, varlen) in CASES.items():
        torch.manual_seed(0)
        m = dca.UNetCondition2D(**getattr(dca, fn)()).set_compute_dtype(dt)
        plan = m.make_plan(n_bj, n_cls, n_cls, torch.device(device), S=S, varlen=varlen)
        out[name] = dict(ctx=_ops(plan.ctx_pb), main=_ops(plan.pb))
    return out


def record(path):
    with open(path, "w") as f:
        json.dump(plan_lists(), f, indent=0, sort_keys=True)
        f.write("\n")
