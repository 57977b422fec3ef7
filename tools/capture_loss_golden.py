#!/usr/bin/env python3
"""Capture golden values of the REFERENCE's own `DiffusionClassifier.loss` (reference diffusion/diffusion_classifier.py:295-344) on the
stand-in backbone of tests/standin.py, with the stubs tools/capture_goldens.py uses (its recipe: SURVEY.md Appendix B).  Needs a checkout
of the reference: its directory is the first argument, or $REFERENCE_ROOT.  Output: tests/golden/loss_cases.npz — data only (inputs, the
stand-in's weights, the draws in call order, the expected loss); no reference source is copied.

One case per prediction parameterisation, so both forms of the truncated-SNR weight are recorded; the seeds are fixed and the injected
t are spread over [0, 1] by the generator, so draws on both sides of the clamp at snr = 5 occur (checked below).
"""
import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import accelerate  # noqa: F401  (must precede the stubs, see Appendix B step 1)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
if not REFERENCE or not os.path.isdir(REFERENCE):
    sys.exit("usage: capture_loss_golden.py REFERENCE_ROOT (or set $REFERENCE_ROOT): a checkout of the reference project")

comet = types.ModuleType("comet_ml")
comet.Experiment = type("Experiment", (), {})
comet.ExistingExperiment = type("ExistingExperiment", (), {})
sys.modules["comet_ml"] = comet


class _EMA(nn.Module):
    def __init__(self, model, beta=None, update_after_step=None, update_every=None):
        super().__init__()
        self.ema_model = copy.deepcopy(model)

    def forward(self, *a, **k):
        return self.ema_model(*a, **k)


ema = types.ModuleType("ema_pytorch")
ema.EMA = _EMA
sys.modules["ema_pytorch"] = ema

sys.path.insert(0, REFERENCE)
from diffusion.diffusion_classifier import DiffusionClassifier  # noqa: E402  (the reference)
from standin import TinyBackbone  # noqa: E402


class Bag:
    def __init__(self, **kw):
        self.__dict__["d"] = kw

    def __getattr__(self, k):
        return self.__dict__["d"].get(k)


OUT = os.path.join(ROOT, "tests", "golden", "loss_cases.npz")
CFG = dict(schedule="cosine", noise_d=32, image_size=32, cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, encoder_type="nn",
           classes=4, n_stages=1, evaluation_per_stage=[6], n_keep_per_stage=[1], n_fast_classes=2)


def capture(tag, pred_param, seed, BS=4, ch=3, hw=6, hid=8):
    torch.manual_seed(100 + seed)
    bb = TinyBackbone(ch=ch, hid=hid, n_classes=CFG["classes"], mode="nn")
    dc = DiffusionClassifier(bb, Bag(pred_param=pred_param, **CFG))
    x = torch.rand(BS, ch, hw, hw) * 2 - 1
    labels = torch.randint(0, CFG["classes"], (BS,))
    rec = []                                             # the draws in call order: ("rand", t), ("randn_like", eps)
    o_rand, o_randn_like = torch.rand, torch.randn_like

    def rand(*a, **k):
        r = o_rand(*a, **k); rec.append(("rand", r.clone())); return r

    def randn_like(*a, **k):
        r = o_randn_like(*a, **k); rec.append(("randn_like", r.clone())); return r

    torch.manual_seed(seed)
    torch.rand, torch.randn_like = rand, randn_like
    try:
        with torch.no_grad():
            out = dc.loss(x, labels)
    finally:
        torch.rand, torch.randn_like = o_rand, o_randn_like
    assert [k for k, _ in rec] == ["rand", "randn_like"], [k for k, _ in rec]
    t, eps = rec[0][1], rec[1][1]
    snr = torch.exp(dc.schedule(t))
    assert bool((snr > 5).any()) and bool((snr < 5).any()), snr           # both sides of the clamp
    arrs = {tag + ".x": x.numpy(), tag + ".labels": labels.numpy(), tag + ".t": t.numpy(), tag + ".eps": eps.numpy(),
            tag + ".loss": out.numpy(), tag + ".seed": np.int64(seed), tag + ".pred_param": np.array(pred_param),
            tag + ".encoder.weight": dc.encoder.weight.detach().numpy()}
    for k, v in bb.state_dict().items():
        arrs[f"{tag}.bb.{k}"] = v.numpy()
    print("loss", tag, pred_param, "seed", seed, "->", float(out), "dtype", out.dtype, "snr", [round(float(s), 3) for s in snr])
    return arrs


if __name__ == "__main__":
    arrs = {}
    for k, v in CFG.items():
        arrs["cfg." + k] = np.array(v)
    arrs.update(capture("eps", "eps", 41))
    arrs.update(capture("v", "v", 43))
    np.savez_compressed(OUT, **arrs)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
