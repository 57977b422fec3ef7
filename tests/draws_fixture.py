"""`DiffusionClassifier._trial_draws` under the two cosine schedules, as tests/golden/cosine_trial_draws.json records it (the fp32
bytes of logsnr / alpha / sigma as hex).  The fixture was written by `record()` on the commit before the 'scaled_linear' schedule
existed; tests/test_sd_unet_host.py recomputes the draws and compares the bytes.  Host only."""
import contextlib
import io
import json
import os

import torch

import diffusion_classifier_amd as dca

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cosine_trial_draws.json")
T, BS = 5, 3


def classifier(schedule, **over):
    cfg = dict(pred_param="eps", schedule=schedule, noise_d=32, image_size=64, cfg_w=0.0, ema_beta=0.999, ema_warmup=0,
               ema_update_freq=1, encoder_type="nn", classes=3, n_stages=1, evaluation_per_stage=[T], n_keep_per_stage=[1],
               n_fast_classes=2, compute_dtype="f32")
    cfg.update(over)
    with contextlib.redirect_stdout(io.StringIO()):
        return dca.DiffusionClassifier(dca.UNetCondition2D(**dca.small_unet_kwargs()), dca.Config(**cfg))


def _hex(t):
    return t.detach().to(torch.float32).contiguous().numpy().tobytes().hex()


def draws():
    out = {}
    x = torch.zeros(BS, 3, 4, 4)
    t = torch.cat([torch.tensor([0.0, 1.0, 0.5]), torch.linspace(0.001, 0.999, T * BS - 3)]).reshape(T, BS)
    for schedule in ("cosine", "shifted_cosine"):
        dc = classifier(schedule)
        d = dc._trial_draws(x, T, t, torch.zeros(T, BS, 3, 4, 4), "reference", 0)
        out[schedule + "/given_t"] = {k: _hex(d[k]) for k in ("logsnr", "alpha", "sigma")}
        torch.manual_seed(11)
        d = dc._trial_draws(x, T, None, None, "reference", 0)
        out[schedule + "/reference_rng"] = {k: _hex(d[k]) for k in ("logsnr", "alpha", "sigma")}
        torch.manual_seed(11)
        d = dc._trial_draws(x, T, None, None, "philox", 3)
        out[schedule + "/philox"] = {k: _hex(d[k]) for k in ("logsnr", "alpha", "sigma")}
    return out


def record(path):
    with open(path, "w") as f:
        json.dump(draws(), f, indent=0, sort_keys=True)
        f.write("\n")
