"""Measures the deterministic samplers on the GPU, on the configuration tools/bench_counterfactual.py times: the CheXpert DWT UNet
(12 x 128 x 128, random weights, v-prediction, cfg_w = 2), 8 images, K = 2 classes, from_t = 0.5, bf16 by default.

    python tools/bench_solver.py [--dtype bf16] [--images 8] [--classes 2] [--steps 8] [--reps 7] [--warmup 2] [--timeout 900]

Two records, one JSON line on stdout, nothing gates on it:
  timing          `counterfactual(x, classes, from_t)` with the ancestral sampler at `steps` sampling steps (steps + 1 backbone passes: the
                  default path) against config.sampler = "dpmpp_2m" at steps / 4 (steps / 4 passes), the same initial draw, alternating,
                  HIP events around the whole call, medians of `reps`; and the max-abs / mean-abs difference of the two calls' maps
  reconstruction  `counterfactual(x, [c], from_t, start="invert", invert_class=c)` with cfg_w = 0 in f32: the image inverted and decoded
                  under the same class, max-abs and mean-abs of sample - x for sampling_steps in {16, 64}.  The weights are random:
                  the numbers say how the first-order inversion error shrinks with the step count, not how a trained model behaves.
The measurement runs in a child process under its own time limit (the parent never opens the GPU).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import diffusion_classifier_amd as dca
    from diffusion_classifier_amd import _lib as L
    L.require_gpu()
    dev = "cuda:0"
    torch.manual_seed(0)
    kw = dca.chexpert_dwt_unet_kwargs()
    size = kw["sample_size"]
    cfg = dict(pred_param="v", schedule="cosine", noise_d=size, image_size=size, cfg_w=2.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1,
               encoder_type="nn", classes=a.classes, n_stages=1, evaluation_per_stage=[1], n_keep_per_stage=[1], n_fast_classes=2,
               compute_dtype=a.dtype, sampling_steps=a.steps)
    dc = dca.DiffusionClassifier(dca.UNetCondition2D(**kw), dca.Config(**cfg)).to(dev)
    dc.ema.ema_model.set_compute_dtype(a.dtype)
    x = (torch.rand(a.images, kw["in_channels"], size, size, device=dev) * 2 - 1) * 0.5
    cl = torch.arange(a.classes).repeat(a.images, 1)

    def call(sampler, steps):
        dc.config.sampler, dc.config.sampling_steps = sampler, steps
        torch.manual_seed(1)
        return dc.counterfactual(x, cl, a.from_t)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    forms = {"ddpm": (None, a.steps), "dpmpp_2m": ("dpmpp_2m", a.steps // 4)}
    for _ in range(a.warmup):
        outs = {k: call(*v) for k, v in forms.items()}
    torch.cuda.synchronize()
    dm = (outs["ddpm"].maps - outs["dpmpp_2m"].maps).abs()
    ms = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, v in forms.items():
            ms[k].append(timed(lambda: call(*v))[0])
    med = {k: statistics.median(v) for k, v in ms.items()}

    # reconstruction: invert and decode under the same class, no guidance, f32
    dc.ema.ema_model.set_compute_dtype("f32")
    dc.cfg_w = 0.0
    c0 = torch.zeros(a.images, dtype=torch.int64)
    rec = {}
    for sampler in ("ddim", "dpmpp_2m"):
        for n in (16, 64):
            dc.config.sampler, dc.config.sampling_steps = sampler, n
            out = dc.counterfactual(x, c0.view(-1, 1), a.from_t, start="invert", invert_class=c0)
            d = (out.samples[:, 0] - x).abs()
            rec[f"{sampler}_{n}"] = dict(max_abs=float(d.max()), mean_abs=float(d.mean()))
    dc.check_device_errors()
    print(json.dumps(dict(workload="chexpert256-dwt-unet counterfactual, ancestral vs dpmpp_2m", dtype=a.dtype, images=a.images, classes=a.classes,
                          from_t=a.from_t, reps=a.reps, warmup=a.warmup, ddpm_sampling_steps=a.steps, ddpm_backbone_passes=a.steps + 1,
                          dpmpp_2m_sampling_steps=a.steps // 4, dpmpp_2m_backbone_passes=a.steps // 4,
                          ddpm_call_ms=[round(v, 2) for v in sorted(ms["ddpm"])], dpmpp_2m_call_ms=[round(v, 2) for v in sorted(ms["dpmpp_2m"])],
                          ddpm_call_ms_median=round(med["ddpm"], 2), dpmpp_2m_call_ms_median=round(med["dpmpp_2m"], 2),
                          speedup=round(med["ddpm"] / med["dpmpp_2m"], 3),
                          maps_max_abs_difference=float(dm.max()), maps_mean_abs_difference=float(dm.mean()),
                          maps_mean_abs_ddpm=float(outs["ddpm"].maps.abs().mean()),
                          reconstruction_f32_w0=rec)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--steps", type=int, default=8, help="sampling steps of the ancestral sampler; dpmpp_2m runs a quarter of them")
    ap.add_argument("--from-t", dest="from_t", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the measuring child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5 (the figure is a median)")
    if a.steps < 4 or a.steps % 4:
        ap.error("--steps must be a positive multiple of 4")
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(f"bench_solver: the measurement did not finish within {a.timeout} s", file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
