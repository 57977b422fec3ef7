"""Times counterfactual sampling on the GPU: the CheXpert DWT UNet (12 x 128 x 128, random weights), 8 images, K = 2 classes, 8 sampling
steps, from_t = 0.5, bf16 by default — `DiffusionClassifier.counterfactual` against the same work done as K calls of `sample` with the
seed reset in front of each, in the same process.

    python tools/bench_counterfactual.py [--dtype bf16] [--images 8] [--classes 2] [--steps 8] [--reps 7] [--warmup 2] [--timeout 600]

The measurement runs in a child process under its own time limit (the parent never opens the GPU).  The child warms both forms up,
then times them alternately, `reps` times each, with HIP events on the launch stream around the whole call, and reports the median of
each in milliseconds per sampling step (a call makes steps + 1 backbone passes: the last one keeps the mean).  One JSON line on stdout.
Nothing gates on it.
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
    dc.ema.ema_model.set_compute_dtype(a.dtype)            # `sample` and `counterfactual` run the backbone in the dtype it holds
    x = (torch.rand(a.images, kw["in_channels"], size, size, device=dev) * 2 - 1) * 0.5
    cl = torch.arange(a.classes).repeat(a.images, 1)
    labs = [cl[:, k].to(dev) for k in range(a.classes)]

    def one_call():
        torch.manual_seed(1)
        return dc.counterfactual(x, cl, a.from_t).samples

    def reseeded():
        outs = []
        for lab in labs:
            torch.manual_seed(1)
            outs.append(dc.sample(x, lab, from_t=a.from_t))
        return torch.stack(outs, dim=1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for _ in range(a.warmup):
        got, want = one_call(), reseeded()
    torch.cuda.synchronize()
    diff = (got - want).abs().max().item()
    ms = {"counterfactual": [], "reseeded_sample": []}
    for _ in range(a.reps):
        ms["counterfactual"].append(timed(one_call)[0])
        ms["reseeded_sample"].append(timed(reseeded)[0])
    dc.check_device_errors()
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps(dict(workload="chexpert256-dwt-unet counterfactual", dtype=a.dtype, images=a.images, classes=a.classes,
                          sampling_steps=a.steps, from_t=a.from_t, reps=a.reps, warmup=a.warmup,
                          counterfactual_ms_per_step=round(med["counterfactual"] / a.steps, 3),
                          reseeded_sample_ms_per_step=round(med["reseeded_sample"] / a.steps, 3),
                          counterfactual_call_ms=[round(v, 2) for v in sorted(ms["counterfactual"])],
                          reseeded_sample_call_ms=[round(v, 2) for v in sorted(ms["reseeded_sample"])],
                          speedup=round(med["reseeded_sample"] / med["counterfactual"], 3), max_abs_difference=diff)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--from-t", dest="from_t", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=600, help="seconds for the measuring child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5 (the figure is a median)")
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(f"bench_counterfactual: the measurement did not finish within {a.timeout} s", file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
