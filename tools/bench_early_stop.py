"""Times per-image early stopping (config key `stop_margin_z`) on the GPU: the CIFAR-10 UNet (random weights), 16 images, 10 classes x 50
trials, bf16, stages [10, 50] keeping [10, 1], rng="philox" with a fixed seed — the same call three ways in one process:

    off       the key unset
    never     stop_margin_z = +inf: the per-stage synchronisation and the extra launches, nothing stops (labels must equal `off`)
    median    stop_margin_z = the median first-checkpoint z-score of `off`: about half of the images stop after 10 trials

    python tools/bench_early_stop.py [--dtype bf16] [--images 16] [--reps 7] [--warmup 2] [--timeout 900]

The measurement runs in a child process under its own time limit (the parent never opens the GPU).  The child warms every form up
(every plan size the timed calls use), then times the three alternately, `reps` times each, host clock around a call that ends in a
device synchronise, and reports the median call time of each, the overhead never / off, the speed-up off / median and, beside it, the
(trial, image) pairs `median` scored over those of `off`.  One JSON line on stdout.  Nothing gates on it.  The weights are random:
which share of the images of a trained model is decided early is a property of that model and is not measured here.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import diffusion_classifier_amd as dca
    from diffusion_classifier_amd import _lib as L
    from diffusion_classifier_amd import posterior as P
    L.require_gpu()
    dev = "cuda:0"
    torch.manual_seed(0)
    kw = dca.cifar10_unet_kwargs()
    size = kw["sample_size"]
    ends = [a.first, a.trials]
    cfg = dict(pred_param="eps", schedule="cosine", noise_d=size, image_size=size, cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1,
               encoder_type="nn", classes=10, n_stages=2, evaluation_per_stage=ends, n_keep_per_stage=[10, 1], n_fast_classes=2,
               compute_dtype=a.dtype)
    dc = dca.DiffusionClassifier(dca.UNetCondition2D(**kw), dca.Config(**cfg)).to(dev)
    x = torch.rand(a.images, kw["in_channels"], size, size, device=dev) * 2 - 1
    t = torch.rand(a.trials, a.images)

    def call(z_stop, **extra):
        dc.config.stop_margin_z = z_stop
        return dc.classify(x, t=t, rng="philox", seed=7, **extra)

    lab_off, err = call(None, return_errors=True)
    z = P.class_posterior_hip(err.to(dev), ends[0]).margin_z
    thr = float(z.median())
    forms = {"off": None, "never": float("inf"), "median": thr}
    lab_med, t_done = call(thr, return_trials=True)
    pairs_ratio = float(t_done.sum()) / (a.images * a.trials)
    same_never = bool(torch.equal(call(float("inf")), lab_off))

    def timed(z_stop):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(z_stop)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        for zs in forms.values():
            timed(zs)
    ms = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, zs in forms.items():
            ms[k].append(timed(zs))
    dc.check_device_errors()
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps(dict(workload="cifar10-unet 10 classes, stages %s" % ends, dtype=a.dtype, images=a.images, reps=a.reps, warmup=a.warmup,
                          call_ms={k: round(v, 2) for k, v in med.items()},
                          call_ms_all={k: [round(v, 2) for v in sorted(vs)] for k, vs in ms.items()},
                          overhead_never_over_off=round(med["never"] / med["off"], 4),
                          speedup_off_over_median=round(med["off"] / med["median"], 3),
                          pairs_scored_median_over_off=round(pairs_ratio, 4), threshold=thr,
                          images_stopped_early=int((t_done < a.trials).sum()), never_labels_equal_off=same_never)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--trials", type=int, default=50)
    ap.add_argument("--first", type=int, default=10, help="trials of the first stage (the only checkpoint)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the measuring child process")
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
        print(f"bench_early_stop: the measurement did not finish within {a.timeout} s", file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
