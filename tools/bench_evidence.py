"""Times classify(return_evidence=True) against the plain call on the GPU: the flagship workload of bench.py (CIFAR-10 UNet, random
weights, 16 images, 10 classes x 50 trials, bf16, rng="philox"), flag off and flag on in ONE process, warm.

    python tools/bench_evidence.py [--dtype bf16] [--images 16] [--steps 20] [--warmup 3] [--timeout 900] [--out FILE.json]

The measurement runs in a child process under its own time limit (the parent never opens the GPU).  The child warms both forms up
(each builds its own plans), then times them alternately, `steps` times each: every step starts with the host-to-device copy of its
batch from pinned memory, as in bench.py, and ends in a device synchronise; the figure is the median step time of each form.  A second
figure per form is bench.py's own: `steps` calls back to back between two synchronisations, divided by `steps` (the host side of step
i + 1 then runs under the kernels of step i) — the number to hold against bench.py's ms_per_step.  Next to the ratios it prints the
bytes the map op adds with 64-bit atomics per step (units x H x W x 8) and the time that would take at the chip's float-atomic rate of
about 1.3 TB/s: an estimate to compare with, not a measurement.  One JSON line on stdout (and in --out).  Nothing gates on it.
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
    L.require_gpu()
    dev = "cuda:0"
    torch.manual_seed(0)
    kw = dca.cifar10_unet_kwargs()
    size, classes, T = kw["sample_size"], 10, a.trials
    cfg = dict(pred_param="eps", schedule="cosine", noise_d=size, image_size=size, cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1,
               encoder_type="nn", classes=classes, n_stages=1, evaluation_per_stage=[T], n_keep_per_stage=[1], n_fast_classes=2,
               fast_classification=False, compute_dtype=a.dtype)
    dc = dca.DiffusionClassifier(dca.UNetCondition2D(**kw), dca.Config(**cfg)).to(dev)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(a.images, kw["in_channels"], size, size, generator=g) * 2 - 1).to(dev)
    xh = torch.empty(x.shape, dtype=x.dtype, pin_memory=True)
    xh.copy_(x)

    def step(flag, seed):
        x.copy_(xh, non_blocking=True)
        return dc.classify(x, rng="philox", seed=seed, return_evidence=flag)

    lab_off = step(False, 1)
    lab_on, ev = step(True, 1)
    same = bool(torch.equal(lab_off, lab_on))
    finite = bool(torch.isfinite(ev.mean_map).all()) and int(ev.invalid.sum()) == 0
    for i in range(a.warmup):
        for flag in (False, True):
            step(flag, 100 + i)
    ms = {False: [], True: []}
    for i in range(a.steps):
        for flag in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(flag, 1234 + i)
            torch.cuda.synchronize()
            ms[flag].append((time.perf_counter() - t0) * 1e3)
    block = {}
    for flag in (False, True, False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(flag, 1234 + i)
        torch.cuda.synchronize()
        block.setdefault(flag, []).append((time.perf_counter() - t0) * 1e3 / a.steps)
    dc.check_device_errors()
    med = {k: statistics.median(v) for k, v in ms.items()}
    atomic_bytes = a.images * classes * T * size * size * 8
    rec = dict(workload=f"cifar10-unet {classes} classes x {T} trials", dtype=a.dtype, images=a.images, steps=a.steps, warmup=a.warmup,
               step_ms_off=round(med[False], 3), step_ms_on=round(med[True], 3), ratio_on_over_off=round(med[True] / med[False], 4),
               step_ms_off_all=[round(v, 3) for v in sorted(ms[False])], step_ms_on_all=[round(v, 3) for v in sorted(ms[True])],
               back_to_back_ms_per_step_off=[round(v, 3) for v in block[False]], back_to_back_ms_per_step_on=[round(v, 3) for v in block[True]],
               back_to_back_ratio=round(min(block[True]) / min(block[False]), 4),
               images_per_s_off=round(a.images / (min(block[False]) * 1e-3), 2),
               atomic_bytes_per_step=atomic_bytes, atomic_ms_at_1p3_TBps_estimate=round(atomic_bytes / 1.3e12 * 1e3, 4),
               labels_equal=same, maps_finite=finite)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--trials", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the measuring child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 (the figure is a median)")
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(f"bench_evidence: the measurement did not finish within {a.timeout} s", file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
