"""Times `classify` of a DiT-XL/2 as diffusers publishes it (16 heads of 72, 28 layers, patch 2, 32 x 32 x 4 latents, 8 output channels:
eps and a learned variance; random weights) under schedule='ddpm_linear': `--images` latents against `--classes` classes, staged as
`--trials` / `--keep` say — the workload of Li et al.'s ImageNet experiment, the number of DESIGN §6s.

    python tools/bench_dit_dir.py [--dtype bf16] [--images 1] [--classes 1000] [--trials 1,3] [--keep 10,1] [--layers 28] [--reps 2]
                                  [--warmup 1] [--units-per-launch N] [--timeout 900] [--json PATH]

`--trials` are the cumulative trial counts at the stage ends (config.evaluation_per_stage), `--keep` the classes that survive each stage
(config.n_keep_per_stage; the last must be 1).  The measurement runs in a child process under its own time limit (the parent never
opens the GPU).  The child warms the classifier up, takes `reps` classify calls between one event pair, then one more whose launches
carry a HIP event pair around every op (dc_run_plan_timed): the per-op times summed by kernel.  One JSON line on stdout (and in
--json).  Nothing gates on it.
"""
import argparse
import contextlib
import json
import os
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
    trials, keep = [int(v) for v in a.trials.split(",")], [int(v) for v in a.keep.split(",")]
    cfg = dict(pred_param="eps", schedule="ddpm_linear", noise_d=32, image_size=32, cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1,
               encoder_type="DiT", classes=a.classes, n_stages=len(trials), evaluation_per_stage=trials, n_keep_per_stage=keep,
               n_fast_classes=2, compute_dtype=a.dtype, units_per_launch=a.units_per_launch)
    with contextlib.redirect_stdout(sys.stderr):
        with torch.device(dev):                       # 750 M random parameters: drawn on the device, not on the host
            model = dca.DiT(out_channels=8, num_layers=a.layers, num_embeds_ada_norm=max(1000, a.classes))
        dc = dca.DiffusionClassifier(model, dca.Config(**cfg)).to(dev)
    x = torch.randn(a.images, 4, 32, 32, device=dev)
    for i in range(a.warmup):
        dc.classify(x, rng="philox", seed=i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(a.reps):
        labels = dc.classify(x, rng="philox", seed=100 + i)
    e1.record()
    e1.synchronize()
    dc._timed_sink = []
    dc.classify(x, rng="philox", seed=200)
    sink, dc._timed_sink = dc._timed_sink, None
    dc.check_device_errors()
    kern, total, flops, units = {}, 0.0, 0.0, 0
    for plan, ms in sink:
        units += plan.n_bj * plan.n_cls
        for t, mt in zip(ms, plan.pb.meta):
            name = mt.get("family", "?") + ("/" + mt["variant"] if "variant" in mt else "")
            k = kern.setdefault(name, dict(ops=0, ms=0.0, flops=0.0, bytes=0.0))
            k["ops"] += 1
            k["ms"] += t
            k["flops"] += mt.get("flops", 0.0)
            k["bytes"] += mt.get("bytes", 0.0)
            total += t
            flops += mt.get("flops", 0.0)
    table = {n: dict(ops=v["ops"], ms=round(v["ms"], 3), share=round(v["ms"] / total, 4),
                     tflops=round(v["flops"] / v["ms"] / 1e9, 1) if v["ms"] > 0 else None,
                     tbs=round(v["bytes"] / v["ms"] / 1e9, 2) if v["ms"] > 0 else None)
             for n, v in sorted(kern.items(), key=lambda kv: -kv[1]["ms"])}
    rec = dict(workload="DiT-XL/2 (learned variance), one classify call", dtype=a.dtype, layers=a.layers, images=a.images, classes=a.classes,
               evaluation_per_stage=trials, n_keep_per_stage=keep, units_launched=units, launches=len(sink), ops=sum(len(ms) for _, ms in sink),
               labels=labels.cpu().tolist(), classify_ms=round(e0.elapsed_time(e1) / a.reps, 3), sum_of_op_ms=round(total, 3),
               ms_per_unit=round(total / units, 4), algorithmic_tflop=round(flops / 1e12, 3), tflops_over_ops=round(flops / total / 1e9, 1),
               per_kernel=table)
    line = json.dumps(rec)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--images", type=int, default=1)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--trials", default="1,3", help="cumulative trials at the stage ends, comma separated (evaluation_per_stage)")
    ap.add_argument("--keep", default="10,1", help="classes kept after each stage, comma separated (n_keep_per_stage; the last is 1)")
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--units-per-launch", type=int, default=None, help="config.units_per_launch (default: the package's rule)")
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the measuring child process")
    ap.add_argument("--json", default=None, help="also write the record to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(f"bench_dit_dir: the measurement did not finish within {a.timeout} s", file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
