"""Times one `classify` step of the Stable Diffusion 1.5 UNet (`sd15_unet_kwargs()`, random weights) under schedule='scaled_linear': a
prompt table of `--classes` prompts of `--tokens` tokens, `--images` latents of `--latent` x `--latent`, `--trials` noise draws — the
table of DESIGN §6o.

    python tools/bench_sd_unet.py [--dtype bf16] [--latent 32] [--images 1] [--classes 4] [--trials 2] [--tokens 77] [--reps 3]
                                  [--warmup 1] [--timeout 600] [--json PATH]

The measurement runs in a child process under its own time limit (the parent never opens the GPU).  The child warms the classifier up,
takes `reps` classify calls between one event pair, then one more whose launches carry a HIP event pair around every op
(dc_run_plan_timed): the per-op times summed by kernel, and the share of them spent in FALLBACK routes — launches that exist only because a
faster route does not take the width: GroupNorm passes (the producer-side and conv-fused forms want whole 4-channel quads per group and,
for the producer, 128-channel tiles), the register-staged igemm<...> kernels and the exact fp32 attention kernels.  One JSON line on stdout
(and in --json).  Nothing gates on it.
"""
import argparse
import contextlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def is_fallback(mt):
    kernel = str(mt.get("variant") or mt.get("family"))
    return mt.get("family") == "groupnorm" or kernel.startswith("igemm<") or kernel in ("fp32", "exact")


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import diffusion_classifier_amd as dca
    from diffusion_classifier_amd import _lib as L
    L.require_gpu()
    dev = "cuda:0"
    torch.manual_seed(0)
    kw = dict(dca.sd15_unet_kwargs(), sample_size=a.latent)
    cfg = dict(pred_param="eps", schedule="scaled_linear", noise_d=a.latent, image_size=a.latent, cfg_w=0.0, ema_beta=0.999, ema_warmup=0,
               ema_update_freq=1, encoder_type="prompt", prompt_tokens=a.tokens, classes=a.classes, n_stages=1, evaluation_per_stage=[a.trials],
               n_keep_per_stage=[1], n_fast_classes=2, compute_dtype=a.dtype)
    with contextlib.redirect_stdout(sys.stderr):
        dc = dca.DiffusionClassifier(dca.StableDiffusionUNet(**kw), dca.Config(**cfg)).to(dev)
    x = torch.randn(a.images, 4, a.latent, a.latent, device=dev)
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
    kern, total, fallback, flops = {}, 0.0, 0.0, 0.0
    for plan, ms in sink:
        for t, mt in zip(ms, plan.pb.meta):
            name = mt.get("family", "?") + ("/" + mt["variant"] if "variant" in mt else "")
            k = kern.setdefault(name, dict(ops=0, ms=0.0, flops=0.0, bytes=0.0, fallback=is_fallback(mt)))
            k["ops"] += 1
            k["ms"] += t
            k["flops"] += mt.get("flops", 0.0)
            k["bytes"] += mt.get("bytes", 0.0)
            total += t
            flops += mt.get("flops", 0.0)
            fallback += t if is_fallback(mt) else 0.0
    table = {n: dict(ops=v["ops"], ms=round(v["ms"], 3), share=round(v["ms"] / total, 4), fallback=v["fallback"],
                     tflops=round(v["flops"] / v["ms"] / 1e9, 1) if v["ms"] > 0 else None,
                     tbs=round(v["bytes"] / v["ms"] / 1e9, 2) if v["ms"] > 0 else None)
             for n, v in sorted(kern.items(), key=lambda kv: -kv[1]["ms"])}
    units = a.images * a.trials * a.classes
    rec = dict(workload="SD 1.5 UNet, one classify step", dtype=a.dtype, latent=a.latent, images=a.images, classes=a.classes, trials=a.trials,
               tokens=a.tokens, units=units, launches=len(sink), ops=sum(len(ms) for _, ms in sink), labels=labels.cpu().tolist(),
               classify_ms=round(e0.elapsed_time(e1) / a.reps, 3), sum_of_op_ms=round(total, 3), ms_per_unit=round(total / units, 3),
               algorithmic_tflop=round(flops / 1e12, 3), tflops_over_ops=round(flops / total / 1e9, 1),
               fallback_ms=round(fallback, 3), fallback_share=round(fallback / total, 4), per_kernel=table)
    line = json.dumps(rec)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--latent", type=int, default=32, help="latent height = width (a power of two); the image is 8x as large")
    ap.add_argument("--images", type=int, default=1)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--trials", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=77)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=600, help="seconds for the measuring child process")
    ap.add_argument("--json", default=None, help="also write the record to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(f"bench_sd_unet: the measurement did not finish within {a.timeout} s", file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
