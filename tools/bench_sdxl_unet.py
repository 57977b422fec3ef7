"""Times one `classify` call of the Stable Diffusion XL base UNet (`sdxl_unet_kwargs()`, random weights, the published geometry) under
schedule='scaled_linear' and encoder_type='clip_dual': a prompt table of `--classes` prompts of `--tokens` tokens and the pooled table
next to it (both random, set through `set_prompt` / `set_pooled`: the text encoders are not what is timed), `--images` latents of
`--latent` x `--latent`, `--trials` noise draws — "where the workload starts" in DESIGN §6.

    python tools/bench_sdxl_unet.py [--dtype bf16] [--latent 32] [--images 1] [--classes 4] [--trials 2] [--tokens 77] [--reps 2]
                                    [--warmup 1] [--timeout 900] [--json PATH]

The measurement runs in a child process under its own time limit (the parent never opens the GPU).  encoder_type='clip_dual' wants
two text-encoder directories: the child writes two random ones of the published WIDTHS (768, and 1280 with a projection to 1280) but
two thin layers each into a temporary directory, which is all the classifier's width checks read.  The child warms up, takes `reps`
classify calls between one event pair, then one more whose launches carry a HIP event pair around every op (dc_run_plan_timed): the
per-op times summed by kernel.  One JSON line on stdout (and in --json).  Nothing gates on it, nothing is tuned for it.
"""
import argparse
import contextlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_text_encoder(path, cls, **kw):
    from safetensors.torch import save_file
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(kw, fh)
    save_file({k: v.contiguous() for k, v in cls(**kw).state_dict().items()}, os.path.join(path, "model.safetensors"))
    return path


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import diffusion_classifier_amd as dca
    from diffusion_classifier_amd import _lib as L
    from diffusion_classifier_amd.nets.clip import CLIPTextEncoder, CLIPTextEncoderWithProjection
    L.require_gpu()
    dev = "cuda:0"
    torch.manual_seed(0)
    kw = dict(dca.sdxl_unet_kwargs(), sample_size=a.latent)
    thin = dict(vocab_size=128, intermediate_size=64, num_hidden_layers=2, max_position_embeddings=77)
    with tempfile.TemporaryDirectory() as tmp:
        p1 = write_text_encoder(os.path.join(tmp, "text_encoder"), CLIPTextEncoder, hidden_size=768, num_attention_heads=12, **thin)
        p2 = write_text_encoder(os.path.join(tmp, "text_encoder_2"), CLIPTextEncoderWithProjection, hidden_size=1280, num_attention_heads=20,
                                projection_dim=1280, hidden_act="gelu", **thin)
        cfg = dict(pred_param="eps", schedule="scaled_linear", noise_d=a.latent, image_size=a.latent, cfg_w=0.0, ema_beta=0.999, ema_warmup=0,
                   ema_update_freq=1, encoder_type="clip_dual", clip_path=p1, clip2_path=p2, prompt_tokens=a.tokens, classes=a.classes,
                   n_stages=1, evaluation_per_stage=[a.trials], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype=a.dtype)
        with torch.device(dev):                                               # 2.6 G parameters: initialised on the device
            unet = dca.StableDiffusionXLUNet(**kw)
        with contextlib.redirect_stdout(sys.stderr):
            dc = dca.DiffusionClassifier(unet, dca.Config(**cfg))
    dc = dc.to(dev)
    for row in range(a.classes + 1):
        dc.encoder.set_prompt(row, torch.randn(a.tokens, 2048))
        dc.set_pooled(row, torch.randn(1280))
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
    kern, total, flops = {}, 0.0, 0.0
    for plan, ms in sink:
        for t, mt in zip(ms, plan.pb.meta):
            name = mt.get("family", "?") + ("/" + mt["variant"] if "variant" in mt else "")
            k = kern.setdefault(name, dict(ops=0, ms=0.0, flops=0.0))
            k["ops"] += 1
            k["ms"] += t
            k["flops"] += mt.get("flops", 0.0)
            total += t
            flops += mt.get("flops", 0.0)
    table = {n: dict(ops=v["ops"], ms=round(v["ms"], 3), share=round(v["ms"] / total, 4),
                     tflops=round(v["flops"] / v["ms"] / 1e9, 1) if v["ms"] > 0 else None)
             for n, v in sorted(kern.items(), key=lambda kv: -kv[1]["ms"])}
    units = a.images * a.trials * a.classes
    plan = sink[0][0]
    rec = dict(workload="SDXL-base UNet, one classify call", dtype=a.dtype, latent=a.latent, images=a.images, classes=a.classes,
               trials=a.trials, tokens=a.tokens, units=units, launches=len(sink), ops=sum(len(ms) for _, ms in sink),
               ctx_ops=len(plan.ctx_pb.meta), ctx_arena_mb=round(plan.ctx_pb.arena_bytes / 2 ** 20, 1),
               arena_mb=round(plan.pb.arena_bytes / 2 ** 20, 1), labels=labels.cpu().tolist(),
               classify_ms=round(e0.elapsed_time(e1) / a.reps, 3), sum_of_op_ms=round(total, 3), ms_per_unit=round(total / units, 3),
               algorithmic_tflop=round(flops / 1e12, 3), tflops_over_ops=round(flops / total / 1e9, 1), per_kernel=table)
    line = json.dumps(rec)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--latent", type=int, default=32, help="latent height = width (a multiple of 4); the image is 8x as large")
    ap.add_argument("--images", type=int, default=1)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--trials", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=77)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
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
        print(f"bench_sdxl_unet: the measurement did not finish within {a.timeout} s", file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
