"""Times the decoder of the Stable Diffusion AutoencoderKL (`sd_vae_kwargs()`, random weights) as its launch plan on the GPU: 32x32 latents
to 256x256 images, batch 16, bf16 by default — the table of DESIGN §6n.

    python tools/bench_vae.py [--dtype bf16] [--batch 16] [--latent 32] [--reps 5] [--warmup 3] [--timeout 300] [--json PATH]

The measurement runs in a child process under its own time limit (the parent never opens the GPU).  The child warms the plan up, takes
`reps` passes of dc_run_plan_timed (a HIP event pair around every op) and keeps the median per op, summed by kernel family with the plan's
algorithmic FLOP and byte counts; `reps` back-to-back plan runs between one event pair give the time without the event pairs.  One JSON line
on stdout (and in --json).  Nothing gates on it.
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
    kw = dca.sd_vae_kwargs()
    m = dca.VAEDecoder(**kw)
    x = torch.randn(a.batch, kw["latent_channels"], a.latent, a.latent, device=dev)
    m = m.to(dev).set_compute_dtype(a.dtype)
    out = m(x)
    finite = bool(torch.isfinite(out).all())
    plan = next(iter(m._plans.values()))
    for _ in range(a.warmup):
        plan.run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        plan.run()
    e1.record()
    e1.synchronize()
    passes = [plan.run_timed() for _ in range(a.reps)]
    per_op = [statistics.median(p[i] for p in passes) for i in range(len(passes[0]))]
    fam = {}
    for t, mt in zip(per_op, plan.pb.meta):
        name = mt.get("family", "?") + ("/" + mt["variant"] if "variant" in mt else "")
        f = fam.setdefault(name, dict(ops=0, ms=0.0, flops=0.0, bytes=0.0))
        f["ops"] += 1
        f["ms"] += t
        f["flops"] += mt.get("flops", 0.0)
        f["bytes"] += mt.get("bytes", 0.0)
    table = {k: dict(ops=v["ops"], ms=round(v["ms"], 4), tflops=round(v["flops"] / v["ms"] / 1e9, 1) if v["ms"] > 0 else None,
                     tbs=round(v["bytes"] / v["ms"] / 1e9, 2) if v["ms"] > 0 else None)
             for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"])}
    rec = dict(workload="SD AutoencoderKL decoder", dtype=a.dtype, batch=a.batch, latent=a.latent, ops=len(per_op), finite=finite,
               back_to_back_ms=round(e0.elapsed_time(e1) / a.reps, 4), sum_of_op_ms=round(sum(per_op), 4),
               algorithmic_gflop=round(sum(mt.get("flops", 0.0) for mt in plan.pb.meta) / 1e9, 1), per_family=table)
    line = json.dumps(rec)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--latent", type=int, default=32, help="latent height = width; the image is 8x as large")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds for the measuring child process")
    ap.add_argument("--json", default=None, help="also write the record to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(f"bench_vae: the measurement did not finish within {a.timeout} s", file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
