"""Times the T5 encoder plan at the t5-base shape on the GPU: 12 layers, d_model 768, 12 heads of 64, d_ff 3072, random weights,
11 prompts x 77 tokens (10 classes and the null prompt), bf16 by default.

    python tools/bench_t5.py [--dtype bf16] [--prompts 11] [--tokens 77] [--reps 30] [--warmup 5] [--timeout 300]

The measurement runs in a child process under its own time limit (the parent never opens the GPU, and a limit that expires ends the
measurement instead of leaving it behind).  The child warms the plan up, times `reps` plan runs one by one with HIP events on the launch
stream, and reports the median and the spread; then one pass of dc_run_plan_timed gives the per-op split, summed by kernel family.  One
JSON line on stdout.  Nothing gates on it: the encoder runs once per class set, not per trial.
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
    from diffusion_classifier_amd import _lib as L
    from diffusion_classifier_amd.nets.t5 import T5Encoder
    L.require_gpu()
    dev = "cuda:0"
    torch.manual_seed(0)
    m = T5Encoder(vocab_size=32128, d_model=768, d_kv=64, d_ff=3072, num_layers=12, num_heads=12)
    with torch.no_grad():                  # T5's own initialisation scales (factor 1.0): q carries d_model^-1/2 * d_kv^-1/2, the rest fan-in
        for k, p in m.named_parameters():
            if k.endswith((".q.weight",)):
                p.normal_(0.0, (768 * 64) ** -0.5)
            elif k.endswith((".k.weight", ".v.weight", ".wi.weight")):
                p.normal_(0.0, 768 ** -0.5)
            elif k.endswith(".o.weight"):
                p.normal_(0.0, (12 * 64) ** -0.5)
            elif k.endswith(".wo.weight"):
                p.normal_(0.0, 3072 ** -0.5)
    m = m.to(dev).set_compute_dtype(a.dtype)
    ids = torch.randint(1, 32128, (a.prompts, a.tokens), device=dev)
    lens = torch.randint(a.tokens // 4, a.tokens + 1, (a.prompts,))
    lens[0] = a.tokens
    mask = (torch.arange(a.tokens)[None, :] < lens[:, None]).long().to(dev)
    out = m(ids, mask)
    assert torch.isfinite(out).all()
    plan = next(iter(m._plans.values()))
    for _ in range(a.warmup):
        plan.run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    per_op = plan.run_timed()
    split = {}
    for t, mt in zip(per_op, plan.pb.meta):
        fam = mt.get("family", "?") + (":" + mt["variant"] if "variant" in mt else "")
        split[fam] = split.get(fam, 0.0) + t
    flops = sum(mt.get("flops", 0.0) for mt in plan.pb.meta)
    ms.sort()
    print(json.dumps(dict(workload="t5-base encoder", dtype=a.dtype, prompts=a.prompts, tokens=a.tokens, lengths=lens.tolist(),
                          ops=len(per_op), reps=a.reps, median_ms=round(statistics.median(ms), 4), min_ms=round(ms[0], 4),
                          p90_ms=round(ms[int(0.9 * (len(ms) - 1))], 4), algorithmic_gflop=round(flops / 1e9, 2),
                          timed_pass_ms=round(sum(per_op), 4),
                          per_family_ms={k: round(v, 4) for k, v in sorted(split.items(), key=lambda kv: -kv[1])})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--prompts", type=int, default=11)
    ap.add_argument("--tokens", type=int, default=77)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds for the measuring child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(f"bench_t5: the measurement did not finish within {a.timeout} s", file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
