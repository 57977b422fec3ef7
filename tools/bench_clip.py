"""Times the CLIP text encoder plan at the ViT-L/14 text shape on the GPU: 12 layers, 768 channels, 12 heads of 64, 3072 hidden,
quick-GELU, random weights, 11 prompts x 77 tokens (10 classes and the null prompt) without a mask, bf16 by default.

    python tools/bench_clip.py [--dtype bf16] [--prompts 11] [--tokens 77] [--reps 30] [--warmup 5] [--timeout 300] [--json PATH]

The measurement runs in a child process under its own time limit (the parent never opens the GPU, and a limit that expires ends the
measurement instead of leaving it behind).  The child warms the plan up, times `reps` plan runs one by one with HIP events on the launch
stream, and reports the median and the spread; one pass of dc_run_plan_timed gives the per-op split, summed by kernel family.  Where
`transformers` is installed, the same weights run through eager `CLIPTextModel` in the same dtype on the same GPU in the same process:
its median over the same number of runs and the relative L2 between the two outputs are reported next to the plan's.  One JSON line on
stdout (and in --json).  Nothing gates on it: the encoder runs once per class set, not per trial.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
             max_position_embeddings=77, hidden_act="quick_gelu")


def _timed(fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(ms[0], 4), p90_ms=round(ms[int(0.9 * (len(ms) - 1))], 4))


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from diffusion_classifier_amd import _lib as L
    from diffusion_classifier_amd.nets.clip import CLIPTextEncoder
    L.require_gpu()
    dev = "cuda:0"
    torch.manual_seed(0)
    m = CLIPTextEncoder(**SHAPE)
    with torch.no_grad():                  # CLIP's own initialisation scales, roughly: fan-in for the matrices, small embeddings
        for k, p in m.named_parameters():
            if k.endswith("embedding.weight"):
                p.normal_(0.0, 0.02)
            elif k.endswith("proj.weight") or k.endswith("fc1.weight"):
                p.normal_(0.0, 768 ** -0.5)
            elif k.endswith("fc2.weight"):
                p.normal_(0.0, 3072 ** -0.5)
    m = m.to(dev).set_compute_dtype(a.dtype)
    ids = torch.randint(1, SHAPE["vocab_size"], (a.prompts, a.tokens), device=dev)
    out = m(ids)
    assert torch.isfinite(out).all()
    plan = next(iter(m._plans.values()))
    for _ in range(a.warmup):
        plan.run()
    torch.cuda.synchronize()
    rec = dict(workload="CLIP ViT-L/14 text encoder", dtype=a.dtype, prompts=a.prompts, tokens=a.tokens, reps=a.reps)
    rec.update(_timed(plan.run, a.reps))
    per_op = plan.run_timed()
    split = {}
    for t, mt in zip(per_op, plan.pb.meta):
        fam = mt.get("family", "?") + (":" + mt["variant"] if "variant" in mt else "")
        split[fam] = split.get(fam, 0.0) + t
    rec.update(ops=len(per_op), algorithmic_gflop=round(sum(mt.get("flops", 0.0) for mt in plan.pb.meta) / 1e9, 2),
               timed_pass_ms=round(sum(per_op), 4), per_family_ms={k: round(v, 4) for k, v in sorted(split.items(), key=lambda kv: -kv[1])})
    try:
        from transformers import CLIPTextConfig, CLIPTextModel
    except ImportError:
        rec["eager_transformers"] = None
    else:
        tdt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
        hf = CLIPTextModel(CLIPTextConfig(**SHAPE)).eval()
        own = set(hf.state_dict())
        sd = {(k if k in own else k[len("text_model."):]): v for k, v in m.state_dict().items()}
        hf.load_state_dict(sd, strict=False)
        hf = hf.to(dev, tdt)
        with torch.no_grad():
            ref = hf(input_ids=ids).last_hidden_state.float()
            for _ in range(a.warmup):
                hf(input_ids=ids)
            torch.cuda.synchronize()
            eager = _timed(lambda: hf(input_ids=ids), a.reps)
        eager["rel_l2_plan_vs_eager"] = float(((out - ref).norm() / ref.norm()).item())
        rec["eager_transformers"] = eager
    line = json.dumps(rec)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--prompts", type=int, default=11)
    ap.add_argument("--tokens", type=int, default=77)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
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
        print(f"bench_clip: the measurement did not finish within {a.timeout} s", file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
