#!/usr/bin/env python3
"""Micro-benchmark of dc_cross_attention at a prompt of 77 tokens on the site shapes of the benched UNet (8000 units: 64 tokens x 8
heads of 32, 16 tokens x 8 heads of 64) and of the CheXpert-DWT UNet (256 tokens x 8 heads of 64), f16 / bf16, contexts picked per unit
through a ctx_of_unit map (unit -> class), against F.scaled_dot_product_attention on the same GPU with K / V gathered per unit (what
the reference's stack would run; the gather itself is not timed).  Reports ms and TB/s of the q + out stream the kernel is bound by
(developer tool; DCAMD_LIB selects the library, so A/B builds can be timed in one session).

  python tools/bench_cross_attention.py [units] [S] [--json OUT.json] [--kv-len 8,20,77]

--kv-len: also time dc_cross_attention_len with every context at each of the given key counts (of S rows per context), in rounds that
alternate with dc_cross_attention on the same buffers (median, min and max of the rounds): what the skipped key blocks of short
prompts save, and what the length costs at full length.  Without the option the output is what it was.
"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from diffusion_classifier_amd import _lib as L

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
kv_lens = [int(v) for v in sys.argv[sys.argv.index("--kv-len") + 1].split(",")] if "--kv-len" in sys.argv else []
args = [a for a in args if a != out_json and not (kv_lens and a == sys.argv[sys.argv.index("--kv-len") + 1])]
units = int(args[0]) if len(args) > 0 else 8000
S = int(args[1]) if len(args) > 1 else 77
n_ctx, reps = 10, 200


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternated(fns, rounds=5):
    """Time the calls in alternating rounds -> per call (median, min, max) ms."""
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ms[i].append(timed(fn))
    return [(sorted(m)[len(m) // 2], min(m), max(m)) for m in ms]


rows, len_rows = [], []
for dt, td, name in ((L.DC_F16, torch.float16, "f16"), (L.DC_BF16, torch.bfloat16, "bf16")):
    for site, Lq, heads, d, n in (("cfg2 8x8", 64, 8, 32, units), ("cfg2 4x4", 16, 8, 64, units), ("cfg3 16x16", 256, 8, 64, max(1, units // 10))):
        C = heads * d
        torch.manual_seed(1)
        q = torch.randn(n, Lq, C, device="cuda").to(td)
        kv = torch.randn(n_ctx, S, 2 * C, device="cuda").to(td)                 # K | V as the context plan's stacked GEMM leaves them
        ctx_of_unit = (torch.arange(n, device="cuda", dtype=torch.int32) % n_ctx).contiguous()
        out = torch.empty(n, Lq, C, dtype=td, device="cuda")
        p = L.CrossAttentionParams(q=q.data_ptr(), k=kv.data_ptr(), v=kv.data_ptr() + C * 2, out=out.data_ptr(), q_map=None,
                                   kv_map=ctx_of_unit.data_ptr(), dtype=dt, n=n, Lq=Lq, S=S, heads=heads, d=d, ld_q=C, ld_kv=2 * C,
                                   ld_out=C, scale=d ** -0.5)
        ms = timed(lambda: L.check(L.lib().dc_cross_attention(p, L.stream_ptr()), "dc_cross_attention"))
        kern = L.lib().dc_cross_attention_variant(p).decode()
        # the reference's stack: SDPA on [n, heads, Lq, d] with the K / V of every unit gathered beforehand
        idx = ctx_of_unit.long()
        qh = q.view(n, Lq, heads, d).transpose(1, 2)
        kh = kv[idx, :, :C].reshape(n, S, heads, d).transpose(1, 2).contiguous()
        vh = kv[idx, :, C:].reshape(n, S, heads, d).transpose(1, 2).contiguous()
        ms_sdpa = timed(lambda: F.scaled_dot_product_attention(qh, kh, vh))
        ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(n, Lq, C)
        diff = (out.float() - ref.float()).abs().max().item()
        stream = 2.0 * n * Lq * C * 2                                           # q in + out back, bytes
        row = dict(dtype=name, site=site, n=n, Lq=Lq, heads=heads, d=d, S=S, kernel=kern, ms=round(ms, 4), tb_per_s=round(stream / ms / 1e9, 3),
                   gflop=round(4.0 * n * heads * Lq * S * d / 1e9, 2), sdpa_ms=round(ms_sdpa, 4), sdpa_tb_per_s=round(stream / ms_sdpa / 1e9, 3),
                   max_abs_diff_vs_sdpa=diff)
        rows.append(row)
        print(f"{name} {site}: n={n} Lq={Lq} heads={heads} d={d} S={S} [{kern}]: {ms:.3f} ms  {row['tb_per_s']:.2f} TB/s (q + out)   "
              f"SDPA, K/V gathered: {ms_sdpa:.3f} ms  {row['sdpa_tb_per_s']:.2f} TB/s   max |diff| {diff:.2e}")
        if kv_lens:
            lens = [torch.full((n_ctx,), ln, dtype=torch.int32, device="cuda") for ln in kv_lens]
            pl = [L.CrossAttentionLenParams(kv_len=t.data_ptr(), **{f: getattr(p, f) for f, _ in L.CrossAttentionParams._fields_}) for t in lens]
            calls = [lambda: L.check(L.lib().dc_cross_attention(p, L.stream_ptr()), "dc_cross_attention")]
            calls += [lambda x=x: L.check(L.lib().dc_cross_attention_len(x, L.stream_ptr()), "dc_cross_attention_len") for x in pl]
            res = alternated(calls)
            for ln, (med, lo, hi) in zip(["full"] + kv_lens, res):
                lr = dict(dtype=name, site=site, n=n, Lq=Lq, heads=heads, d=d, S=S, kernel=kern,
                          call="dc_cross_attention" if ln == "full" else "dc_cross_attention_len", kv_len=S if ln == "full" else ln,
                          ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), tb_per_s=round(stream / med / 1e9, 3))
                len_rows.append(lr)
                print(f"    {lr['call']} kv_len={lr['kv_len']}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f})  {lr['tb_per_s']:.2f} TB/s (q + out)")
if out_json:
    with open(out_json, "w") as fh:
        rec = dict(tool="tools/bench_cross_attention.py", units=units, S=S, n_ctx=n_ctx, reps=reps, rows=rows)
        if kv_lens:
            rec.update(kv_lens=kv_lens, rounds=5, len_rows=len_rows)
        json.dump(rec, fh, indent=1)
