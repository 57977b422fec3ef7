#!/usr/bin/env python3
"""Micro-benchmark of dc_attention on the DiT-B/4 shape (1024 tokens, 12 heads x 64, f16 / bf16), a 4096-token one, and head dim 96:
the CheXpert experiment UNet's 768-channel level (1024 / 4096 tokens x 8 heads) and DiT-XL/2 (256 tokens x 16 heads of 72, padded to 96);
the one-wave-per-pair kernel (64 and 16 tokens x 8 heads x 64) and the whole-sequence kernel (64 tokens x 8 heads x 96) at batches of
about 3 GB of q / k / v + output per call, so that ten calls take tens of milliseconds
(developer tool; DCAMD_LIB selects the library, so A/B builds can be timed in one session).

  python tools/bench_attention.py [n_samples]
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diffusion_classifier_amd import _lib as L

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
for dt, td in ((L.DC_F16, torch.float16), (L.DC_BF16, torch.bfloat16)):
    for Lq, heads, d, nn in ((1024, 12, 64, n), (4096, 12, 64, max(1, n // 16)),
                             (1024, 8, 96, n), (4096, 8, 96, max(1, n // 16)), (256, 16, 96, 4 * n),
                             (64, 8, 64, 128 * n), (16, 8, 64, 512 * n), (64, 8, 96, 96 * n)):
        Cc = heads * d
        torch.manual_seed(1)
        qkv = (torch.randn(nn, Lq, 3 * Cc, device="cuda") * 1.2).to(td)
        out = torch.empty(nn, Lq, Cc, dtype=td, device="cuda")
        p = L.AttentionParams(q=qkv.data_ptr(), k=qkv.data_ptr() + Cc * 2, v=qkv.data_ptr() + 2 * Cc * 2, out=out.data_ptr(), dtype=dt,
                              n=nn, L=Lq, heads=heads, d=d, ld_qkv=3 * Cc, ld_out=Cc, scale=d ** -0.5)
        for _ in range(3):
            L.check(L.lib().dc_attention(p, L.stream_ptr()), "attn")
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 10
        e0.record()
        for _ in range(reps):
            L.check(L.lib().dc_attention(p, L.stream_ptr()), "attn")
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        fl = 4.0 * nn * heads * Lq * Lq * d
        vf = getattr(L.lib(), "dc_attention_variant", None)      # (absent from libraries older than this tool)
        kern = vf(p).decode() if vf is not None else "?"
        print(f"{'f16' if dt == L.DC_F16 else 'bf16'} L={Lq} heads={heads} d={d} n={nn} [{kern}]: {ms:.3f} ms  {fl / ms / 1e9:.0f} TFLOP/s  "
              f"checksum {out.float().abs().mean().item():.6f}")
