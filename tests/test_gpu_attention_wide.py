"""GPU: the two kernels behind dc_attention_wide — attn_wide_kernel ("wide": four waves per query tile, each on a quarter of the head
dimension) and attn_wide_f32_kernel ("fp32": attn_exact_run with 32-wide slices) — against the fp64 reference over EVERY output element
with the per-element bound of tests/attention_cases.py (operands, reference, bound and checker are imported from there, unchanged).

The "wide" route rounds P to the compute type for P.V and keeps the row sum unrounded, like the flash kernel: its cases carry
expect="flash" for the reference's error model, the exact route's carry "fp32"; `route` is the dc_attention_wide_variant string that is
asserted on the real pointers before each launch.  The partial-score sum across the four waves is one more summation order of a length-d
dot product, which the bound's (d + 4) 2^-24 term covers for any order.  Operands carry NaN in the pad column and lead element of the
"unaligned" layout and in a guard region behind the last row; the output holds a sentinel that must survive outside the rows written.

Cases: d in {256, 512} x L in {1, 31, 32, 33, 64, 100, 257} (a lone key; one short of the 32-key block, the block, the block plus one;
two blocks; several blocks with a ragged tail, and with L = 257 a last query tile of one query) x heads in {1, 2} x layouts {fused,
split, unaligned} x {bf16, f16, f32} x {random, negative}, n = 2.

Largest err / bound on an MI355X: "wide" 0.33 (bf16, d = 256, L = 33); "fp32" with unaligned bf16 operands 0.78 (d = 256, L = 32: with no
rounded P the bound is little more than the rounding of the stored value); "fp32" in f32 below 1e-3."""
import time

import pytest
import torch

import attention_cases as A
from diffusion_classifier_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS, LENGTHS, HEADS = (256, 512), (1, 31, 32, 33, 64, 100, 257), (1, 2)
LAYOUTS, MODES = ("fused", "split", "unaligned"), ("random", "negative")


def wide_case(dt, d, Lq, heads, layout, mode, n=2):
    C = heads * d
    route = "wide" if dt != A.F32 and layout != "unaligned" else "fp32"
    return dict(name=f"{route}_{A.DTN[dt]}_d{d}_L{Lq}_n{n}h{heads}_{layout}_{mode}", dtype=dt, n=n, L=Lq, heads=heads, d=d,
                ld_qkv={"fused": 3 * C, "split": C, "unaligned": 3 * C + 1}[layout], ld_out=C,
                scale=float(torch.tensor(d ** -0.5, dtype=torch.float32)), expect="flash" if route == "wide" else "fp32", route=route,
                layout=layout, mode=mode)


CASES = [wide_case(dt, d, Lq, h, lay, mode) for dt in (A.BF16, A.F16, A.F32) for d in DIMS for Lq in LENGTHS for h in HEADS
         for lay in LAYOUTS for mode in MODES]
_REF = {}


def operands_and_reference(c):
    """Computed once per (type, shape, mode, error model) and shared by the layouts; never modified."""
    key = (c["dtype"], c["n"], c["L"], c["heads"], c["d"], c["mode"], c["expect"])
    if key not in _REF:
        o = A.make_operands(c)
        if c["mode"] == "negative":
            assert float(A.logits(c, o).max()) <= -8.0, c["name"]
        _REF[key] = (o, *A.reference(c, o))
    return _REF[key]


def device_operands(c, o):
    bufs, iq, ik, iv = A.pack(c, o)
    dev = [b.to(DEV) for b in bufs]
    es = dev[0].element_size()
    return dev, tuple(dev[i].data_ptr() + off * es for i, off in (iq, ik, iv))


def launch(c, ptrs, out):
    p = L.AttentionWideParams(**A.attention_fields(c, *ptrs, out.data_ptr()))
    variant = L.lib().dc_attention_wide_variant(p).decode()
    assert variant == c["route"], (c["name"], variant)
    L.check(L.lib().dc_attention_wide(p, L.stream_ptr()), "dc_attention_wide")


def test_the_case_table_covers_what_it_says():
    assert len(CASES) == 3 * 2 * 7 * 2 * 3 * 2 and len({c["name"] for c in CASES}) == len(CASES)
    assert {c["route"] for c in CASES if c["dtype"] != A.F32 and c["layout"] != "unaligned"} == {"wide"}
    assert {c["route"] for c in CASES if c["dtype"] == A.F32 or c["layout"] == "unaligned"} == {"fp32"}
    assert all(c["n"] == 2 for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_attention_wide_against_fp64_reference(c):
    t0 = time.time()
    o, ref, bound = operands_and_reference(c)
    dev, ptrs = device_operands(c, o)
    out = A.new_output(c, DEV)
    launch(c, ptrs, out)
    torch.cuda.synchronize()
    buf = out.cpu()
    problems, worst = A.check_output(c, buf, ref, bound)
    err = float((A.body(c, buf).double() - ref).abs().max())
    print(f"{c['name']}: worst err / bound {worst:.4f}, max |err| {err:.2e}; whole case {time.time() - t0:.2f} s")
    assert not problems, (c["name"], problems)


@pytest.mark.parametrize("c", [wide_case(A.BF16, 512, 257, 2, "fused", "random"), wide_case(A.F32, 512, 257, 2, "fused", "random")],
                         ids=lambda c: c["name"])
def test_attention_wide_repeated_launches_are_bit_identical(c):
    """Launch-to-launch bit-identity at d = 512, L = 257, other traffic in between; and a sample's bits do not depend on its neighbour."""
    o, _, _ = operands_and_reference(c)
    dev, ptrs = device_operands(c, o)
    outs = []
    for _ in range(3):
        out = A.new_output(c, DEV)
        torch.randn(1 << 20, device=DEV).sum()
        launch(c, ptrs, out)
        outs.append(out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(A.body(c, outs[0]).float()).all())
    for o2 in outs[1:]:
        differ = int((A._bits(o2) != A._bits(outs[0])).sum())
        assert differ == 0, f"{c['name']}: a repeated launch differs in {differ} elements"
    swapped = {x: o[x].flip(0) for x in ("q", "k", "v")}                       # the two samples trade places
    dev2, ptrs2 = device_operands(c, swapped)
    out2 = A.new_output(c, DEV)
    launch(c, ptrs2, out2)
    torch.cuda.synchronize()
    a = A.body(c, outs[0].cpu()).view(2, c["L"], -1)
    b = A.body(c, out2.cpu()).view(2, c["L"], -1)
    assert torch.equal(A._bits(a[0].contiguous()), A._bits(b[1].contiguous())) and torch.equal(A._bits(a[1].contiguous()), A._bits(b[0].contiguous()))
