"""GPU: the two attention bodies of csrc/attn_strip.h behind dc_cross_attention, dc_cross_attention_len, dc_attention_bias and
dc_attention_causal — all 48 template instances — against an fp64 reference over EVERY output element with a derived per-element bound
(tests/strip_attention_cases.py: the cases, the operands, the reference, the bound and the checker; tests/test_strip_attention_cases.py pins
their routing and holds the checker against an emulation of each body and against planted faults on the host).

Every case: the operands are rounded to the compute type first and the reference is formed from exactly those; the variant string is asserted
on the real pointers before the launch; the output buffer is pre-filled with a sentinel, and pad columns (ld_out > heads d), everything behind
the last row and a guard region must still hold it bit for bit; every value of a live row finite and inside its bound, every row at or past a
length an exact zero; the gaps of q / k / v, the rows at or past a length, the contexts nobody maps to and a guard region behind the last row
hold NaN, so a read of one shows.  The flat tolerances of the older strip-family tests stay as a second, outer assertion."""
import time

import pytest
import torch

import strip_attention_cases as S
from attention_cases import BF16, F16, F32
from diffusion_classifier_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}


def outer_tolerance(c):
    """max |got - ref| as the older tests allow it: 1.5e-2 in 16 bit and 2e-5 in f32 on random and negative data
    (tests/test_gpu_cross_attention.py, test_gpu_t5_ops.py, test_gpu_clip_ops.py); "peaked": test_cross_attention_with_large_logits in 16 bit
    and, as that test has no f32 form, test_attention_with_large_logits' 2e-4 in f32."""
    if c["mode"] == "peaked":
        return {F32: 2e-4, BF16: 4e-2, F16: 6e-3}[c["dtype"]]
    return 2e-5 if c["dtype"] == F32 else 1.5e-2


def device_operands(c, o):
    """(everything that must outlive the launch, the parameter fields)."""
    bufs, iq, ik, iv = S.pack(c, o)
    dev = [b.to(DEV) for b in bufs]
    es = dev[0].element_size()
    q, k, v = (dev[i].data_ptr() + off * es for i, off in (iq, ik, iv))
    i32 = lambda x: None if x is None else torch.tensor(x, dtype=torch.int32, device=DEV)
    lens, qm, km = i32(c["lens"]), i32(c.get("q_map")), i32(c.get("kv_map"))
    bias = o["bias"].to(DEV) if "bias" in o else None
    out = S.new_output(c, DEV)
    ptr = lambda t: None if t is None else t.data_ptr()
    return (dev, lens, qm, km, bias, out), S.fields(c, q, k, v, out.data_ptr(), ptr(lens), ptr(qm), ptr(km), ptr(bias)), out


@pytest.mark.parametrize("c", S.CASES, ids=lambda c: c["name"])
def test_strip_attention_kernel_against_fp64_reference(c):
    t0 = time.time()
    o = S.make_operands(c)
    ref, bound, live = S.reference(c, o)
    t1 = time.time()
    keep, f, out = device_operands(c, o)
    p = getattr(L, S.PARAMS[c["entry"]])(**f)
    variant = getattr(L.lib(), S.ENTRY[c["entry"]] + "_variant")(p).decode()
    assert variant == c["expect"], (c["name"], variant)
    L.check(getattr(L.lib(), S.ENTRY[c["entry"]])(p, L.stream_ptr()), S.ENTRY[c["entry"]])
    torch.cuda.synchronize()
    buf = out.cpu()
    problems, worst = S.check_output(c, buf, ref, bound, live)
    err = S.max_abs_err(c, buf, ref, live)
    cell = (c["entry"], c["expect"], S.DTN[c["dtype"]])
    WORST[cell] = max(WORST.get(cell, 0.0), worst)
    print(f"{c['name']} {c['instance']}: worst err / bound {worst:.4f}, max |err| {err:.2e}; largest err / bound of {cell} so far {WORST[cell]:.4f}; "
          f"reference {t1 - t0:.2f} s, whole case {time.time() - t0:.2f} s")
    assert not problems, (c["name"], problems)
    assert err < outer_tolerance(c), (c["name"], err)
