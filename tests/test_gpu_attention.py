"""GPU: the four kernels behind dc_attention — attn_wave_kernel, attn_mfma_kernel, attn_flash_t_kernel, attn_self_f32_kernel — every instance
and every route, against an fp64 reference over EVERY output element with a derived per-element bound (tests/attention_cases.py: the cases,
the operands, the reference, the bound and the checker; tests/test_attention_cases.py pins their routing and holds the checker against an
emulation of each route and against planted faults on the host).

Every case: the operands are rounded to the compute type first and the reference is formed from exactly those; the variant string is asserted
on the real pointers before the launch; the output buffer is pre-filled with a sentinel, and pad columns (ld_out > heads d), everything behind
row n L and a guard region must still hold it bit for bit; every value finite and inside its bound; the pad columns of q/k/v and a guard
region behind their last row hold NaN, so a read of one shows.  The tolerances of test_gpu_ops.py's attention tests stay as a second, outer
assertion."""
import time

import pytest
import torch

import attention_cases as A
from diffusion_classifier_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def outer_tolerance(c):
    """max |got - ref| as the older tests allow it: test_attention_with_large_logits for "peaked", test_attention_long_sequences_flash for the
    flash kernel, test_attention_f32_long_sequences beyond 256 tokens in fp32, test_attention everywhere else."""
    dt = c["dtype"]
    if c["mode"] == "peaked":
        return {A.F32: 2e-4, A.BF16: 4e-2, A.F16: 6e-3}[dt]
    if dt == A.F32:
        return 2e-5 if c["L"] <= 256 else 5e-5
    if c["expect"] == "flash":
        return 2e-2 if dt == A.BF16 else 3e-3
    return 1.5e-2


def device_operands(c, o):
    """(device tensors, (q, k, v) addresses); the tensors must outlive the launch."""
    bufs, iq, ik, iv = A.pack(c, o)
    dev = [b.to(DEV) for b in bufs]
    es = dev[0].element_size()
    return dev, tuple(dev[i].data_ptr() + off * es for i, off in (iq, ik, iv))


def launch(c, ptrs, out):
    p = L.AttentionParams(**A.attention_fields(c, *ptrs, out.data_ptr()))
    variant = L.lib().dc_attention_variant(p).decode()
    assert variant == c["expect"], (c["name"], variant)
    L.check(L.lib().dc_attention(p, L.stream_ptr()), "dc_attention")


@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c["name"])
def test_attention_kernel_against_fp64_reference(c):
    t0 = time.time()
    o = A.make_operands(c)
    ref, bound = A.reference(c, o)
    t1 = time.time()
    dev, ptrs = device_operands(c, o)
    out = A.new_output(c, DEV)
    launch(c, ptrs, out)
    torch.cuda.synchronize()
    buf = out.cpu()
    problems, worst = A.check_output(c, buf, ref, bound)
    err = float((A.body(c, buf).double() - ref).abs().max())
    print(f"{c['name']} {c['instance']}: worst err / bound {worst:.4f}, max |err| {err:.2e}; reference {t1 - t0:.2f} s, whole case {time.time() - t0:.2f} s")
    assert not problems, (c["name"], problems)
    assert err < outer_tolerance(c), (c["name"], err)


@pytest.mark.parametrize("c", A.PLACEMENT_CASES, ids=lambda c: c["name"])
def test_attention_bits_do_not_depend_on_placement(c):
    """Every kernel sums in a fixed order per (sample, head) pair: a sample's output bits are the same alone (n = 1) and as samples 0 and 2 of
    a batch of three, where it lands on other waves, workgroups and pair groups."""
    assert c["n"] == 1
    c3 = dict(c, n=3)
    o1 = A.make_operands(c)
    o3 = A.make_operands(c3, seed=1)
    for x in ("q", "k", "v"):
        o3[x][0] = o1[x][0]
        o3[x][2] = o1[x][0]
    outs = []
    for cc, oo in ((c, o1), (c3, o3)):
        dev, ptrs = device_operands(cc, oo)
        out = A.new_output(cc, DEV)
        launch(cc, ptrs, out)
        torch.cuda.synchronize()
        outs.append(A.body(cc, out.cpu()).view(cc["n"], cc["L"], -1))
    alone, batch = outs
    assert bool(torch.isfinite(alone.float()).all())
    for i in (0, 2):
        differ = (A._bits(batch[i].contiguous()) != A._bits(alone[0].contiguous()))
        assert not bool(differ.any()), f"{c['name']}: sample {i} of 3 differs from the sample alone in {int(differ.sum())} elements, heads {sorted({int(j) // c['d'] for j in differ.nonzero()[:, 1]})}"
    assert not torch.equal(batch[1], batch[0])


@pytest.mark.parametrize("c", A.REPEAT_CASES, ids=lambda c: c["name"])
def test_attention_kernels_are_deterministic_at_size(c):
    """Launch-to-launch bit-identity on 512 (sample, head) pairs, other traffic in between."""
    dev, ptrs = device_operands(c, A.make_operands(c))
    outs = []
    for _ in range(3):
        out = A.new_output(c, DEV)
        torch.randn(1 << 22, device=DEV).sum()
        launch(c, ptrs, out)
        outs.append(out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(A.body(c, outs[0]).float()).all())
    for o2 in outs[1:]:
        differ = int((A._bits(o2) != A._bits(outs[0])).sum())
        assert differ == 0, f"{c['name']}: a repeated launch differs in {differ} elements"
