"""GPU: igemm_xreg<T,96xN> — every compiled instance (bf16 / f16, plain / GEGLU, the K <= 256 and K <= 512 register layouts), its weight
ring at every slice count, ragged M, the row vector of two samples per wave, the fused row LayerNorm — and the register-staged
igemm<T,128x128> / igemm<T,128x32> with every branch of the element-wise epilogue, against an fp64 reference over EVERY output element
with a derived per-element bound (tests/gemm_small_cases.py: the cases, the operands, the reference, the bound and the checker;
tests/test_gemm_small_cases.py pins their routing and holds the checker against planted faults on the host).

Every case: the operands are rounded to their types first and the reference is formed from exactly those; the variant string is asserted
on the real pointers before the launch; the output buffer is pre-filled with a sentinel, and pad columns (out_ld > channels), everything
behind row M, a guard region and the elements in front of an offset output pointer must still hold it bit for bit; every value finite and
inside its bound; the pad columns of the residual, the tables and a sliced source hold NaN, so a read of one shows.  igemm_xreg is
launched twice and the two buffers must agree bit for bit.  The tolerances of test_gpu_ops.py's GEMM tests stay as a second, outer
assertion."""
import time

import pytest
import torch

import gemm_small_cases as S
import gemm_tile_cases as G
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTER = {L.DC_F32: 2e-5, L.DC_BF16: 1.2e-2, L.DC_F16: 2e-3}      # max |err| / max |ref|, as test_gpu_ops.TOL


def _padded(t, ld, dtype):
    """[..., channels] -> [..., ld] in dtype, NaN in the pad columns."""
    out = torch.full(t.shape[:-1] + (ld,), float("nan"), dtype=dtype)
    out[..., : t.shape[-1]] = t.to(dtype)
    return out


def device_operands(c, o):
    """{pointer field: device tensor} for a case's operands (the allocations: S.pointers moves src0 / bias to where dc_igemm reads)."""
    dt, td = c["dtype"], G.TD[c["dtype"]]
    x0 = torch.full(o["x0"].shape[:-1] + (c["ld0"],), float("nan"), dtype=td)       # the column slice [col0, col0 + C0) of a wider matrix
    x0[..., c["col0"]: c["col0"] + c["C0"]] = o["x0"].to(td)
    d = {"src0": x0.to(DEV)}
    if c["C1"]:
        d["src1"] = o["x1"].to(td).to(DEV)
    w, b = o["w"], o.get("bias")
    if c["act"] == G.ACT_GEGLU:                           # packed rows: 16 value rows, 16 gate rows, ...
        perm = E.geglu_perm(c["Cout"] // 2)
        w, b = w[perm], (None if b is None else b[perm])
    d["W"] = E.pack_matrix(w, dt, DEV, tile_n=c["tile_n"])      # k = tap * (C0 + C1) + c already: the packed form of a conv is that of its GEMM
    if b is not None:
        lead = c["bias_off"] // 4
        d["bias"] = torch.cat([torch.full((lead,), float("nan")), b.contiguous()]).to(DEV)
    for f in ("map0", "map1", "rowvec_map", "gate_map", "res_map"):
        if f in o:
            d[f] = o[f].to(DEV)
    for f in ("rowvec", "gate"):
        if f in o:
            d[f] = _padded(o[f], c[f + "_ld"], torch.float32).to(DEV)
    if "residual" in o:
        d["residual"] = _padded(o["residual"], c["res_ld"], G.TD[c["res_dtype"]]).to(DEV)
    return d


def new_output(c):
    """(allocation, the flat buffer dc_igemm writes): sentinel everywhere; the buffer starts out_off bytes into the allocation."""
    lead = c["out_off"] // S.esize(c["out_dtype"])
    alloc = torch.full((lead + S.rows(c) * c["out_ld"] + G.GUARD,), G.SENTINEL, dtype=G.TD[c["out_dtype"]], device=DEV)
    return alloc, alloc[lead:]


def launch(c, d, alloc):
    kw = S.igemm_fields(c, {**{f: t.data_ptr() for f, t in d.items()}, "out": alloc.data_ptr()})
    p = L.IgemmParams(**kw)
    variant = L.lib().dc_igemm_variant(p).decode()
    assert variant == c["expect"], (c["name"], variant)
    L.check(L.lib().dc_igemm(p, L.stream_ptr()), "dc_igemm")


@pytest.mark.parametrize("c", S.CASES, ids=lambda c: c["name"])
def test_small_kernel_against_fp64_reference(c):
    t0 = time.time()
    o = S.make_operands(c)
    ref, bound = S.reference(c, o)
    t1 = time.time()
    d = device_operands(c, o)
    alloc, out = new_output(c)
    launch(c, d, alloc)
    torch.cuda.synchronize()
    front, buf = alloc[: alloc.numel() - out.numel()].cpu(), out.cpu()
    problems, worst = S.check_output(c, buf, ref, bound)
    if front.numel() and not bool((G._bits(front) == G._bits(torch.full((1,), G.SENTINEL, dtype=front.dtype))[0]).all()):
        problems.append("elements in front of the offset output pointer were written")
    M, co, ld = S.rows(c), S.cout_out(c), c["out_ld"]
    got = buf[: M * ld].view(M, ld)[:, :co].double()
    outer = float((got - ref).abs().max() / ref.abs().max())
    print(f"{c['name']} [{S.family(c)}] {c['expect']}: M={M} K={S.k_total(c)} channels={co}: worst err / bound {worst:.4f}, max err / max |ref| {outer:.2e}; "
          f"reference {t1 - t0:.1f} s, whole case {time.time() - t0:.1f} s")
    assert not problems, (c["name"], problems)
    # the type that rounds the stored value sets the outer tolerance; an fp32 output of 16-bit operands: only the accumulation order differs
    tol = (2e-5 if c["dtype"] == G.F32 else 2e-3) if c["out_dtype"] == G.F32 else max(OUTER[c["dtype"]], OUTER[c["out_dtype"]])
    assert outer < tol, (c["name"], outer)
    if "xreg" in c["expect"]:       # launch-to-launch identity: a trimmed variant of this kernel once computed different values on every launch
        alloc2, out2 = new_output(c)
        launch(c, d, alloc2)
        torch.cuda.synchronize()
        differ = int((G._bits(out2) != G._bits(out)).sum())
        assert differ == 0, f"{c['name']}: a repeated launch differs in {differ} elements"
