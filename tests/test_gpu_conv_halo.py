"""GPU: the 3x3 halo-convolution family behind dc_igemm — conv3_halo<T,4w|8w> in every instance launch_halo picks (staggered and lock-step,
buffer-descriptor and per-lane loaders, the 4x4 mosaic), conv3_ws<T,gn>, conv3_thin<T>, the four-phase upsample form conv3_up4<T,4w|8w> and
igemm_pipe_up4 — against an fp64 reference over EVERY output element with a derived per-element bound (tests/conv_halo_cases.py: the cases,
the operands, the reference, the bound and the checker; tests/test_conv_halo_cases.py pins their routing and holds the checker against
planted faults on the host).

Every case: the operands are rounded to the compute type first and the reference is formed from exactly those; every source, the residual
and the row-vector table lie inside a larger NaN-filled allocation (a guard in front and behind, NaN in the pad columns), so a fetch from
outside an image shows; the GroupNorm affine of the fused prologue is made on the host; the variant string is asserted on the real pointers
before the launch; the output buffer is pre-filled with a sentinel, and pad columns, everything behind row M and a guard region must still
hold it bit for bit; every value finite and inside its bound; the quad records, where the case has them, against their own reference.  The
tolerances of test_gpu_ops.py's conv tests stay as a second, outer assertion."""
import time

import pytest
import torch

import conv_halo_cases as G
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTER = {L.DC_F32: 2e-5, L.DC_BF16: 1.2e-2, L.DC_F16: 2e-3}          # max |err| / max |ref|, as test_gpu_ops.TOL
OUTER_GN = {L.DC_F32: 3e-5, L.DC_BF16: 1.5e-2, L.DC_F16: 2e-3}       # as test_conv3x3_with_fused_groupnorm_prologue
POISON = G.GUARD                                                     # NaN elements in front of and behind every embedded operand


class Embedded:
    """t [..., C] (CPU) as rows of `ld` elements inside a NaN-filled device allocation; .ptr: the address of its first element."""

    def __init__(self, t, ld, dtype):
        C = t.shape[-1]
        r = t.reshape(-1, C)
        flat = torch.full((2 * POISON + r.shape[0] * ld,), float("nan"), dtype=dtype)
        flat[POISON: POISON + r.shape[0] * ld].view(r.shape[0], ld)[:, :C] = r.to(dtype)
        self.alloc = flat.to(DEV)
        self.ptr = self.alloc.data_ptr() + POISON * self.alloc.element_size()
        assert self.ptr % 16 == 0


def device_operands(c, o):
    """({pointer field: address}, the tensors that must outlive the launch)."""
    dt, td = c["dtype"], G.TD[c["dtype"]]
    keep, p = [], {}

    def put(name, obj, addr=None):
        keep.append(obj)
        p[name] = obj.data_ptr() if addr is None else addr

    e = Embedded(o["x0"], c["ld0"], td)
    put("src0", e, e.ptr)
    if c["C1"]:
        e = Embedded(o["x1"], c["ld1"], td)
        put("src1", e, e.ptr)
    if c["C2"]:
        e = Embedded(o["x2"], c["ld2"], td)
        put("src2", e, e.ptr)
        put("W2", E.pack_matrix(o["w2"], dt, DEV))
    put("W", E.pack_up4(o["w"], dt, DEV, c["tile_n"]) if c["up4"] else E.pack_conv3x3(o["w"], dt, DEV, c["tile_n"]))
    if "bias" in o:
        put("bias", o["bias"].contiguous().to(DEV))
    if "rowvec" in o:
        e = Embedded(o["rowvec"], c["rowvec_ld"], torch.float32)
        put("rowvec", e, e.ptr)
    if "residual" in o:
        e = Embedded(o["residual"], c["res_ld"], td)
        put("residual", e, e.ptr)
    for f in ("map0", "map1", "map2", "rowvec_map", "res_map"):
        if f in o:
            put(f, o[f].to(DEV))
    if "gn" in c["use"]:
        put("gn_scale", o["gn_scale"].contiguous().to(DEV))
        put("gn_shift", o["gn_shift"].contiguous().to(DEV))
    return p, keep


def launch(c, ptrs, out, qs):
    kw = G.igemm_fields(c, dict(ptrs, out=out.data_ptr(), qstats=None if qs is None else qs.data_ptr()))
    p = L.IgemmParams(**kw)
    variant = L.lib().dc_igemm_variant(p).decode()
    assert variant == c["expect"], (c["name"], variant)
    L.check(L.lib().dc_igemm(p, L.stream_ptr()), "dc_igemm")


def set_env(c, monkeypatch):
    monkeypatch.delenv("DCAMD_HALO_NO_STAG", raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_halo_conv_against_fp64_reference(c, monkeypatch):
    set_env(c, monkeypatch)
    t0 = time.time()
    o = G.make_operands(c)
    ref, bound, det = G.reference(c, o, detail=True)
    t1 = time.time()
    ptrs, keep = device_operands(c, o)
    out = G.new_output(c, DEV)
    qs = G.new_qstats(c, DEV) if "qstats" in c["use"] else None
    launch(c, ptrs, out, qs)
    torch.cuda.synchronize()
    buf = out.cpu()
    problems, worst = G.check_output(c, buf, ref, bound)
    worst_q = 0.0
    if qs is not None:        # the same again with the quad records: their own worst ratio is printed apart
        problems, worst_q = G.check_output(c, buf, ref, bound, qs.cpu(), det["e"])
    M, co, ld = G.rows(c), c["Cout"], c["out_ld"]
    got = buf[: M * ld].view(M, ld)[:, :co].double()
    outer = float((got - ref).abs().max() / ref.abs().max())
    print(f"{c['name']} [{c['family']}] {c['expect']} = {c['instance']}: M={M} K={G.k_all(c)} Cout={co}: worst err / bound {worst:.4f}" +
          (f" (with the quad records {worst_q:.4f})" if qs is not None else "") + f", max err / max |ref| {outer:.2e}; reference {t1 - t0:.1f} s, whole case {time.time() - t0:.1f} s")
    assert not problems, (c["name"], problems)
    tol = (OUTER_GN if "gn" in c["use"] else OUTER)[c["dtype"]]
    if c["out_dtype"] == G.F32 and c["dtype"] != G.F32:
        tol = 2e-3
    assert outer < tol, (c["name"], outer)


@pytest.mark.parametrize("name", G.REPEAT_CASES)
def test_halo_convs_are_deterministic(name, monkeypatch):
    """Launch-to-launch bit-identity, outputs and quad records, other traffic in between."""
    c = G.by_name(name)
    set_env(c, monkeypatch)
    ptrs, keep = device_operands(c, G.make_operands(c))
    outs = []
    for _ in range(3):
        out = G.new_output(c, DEV)
        qs = G.new_qstats(c, DEV) if "qstats" in c["use"] else None
        torch.randn(1 << 22, device=DEV).sum()
        launch(c, ptrs, out, qs)
        outs.append((out, qs))
    torch.cuda.synchronize()
    for o2, q2 in outs[1:]:
        differ = int((G._bits(o2) != G._bits(outs[0][0])).sum())
        assert differ == 0, f"{name}: a repeated launch differs in {differ} elements"
        if q2 is not None:
            differ = int((G._bits(q2) != G._bits(outs[0][1])).sum())
            assert differ == 0, f"{name}: a repeated launch differs in {differ} quad-record values"
