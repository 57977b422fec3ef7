"""GPU: the three tile kernels behind dc_igemm's GEMMs and stride-2 convs — igemm_wide8<256x256>, igemm_pipe<256x128,3st>,
igemm_pipe<128x128,2st> — each instance and each branch of the shared lane-resident epilogue, against an fp64 reference over EVERY output
element with a derived per-element bound (tests/gemm_tile_cases.py: the cases, the operands, the reference, the bound and the checker;
tests/test_gemm_tile_cases.py pins their routing and holds the checker against planted faults on the host).

Every case: the operands are rounded to the compute type first and the reference is formed from exactly those; the variant string is asserted
on the real pointers before the launch; the output buffer is pre-filled with a sentinel, and pad columns (out_ld > channels), everything behind
row M and a guard region must still hold it bit for bit; every value finite and inside its bound; the pad columns of the residual hold NaN, so
a read of one shows.  The tolerances of test_gpu_ops.py's GEMM tests stay as a second, outer assertion."""
import time

import pytest
import torch

import gemm_tile_cases as G
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTER = {L.DC_F32: 2e-5, L.DC_BF16: 1.2e-2, L.DC_F16: 2e-3}      # max |err| / max |ref|, as test_gpu_ops.TOL


def device_operands(c, o):
    """{pointer field: device tensor} for a case's operands (the tensors must outlive the launch)."""
    dt, td = c["dtype"], G.TD[c["dtype"]]
    d = {"src0": o["x0"].to(td).to(DEV)}
    if c["C1"]:
        d["src1"] = o["x1"].to(td).to(DEV)
    w, b = o["w"], o.get("bias")
    if c["act"] == G.ACT_GEGLU:                           # packed rows: 16 value rows, 16 gate rows, ...
        perm = E.geglu_perm(c["Cout"] // 2)
        w, b = w[perm], (None if b is None else b[perm])
    d["W"] = E.pack_matrix(w, dt, DEV)                    # k = tap * (C0 + C1) + c already: the packed form of a conv is that of its GEMM
    if b is not None:
        d["bias"] = b.contiguous().to(DEV)
    for f in ("map0", "map1", "rowvec_map", "gate_map", "res_map"):
        if f in o:
            d[f] = o[f].to(DEV)
    for f in ("rowvec", "gate"):
        if f in o:
            d[f] = o[f].contiguous().to(DEV)
    if "residual" in o:
        r = o["residual"]
        rd = torch.full((r.shape[0], r.shape[1], c["res_ld"]), float("nan"), dtype=td)
        rd[..., : r.shape[2]] = r.to(td)
        d["residual"] = rd.to(DEV)
    return d


def launch(c, d, out):
    kw = G.igemm_fields(c, {**{f: t.data_ptr() for f, t in d.items()}, "out": out.data_ptr()})
    p = L.IgemmParams(**kw)
    variant = L.lib().dc_igemm_variant(p).decode()
    assert variant == c["expect"], (c["name"], variant)
    L.check(L.lib().dc_igemm(p, L.stream_ptr()), "dc_igemm")


def set_env(c, monkeypatch):
    monkeypatch.delenv("DCAMD_PIPE_CHIP_TILES", raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_tile_kernel_against_fp64_reference(c, monkeypatch):
    set_env(c, monkeypatch)
    t0 = time.time()
    o = G.make_operands(c)
    ref, bound = G.reference(c, o)
    t1 = time.time()
    d = device_operands(c, o)
    out = G.new_output(c, DEV)
    launch(c, d, out)
    torch.cuda.synchronize()
    buf = out.cpu()
    problems, worst = G.check_output(c, buf, ref, bound)
    M, co, ld = G.rows(c), G.cout_out(c), c["out_ld"]
    got = buf[: M * ld].view(M, ld)[:, :co].double()
    outer = float((got - ref).abs().max() / ref.abs().max())
    print(f"{c['name']} [{G.family(c)}] {c['expect']}: M={M} K={G.k_total(c)} channels={co}: worst err / bound {worst:.4f}, max err / max |ref| {outer:.2e}; "
          f"reference {t1 - t0:.1f} s, whole case {time.time() - t0:.1f} s")
    assert not problems, (c["name"], problems)
    tol = (2e-5 if c["dtype"] == G.F32 else 2e-3) if c["out_dtype"] == G.F32 else OUTER[c["dtype"]]
    assert outer < tol, (c["name"], outer)


@pytest.mark.parametrize("name", G.REPEAT_CASES)
def test_tile_kernels_are_deterministic_at_size(name, monkeypatch):
    """Launch-to-launch bit-identity on grids larger than the chip, other traffic in between: one igemm_wide8 instance per epilogue variant and
    the 256x128 tile in both forms."""
    c = G.by_name(name)
    set_env(c, monkeypatch)
    d = device_operands(c, G.make_operands(c))
    outs = []
    for _ in range(3):
        out = G.new_output(c, DEV)
        torch.randn(1 << 22, device=DEV).sum()
        launch(c, d, out)
        outs.append(out)
    torch.cuda.synchronize()
    for o2 in outs[1:]:
        differ = int((G._bits(o2) != G._bits(outs[0])).sum())
        assert differ == 0, f"{name}: a repeated launch differs in {differ} elements"
