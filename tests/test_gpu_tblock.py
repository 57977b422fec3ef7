"""GPU: dc_tblock_front (csrc/tblock.hip) against the cases of tests/tblock_cases.py — exact cases bit for bit against a closed formula,
full-chain cases element by element against an fp64 reference with the documented rounding points and the bound KAPPA u S + output
rounding (tests/test_tblock_cases.py holds the table, the emulations that measure KAPPA and the checker to account on the host).

Every case: the operands are rounded to the compute type first and the reference is formed from exactly those; x and the row-vector table
lie inside larger NaN-filled allocations (a guard in front and behind, NaN in the pad columns), so a 16-byte load from a pad column shows;
the output allocation is pre-filled with a sentinel, and pad columns, a guard in front, everything behind row n * 64 and a guard behind
must still hold it bit for bit; dc_tblock_front_ok says 1 on the real parameters before the launch.  The 3-ulp max norm of
test_gpu_ops.test_tblock_front_matches_the_separate_launches stays as a second, outer assertion."""
import time

import pytest
import torch

import tblock_cases as G
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DC_ERR_ARG, DC_ERR_SHAPE, DC_ERR_ALIGN = -1, -2, -4


class Embedded:
    """t [..., C] (CPU) as rows of `ld` elements inside a NaN-filled device allocation; .ptr: the address of its first element."""

    def __init__(self, t, ld, dtype):
        self.alloc = G.embedded(t, ld, dtype).to(DEV)
        self.ptr = self.alloc.data_ptr() + G.GUARD * self.alloc.element_size()
        assert self.ptr % 16 == 0


def device_operands(c, o):
    """({pointer field: address}, the tensors that must outlive the launch)."""
    dt, td = c["dtype"], G.TD[c["dtype"]]
    keep, p = [], {}

    def put(name, obj, addr=None):
        keep.append(obj)
        p[name] = obj.data_ptr() if addr is None else addr

    e = Embedded(o["x"], c["ldx"], td)
    put("x", e, e.ptr)
    for f in ("Wp", "Wqkv", "Wo"):
        put(f, E.pack_matrix(o[f], dt, DEV))
    for f, src in (("bp", "bp"), ("ln_g", "ln_g"), ("ln_b", "ln_b"), ("bo", "bo")):
        if src in o:
            put(f, o[src].float().contiguous().to(DEV))
    if "rowvec" in o:
        e = Embedded(o["rowvec"], c["rowvec_ld"], torch.float32)
        put("rowvec", e, e.ptr)
    if "rowvec_map" in o:
        put("rowvec_map", o["rowvec_map"].to(DEV))
    return p, keep


def params(c, ptrs, out, **over):
    kw = G.front_fields(c, dict(ptrs, out=out.data_ptr() + G.GUARD * out.element_size()))
    kw.update(over)
    return L.TblockFrontParams(**kw)


def launch(c, ptrs, out):
    p = params(c, ptrs, out)
    assert L.lib().dc_tblock_front_ok(p) == 1, c["name"]
    L.check(L.lib().dc_tblock_front(p, L.stream_ptr()), "dc_tblock_front")


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_tblock_front_against_reference(c):
    t0 = time.time()
    cc, o, ref, S, want = G.prepared(c["name"])
    t1 = time.time()
    ptrs, keep = device_operands(c, o)
    out = G.new_output(c, DEV)
    launch(c, ptrs, out)
    torch.cuda.synchronize()
    buf = out.cpu()
    problems, worst = G.check_output(c, buf, ref, want)
    M, ld = G.rows(c), c["ld_out"]
    got = buf[G.GUARD: G.GUARD + M * ld].view(M, ld)[:, :G.C_CH]
    if c["kind"] == "exact":
        print(f"{c['name']} [{c['mode']}] n={c['n']} heads={c['heads']} use={sorted(c['use'])} layout={c['layout']}: {int(worst)} representable values off "
              f"the expected bits; whole case {time.time() - t0:.1f} s")
        ref = want.view(G.TD[c["dtype"]]).double()           # the outer norm against the expected values themselves
    else:
        fwd = G.forward_ratio(c, got.float(), ref, S, stored=True)
        print(f"{c['name']} [{c['mode']}] n={c['n']} heads={c['heads']} use={sorted(c['use'])} layout={c['layout']}: worst err / bound {worst:.4f}, "
              f"forward error / (u S) {fwd:.4f} (KAPPA {G.KAPPA}); reference {t1 - t0:.1f} s, whole case {time.time() - t0:.1f} s")
    outer = float((got.double() - ref).abs().max() / ref.abs().max())
    print(f"    max err / max |ref| {outer:.2e} (bound {3 * G.U_OUT[c['dtype']]:.2e})")
    assert not problems, (c["name"], problems)
    assert outer < 3 * G.U_OUT[c["dtype"]], (c["name"], outer)


@pytest.mark.parametrize("name", G.REPEAT_CASES)
def test_tblock_front_is_deterministic(name):
    """Launch-to-launch bit-identity, other traffic in between."""
    c = G.by_name(name)
    ptrs, keep = device_operands(c, G.make_operands(c))
    outs = []
    for _ in range(3):
        out = G.new_output(c, DEV)
        torch.randn(1 << 22, device=DEV).sum()
        launch(c, ptrs, out)
        outs.append(out)
    torch.cuda.synchronize()
    for o2 in outs[1:]:
        differ = int((G._bits(o2) != G._bits(outs[0])).sum())
        assert differ == 0, f"{name}: a repeated launch differs in {differ} elements"


@pytest.mark.parametrize("what,status", [("ldx_260", DC_ERR_SHAPE), ("rowvec_ld_258", DC_ERR_ALIGN), ("rowvec_8_bytes_off", DC_ERR_ALIGN),
                                         ("scale_0", DC_ERR_ARG), ("heads_2", DC_ERR_SHAPE)])
def test_tblock_front_refuses_what_it_does_not_serve(what, status):
    """Refused with the documented status before any launch: the output allocation keeps its sentinel everywhere."""
    c = G.by_name("epilogue_exact_bf16_full")
    assert {"bo", "rowvec", "rowvec_map"} <= c["use"]
    ptrs, keep = device_operands(c, G.make_operands(c))
    out = G.new_output(c, DEV)
    over = {"ldx_260": dict(ldx=260), "rowvec_ld_258": dict(rowvec_ld=258), "rowvec_8_bytes_off": dict(rowvec=ptrs["rowvec"] + 8),
            "scale_0": dict(scale=0.0), "heads_2": dict(heads=2)}[what]
    good = params(c, ptrs, out)
    assert L.lib().dc_tblock_front_ok(good) == 1
    rc = L.lib().dc_tblock_front(params(c, ptrs, out, **over), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == status, (what, rc, L.lib().dc_last_error().decode())
    sent = G._bits(torch.full((1,), G.SENTINEL, dtype=out.dtype))[0]
    assert bool((G._bits(out.cpu()) == sent).all()), f"{what}: the refused call wrote to the output"
    if what in ("ldx_260", "heads_2"):
        assert L.lib().dc_tblock_front_ok(params(c, ptrs, out, **over)) == 0
