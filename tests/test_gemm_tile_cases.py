"""The tile-kernel parity cases (tests/gemm_tile_cases.py) held to account without a GPU: every case is routed to the kernel it names, the
table covers every instance it claims to, and the checker the GPU test relies on passes a plain emulation of the kernels and fails each of
a list of planted faults.  dc_igemm_variant and dc_igemm's refusals run on the host alone, as in tests/test_igemm_dispatch.py."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import gemm_tile_cases as G
import test_igemm_dispatch as D

FAKE = D.FAKE
SMALL = [c for c in G.CASES if not c["big"]]


def _lib():
    mod = D._load_lib()
    return mod, mod.lib()


def _variant(c, monkeypatch):
    mod, lib = _lib()
    monkeypatch.delenv("DCAMD_PIPE_CHIP_TILES", raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    return lib.dc_igemm_variant(mod.IgemmParams(**G.igemm_fields(c, {f: FAKE for f in G.PTR_FIELDS}))).decode()


# ---- a. routing -----------------------------------------------------------------------------------------------------------------
def test_case_names_are_unique_and_envs_are_the_per_call_switch_only():
    names = [c["name"] for c in G.CASES]
    assert len(names) == len(set(names))
    assert all(set(c["env"]) <= {"DCAMD_PIPE_CHIP_TILES"} for c in G.CASES)
    assert all(G.by_name(n)["big"] for n in G.REPEAT_CASES)
    for c in G.CASES:       # the tag says which epilogue instance runs
        assert c["act"] == G.TAG_ACT[c["tag"]] and (("gate" in c["use"]) == (c["tag"] == "gate")), c["name"]


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_every_case_is_routed_to_the_kernel_it_names(c, monkeypatch):
    assert _variant(c, monkeypatch) == c["expect"], c["name"]


def test_wide_cases_have_the_properties_they_are_there_for():
    """What the igemm_wide8 list promises, computed from the cases: tile counts, K-tile counts, ragged last tiles, seams, sample sizes, weights
    on both sides of the 16 MiB tile-order rule."""
    wide = [c for c in G.CASES if G.family(c) == "wide"]
    tiles = lambda c: ((G.rows(c) + 255) // 256) * ((c["Cout"] + 255) // 256)
    nk = lambda c: G.k_total(c) // G.BKE[c["dtype"]]
    last = lambda c: G.rows(c) % 256
    wbytes = lambda c: ((c["Cout"] + 127) // 128 * 128) * G.k_total(c) * (4 if c["dtype"] == G.F32 else 2)
    assert all(tiles(c) >= 400 for c in wide)
    for dt in (G.F32, G.BF16, G.F16):
        mine = [c for c in wide if c["dtype"] == dt]
        assert any(nk(c) % 2 == 1 for c in mine), dt                                         # an odd number of K-tiles
        assert any(0 < last(c) < 64 for c in mine) or dt == G.F16, dt
    assert {nk(c) for c in wide} >= {4, 5, 48}
    assert any(0 < last(c) < 32 for c in wide) and any(32 < last(c) < 64 for c in wide)
    assert any(c["Cout"] % 256 > 128 and c["out_ld"] > c["Cout"] for c in wide)              # channel tail inside the second 128-half
    assert any(c["C1"] and (c["C0"] // G.BKE[c["dtype"]]) % 2 == 1 and {"map0", "map1"} <= c["use"] for c in wide)
    assert any(c["Hout"] <= 24 and "rowvec_map" in c["use"] for c in wide) and any(c["Hout"] >= 256 and "rowvec" in c["use"] for c in wide)
    assert any("rowvec" in c["use"] and 64 < c["Hout"] and c["Hout"] % 64 for c in wide)     # a sample boundary inside a wave
    assert any("res_map" in c["use"] and c["res_ld"] > G.cout_out(c) for c in wide)
    assert any(c["tag"] == "gate" and "gate_map" in c["use"] and "residual" in c["use"] and c["out_dtype"] != G.F32 for c in wide)
    assert any(c["dtype"] != G.F32 and c["out_dtype"] == G.F32 for c in wide) and any(c["dtype"] != G.F32 and c["out_dtype"] == c["dtype"] for c in wide)
    assert any(wbytes(c) > 16 << 20 for c in wide) and any(wbytes(c) <= 16 << 20 for c in wide)
    assert any(c["tag"] == "geglu" and {"bias", "residual"} <= c["use"] for c in wide) and any(c["tag"] == "gelu_tanh" and "bias" in c["use"] for c in wide)


# ---- b. coverage ----------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_instance_or_proves_it_unreachable(monkeypatch):
    have = {(G.family(c), c["dtype"], c["tag"]) for c in G.CASES}
    dts = (G.F32, G.BF16, G.F16)
    wide = {("wide", dt, tag) for dt in dts for tag in ("none", "geglu", "gelu_tanh", "gate")}            # the 12 compiled igemm_wide8 instances
    assert wide <= have, wide - have
    pipe = {(f, dt, tag) for f in ("pipe128_slim", "pipe128_tap", "pipe256_slim", "pipe256_tap") for dt in dts for tag in G.BRANCHES}
    assert pipe <= have, pipe - have                                                                     # the 60 cells, none unreachable
    # two cases per dtype reach the 256-row tile with no switch set, one slim, one tap-gather
    for dt in dts:
        nat = [c for c in G.CASES if G.family(c).startswith("pipe256") and not c["env"] and c["dtype"] == dt]
        assert {c["taps"] for c in nat} == {1, 9}, dt
    # what the table does not reach must be out of the dispatcher's reach too, on a probe grid
    everything = wide | pipe | {("wide", dt, "silu") for dt in dts}
    assert everything - have == set(G.UNREACHABLE)
    mod, lib = _lib()
    monkeypatch.delenv("DCAMD_PIPE_CHIP_TILES", raising=False)
    for (fam, dt, tag) in G.UNREACHABLE:
        assert (fam, tag) == ("wide", "silu")
        n = 0
        for M, K, cout, extra in itertools.product((256 * 400, 256 * 2000 + 7, 256 * 50), (128, 256, 320, 768, 3072), (256, 512, 1024, 3072),
                                                   ((), ("bias",), ("bias", "residual"), ("rowvec",))):
            c = G._case("probe", dt, tag, n_img=1, HW=M, C0=K, Cout=cout, use=set(extra), expect="%s")
            v = lib.dc_igemm_variant(mod.IgemmParams(**G.igemm_fields(c, {f: FAKE for f in G.PTR_FIELDS}))).decode()
            assert "wide8" not in v and "igemm" in v, (c, v)
            n += 1
        assert n == 240


# ---- the GEGLU refusal ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["rowvec", "gate"])
@pytest.mark.parametrize("base", ["wide_bf16_geglu_residual", "pipe128_slim_f32_geglu", "pipe256_tap_f16_geglu"])
def test_geglu_with_a_row_vector_or_a_gate_is_refused(base, field):
    """Neither GEGLU epilogue applies them; dc_igemm used to accept the call and drop them."""
    mod, lib = _lib()
    c = G.by_name(base)
    kw = G.igemm_fields(c, {f: FAKE for f in G.PTR_FIELDS})
    p = mod.IgemmParams(**kw)
    assert lib.dc_igemm_variant(p).decode() != "invalid"
    kw[field] = FAKE
    kw[field + "_ld"] = G.cout_out(c)
    p = mod.IgemmParams(**kw)
    assert lib.dc_igemm_variant(p).decode() == "invalid"
    assert lib.dc_igemm(p, None) == -1                      # DC_ERR_ARG, before any launch
    msg = lib.dc_last_error().decode()
    assert field in msg and "GEGLU" in msg, msg


# ---- c. the checker checks ------------------------------------------------------------------------------------------------------
FAULTS = ["ktile_dropped", "residual_of_next_sample", "vector_of_next_sample", "bias_after_activation", "channels_c_c4_swapped", "pad_column_written",
          "row_past_m_written"]


def applicable(c, fault):
    use = c["use"]
    return {"ktile_dropped": True, "residual_of_next_sample": "residual" in use, "vector_of_next_sample": bool(use & {"rowvec", "gate"}) and c["act"] != G.ACT_GEGLU,
            "bias_after_activation": c["act"] != G.ACT_NONE and "bias" in use, "channels_c_c4_swapped": True,
            "pad_column_written": c["out_ld"] > G.cout_out(c), "row_past_m_written": True}[fault]


def emulate(c, o, fault=None):
    """The kernel, plainly: operands as the compute type holds them, fp32 accumulation one K-tile at a time, the epilogue in fp32 in the
    documented order with the device's activation formulas, the output rounded to its type into a sentinel-filled buffer."""
    dt, g = c["dtype"], G.BKE[c["dtype"]]
    A, W = G.a_matrix(c, o, torch.float32), o["w"]
    M, K = A.shape
    HWo = c["Hout"] * c["Wout"]
    acc = torch.zeros(M, c["Cout"])
    for k0 in range(0, K, g):
        part = A[:, k0:k0 + g] @ W[:, k0:k0 + g].t()
        if fault == "ktile_dropped" and k0 == g * (K // g // 2):
            part[M // 2] = 0.0
        acc += part
    samp = torch.arange(M) // HWo

    def table(name, mname, shift):      # shift: the table row of the neighbouring sample
        idx = o[mname].long()[samp] if mname in o else samp
        return o[name][(idx + shift) % o[name].shape[0]]
    shift = 1 if fault == "vector_of_next_sample" else 0
    late = fault == "bias_after_activation"
    x = acc
    pre_terms = []
    if "bias" in o:
        pre_terms.append(o["bias"])
    if "rowvec" in o and c["act"] != G.ACT_GEGLU:
        pre_terms.append(table("rowvec", "rowvec_map", shift))
    if not late:
        for t in pre_terms:
            x = x + t
    fast = dt != G.F32
    if c["act"] == G.ACT_SILU:
        x = G.silu_device(x, fast)
    elif c["act"] == G.ACT_GELU_TANH:
        x = G.gelu_tanh_device(x, fast)
    elif c["act"] == G.ACT_GEGLU:
        u, gg = x.chunk(2, dim=-1)
        x = u * G.gelu_erf_device(gg, fast)
    if late:
        for t in pre_terms:
            x = x + (t if c["act"] != G.ACT_GEGLU else t.chunk(2, dim=-1)[0])
    if "gate" in o:
        x = x * table("gate", "gate_map", shift)
    if "residual" in o:
        rs = 1 if fault == "residual_of_next_sample" else 0
        ridx = o["res_map"].long()[samp] if "res_map" in o else samp
        x = x + o["residual"][(ridx + rs) % o["residual"].shape[0], torch.arange(M) % HWo]
    if fault == "channels_c_c4_swapped":
        r = M // 3
        x = x.clone()
        x[r, 8:16] = torch.cat([x[r, 12:16], x[r, 8:12]])
    co, ld = G.cout_out(c), c["out_ld"]
    buf = G.new_output(c)
    buf[: M * ld].view(M, ld)[:, :co] = x.to(G.TD[c["out_dtype"]])
    if fault == "pad_column_written":
        buf[(M // 2) * ld + co] = 0.0
    if fault == "row_past_m_written":
        buf[M * ld + 3] = 0.0
    return buf


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c["name"])
def test_the_checker_passes_the_emulated_kernel_and_fails_every_planted_fault(c):
    o = G.make_operands(c)
    ref, bound = G.reference(c, o)
    assert ref.shape == (G.rows(c), G.cout_out(c)) and bool((bound > 0).all())
    problems, worst = G.check_output(c, emulate(c, o), ref, bound)
    print(f"{c['name']}: emulation err / bound {worst:.3f}")
    assert not problems, problems
    for fault in FAULTS:
        if applicable(c, fault):
            problems, worst = G.check_output(c, emulate(c, o, fault), ref, bound)
            assert problems, f"{c['name']}: the checker lets '{fault}' through (worst err / bound {worst:.3g})"


def test_every_fault_is_planted_in_every_family_and_dtype():
    for fault in FAULTS:
        cells = {(G.family(c), c["dtype"]) for c in SMALL if applicable(c, fault)}
        assert len(cells) == 12, (fault, cells)


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("tag", ["silu", "gelu_tanh", "geglu"])
def test_the_activation_error_bound_holds_with_the_factor_two_to_spare(tag, fast):
    """e_act against the device formulas evaluated in fp32 on the CPU, over the tails (|x| up to 12) and the neighbourhood of 0: it holds by
    itself, so the factor 2 it carries inside the bound (gemm_tile_cases.reference) is spare."""
    tiny = torch.logspace(-30, -1, 2000)
    x = torch.cat([torch.linspace(-12, 12, 400001), tiny, -tiny, torch.zeros(1), torch.randn(100000, generator=torch.Generator().manual_seed(5)) * 3]).float()
    fn, exact = {"silu": (G.silu_device, F.silu), "gelu_tanh": (G.gelu_tanh_device, lambda t: F.gelu(t, approximate="tanh")),
                 "geglu": (G.gelu_erf_device, F.gelu)}[tag]
    err = (fn(x, fast).double() - exact(x.double())).abs()
    ratio = err / G.e_act(tag, x.double(), fast)
    i = int(ratio.argmax())
    print(f"{tag} fast={fast}: largest err / e_act {float(ratio[i]):.3f} at x = {float(x[i])!r}")
    assert float(ratio[i]) <= 1.0, (float(x[i]), float(err[i]))
    assert G.LIP >= 1.129


def test_the_bound_is_a_statement_about_rounding_not_about_magnitude():
    """A correctly rounded 16-bit output uses most of its bound (the rounding term is tight by nature), fp32 accumulation little of the
    accumulation term: the bound has no slack to hide a fault in."""
    c = G.by_name("pipe128_slim_bf16_none")
    o = G.make_operands(c)
    ref, bound = G.reference(c, o)
    _, worst = G.check_output(c, emulate(c, o), ref, bound)
    assert 0.5 < worst <= 1.0, worst
    c = G.by_name("pipe128_slim_f32_none")
    o = G.make_operands(c)
    ref, bound = G.reference(c, o)
    _, worst = G.check_output(c, emulate(c, o), ref, bound)
    assert worst < 0.2, worst
