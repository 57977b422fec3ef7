"""The parity cases of igemm_xreg and the register-staged igemm kernels (tests/gemm_small_cases.py) held to account without a GPU: every
case is routed to the kernel it names, the table covers every instance, fallback reason and mechanism it claims to, and the checker the
GPU test relies on passes a plain emulation of the kernels and fails each of a list of planted faults.  dc_igemm_variant runs on the host
alone, as in tests/test_igemm_dispatch.py; no DCAMD_* switch is set: these kernels need none."""
import pytest
import torch

import gemm_small_cases as S
import gemm_tile_cases as G
import test_gemm_tile_cases as T
import test_igemm_dispatch as D

FAKE = D.FAKE
F32, BF16, F16 = G.F32, G.BF16, G.F16
DTS = (F32, BF16, F16)
XREG = [c for c in S.CASES if "xreg" in c["expect"]]
REG128 = [c for c in S.CASES if S.family(c) == "reg128"]
REG32 = [c for c in S.CASES if S.family(c) == "reg32"]
LN = [c for c in S.CASES if c["ln"]]


def _variant(c, **over):
    mod = D._load_lib()
    kw = dict(S.igemm_fields(c, {f: FAKE for f in S.PTR_FIELDS}), **over)
    return mod.lib().dc_igemm_variant(mod.IgemmParams(**kw)).decode()


# ---- a. routing -----------------------------------------------------------------------------------------------------------------
def test_case_names_are_unique_and_no_switch_is_set():
    names = [c["name"] for c in S.CASES]
    assert len(names) == len(set(names))
    assert all(c["env"] == {} for c in S.CASES)
    for c in S.CASES:       # the tag says which epilogue runs
        assert c["act"] == S.TAG_ACT[c["tag"]] and (("gate" in c["use"]) == c["tag"].endswith("gate")), c["name"]
        assert c["fast_act"] == ("xreg" in c["expect"]), c["name"]        # igemm_epilogue: expf / IEEE divide in every type


@pytest.mark.parametrize("c", S.CASES, ids=lambda c: c["name"])
def test_every_case_is_routed_to_the_kernel_it_names(c):
    # the offset pointers are offset in the fake addresses too (S.pointers)
    assert _variant(c) == c["expect"], c["name"]


def test_47_rows_per_sample_with_a_row_vector_do_not_take_xreg():
    for name in ("xreg_bf16_a_k128_rv48", "xreg_f16_b_k320_rv48"):
        c = S.by_name(name)
        assert "xreg" in _variant(c)
        assert "xreg" not in _variant(c, Hin=47, Hout=47), name


@pytest.mark.parametrize("c", REG128, ids=lambda c: c["name"])
def test_each_fallback_reason_alone_sends_the_case_to_the_fallback(c):
    """With the named reason taken away the same problem takes a kernel with the lane-resident epilogue."""
    why = c["why"][0]
    co = S.cout_out(c)
    fix = {"cout_100": dict(Cout=104, out_ld=104, res_ld=104), "cout_99_partial_quad": dict(Cout=104, out_ld=104, rowvec_ld=104),
           "out_ld_99": dict(Cout=104, out_ld=104, res_ld=104), "out_ld_102": dict(out_ld=104), "out_ptr_plus_8": dict(out=FAKE), "bias_ptr_plus_4": dict(bias=FAKE),
           "rowvec_ld_mod_4": dict(rowvec_ld=co + 4), "res_f32_on_16bit": dict(res_dtype=c["dtype"]), "res_bf16_on_f32": dict(res_dtype=c["dtype"]),
           "res_f16_on_bf16": dict(res_dtype=c["dtype"]), "out_bf16_of_f32": dict(out_dtype=c["dtype"]), "out_f16_of_f32": dict(out_dtype=c["dtype"]),
           "out_f16_of_bf16": dict(out_dtype=c["dtype"]), "out_bf16_of_f16": dict(out_dtype=c["dtype"]), "silu_gate": dict(act=G.ACT_NONE),
           "gelu_tanh_gate": dict(act=G.ACT_NONE), "geglu_out_ld_84": dict(out_ld=88), "cout_260": dict(Cout=264, out_ld=264, res_ld=264, rowvec_ld=264)}[why]
    kw = S.igemm_fields(c, {f: FAKE for f in S.PTR_FIELDS})
    kw.update(fix)
    mod = D._load_lib()
    v = mod.lib().dc_igemm_variant(mod.IgemmParams(**kw)).decode()
    assert v.startswith(("igemm_pipe<", "igemm_xreg<", "igemm_wide8<")), (c["name"], why, v)


# ---- b. coverage ----------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_instance():
    # the 8 compiled igemm_xreg instances (dtype x GEGLU x layout), each with and without the row LayerNorm
    have = {(c["dtype"], c["act"] == G.ACT_GEGLU, S.family(c), bool(c["ln"])) for c in XREG}
    want = {(dt, gg, lay, ln) for dt in (BF16, F16) for gg in (False, True) for lay in ("xreg96", "xreg64") for ln in (False, True)}
    assert have == want, want - have
    # the 6 igemm_kernel instances x the four forms
    have = {(S.family(c), c["dtype"], c["form"]) for c in REG128 + REG32}
    want = {(f, dt, form) for f in ("reg128", "reg32") for dt in DTS for form in S.FORMS}
    assert have == want, want - have
    # every fallback reason in each dtype it can occur in, one reason per case
    have = {(c["why"][0], c["dtype"]) for c in REG128 if c["why"][0] in S.REASONS}
    want = {(why, dt) for why, (dts, _) in S.REASONS.items() for dt in dts}
    assert have == want and all(len(c["why"]) == 1 for c in REG128), want - have
    # every epilogue branch of igemm_epilogue with every dtype: load_as / store_as across the three types, vector and scalar stores, GEGLU,
    # activation followed by gate
    for dt in DTS:
        mine = [c for c in REG128 + REG32 if c["dtype"] == dt]
        assert {c["tag"] for c in mine} >= {"none", "silu", "gelu_tanh", "geglu", "gate", "silu_gate", "gelu_tanh_gate"}, dt
        assert {c["out_dtype"] for c in mine} == {F32, BF16, F16}, dt
        assert any(c["res_dtype"] != dt and "residual" in c["use"] for c in mine) and any(c["res_dtype"] == dt and "residual" in c["use"] for c in mine), dt
        assert any(c["out_ld"] & 3 for c in mine) and any((c["out_ld"] & 3) == 0 and S.cout_out(c) % 4 for c in mine), dt      # scalar everywhere / one partial quad
        assert any("rowvec_map" in c["use"] for c in mine) and any("gate_map" in c["use"] for c in mine) and any("res_map" in c["use"] for c in mine), dt
    assert {c["res_dtype"] for c in REG128 if "residual" in c["use"]} == {F32, BF16, F16} and {c["out_dtype"] for c in REG128} == {F32, BF16, F16}
    assert any(c["tag"] == "geglu" and (c["Cout"] % 128) and c["out_ld"] % 8 for c in REG128)          # a part-empty N tile under GEGLU: the bias reads stay inside


def test_register_staged_cases_have_the_properties_they_are_there_for():
    """Computed from the table: extents, M, tile counts and orders, K-step counts, seams, and the 128x32 tile's own list."""
    reg = REG128 + REG32
    tiles_m = lambda c: (S.rows(c) + 127) // 128
    tiles_n = lambda c: (c["Cout"] + c["tile_n"] - 1) // c["tile_n"]
    nk = lambda c: S.k_total(c) // G.BKE[c["dtype"]]
    wbytes = lambda c: tiles_n(c) * c["tile_n"] * S.k_total(c) * S.esize(c["dtype"])
    n_fast = lambda c: tiles_n(c) > 1 and (wbytes(c) <= 2 << 20 or (c["taps"] == 1 and wbytes(c) <= 16 << 20))
    for c in reg:
        if c["form"] != "tap1" and "8x8" not in c["name"]:
            assert (c["Hin"], c["Win"]) in ((5, 7), (6, 10)), c["name"]
    for fam in (REG128, REG32):
        assert {S.rows(c) for c in fam} >= {105, 300}
        big = [c for c in fam if tiles_m(c) == 11]
        assert any((tiles_m(c) * tiles_n(c)) % 8 and n_fast(c) for c in big), "11 M tiles, N fastest, a remainder in the XCD map"
    assert any(tiles_m(c) == 11 and (tiles_m(c) * tiles_n(c)) % 8 and not n_fast(c) and tiles_n(c) > 1 and c["taps"] == 9 and wbytes(c) > 2 << 20 for c in REG128)
    for dt in DTS:
        mine = [c for c in reg if c["dtype"] == dt]
        assert any(nk(c) == 1 and c["taps"] == 1 for c in mine), dt                    # the main loop's `more` is false at once
        assert {nk(c) for c in mine} >= {1, 2, 9, 27}, (dt, {nk(c) for c in mine})
        assert any(c["C1"] and (c["C0"] // G.BKE[dt]) % 2 == 1 and {"map0", "map1"} <= c["use"] for c in mine), dt      # seam after an odd number of K-steps
        assert any(c["C1"] and c["taps"] == 9 for c in mine) and any(c["C1"] and c["taps"] == 1 for c in mine), dt
    # the 128x32 tile: the DiT final projection, conv_out, Cout 3 / 40, SiLU, residual, sample maps — in every dtype
    for dt in DTS:
        mine = [c for c in REG32 if c["dtype"] == dt]
        dit = {c["C0"] for c in mine if c["taps"] == 1 and c["Cout"] == 32 and "bias" in c["use"] and c["out_dtype"] == F32 and c["Hout"] == 50}
        assert dit >= ({192, 384} if dt == F32 else {384, 768, 1152}), (dt, dit)
        assert any(c["form"] == "c3s1" and (c["Hin"], c["Win"]) == (8, 8) and c["C1"] and c["Cout"] == 4 and c["out_dtype"] == F32 for c in mine), dt
        assert any(c["Cout"] == 3 for c in mine) and any(c["Cout"] == 40 for c in mine) and any(c["tag"] == "silu" for c in mine), dt
        assert any("residual" in c["use"] for c in mine) and any({"map0", "map1"} <= c["use"] for c in mine) and any("res_map" in c["use"] for c in mine), dt


def test_xreg_cases_have_the_properties_they_are_there_for():
    """What the igemm_xreg list promises, computed from the cases: slice counts against the ring, seams, ragged M against either layout,
    samples wandering through the waves, epilogue paths, channel tails, the LayerNorm inputs."""
    tiles_n = lambda c: (c["Cout"] + 127) // 128
    spn = lambda c: S.k_total(c) // 64
    for dt in (BF16, F16):
        mine = [c for c in XREG if c["dtype"] == dt]
        assert all(c["taps"] == 1 and tiles_n(c) >= 3 and S.rows(c) <= 400 and c["Cout"] <= 648 for c in mine)
        assert {spn(c) for c in mine} >= {1, 2, 3, 4, 5, 7, 8}
        assert any(spn(c) == 1 and tiles_n(c) == 3 for c in mine) and any(spn(c) == 1 and tiles_n(c) == 5 for c in mine)     # Q = 3 = prefetch distance; 5 tiles
        assert {(c["C0"], c["C1"]) for c in mine if c["C1"]} >= {(64, 128), (192, 64), (256, 64)}
        for c in mine:
            if c["C1"]:
                o = S.make_operands(c)
                assert c["n_src"] < c["n_img"] and not torch.equal(o["map0"], o["map1"]), c["name"]
        for lay, wg in (("xreg96", 96), ("xreg64", 64)):
            lm = [c for c in mine if S.family(c) == lay]
            half = wg // 2
            assert any(S.rows(c) == half + 2 and c["n_img"] == 1 for c in lm), lay                      # the second wave row holds 2 real rows
            assert any(S.rows(c) == wg + 1 for c in lm), lay
            assert any(0 < S.rows(c) % wg <= half for c in lm if S.rows(c) > wg), lay                   # the last workgroup's second wave row is past M
            rv = {(c["Hout"], "rowvec_map" in c["use"]) for c in lm if "rowvec" in c["use"]}
            assert {h for h, _ in rv} >= {48, 49, 50} and {m for _, m in rv} == {False, True}, (lay, rv)
            assert any("rowvec" in c["use"] and c["Hout"] % half for c in lm), lay                       # a wave that holds two samples
            assert any("res_map" in c["use"] and c["res_ld"] > S.cout_out(c) for c in lm) and any(c["out_ld"] > S.cout_out(c) for c in lm), lay
            assert any(c["out_dtype"] == F32 for c in lm) and any(c["ld0"] > c["C0"] and c["col0"] for c in lm), lay
            ln = [c for c in lm if c["ln"]]
            assert any(c["ln"] == "tiny" for c in ln) and any(c["const_row"] for c in ln) and any(c["ln"] == "offset" for c in ln), lay
            assert any(c["ln"] == "tiny" and c["act"] == G.ACT_GEGLU for c in ln), lay
        assert any(c["Cout"] == 264 for c in mine) and any(c["Cout"] == 648 for c in mine)
        gg = [c for c in mine if c["act"] == G.ACT_GEGLU]
        assert any(c["Cout"] == 288 and "bias" in c["use"] for c in gg) and any("bias" not in c["use"] for c in gg)
        ln = [c for c in mine if c["ln"]]
        assert any("residual" in c["use"] for c in ln) and any(S.rows(c) % (96 if S.family(c) == "xreg96" else 64) for c in ln)
    for c in LN:       # what the inputs are there for, from the operands themselves
        o = S.make_operands(c)
        x = S.a_matrix(c, o)
        var, mean = x.var(1, unbiased=False), x.mean(1)
        if c["ln"] == "tiny":
            assert 5e-5 < float(var.median()) < 2e-4 and c["ln_eps"] == 1e-5, (c["name"], float(var.median()))
        if c["ln"] == "offset":
            assert 95 < float(mean.median()) < 105 and 0.5 < float(var.median()) < 2, c["name"]
        if c["const_row"]:
            rows_ = S.const_rows(c, o)
            assert rows_ and all(float(var[r]) == 0.0 for r in rows_), c["name"]


# ---- c. the checker checks ------------------------------------------------------------------------------------------------------
FAULTS = T.FAULTS + ["slice_of_previous_tile", "rowvec_of_first_sample_only", "ln_eps_dropped", "ln_mean_of_neighbour_row", "ln_not_rounded",
                     "seam_chunk_from_src0", "residual_read_as_compute_type", "gate_before_activation", "tail_quad_dropped"]


def applicable(c, fault):
    use, co, xr = c["use"], S.cout_out(c), "xreg" in c["expect"]
    if fault in T.FAULTS:
        tables = {"residual_of_next_sample": c["n_res"] if "res_map" in use else c["n_img"],          # a table of one row has no neighbour
                  "vector_of_next_sample": min(c["n_vec"] if m in use else c["n_img"] for m in ("rowvec_map", "gate_map"))}
        return T.applicable(c, fault) and (fault != "channels_c_c4_swapped" or co >= 16) and tables.get(fault, 2) > 1
    return {"slice_of_previous_tile": xr,                                              # only igemm_xreg streams weight slices through a ring
            "rowvec_of_first_sample_only": xr and "rowvec" in use and c["Hout"] % S.wave_rows(c) != 0,
            # eps = 1e-5 against a row variance of 9 or 1 moves the operand by 1e-6 relative: below every rounding.  Against 1e-4: by 5 %
            "ln_eps_dropped": c["ln"] == "tiny" or c["const_row"],
            "ln_mean_of_neighbour_row": bool(c["ln"]),
            # an unrounded operand differs from the rounded one by half a spacing at most: behind a 16-bit output's own rounding that is
            # within the bound by nature, so the fault is planted where the output is fp32.  f16: half a spacing is 2^-12 relative, K
            # such errors of random sign add up as sqrt(K) while the bound's accumulation term 2 (K + 8) 2^-24 |A| |W|^T grows as K
            # against a sum of sqrt(K): from K = 448 on the fault lies inside it by nature
            "ln_not_rounded": bool(c["ln"]) and c["out_dtype"] == F32 and (c["dtype"] == BF16 or c["C0"] <= 320),
            "seam_chunk_from_src0": c["C1"] > 0,
            "residual_read_as_compute_type": "residual" in use and c["res_dtype"] != c["dtype"],
            "gate_before_activation": c["act"] != G.ACT_NONE and "gate" in use,
            "tail_quad_dropped": co % 4 != 0}[fault]


def emulate(c, o, fault=None):
    """The kernel, plainly: operands as the compute type holds them (a LayerNorm case: the kernel's two-pass fp32 LayerNorm rounded to the
    type), fp32 accumulation one K-step at a time, the epilogue in fp32 in the documented order with the device's activation formulas, the
    output rounded to its type into a sentinel-filled buffer."""
    dt, g = c["dtype"], G.BKE[c["dtype"]]
    if fault == "seam_chunk_from_src0":       # the first K-step of src1 comes from src0 (same sample map as src0, same channel offset)
        x0 = o["x0"][o["map0"].long()] if "map0" in o else o["x0"]
        x1 = (o["x1"][o["map1"].long()] if "map1" in o else o["x1"]).clone()
        x1[..., :g] = x0[..., :g]
        o = {k: v for k, v in o.items() if k not in ("map0", "map1")}
        o.update(x0=x0, x1=x1)
    A, W = G.a_matrix(c, o, torch.float32), o["w"]
    if c["ln"]:
        A = S.ln_device(c, A, eps=0.0 if fault == "ln_eps_dropped" else None, mean_shift=1 if fault == "ln_mean_of_neighbour_row" else 0,
                        rounded=fault != "ln_not_rounded")
    M, K = A.shape
    HWo = c["Hout"] * c["Wout"]
    gg = c["act"] == G.ACT_GEGLU
    acc = torch.zeros(M, c["Cout"])
    for k0 in range(0, K, g):
        Wk = W[:, k0:k0 + g]
        if fault == "slice_of_previous_tile" and k0 == 0:
            # N tile 1 (channels 128..255; GEGLU: value and gate rows 64..127 of either half) multiplies the first slice of tile 0's rows
            Wk = Wk.clone()
            if gg:
                h = c["Cout"] // 2
                Wk[64:128], Wk[h + 64:h + 128] = W[0:64, :g], W[h:h + 64, :g]
            else:
                Wk[128:256] = W[0:128, :g]
        part = A[:, k0:k0 + g] @ Wk.t()
        if fault == "ktile_dropped" and k0 == g * (K // g // 2):
            part[M // 2] = 0.0
        acc += part
    samp = torch.arange(M) // HWo

    def table(name, mname, shift, first_of_wave=False):      # shift: the table row of the neighbouring sample
        s = samp
        if first_of_wave:                                      # every row of a wave takes the sample of the wave's first row
            wr = S.wave_rows(c)
            s = samp[(torch.arange(M) // wr) * wr]
        idx = o[mname].long()[s] if mname in o else s
        return o[name][(idx + shift) % o[name].shape[0]]
    shift = 1 if fault == "vector_of_next_sample" else 0
    late = fault == "bias_after_activation"
    x = acc
    pre_terms = []
    if "bias" in o:
        pre_terms.append(o["bias"])
    if "rowvec" in o and not gg:
        pre_terms.append(table("rowvec", "rowvec_map", shift, fault == "rowvec_of_first_sample_only"))
    if not late:
        for t in pre_terms:
            x = x + t
    gate = table("gate", "gate_map", shift) if "gate" in o else None
    if fault == "gate_before_activation":
        x, gate = x * gate, None
    fast = c["fast_act"]
    if c["act"] == G.ACT_SILU:
        x = G.silu_device(x, fast)
    elif c["act"] == G.ACT_GELU_TANH:
        x = G.gelu_tanh_device(x, fast)
    elif gg:
        u, gv = x.chunk(2, dim=-1)
        x = u * G.gelu_erf_device(gv, fast)
    if late:
        for t in pre_terms:
            x = x + (t if not gg else t.chunk(2, dim=-1)[0])
    if gate is not None:
        x = x * gate
    if "residual" in o:
        res = o["residual"]
        if fault == "residual_read_as_compute_type":          # the same bytes, taken as elements of the compute type
            raw = res.to(G.TD[c["res_dtype"]]).contiguous().view(-1).view(G.TD[dt])
            res = raw.repeat(2)[: res.numel()].float().view(res.shape)
        rs = 1 if fault == "residual_of_next_sample" else 0
        ridx = o["res_map"].long()[samp] if "res_map" in o else samp
        x = x + res[(ridx + rs) % res.shape[0], torch.arange(M) % HWo]
    if fault == "channels_c_c4_swapped":
        r = M // 3
        x = x.clone()
        x[r, 8:16] = torch.cat([x[r, 12:16], x[r, 8:12]])
    co, ld = S.cout_out(c), c["out_ld"]
    buf = S.new_output(c)
    keep = co - co % 4 if fault == "tail_quad_dropped" else co
    buf[: M * ld].view(M, ld)[:, :keep] = x.to(G.TD[c["out_dtype"]])[:, :keep]
    if fault == "pad_column_written":
        buf[(M // 2) * ld + co] = 0.0
    if fault == "row_past_m_written":
        buf[M * ld + 3] = 0.0
    return buf


@pytest.mark.parametrize("c", S.CASES, ids=lambda c: c["name"])
def test_the_checker_passes_the_emulated_kernel_and_fails_every_planted_fault(c):
    o = S.make_operands(c)
    ref, bound = S.reference(c, o)
    assert ref.shape == (S.rows(c), S.cout_out(c)) and bool((bound > 0).all())
    problems, worst = S.check_output(c, emulate(c, o), ref, bound)
    print(f"{c['name']}: emulation err / bound {worst:.3f}")
    assert not problems, problems
    for r in S.const_rows(c, o):          # variance 0: the normalised row is exactly 0 and the output bias (+ residual) alone
        want = (o["bias"].double() if "bias" in o else 0.0) + (S.residual_rows(c, o)[r].double() if "residual" in o else 0.0)
        assert torch.equal(ref[r], want + torch.zeros_like(ref[r])), c["name"]
    for fault in FAULTS:
        if applicable(c, fault):
            problems, worst = S.check_output(c, emulate(c, o, fault), ref, bound)
            assert problems, f"{c['name']}: the checker lets '{fault}' through (worst err / bound {worst:.3g})"


def test_every_fault_is_planted_in_every_family_and_dtype_it_can_occur_in():
    fams, x16 = ("xreg96", "xreg64", "reg128", "reg32"), ("xreg96", "xreg64")
    everywhere = {(f, dt) for f in fams for dt in ((BF16, F16) if f in x16 else DTS)}
    xr = {(f, dt) for f in x16 for dt in (BF16, F16)}
    want = {"ktile_dropped": everywhere, "residual_of_next_sample": everywhere, "vector_of_next_sample": everywhere, "bias_after_activation": everywhere,
            "channels_c_c4_swapped": everywhere, "pad_column_written": everywhere, "row_past_m_written": everywhere,
            "slice_of_previous_tile": xr, "rowvec_of_first_sample_only": xr,                         # the ring and TWO_SAMP are igemm_xreg's alone
            "ln_eps_dropped": xr, "ln_mean_of_neighbour_row": xr, "ln_not_rounded": xr,              # ... and so is the row LayerNorm
            "seam_chunk_from_src0": everywhere,
            "residual_read_as_compute_type": {("reg128", dt) for dt in DTS},                         # the lane epilogue admits the compute type only
            "gate_before_activation": {("reg128", dt) for dt in DTS},                                # an activation with a gate is a fallback reason
            "tail_quad_dropped": {(f, dt) for f in ("reg128", "reg32") for dt in DTS}}               # the lane epilogue needs channels % 8 == 0
    assert set(want) == set(FAULTS)
    for fault in FAULTS:
        cells = {(S.family(c), c["dtype"]) for c in S.CASES if applicable(c, fault)}
        assert cells == want[fault], (fault, want[fault] ^ cells)


# ---- d. the bound -----------------------------------------------------------------------------------------------------------------
def test_the_bound_is_a_statement_about_rounding_not_about_magnitude():
    """A correctly rounded 16-bit output uses most of its bound (the rounding term is tight by nature), fp32 accumulation little of the
    accumulation term: the bound has no slack to hide a fault in."""
    for name in ("xreg_bf16_a_k128_rv48", "xreg_f16_b_k448_m65", "reg128_bf16_c3s1_cout_100", "reg128_f32_tap1_out_bf16_of_f32", "reg32_f16_c3s1_cout3_out_ld5",
                 "xreg_bf16_a_ln_k192_res_const_row", "xreg_f16_a_ln_k128_tiny_var"):
        c = S.by_name(name)
        o = S.make_operands(c)
        ref, bound = S.reference(c, o)
        _, worst = S.check_output(c, emulate(c, o), ref, bound)
        assert c["out_dtype"] != F32 and 0.5 < worst <= 1.0, (name, worst)
    for c in S.CASES:
        if c["dtype"] == F32 and c["out_dtype"] == F32:
            o = S.make_operands(c)
            ref, bound = S.reference(c, o)
            _, worst = S.check_output(c, emulate(c, o), ref, bound)
            assert worst < 0.2, (c["name"], worst)


@pytest.mark.parametrize("c", LN, ids=lambda c: c["name"])
def test_the_layernorm_ambiguity_is_a_small_part_of_the_bound(c):
    """From the reference alone: the median over output elements of (ambiguity term / bound) is at most 0.5 — the flagged operand elements
    do not dilute the bound — and the plain fp32 emulation of the kernel's LayerNorm differs from the correctly rounded operand on flagged
    elements only."""
    o = S.make_operands(c)
    ref, bound, d = S.reference(c, o, detail=True)
    med = float((d["amb"] / bound).median())
    a, amb, flagged = S.ln_prologue(c, o)
    dev = S.ln_device(c, S.a_matrix(c, o, torch.float32)).double()
    differ = dev != a
    print(f"{c['name']}: flagged {100 * d['flagged_share']:.2f} % of the operand, median ambiguity / bound {med:.3f}, the emulation differs on "
          f"{100 * float(differ.double().mean()):.4f} %")
    assert med <= 0.5, (c["name"], med)
    assert d["flagged_share"] < 0.2, (c["name"], d["flagged_share"])
    assert not bool((differ & ~flagged).any()) and bool(((dev - a).abs() <= amb).all()), c["name"]
