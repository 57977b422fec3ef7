"""The dc_tblock_front parity cases (tests/tblock_cases.py) held to account without a GPU: the table covers what it claims to, the exact
cases meet the preconditions that make them exact, two independent CPU emulations of the kernel reproduce every exact case bit for bit and
stay at or below KAPPA / 2 on every full-chain case (that IS the measurement of KAPPA), and the checker the GPU test relies on fails each
of a list of faults planted into the emulations, in every case stated as sensitive to it.  dc_tblock_front_ok runs on the host alone."""
import math

import pytest
import torch

import tblock_cases as G
import test_igemm_dispatch as D

FAKE = D.FAKE
SEEDS = (None, 1, 2, 3)          # operand draws per full-chain case over which KAPPA is measured (n = 513: the first alone)
SMALL = [c for c in G.CASES if c["n"] <= 8]
CHAIN = [c for c in G.CASES if c["kind"] == "chain"]
EXACT = [c for c in G.CASES if c["kind"] == "exact"]
HOWS = ("chunk32", "plain")


# ---- a. the table -----------------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_claims():
    names = [c["name"] for c in G.CASES]
    assert len(names) == len(set(names))
    assert all(c["why"] and c["layout"] == {k: c[k] for k in ("ldx", "ld_out", "rowvec_ld")} for c in G.CASES)
    for kind, cases in (("exact", EXACT), ("chain", CHAIN)):
        assert {(c["dtype"], c["heads"]) for c in cases} == {(dt, h) for dt in G.DTS for h in (4, 8)}, kind
    assert {(c["mode"], c["dtype"], c["heads"]) for c in CHAIN} == {(m, dt, h) for m in G.CHAIN_MODES for dt in G.DTS for h in (4, 8)}
    assert {(c["mode"], c["dtype"]) for c in EXACT} == {(m, dt) for m in G.EXACT_MODES for dt in G.DTS}
    assert {(c["mode"], c["heads"]) for c in EXACT if c["mode"] != "epilogue_exact"} == {(m, h) for m in ("one_hot", "uniform") for h in (4, 8)}
    for dt in G.DTS:
        mine = [c for c in G.CASES if c["dtype"] == dt]
        # every pointer subset engine.PlanBuilder.tblock_front can emit (bo always; the class vector none, per sample, or through a map), and null bo
        uses = {c["use"] for c in mine}
        assert uses >= {frozenset(u) for u in (("bo",), ("bo", "rowvec"), ("bo", "rowvec", "rowvec_map"), ("rowvec", "rowvec_map"), ())}, (dt, uses)
        assert any(c["ldx"] > G.C_CH for c in mine) and any(c["ld_out"] > G.C_CH for c in mine) and any(c["rowvec_ld"] > G.C_CH for c in mine)
        assert any(c["ldx"] == 264 and c["ld_out"] == 272 and c["kind"] == "chain" for c in mine)
        assert {1, 3, 8, 513} <= {c["n"] for c in mine if c["kind"] == "chain"} and any(c["n"] == 1 for c in mine if c["kind"] == "exact")
        assert all(c["n"] <= 8 or c["n"] == 513 for c in mine) and sum(c["n"] == 513 for c in mine) == 1
        assert any(c["mode"] == "odd_scale" and abs(c["scale"] * math.sqrt(G.C_CH // c["heads"]) - 0.7) < 1e-12 for c in mine)
        assert all((c["ln_eps"] == 1e-3) == (c["mode"] == "ln_flat") for c in mine)
    for c in G.CASES:          # the engine's conventions for absent pointers; tables read through a map repeat and reorder
        if "rowvec" not in c["use"]:
            assert c["rowvec_ld"] == 0 and c["n_vec"] == 0
        elif "rowvec_map" not in c["use"]:
            assert c["n_vec"] == c["n"]
        else:
            v = G._rowvec_map(c["n"], c["n_vec"]).tolist()
            assert max(v) < c["n_vec"] and v != [i % c["n_vec"] for i in range(c["n"])], (c["name"], v)
            assert c["n"] < 3 or (len(set(v)) < len(v) and v != sorted(v)), (c["name"], v)
    kinds = [(G.by_name(n)["kind"], G.by_name(n)["mode"], G.by_name(n)["dtype"]) for n in G.REPEAT_CASES]
    assert sorted(kinds) == sorted([("exact", "one_hot", dt) for dt in G.DTS] + [("chain", "peaked", dt) for dt in G.DTS])


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_every_case_is_a_shape_the_kernel_serves(c):
    mod = D._load_lib()
    p = mod.TblockFrontParams(**G.front_fields(c, {f: FAKE for f in G.PTR_FIELDS}))
    assert mod.lib().dc_tblock_front_ok(p) == 1


@pytest.mark.parametrize("c", EXACT, ids=lambda c: c["name"])
def test_exact_cases_meet_their_preconditions(c):
    """What makes every accumulation exact in any order and every rounding point but the last a no-op, on the operands alone."""
    o = G.make_operands(c)
    td = G.TD[c["dtype"]]
    holds = lambda t: torch.equal(t.to(td).double(), t.double())
    x, Wp, Wqkv, Wo = o["x"].double(), o["Wp"].double(), o["Wqkv"].double(), o["Wo"].double()
    d = G.C_CH // c["heads"]
    h = x @ Wp.t() + o["bp"].double()
    # h: a multiple of 2^-2 far below 256 that the type holds; its partial sums are integers below 2^24
    assert torch.equal(h * 4, (h * 4).round()) and float(h.abs().max()) < 256 and holds(h)
    assert torch.equal(x, x.round()) and torch.equal(Wp, Wp.round()) and float((x.abs() @ Wp.abs().t()).max()) < 2 ** 24
    bo = o["bo"].double() if "bo" in o else torch.zeros(G.C_CH, dtype=torch.float64)
    rv = G.rowvec_rows(c, o)
    assert torch.equal(bo * 256, (bo * 256).round()) and torch.equal(rv * 256, (rv * 256).round()) and torch.equal(o["bp"] * 4, (o["bp"] * 4).round())
    if c["mode"] == "epilogue_exact":
        assert float(x.abs().max()) <= 3 and bool(((Wp != 0).sum(1) == 8).all()) and set(Wp.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert float(h.abs().max()) < 32 and not bool(Wqkv[2 * G.C_CH:].any())            # V = 0: o = 0 whatever p is
        assert float(Wqkv[: 2 * G.C_CH].abs().max()) > 0 and not torch.equal(Wo, Wo.round())  # the softmax and to_out still run on noise
        out = (bo + rv) + h
    else:
        eye = torch.eye(G.C_CH, dtype=torch.float64)
        assert torch.equal(Wp, eye) and not o["bp"].any() and torch.equal(o["ln_g"], torch.ones(G.C_CH)) and not o["ln_b"].any() and c["ln_eps"] == 1e-5
        # balanced +-1 rows: mean 0 and variance 1 exactly, hn = +-1 / sqrt(1 + 1e-5), which both types round to +-1 (with an fp32 ulp to spare)
        assert set(x.unique().tolist()) == {-1.0, 1.0} and not bool(x.sum(-1).any())
        for r in (1.0 / math.sqrt(1.0 + 1e-5), (1.0 / math.sqrt(1.0 + 1e-5)) * (1 - 2.0 ** -20)):
            assert float(torch.tensor(r).to(td)) == 1.0
        assert torch.equal(Wqkv[G.C_CH: 2 * G.C_CH], eye) and torch.equal(Wo, Wo.round()) and float(Wo.abs().sum(1).max()) <= 8
        if c["mode"] == "one_hot":
            beta = G.BETA[d]
            assert torch.equal(Wqkv[: G.C_CH], beta * eye) and math.log2(beta) == round(math.log2(beta)) and holds(torch.tensor(beta))
            gap = G.one_hot_gap(c, o["x"])
            assert gap > G.GAP_LOG2, gap                                  # every other key's p underflows fp32 (2^-149): p is one-hot, ps = 1
            Wv = Wqkv[2 * G.C_CH:]
            assert torch.equal(Wv, Wv.round()) and float(Wv.abs().sum(1).max()) <= 4
            ov = x @ Wv.t()
            # beta d is a power of two: max * sc2 is exact in fp32, the own key's exponent is exactly 0
            assert math.log2(beta * d) == round(math.log2(beta * d))
            # the rows of v differ between tokens: another token's row is another result
            assert all(len({tuple(r) for r in ov[s].tolist()}) == G.L_TOK for s in range(c["n"]))
        else:
            assert not bool(Wqkv[: G.C_CH].any()) and torch.equal(Wqkv[2 * G.C_CH:], eye)
            cs = x.sum(1)
            assert torch.equal(cs, (cs / 64).round() * 64)                # column sums: multiples of 64, the mean an integer
            ov = (cs / 64)[:, None, :].expand(-1, G.L_TOK, -1)
            # a constant column in every 4-channel lane slot of every fragment: a wrong sum shows wherever it happens
            assert bool((cs.view(c["n"], 64, 4).abs().amax(-1) == 64).all())
        assert holds(ov) and float((ov.abs() @ Wo.abs().t()).max()) <= 64
        out = ((ov @ Wo.t() + bo) + rv) + h
    # the last sum is exact in fp32 (multiples of 2^-8 below 2^15) and a real rounding in the 16-bit type
    assert torch.equal(out * 256, (out * 256).round()) and float(out.abs().max()) < 2 ** 15
    assert not holds(out), "the output rounding must be a real rounding somewhere"
    bits = G.expected_bits(c, o)
    assert torch.equal(bits, G._bits(out.to(td)).reshape(-1, G.C_CH))
    # and the fp64 reference of the chain cases, rounded, says the same
    ref, _, mid = G.reference(c, o)
    assert torch.equal(G._bits(ref.to(td)), bits)
    if c["mode"] != "epilogue_exact":
        assert torch.equal(mid["hn"], x) and torch.equal(mid["o"], ov.double())


def test_chain_modes_have_the_data_they_are_there_for():
    for c in CHAIN:
        if c["n"] > 8:
            continue
        o = G.make_operands(c)
        ref, S, mid = G.reference(c, o)
        h, logits = mid["h"], mid["logits"]
        spread = float((logits.amax(-1) - logits.amin(-1)).max())
        how_much_h = float((h.abs().reshape(-1, G.C_CH) / S).median())
        sp = 2.0 * G.U_OUT[c["dtype"]]
        if c["mode"] == "peaked":
            assert float(logits.abs().max()) > 30 and spread > 40, (c["name"], spread)
        elif c["mode"] == "attn_dominant":
            assert how_much_h < 0.02 and not c["use"], (c["name"], how_much_h)
        elif c["mode"] == "ln_offset":
            assert float((h.mean(-1).abs() / h.std(-1)).min()) > 5, c["name"]
        elif c["mode"] == "ln_flat":
            var = h.var(-1, unbiased=False)
            assert float(((h - 1.0).abs().amax(-1) / sp).max()) <= 8 and float(var.max()) < 0.1 * c["ln_eps"], c["name"]
        else:
            assert float(logits.abs().max()) < 10 and how_much_h > 0.1


# ---- b. the emulations, KAPPA, the planted faults -----------------------------------------------------------------------------------
# fault -> (which cases must catch it, why the others cannot)
SENSITIVE = {
    "k_heads_swapped": (lambda c: c["heads"] == 8 and (c["mode"] == "one_hot" or (c["kind"] == "chain" and c["mode"] != "ln_flat")),
                        "needs two heads per wave and scores that depend on the key"),
    "scale_other_width": (lambda c: c["kind"] == "chain" and c["mode"] != "ln_flat",
                          "exact cases have a gap of > 160 (one-hot at either scale) or zero scores; ln_flat's logits are below 0.5"),
    "quarter_max": (lambda c: c["mode"] == "one_hot" or (c["kind"] == "chain" and c["mode"] != "ln_flat"), "needs scores that differ between lane groups"),
    "sum48": (lambda c: c["mode"] != "epilogue_exact", "epilogue_exact has o = 0 at any row sum"),
    "p_tiles_swapped": (lambda c: c["mode"] == "one_hot" or (c["kind"] == "chain" and c["mode"] != "ln_flat"), "needs p that differs between keys"),
    "to_out_chunk0_for_7": (lambda c: c["mode"] != "epilogue_exact", "epilogue_exact has o = 0"),
    "rowvec_unmapped": (lambda c: "rowvec_map" in c["use"], "needs a map"),
    "h_shifted_16": (lambda c: True, ""),
    "ln_b_dropped": (lambda c: c["kind"] == "chain", "exact cases have ln_b = 0 or V = 0"),
    "ln_eps_dropped": (lambda c: c["mode"] in ("ln_flat", "attn_dominant"), "needs a row variance not far above eps: ln_flat by design, attn_dominant through its small h"),
    "bo_dropped": (lambda c: "bo" in c["use"], "needs bo"),
    "v_from_h": (lambda c: c["kind"] == "chain", "one_hot / uniform have h = hn, epilogue_exact V = 0"),
}


def sensitive(c, fault):
    return c["n"] <= 8 and SENSITIVE[fault][0](c)


def test_every_fault_is_caught_somewhere_and_the_lists_are_what_they_say():
    assert set(SENSITIVE) == set(G.FAULTS) and len(G.FAULTS) == 12
    for fault in G.FAULTS:
        cells = [c for c in SMALL if sensitive(c, fault)]
        assert cells, fault
        assert {c["dtype"] for c in cells} == set(G.DTS), fault
    assert any(sensitive(c, "ln_eps_dropped") and c["mode"] == "ln_flat" for c in SMALL)
    # the faults the exact cases are there for are caught by an exact case, bit for bit
    for fault in ("k_heads_swapped", "quarter_max", "sum48", "p_tiles_swapped", "to_out_chunk0_for_7", "rowvec_unmapped", "h_shifted_16", "bo_dropped"):
        assert any(sensitive(c, fault) for c in EXACT), fault


def test_kappa_is_twice_the_recorded_emulation_maximum():
    top = max(G.RECORDED["emulation"].values())
    assert set(G.RECORDED["emulation"]) == set(G.RECORDED["device"]) == set(G.CHAIN_MODES)
    assert G.KAPPA == pytest.approx(2.0 * math.ceil(top * 10.0) / 10.0, abs=1e-12)
    for mode, dev in G.RECORDED["device"].items():          # the device's ratios are records, never the source of KAPPA
        assert dev is None or dev <= G.KAPPA


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_the_emulations_pass_and_every_planted_fault_fails(c):
    cc, o, ref, S, want = G.prepared(c["name"])
    for how in HOWS:
        val = G.emulate(c, o, how)
        problems, worst = G.check_output(c, G.to_buffer(c, val), ref, want)
        if c["kind"] == "exact":
            print(f"{c['name']} [{how}]: {int(worst)} representable values off")
            assert not problems and worst == 0, (how, problems)
        else:
            ratios = [G.forward_ratio(c, val, ref, S)]
            for seed in SEEDS[1:] if c["n"] <= 8 else ():
                o2 = G.make_operands(c, seed)
                ref2, S2, _ = G.reference(c, o2)
                ratios.append(G.forward_ratio(c, G.emulate(c, o2, how), ref2, S2))
            print(f"{c['name']} [{how}]: forward error / (u S) " + " ".join(f"{r:.3f}" for r in ratios) + f" (recorded {G.RECORDED['emulation'][c['mode']]}, "
                  f"KAPPA / 2 = {G.KAPPA / 2}); err / bound {worst:.3f}")
            assert not problems, (how, problems)
            assert max(ratios) <= G.KAPPA / 2, (how, ratios)
    for fault in G.FAULTS:
        if not sensitive(c, fault):
            continue
        for how in HOWS:
            problems, worst = G.check_output(c, G.to_buffer(c, G.emulate(c, o, how, fault)), ref, want)
            assert problems, f"{c['name']} [{how}]: the checker lets '{fault}' through (worst {worst:.3g})"


# ---- c. poison and sentinel -----------------------------------------------------------------------------------------------------------
POISON_CASES = [next(c["name"] for c in CHAIN if c["dtype"] == dt and c["ldx"] > G.C_CH and c["rowvec_ld"] > G.C_CH) for dt in G.DTS] + \
               ["one_hot_f16_h4", "epilogue_exact_bf16_rowvec_ld260", "epilogue_exact_f16_no_rowvec"]


@pytest.mark.parametrize("name", POISON_CASES)
def test_poisoned_pads_stay_out_of_the_reference_and_planted_writes_are_reported(name):
    c, o, ref, S, want = G.prepared(name)
    assert c["ldx"] > G.C_CH or c["rowvec_ld"] > G.C_CH
    td = G.TD[c["dtype"]]
    flat = G.embedded(o["x"], c["ldx"], td)
    M, ldx = G.rows(c), c["ldx"]
    assert bool(torch.isnan(flat[: G.GUARD].float()).all()) and bool(torch.isnan(flat[G.GUARD + M * ldx:].float()).all())
    if ldx > G.C_CH:
        assert bool(torch.isnan(flat[G.GUARD: G.GUARD + M * ldx].view(M, ldx)[:, G.C_CH:].float()).all())
    o2 = dict(o, x=G.extracted(flat, M, ldx).float().view(c["n"], G.L_TOK, G.C_CH))
    if "rowvec" in o:
        rflat = G.embedded(o["rowvec"], c["rowvec_ld"], torch.float32)
        o2["rowvec"] = G.extracted(rflat, o["rowvec"].shape[0], c["rowvec_ld"])
        assert int(torch.isnan(rflat).sum()) == 2 * G.GUARD + o["rowvec"].shape[0] * (c["rowvec_ld"] - G.C_CH)
    ref2, S2, _ = G.reference(c, o2)
    assert bool(torch.isfinite(ref2).all()) and bool(torch.isfinite(S2).all()) and torch.equal(ref2, G.reference(c, o)[0])
    # the sentinel: a clean buffer passes; a write into a pad column, behind the last row, in front of the first row, a NaN: each reported
    clean = G.to_buffer(c, G.emulate(c, o, "chunk32"))
    assert not G.check_output(c, clean, ref, want)[0]
    ld = c["ld_out"]
    spots = {"behind row": G.GUARD + M * ld + 3, "in front of the first row": G.GUARD - 1, "non-finite": G.GUARD + 5 * ld + 7}
    if ld > G.C_CH:
        spots["pad-column"] = G.GUARD + (M // 2) * ld + G.C_CH
    for label, at in spots.items():
        buf = clean.clone()
        buf[at] = float("nan") if label == "non-finite" else 0.0
        problems, _ = G.check_output(c, buf, ref, want)
        assert any(label in p for p in problems), (label, problems)
