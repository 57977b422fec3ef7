"""The self-attention parity cases (tests/attention_cases.py) held to account without a GPU: every case is routed to the kernel it names,
the table covers every instance it claims to, and the checker the GPU test relies on passes a plain emulation of each route's arithmetic
with room to spare and fails each of a list of planted faults.  dc_attention_variant runs on the host alone (it reads the parameters, never
the memory), as dc_igemm_variant does in tests/test_igemm_dispatch.py."""
import itertools

import pytest
import torch

import attention_cases as A
import test_igemm_dispatch as D


def _lib():
    mod = D._load_lib()
    return mod, mod.lib()


def _variant(c, ptrs=None):
    mod, lib = _lib()
    q, k, v, out = ptrs or A.fake_pointers(c)
    return lib.dc_attention_variant(mod.AttentionParams(**A.attention_fields(c, q, k, v, out))).decode()


EVERY = A.CASES + A.PLACEMENT_CASES + A.REPEAT_CASES


# ---- a. routing -----------------------------------------------------------------------------------------------------------------
def test_case_names_are_unique_and_shapes_are_small():
    names = [c["name"] for c in A.CASES]
    assert len(names) == len(set(names))
    for c in A.CASES:
        assert A.pairs(c) <= 8 and c["L"] <= 1281 and c["why"], c["name"]
        assert c["ld_qkv"] >= c["heads"] * c["d"] and c["ld_out"] >= c["heads"] * c["d"]
    assert all(A.pairs(c) == 512 for c in A.REPEAT_CASES)
    assert {(c["expect"], c["dtype"]) for c in A.PLACEMENT_CASES} == {(r, dt) for r in A.MATRIX_ROUTES for dt in (A.BF16, A.F16)} | \
        {("fp32", dt) for dt in (A.F32, A.BF16, A.F16)}


@pytest.mark.parametrize("c", EVERY, ids=lambda c: c["name"])
def test_every_case_is_routed_to_the_kernel_it_names(c):
    q, k, v, out = A.fake_pointers(c)
    aligned = not ((q | k | v) & 15) and c["ld_qkv"] % 8 == 0
    assert aligned == (c["layout"] != "unaligned" or c["dtype"] == A.F32), c["name"]
    assert _variant(c) == c["expect"], c["name"]
    # the instance is the one the launch code picks for this shape
    r, L, d = c["expect"], c["L"], c["d"]
    want = {"wave": ("wave", A.DTN[c["dtype"]], d, 2 if L <= 32 else 4), "mfma": ("mfma", A.DTN[c["dtype"]], A.mfma_gtag(L, d)), "flash": ("flash", A.DTN[c["dtype"]], d),
            "fp32": ("fp32", A.DTN[c["dtype"]], 24 if d == 96 else 16, "streamed" if L * d > 20480 else "whole")}[r]
    assert c["instance"] == want, c["name"]


def test_unaligned_sixteen_bit_operands_take_the_exact_kernel():
    """The whole-sequence route used not to look at the pointers: at L % 16 == 0, L <= 128, d % 32 == 0 the dispatcher named "mfma" and
    dc_attention returned DC_ERR_ALIGN, while the same pointers ran on the fp32 kernel at L = 40 or 144.  Aligned problems keep their route."""
    for dt in (A.BF16, A.F16):
        for (L, d), aligned_route in (((64, 64), "wave"), ((96, 32), "mfma"), ((128, 96), "mfma"), ((300, 64), "flash"), ((16, 96), "mfma"), ((40, 64), "wave"), ((144, 64), "flash")):
            c = A._case("fp32", dt, d, L, "unaligned")
            assert _variant(c) == "fp32", (dt, L, d)
            f = A._case(aligned_route, dt, d, L, "fused")
            assert _variant(f) == aligned_route, (dt, L, d)
            q, k, v, out = A.fake_pointers(f)
            assert _variant(dict(f, ld_qkv=f["ld_qkv"] + 4)) == "fp32"                              # aligned pointers, ld_qkv % 8 != 0
            for i in range(3):                                                                      # one pointer of the three off
                p = [q, k, v]
                p[i] += 8
                assert _variant(f, (*p, out)) == "fp32", (dt, L, d, i)


# ---- b. coverage ----------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_instance_or_proves_it_unreachable():
    have = {c["instance"] for c in A.CASES}
    T16 = ("bf16", "f16")
    wave = {("wave", t, d, nkt) for t in T16 for d in (32, 64, 128) for nkt in (2, 4)}
    mfma = {("mfma", t, g) for t in T16 for g in ("G4", "G2", "G1", "G4w")}
    flash = {("flash", t, d) for t in T16 for d in (32, 64, 96, 128)}
    fp32 = {("fp32", t, sw, form) for t in ("f32",) + T16 for sw in (16, 24) for form in ("whole", "streamed")}
    assert len(wave) == 12 and wave | mfma | flash | fp32 == have, (wave | mfma | flash | fp32) ^ have
    # the run-time forms of the whole-sequence kernel: every G at every d it can have, with and without a dead pair, Lp != L
    for t, dt in (("bf16", A.BF16), ("f16", A.F16)):
        mine = [c for c in A.CASES if c["expect"] == "mfma" and c["dtype"] == dt]
        for g, ds in (("G4", (32, 64, 96, 128)), ("G2", (32, 64, 96, 128)), ("G1", (32, 64, 96, 128)), ("G4w", (32, 64))):
            assert {c["d"] for c in mine if c["instance"][2] == g} == set(ds), (t, g)
            if g != "G1":
                assert {A.dead_pair(c) for c in mine if c["instance"][2] == g} == {True, False}, (t, g)
        assert {c["L"] for c in mine if A.mfma_lp(c["L"]) != c["L"]} == {16, 80, 112}
        assert {(c["L"], c["d"]) for c in mine} >= {(L, 96) for L in (16, 32, 64, 80, 112, 128)} | {(L, d) for L in (80, 96, 112, 128) for d in (32, 64, 128)}
        fl = [c for c in A.CASES if c["expect"] == "flash" and c["dtype"] == dt]
        for d in (32, 64, 96, 128):
            assert {A.padded_keys(c) > 0 for c in fl if c["d"] == d} == {True, False}, (t, d)           # ragged and not ragged
    # layouts: every instance sees "fused" and one other; modes: "peaked" once per instance, "negative" where keys are masked or padded
    for inst in have:
        mine = [c for c in A.CASES if c["instance"] == inst]
        lay = {c["layout"] for c in mine}
        assert len(lay) >= 2 and (("fused" in lay) != (inst in A.NO_FUSED)), (inst, lay)
        assert any(c["mode"] == "peaked" for c in mine) and any(c["mode"] == "random" for c in mine), inst
        if any(A.padded_keys(c) for c in mine):
            assert any(c["mode"] == "negative" and A.padded_keys(c) for c in mine), inst
    # forms the kernels could run and the table does not reach must be out of the dispatcher's reach too (the plan has none), on a probe grid
    for (route, t, form), why in A.UNREACHABLE.items():
        dt = A.BF16 if t == "bf16" else A.F16
        Ls = (144, 160, 176, 192, 208, 224, 240, 256) if form == "L>128" else (1, 15, 16, 17, 40, 63, 64, 65, 100, 127, 128)
        assert (route, form) in (("mfma", "L>128"), ("flash", "L<=128")) and why
        n = 0
        for L, d, lay, (nn, h) in itertools.product(Ls, (16, 32, 64, 96, 128), ("fused", "wide", "split", "odd_out", "unaligned"), ((1, 1), (2, 3), (64, 8))):
            c = A._case(route, dt, d, L, lay, n=nn, heads=h)
            q, k, v, out = A.fake_pointers(c)
            for o2 in (out, out + 4):
                got = _variant(c, (q, k, v, o2))
                assert got != route and got in ("wave", "mfma", "flash", "fp32"), (c["name"], got)
                n += 1
        assert n == len(Ls) * 5 * 5 * 3 * 2


def test_edge_cases_have_the_property_they_are_there_for():
    """Computed from the cases: live keys in the last tile, wholly masked tiles, dead waves, block counts and their parity, KB."""
    for dt in (A.BF16, A.F16):
        for d in (32, 64, 128):
            for nkt in (2, 4):
                mine = [c for c in A.CASES if c["instance"] == ("wave", A.DTN[dt], d, nkt)]
                live_in_tile = lambda c, t: max(0, min(16, c["L"] - 16 * t))
                assert {c["L"] for c in mine} == ({1, 16, 17, 32} if nkt == 2 else {33, 48, 49, 64})
                assert any(live_in_tile(c, nkt - 1) == 0 and live_in_tile(c, nkt - 2) == 1 for c in mine)      # one live key, then a wholly masked tile
                assert any(live_in_tile(c, nkt - 1) == 1 for c in mine) and any(live_in_tile(c, nkt - 1) == 16 for c in mine)
                assert any(A.pairs(c) % 4 for c in mine) and all(A.pairs(c) in (1, 5, 6) for c in mine)
            assert any(A.pairs(c) == 1 for c in A.CASES if c["expect"] == "wave" and c["d"] == d)
        for d in (32, 64, 96, 128):
            mine = [c for c in A.CASES if c["instance"] == ("flash", A.DTN[dt], d)]
            kb = {32: 128, 64: 64, 96: 64, 128: 32}[d]
            assert all(A.key_block(c) == kb and (c["n"], c["heads"]) == (2, 3) and c["L"] >= 129 for c in mine)
            c129 = [c for c in mine if c["L"] == 129]
            qblocks = lambda c: (c["L"] + 127) // 128
            dead_waves = lambda c: (qblocks(c) * 128 - c["L"]) // 32                                            # wholly dead 32-query waves of the last query block
            assert c129 and all(dead_waves(c) == 3 and c["L"] % kb == 1 for c in c129)
            assert any(c["L"] == 255 and qblocks(c) * 128 - c["L"] == 1 for c in mine)
            assert any(c["L"] == 256 and A.n_blocks(c) % 2 == 0 and A.padded_keys(c) == 0 for c in mine)
            assert any(A.n_blocks(c) % 2 == 1 and c["L"] % kb == kb - 1 for c in mine), d                       # odd block count, ragged tail of KB - 1 keys
            assert any(c["L"] == 300 for c in mine)
            if d == 128:
                assert {159, 161} <= {c["L"] for c in mine}
    f32 = [c for c in A.CASES if c["expect"] == "fp32" and c["dtype"] == A.F32]
    for d in (16, 32, 64, 96, 128):
        assert any(c["d"] == d and c["L"] == A.fp32_qt(d) + 1 and A.n_blocks(c) == 1 for c in f32), d          # a second query tile with one live query
        small = 20480 // d + 1                                                                                  # the smallest streamed length
        assert any(c["d"] == d and c["L"] == small and A.key_block(c) == 8192 // d and A.n_blocks(c) == 3 for c in f32), d
    assert {(c["d"], c["L"]) for c in f32} >= {(128, 160), (96, 213)} and all(A.n_blocks(c) == 1 for c in f32 if (c["d"], c["L"]) in ((128, 160), (96, 213)))
    assert A.fp32_kb(214, 96) == 85 and 214 - 2 * 85 == 44 and [A.fp32_qt(d) for d in (16, 32, 64, 96, 128)] == [256, 128, 64, 64, 32]
    for dt in (A.BF16, A.F16):
        low = {(c["L"], c["d"], c["layout"] == "unaligned") for c in A.CASES if c["expect"] == "fp32" and c["dtype"] == dt}
        assert low >= {(24, 16, False), (100, 16, False), (100, 64, False), (48, 96, False), (64, 64, True), (96, 32, True), (128, 96, True), (300, 64, True)}
    assert A.mfma_g(48, 96) == 0


# ---- c. the emulation -----------------------------------------------------------------------------------------------------------
FAULTS = ["last_key_dropped", "last_block_dropped", "pad_key_unmasked", "no_rescale", "scale_not_applied", "v_of_next_head", "sample_offset_by_ld_out",
          "rowsum_of_neighbour_query", "pad_column_written", "row_past_end_written", "dead_pair_stores"]


def applicable(c, fault):
    """Where a fault can be planted at all, and where it need not show.
    last_key_dropped: not in "peaked" mode — its rows are one-hot, a key matters to the queries it wins, n * heads of them on average and none
    with probability e^-(n heads).  last_block_dropped: the key block of flash / streamed fp32; a 16-key MFMA tile of the whole-sequence
    kernels; the one-block fp32 form has nothing smaller than the sequence to drop.  pad_key_unmasked: only where the kernel holds keys beyond
    L, and it must fail in "negative" mode — in "random" one more key among many with a score near the others' moves the result by less than
    the bound, which is why that mode exists (test_an_unmasked_padded_key_...).  no_rescale: routes whose softmax takes more than one step
    (the emulation steps by key block; the one-block fp32 form rescales per key, inside one step here), with at least a 16-key tile behind
    the first block: L = 129 at KB = 128 has one key there, the max moves for one query in 129, and in "negative" mode by little.
    scale_not_applied: more than one key (the softmax over one key is 1 whatever its score).  v_of_next_head / sample_offset_by_ld_out: more
    than one head / more than one sample in the "wide" layout (the layout in which both strides are padded, by different amounts of bytes).
    rowsum_of_neighbour_query: more than one query.  pad_column_written: ld_out > heads d.  dead_pair_stores: attn_mfma_kernel with G > 1 and a
    last workgroup that is not full."""
    multi = A.n_blocks(c) > 1
    return {"last_key_dropped": c["L"] > 1 and c["mode"] != "peaked", "last_block_dropped": multi or (c["expect"] in ("wave", "mfma") and c["L"] > 16),
            "pad_key_unmasked": A.padded_keys(c) > 0 and c["mode"] == "negative", "no_rescale": multi and c["L"] - A.key_block(c) >= 16,
            "scale_not_applied": c["L"] > 1,
            "v_of_next_head": c["heads"] > 1, "sample_offset_by_ld_out": c["layout"] == "wide" and c["n"] > 1, "rowsum_of_neighbour_query": c["L"] > 1,
            "pad_column_written": c["ld_out"] > c["heads"] * c["d"], "row_past_end_written": True, "dead_pair_stores": A.dead_pair(c)}[fault]


def emulate(c, o, fault=None):
    """The kernel, plainly: fp32 scores (torch's fp32 matmul), an online softmax one key block of the route at a time (running max, the row
    sum of the UNROUNDED p, O and l rescaled when the max moves), P rounded to the compute type in front of P.V on the matrix-core routes,
    the quotient rounded to the output type into a sentinel-filled buffer.  The transposed-score kernels (wave, flash) form
    p = exp2(s * scale log2 e - m * scale log2 e) on the raw scores, the others exp(scale s - m)."""
    n, L, h, d, dt, route = c["n"], c["L"], c["heads"], c["d"], c["dtype"], c["expect"]
    td = A.TD[dt]
    q, k, v = o["q"], o["k"], o["v"]
    if fault == "sample_offset_by_ld_out":          # sample i starts i * L * ld_out elements in, rows keep their stride ld_qkv
        bufs, iq, ik, iv = A.pack(c, o)
        idx = (torch.arange(n).view(n, 1, 1) * L * c["ld_out"] + torch.arange(L).view(1, L, 1) * c["ld_qkv"] + torch.arange(h * d).view(1, 1, -1))
        q, k, v = (bufs[i][off + idx].float().view(n, L, h, d) for i, off in (iq, ik, iv))
    q, k, v = (t.permute(0, 2, 1, 3).contiguous() for t in (q, k, v))                 # [n, h, L, d]
    if fault == "v_of_next_head":
        v = v.roll(-1, dims=1)
    scale = torch.tensor(1.0 if fault == "scale_not_applied" else c["scale"], dtype=torch.float32)
    if fault == "pad_key_unmasked":                 # one of the zero rows the kernel staged behind key L - 1 takes part
        k = torch.cat([k, torch.zeros(n, h, 1, d)], 2)
        v = torch.cat([v, torch.zeros(n, h, 1, d)], 2)
    Lk = k.shape[2]
    raw = route in ("wave", "flash")
    if route == "fp32":
        s = (q * scale) @ k.transpose(-1, -2)
    else:
        s = q @ k.transpose(-1, -2)
        if not raw:
            s = s * scale
    if fault == "last_key_dropped":
        s[..., L - 1] = float("-inf")
    kb = A.key_block(c)
    if fault == "last_block_dropped":
        drop = kb if A.n_blocks(c) > 1 else 16
        s[..., (L - 1) // drop * drop:] = float("-inf")
    sc2 = scale * torch.tensor(1.4426950408889634, dtype=torch.float32)
    m = torch.full((n, h, L, 1), float("-inf"))
    l = torch.zeros(n, h, L, 1)
    O = torch.zeros(n, h, L, d)
    for j0 in range(0, Lk, kb):
        sb = s[..., j0:j0 + kb]
        mn = torch.maximum(m, sb.amax(-1, keepdim=True))
        if raw:
            nms = -mn * sc2
            p, corr = torch.exp2(sb * sc2 + nms), torch.exp2(m * sc2 + nms)
        else:
            p, corr = torch.exp(sb - mn), torch.exp(m - mn)
        if fault == "no_rescale":
            corr = torch.ones_like(corr)
        l = l * corr + p.sum(-1, keepdim=True)
        pr = p.to(td).float() if route in A.MATRIX_ROUTES else p
        O = O * corr + pr @ v[..., j0:j0 + kb, :]
        m = mn
    if fault == "rowsum_of_neighbour_query":
        l = l.roll(1, dims=2)
    x = (O / l).permute(0, 2, 1, 3).reshape(n * L, h * d)
    buf = A.new_output(c)
    A.body(c, buf)[:] = x.to(td)
    M, C, ld = n * L, h * d, c["ld_out"]
    if fault == "pad_column_written":
        buf[(M // 2) * ld + C] = 0.0
    if fault == "row_past_end_written":
        buf[M * ld + 3] = 0.0
    if fault == "dead_pair_stores":                 # pair n * heads = (sample n, head 0): its first row lies behind the last sample
        buf[M * ld: M * ld + d] = x[0, :d].to(td)
    return buf


_shared = {}


def _ref(c):
    """Operands, reference and bound of a case: computed once, shared by the tests below, never modified."""
    if c["name"] not in _shared:
        o = A.make_operands(c)
        _shared[c["name"]] = (o,) + A.reference(c, o)
    return _shared[c["name"]]


@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c["name"])
def test_the_checker_passes_the_emulated_kernel_and_fails_every_planted_fault(c):
    o, ref, bound = _ref(c)
    assert ref.shape == (c["n"] * c["L"], c["heads"] * c["d"]) and bool((bound > 0).all())
    s = A.logits(c, o)
    if c["mode"] == "peaked":
        assert float(s.max()) > 60, float(s.max())
    if c["mode"] == "negative":
        assert float(s.max()) <= -8, float(s.max())
    problems, worst = A.check_output(c, emulate(c, o), ref, bound)
    print(f"{c['name']}: emulation err / bound {worst:.3f}")
    assert not problems, problems
    # the bound has room for the arithmetic it allows for: half of it on the matrix-core routes, 95 % in fp32.  A 16-bit result of the fp32
    # route is the exception by nature: u_P = 0 there, so the bound is the output rounding 1.02 u |ref| plus an fp32-sized e, and a correctly
    # rounded value alone uses up to 1 / 1.02 of it
    limit = 0.05 if c["dtype"] == A.F32 else (0.5 if c["expect"] in A.MATRIX_ROUTES else 0.99)
    assert worst <= limit, (worst, limit)
    for fault in FAULTS:
        if applicable(c, fault):
            problems, worst = A.check_output(c, emulate(c, o, fault), ref, bound)
            assert problems, f"{c['name']}: the checker lets '{fault}' through (worst err / bound {worst:.3g})"


def test_every_fault_is_planted_on_every_route_and_dtype_it_applies_to():
    cells16 = {(r, dt) for r in A.MATRIX_ROUTES for dt in (A.BF16, A.F16)}
    everywhere = cells16 | {("fp32", dt) for dt in (A.F32, A.BF16, A.F16)}
    want = {f: everywhere for f in FAULTS}
    want["pad_key_unmasked"] = cells16                                                  # the fp32 kernel holds no key beyond L
    want["dead_pair_stores"] = {("mfma", A.BF16), ("mfma", A.F16)}
    want["no_rescale"] = {(r, dt) for r, dt in everywhere if r in ("flash", "fp32")}    # the whole-sequence kernels take one step
    for fault in FAULTS:
        cells = {(c["expect"], c["dtype"]) for c in A.CASES if applicable(c, fault)}
        assert cells == want[fault], (fault, cells ^ want[fault])


def test_an_unmasked_padded_key_hides_in_random_data_and_shows_in_negative_scores():
    """Why the "negative" mode exists: on N(0,1) data at flash lengths one zero-score key among hundreds moves a bf16 result by less than the
    bound (this need not fail, and does not); against scores <= -8 it takes over the softmax."""
    c = A.by_name("flash_bf16_d64_L191_n2h3_fused_random")
    o, ref, bound = _ref(c)
    problems, worst = A.check_output(c, emulate(c, o, "pad_key_unmasked"), ref, bound)
    print(f"random: err / bound {worst:.3f} with one padded key unmasked")
    assert worst < 1.0 and applicable(c, "pad_key_unmasked") is False
    c = A.by_name("flash_bf16_d64_L191_n2h3_wide_negative")
    o, ref, bound = _ref(c)
    problems, worst = A.check_output(c, emulate(c, o, "pad_key_unmasked"), ref, bound)
    assert problems and worst > 10.0, worst


# ---- e. the bound ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wave_bf16_d64_L49_n5h1_split_random", "mfma_f16_d96_L80_n2h3_fused_random", "flash_bf16_d32_L300_n2h3_wide_random",
                                  "flash_f16_d128_L161_n2h3_wide_random", "fp32_f32_d64_L321_n2h2_split_random", "fp32_bf16_d64_L100_n2h2_split_random"])
def test_the_bound_scales_with_v(name):
    """Scaling v by 2^10 scales the reference and everything in the bound but the f16 subnormal floor by exactly 2^10 (a power of two: exact
    in fp64)."""
    c = A.by_name(name)
    o = A.make_operands(c)
    ref, bound = A.reference(c, o)
    ref2, bound2 = A.reference(c, dict(o, v=o["v"] * 1024.0))
    fl = A.FLOOR[c["dtype"]]
    assert torch.equal(ref2, ref * 1024.0) and torch.allclose(bound2 - fl, (bound - fl) * 1024.0, rtol=1e-12, atol=0.0)


RATIO_CASES = [c for c in A.CASES if c["mode"] == "random" and c["d"] <= 32 and 16 <= c["L"] <= 300]


def test_the_bound_is_a_statement_about_rounding_not_about_magnitude():
    """The bound is a few unit roundoffs of the result's magnitude w |v| (>= |ref|; |ref| itself passes through zero): below 3 u_out + 1e-4
    of it on the "random" cases of every route and dtype from 16 to 300 tokens up to d = 32.  The ratio's supremum is 3.02 u_out + 4 delta +
    2 (L + 16) 2^-24 (+ sub), reached where one key holds all the weight (L = 1: |ref| = w |v|); the part beyond 3.02 u_out grows with d and L
    by construction (3.6e-4 at d = 128) and is printed below for every "random" case."""
    assert {(c["expect"], c["dtype"]) for c in RATIO_CASES} >= {(r, dt) for r in ("wave", "mfma", "flash", "fp32") for dt in (A.BF16, A.F16)} | {("fp32", A.F32)}
    for c in (c for c in A.CASES if c["mode"] == "random"):
        o, ref, bound = _ref(c)
        n, L, h, d = c["n"], c["L"], c["heads"], c["d"]
        w = torch.softmax(A.logits(c, o), -1)
        mag = (w @ o["v"].double().permute(0, 2, 1, 3).abs()).permute(0, 2, 1, 3).reshape(n * L, h * d)
        assert bool((ref.abs() <= mag * (1 + 1e-12)).all())
        ratio = float(((bound - A.FLOOR[c["dtype"]]) / mag).max())
        print(f"{c['name']}: largest (bound - floor) / (w |v|) = 3 u_out + {ratio - 3 * A.U_OUT[c['dtype']]:.2e}")
        if c in RATIO_CASES:
            assert ratio < 3 * A.U_OUT[c["dtype"]] + 1e-4, (c["name"], ratio)
