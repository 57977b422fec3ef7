"""The strip-family parity cases (tests/strip_attention_cases.py) held to account without a GPU: every case is routed to the kernel it names,
the table reaches all 48 template instances and, for every matrix-core one, each shape of a wave's walk; the checker the GPU test relies on
passes a plain emulation of each body with room to spare and fails each of a list of planted faults.  The *_variant functions run on the
host alone (they read the parameters, never the memory), as dc_attention_variant does in tests/test_attention_cases.py."""
import pytest
import torch

import strip_attention_cases as S
import test_igemm_dispatch as D
from attention_cases import BF16, F16, F32, TD

ENTRIES = ("cross", "cross_len", "bias", "causal")


def _lib():
    mod = D._load_lib()
    return mod, mod.lib()


def _variant(c, f=None):
    mod, lib = _lib()
    p = getattr(mod, S.PARAMS[c["entry"]])(**(f or S.fake_fields(c)))
    return getattr(lib, S.ENTRY[c["entry"]] + "_variant")(p).decode()


# ---- a. routing -----------------------------------------------------------------------------------------------------------------
def test_case_names_are_unique_and_shapes_are_small():
    names = [c["name"] for c in S.CASES]
    assert len(names) == len(set(names))
    for c in S.CASES:
        assert c["n"] * c["heads"] <= 15 and c["why"], c["name"]
        stated = c["rows"] == 512 or (c["expect"] == "fp32" and c["rows"] == S.exact_qt(c) + 1)          # L = 512 once; Lq = QT + 1
        assert c["rows"] <= 100 or stated, c["name"]
        assert c["keys"] <= 515 and c["ld_out"] >= c["heads"] * c["d"], c["name"]


@pytest.mark.parametrize("c", S.CASES, ids=lambda c: c["name"])
def test_every_case_is_routed_to_the_kernel_it_names(c):
    q, k, v, out, aux = S.fake_pointers(c)
    aligned = not ((q | k | v) & 15) and c.get("ld_kv", c.get("ld_qkv")) % 8 == 0 and c.get("ld_q", 0) % 8 == 0 and c["ld_out"] % 4 == 0
    assert aligned == (c["layout"] in ("hard", "plain") or (c["dtype"] == F32 and c["layout"] != "odd_out")), c["name"]
    assert _variant(c) == c["expect"], c["name"]
    t, d = S.DTN[c["dtype"]], c["d"]
    if S.is_cross(c):
        strip = c["dtype"] != F32 and d in (32, 64, 96, 128, 160) and aligned
        want = ("cross", "mfma", t, d, c["entry"] == "cross_len") if strip else ("cross", "fp32", t, 24 if d == 96 else 20 if d == 160 else 16, c["entry"] == "cross_len")
    else:
        want = (c["entry"], "mfma" if (c["dtype"] != F32 and d == 64 and aligned) else "fp32", t)
    assert c["instance"] == want and c["expect"] == want[1], c["name"]
    if c["entry"] == "cross_len":
        assert c["lens"] is not None                      # kv_len = NULL is dc_cross_attention's launch: the LEN instances need an array


def test_cross_attention_refuses_misaligned_pointers():
    """dc_cross_attention and dc_cross_attention_len refuse what dc_attention_bias and dc_attention_causal refuse (DC_ERR_ALIGN): q / k / v /
    out that are not element aligned, q_map / kv_map / kv_len that are not 4-byte aligned.  Through the *_variant functions only, which
    touch no memory."""
    for entry in S.CROSS:
        for dt in (F32, BF16, F16):
            c = S._case(entry, "fp32" if dt == F32 else "mfma", dt, 64, 17, 33, 2, 2, "hard", lens=[33, 5, 7, 1] if entry == "cross_len" else None, maps="both")
            good = S.fake_fields(c)
            assert _variant(c, good) == c["expect"]
            es = 4 if dt == F32 else 2
            for name in ("q", "k", "v", "out"):
                for off in range(1, es):
                    assert _variant(c, dict(good, **{name: good[name] + off})) == "invalid", (entry, dt, name, off)
                assert _variant(c, dict(good, **{name: good[name] + es})) == "fp32", (entry, dt, name)     # element aligned: served, by the exact kernel
            for name in ("q_map", "kv_map") + (("kv_len",) if entry == "cross_len" else ()):
                for off in (1, 2, 3):
                    assert _variant(c, dict(good, **{name: good[name] + off})) == "invalid", (entry, dt, name, off)
                assert _variant(c, dict(good, **{name: good[name] + 4})) == c["expect"]
                assert _variant(c, dict(good, **{name: None})) == c["expect"]
    # the sequence entry points already did
    for entry in ("bias", "causal"):
        c = S._case(entry, "mfma", BF16, 64, 33, None, 3, 2, "hard", lens=(33, 1, 31))
        good = S.fake_fields(c)
        assert _variant(c, dict(good, q=good["q"] + 1)) == "invalid"
        ln = "kv_len" if entry == "bias" else "row_len"
        assert _variant(c, dict(good, **{ln: good[ln] + 2})) == "invalid"


# ---- b. coverage ----------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_all_48_instances():
    have = {c["instance"] for c in S.CASES}
    assert len(S.all_instances()) == 48 and have == S.all_instances(), have ^ S.all_instances()
    for inst in have:
        mine = [c for c in S.CASES if c["instance"] == inst]
        assert any(c["mode"] == "random" for c in mine), inst
        assert any(c["ld_out"] > c["heads"] * c["d"] for c in mine), inst                    # pad columns that must keep the sentinel
        if inst[1] == "mfma":
            assert any(c["mode"] == "negative" and S.padded_keys(c) for c in mine), inst
            assert {c["layout"] for c in mine} >= {"hard", "plain"}, inst
        if inst[0] != "cross":
            assert any(c["lens"] is None for c in mine) and any(c["lens"] is not None for c in mine), inst
    for e in ENTRIES:
        for route, dts in (("mfma", S.T16), ("fp32", (F32,) + S.T16)):
            for dt in dts:
                assert any(c["mode"] == "peaked" for c in S.CASES if (c["entry"], c["expect"], c["dtype"]) == (e, route, dt)), (e, route, dt)


def test_edge_cases_have_the_property_they_are_there_for():
    """Computed from the cases: for every matrix-core instance the shapes of a wave's walk (nplain = 0, = nblk, = nblk - 1 with one and with
    KB - 1 keys in the masked block), a wave with one query tile and fewer than 16 live queries, a dead wave in the last workgroup and a full
    last workgroup; the lengths, maps, doors and block counts the table states."""
    for inst in (i for i in S.all_instances() if i[1] == "mfma"):
        mine = [c for c in S.CASES if c["instance"] == inst]
        KB = S.key_block(mine[0])
        assert KB == (S.cross_kb(inst[3]) if inst[0] == "cross" else 32)
        ws = [w for c in mine for w in S.waves(c) if w["nqt"] > 0]
        in_last = lambda w: min(w["len"], w["nblk"] * KB) - w["nplain"] * KB                 # live keys of the block behind the plain ones
        assert any(w["nplain"] == 0 for w in ws), inst
        if inst[0] == "causal":
            assert all(w["nblk"] == w["nplain"] + 1 for w in ws)                               # the diagonal block always follows
            assert any(w["nplain"] == 15 for w in ws), inst                                  # L = 512: 16 blocks
        else:
            assert any(w["nplain"] == w["nblk"] for w in ws), inst
            assert {w["nblk"] for w in ws} >= {1, 2, 3}, inst                                   # odd and even block counts
        assert any(w["nplain"] == w["nblk"] - 1 and in_last(w) == 1 for w in ws), inst
        assert any(w["nplain"] == w["nblk"] - 1 and in_last(w) == KB - 1 for w in ws), inst
        assert any(w["nqt"] == 1 and w["live"] < 16 for w in ws), inst
        assert any(w["live"] == 32 for w in ws) and any(w["live"] == 17 for w in ws) and any(w["live"] == 16 for w in ws), inst
        assert any(S.dead_waves(c) for c in mine) and any(not S.dead_waves(c) for c in mine), inst
        if inst[0] != "cross":                                                               # kZeroPad: waves wholly of pad queries
            c100 = [c for c in mine if c["rows"] == 100 and c["lens"] and 33 in c["lens"]]
            assert c100, inst
            w33 = [w for w in S.waves(c100[0]) if w["len"] == 33]
            assert [(w["q0"], w["nqt"] > 0, w["live"]) for w in w33] == [(0, True, 32), (32, True, 1), (64, False, 0), (96, False, 0)]
            assert {c["rows"] for c in mine} >= set(S.SEQ_L) | {512}
            assert any(c["lens"] and len(set(c["lens"])) == 3 and {c["lens"][0], c["lens"][1]} == {c["rows"], 1} for c in mine)
        elif not inst[4]:
            assert {c["keys"] for c in mine} >= {1, KB - 1, KB, KB + 1, 2 * KB, 2 * KB + 1, 3 * KB - 1}, inst
            assert {c["rows"] for c in mine} >= {1, 16, 17, 32, 33, 70}, inst
            assert {c["maps"] for c in mine} >= {"identity", "many_q", "kv_repeat"}
            assert any(c["maps"] == "kv_repeat" and c["keys"] % KB for c in mine), inst          # the NaN context behind a ragged one
        else:
            lens = {x for c in mine for x in c["lens"]}
            assert lens >= {0, -3, 1, KB - 1, KB, KB + 1, 2 * KB, 2 * KB + 1, 3 * KB - 1} and any(x == c["keys"] + 5 for c in mine for x in c["lens"]), inst
            assert any(len({w["len"] for w in S.waves(c)[:2]}) == 2 for c in mine), inst    # two lengths inside the first workgroup
            assert any(c["keys"] in c["lens"] for c in mine)
    # d = 32 walks 64-key blocks: 63 / 64 / 65 keys
    assert {c["keys"] for c in S.CASES if c["instance"][:2] == ("cross", "mfma") and c["d"] == 32} >= {63, 64, 65}
    # kv_repeat leaves context 1 to nobody, directly behind the referenced context 0, which is ragged in at least one case per instance
    for c in (c for c in S.CASES if c["maps"] in ("kv_repeat", "both") and c["entry"] == "cross"):
        assert 0 in c["kv_map"] and 1 not in c["kv_map"], c["name"]
    # the exact route: every SW in f32 and in each 16-bit type with and without lengths; the doors; QT + 1; the LDS block counts
    ex = [c for c in S.CASES if c["expect"] == "fp32"]
    for dt in S.T16:
        doors = {(c["d"], c["layout"]) for c in ex if c["entry"] == "cross" and c["dtype"] == dt}
        assert doors >= {(16, "plain"), (64, "ld_odd"), (96, "q_off"), (160, "odd_out")}, doors
        for e in ("bias", "causal"):
            doors = {(c["d"], c["layout"]) for c in ex if c["entry"] == e and c["dtype"] == dt}
            assert {d for d, _ in doors} >= {16, 32, 64, 128} and {lay for d, lay in doors if d == 64} == {"ld_odd", "q_off", "odd_out"}, (e, dt)
    for d in (16, 64, 96, 160):
        B = 4096 // d
        f32 = [c for c in ex if c["entry"] == "cross" and c["dtype"] == F32 and c["d"] == d]
        assert {c["keys"] for c in f32} >= {B, B + 1, 2 * B + 3} and any(c["rows"] == S.exact_qt(c) + 1 for c in f32), d
        assert all(S.key_block(c) == B for c in f32)
    assert max(c["keys"] for c in ex) == 515
    for c in (c for c in ex if c["entry"] == "cross_len"):
        assert S.key_block(c) == min(c["keys"], 4096 // c["d"])                              # from S, whatever the lengths
    assert [S.exact_qt(dict(entry="cross", d=d)) for d in (16, 32, 64, 96, 128, 160)] == [256, 128, 64, 64, 32, 32]
    for e in ("bias", "causal"):
        assert {c["d"] for c in ex if c["entry"] == e and c["dtype"] == F32} == {16, 32, 64, 128}
        assert any(c["d"] == 128 and c["dtype"] != F32 and c["rows"] > 32 for c in ex if c["entry"] == e)   # 16-bit, d = 128, several LDS blocks


# ---- c. the emulation -----------------------------------------------------------------------------------------------------------
FAULTS = ["pad_key_unmasked", "ragged_mask_off_by_one", "last_key_dropped", "last_block_dropped", "no_rescale", "scale_not_applied", "v_of_next_head",
          "rowsum_of_neighbour_query", "q_map_ignored", "kv_map_ignored", "context_stride_is_len", "len_not_clamped", "len_of_next_sample",
          "bias_index_off_by_one", "bias_of_next_head", "bias_sign_flipped", "causal_diagonal_masked", "causal_future_key_visible", "pad_row_not_zero",
          "pad_column_written", "row_past_end_written"]


def _len_index(c, i):
    return S.kv_map(c)[i] if S.is_cross(c) else i


def applicable(c, fault):
    """Where a fault can be planted at all, and where it need not show.
    pad_key_unmasked (no key mask in the ragged block) / ragged_mask_off_by_one (key > len where key >= len is meant: the first zero-staged
    key takes part): the strip route of the three entry points that mask by a key bound, where a live wave holds a ragged block, and they
    must fail in "negative" mode — in "random" one zero-score key among many moves the result by less than the bound
    (test_the_off_by_one_mask_...).  last_key_dropped / last_block_dropped: not in "peaked" mode, whose rows are one-hot (a key matters only
    to the queries it wins); the causal entry has its own fault for its last key; a block: a sample whose walk has more than one.
    no_rescale: more than one block with at least 16 keys behind the first.  scale_not_applied, the bias faults, causal_future_key_visible:
    a query with more than one key.  rowsum_of_neighbour_query: two live queries whose row sums differ (more than one key).
    q_map_ignored / kv_map_ignored (sample i reads q sample / context i): a map that is not the identity.  context_stride_is_len: a referenced context other than the first
    whose length is not S.  len_not_clamped: a referenced length outside [1, keys].  len_of_next_sample: a neighbour with another length.
    pad_row_not_zero: a sample shorter than L."""
    e, strip, n = c["entry"], c["expect"] == "mfma", c["n"]
    sl = [S.sample_len(c, i) for i in range(n)]
    kb = S.key_block(c)
    if e == "causal" and strip:
        blocks = [(x + 31) // 32 for x in sl]
        behind = [x - 32 for x in sl]
    else:
        blocks = [(x + kb - 1) // kb for x in sl]
        behind = [x - kb for x in sl]
    ragged = strip and e != "causal" and any(x % kb for x in sl)
    eff = S.eff_lens(c)
    idx = [_len_index(c, i) for i in range(n)]
    return {
        "pad_key_unmasked": ragged and c["mode"] == "negative", "ragged_mask_off_by_one": ragged and c["mode"] == "negative",
        "last_key_dropped": e != "causal" and c["mode"] != "peaked" and max(sl) > 1,
        "last_block_dropped": c["mode"] != "peaked" and max(blocks) > 1, "no_rescale": any(b > 1 and r >= 16 for b, r in zip(blocks, behind)),
        "scale_not_applied": max(sl) > 1, "v_of_next_head": c["heads"] > 1, "rowsum_of_neighbour_query": any(S.live_rows(c, i) > 1 and sl[i] > 1 for i in range(n)),
        "q_map_ignored": S.is_cross(c) and any(m != i for i, m in enumerate(S.q_map(c))),
        "kv_map_ignored": S.is_cross(c) and any(m != i for i, m in enumerate(S.kv_map(c))),
        "context_stride_is_len": e == "cross_len" and any(j > 0 and eff[j] != c["keys"] for j in idx),
        "len_not_clamped": c["lens"] is not None and any(not 1 <= c["lens"][j] <= c["keys"] for j in idx),
        "len_of_next_sample": c["lens"] is not None and any(eff[(j + 1) % len(eff)] != eff[j] for j in idx),
        "bias_index_off_by_one": e == "bias" and max(sl) > 1, "bias_of_next_head": e == "bias" and max(sl) > 1 and c["heads"] > 1,
        "bias_sign_flipped": e == "bias" and max(sl) > 1,
        "causal_diagonal_masked": e == "causal", "causal_future_key_visible": e == "causal" and max(sl) > 1,
        "pad_row_not_zero": not S.is_cross(c) and min(sl) < c["rows"],
        "pad_column_written": c["ld_out"] > c["heads"] * c["d"], "row_past_end_written": True}[fault]


def _walk(c, qr, query, K, V, kv0, nk, blocks, last, bt, fault, scale):
    """One walk of a body: qr [h, nQ, d] fp32 query rows, query [nQ] their indices, K / V the flat row images [*, h, d] of the packed
    buffers, kv0 the first row of the (sample's) keys, nk the staging bound, blocks the key offsets walked with step KB, last the offset of the
    block that masks (None: none), bt [h, 2 L - 1] or None.  Returns (O [h, nQ, d], l [h, nQ, 1]).
    Strip: raw fp32 scores, p = exp2(fma(s, scale log2 e, -max scale log2 e)) with the max over the raw scores (bias: over
    fma(s, scale log2 e, b log2 e), p = exp2(that - max)), keys at or past nk staged as zeros, P rounded to the compute type for P.V only, the
    row sum unrounded.  Exact: q scaled first, p = exp(s - max), only the live keys staged, a masked key skipped."""
    strip, e = c["expect"] == "mfma", c["entry"]
    h, nQ, d = qr.shape
    KB, L, td = S.key_block(c), c["rows"], TD[c["dtype"]]
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    sc2 = f32(scale) * f32(S.LOG2E)
    m = torch.full((h, nQ, 1), float("-inf"))
    l = torch.zeros(h, nQ, 1)
    O = torch.zeros(h, nQ, d)
    qv = query.view(1, nQ, 1)
    if not strip:
        qr = qr * f32(scale)
    for k0 in blocks:
        key = torch.arange(k0, k0 + KB if strip else min(k0 + KB, nk))
        staged = key < nk
        rows = (kv0 + key).clamp(max=min(K.shape[0], V.shape[0]) - 1)
        kb = torch.where(staged.view(-1, 1, 1), K[rows], torch.zeros(())).permute(1, 0, 2)         # [h, keys, d]
        vb = torch.where(staged.view(-1, 1, 1), V[rows], torch.zeros(())).permute(1, 0, 2)
        s = qr @ kb.transpose(-1, -2)
        kk = key.view(1, 1, -1)
        if bt is not None:
            rel = {"bias_index_off_by_one": kk - qv + L, "bias_sign_flipped": qv - kk + L - 1}.get(fault, kk - qv + L - 1).clamp(0, 2 * L - 2)
            b = torch.gather(bt.view(h, 1, -1).expand(h, nQ, -1), 2, rel.expand(h, nQ, -1))
            s = s * sc2 + b * f32(S.LOG2E) if strip else s + b
        is_last = (k0 == last) or not strip
        if e == "causal":
            mask = {"causal_diagonal_masked": kk >= qv, "causal_future_key_visible": kk > qv + 1}.get(fault, kk > qv) & is_last
        else:
            mask = {"pad_key_unmasked": kk < 0, "ragged_mask_off_by_one": kk > nk}.get(fault, kk >= nk) & is_last
            if fault == "last_key_dropped" and nk > 1:
                mask = mask | (kk == nk - 1)
        s = s.masked_fill(mask.expand(h, nQ, -1), float("-inf"))
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        if strip and bt is None:
            nms = -mn * sc2
            p, corr = torch.exp2(s * sc2 + nms), torch.exp2(m * sc2 + nms)
        elif strip:
            p, corr = torch.exp2(s - mn), torch.exp2(m - mn)
        else:
            p, corr = torch.exp(s - mn), torch.exp(m - mn)
        if fault == "no_rescale":
            corr = torch.where(torch.isfinite(m), torch.ones_like(corr), corr)
        l = l * corr + p.sum(-1, keepdim=True)
        O = O * corr + (p.to(td).float() if strip else p) @ vb
        m = mn
    return O, l


def emulate(c, o, fault=None):
    """The launch, plainly, on the packed buffers of the case (NaN wherever the kernel must not read): the maps, the clamped lengths, one
    walk per sample — per 32-query wave for the causal strip kernel, which walks the blocks 0 .. q0 / 32 and masks in the diagonal one alone —
    zero rows at or past the length, the quotient rounded to the output type into a sentinel-filled buffer."""
    n, R, h, d, e, strip = c["n"], c["rows"], c["heads"], c["d"], c["entry"], c["expect"] == "mfma"
    C, td, KB = h * d, TD[c["dtype"]], S.key_block(c)
    g = S.case_geometry(c)
    bufs, gq, gk, gv = S.pack(c, o)

    def image(where, ld):
        flat = bufs[where[0]][where[1]:]
        M = flat.numel() // ld
        return flat[: M * ld].view(M, ld)[:, :C].float().reshape(M, h, d)

    Q, K, V = image(gq, g["ld_q"]), image(gk, g["ld_kv"]), image(gv, g["ld_kv"])
    if fault == "v_of_next_head":
        V = V.roll(-1, dims=1)
    bt = o.get("bias")
    if bt is not None and fault == "bias_of_next_head":
        bt = bt.roll(-1, dims=0)
    scale = 1.0 if fault == "scale_not_applied" else c["scale"]
    buf = S.new_output(c)
    out = S.body(c, buf).view(n, R, C)
    lens = c["lens"]
    for i in range(n):
        qs = i if fault == "q_map_ignored" else S.q_map(c)[i]
        cs = i if fault == "kv_map_ignored" else S.kv_map(c)[i]
        j = cs if S.is_cross(c) else i
        if cs >= (c["nc"] if S.is_cross(c) else n):        # (kv_map ignored) a context that does not exist: whatever lies there
            out[i] = float("nan")
            continue
        if lens is None:
            ln = c["keys"]
        else:
            raw = lens[(j + 1) % len(lens)] if fault == "len_of_next_sample" else lens[j]
            ln = raw if fault == "len_not_clamped" else min(max(raw, 1), c["keys"])
        kv0 = cs * (ln if fault == "context_stride_is_len" else c["keys"])
        nq = R if S.is_cross(c) else min(ln, R)
        out[i] = 0.0
        if ln <= 0:
            if S.is_cross(c):
                out[i] = float("nan")                      # no block walked: 0 / 0
            continue
        query = torch.arange(nq)
        qr = Q[(qs * R + query).clamp(max=Q.shape[0] - 1)].permute(1, 0, 2)      # (a map ignored: past the last sample lies the NaN guard)
        if strip and e == "causal":
            Os, ls = [], []
            for q0 in range(0, nq, 32):
                blocks = list(range(0, q0 + 32, 32))
                if fault == "last_block_dropped" and len(blocks) > 1:
                    blocks = blocks[:-1]
                O, l = _walk(c, qr[:, q0:q0 + 32], query[q0:q0 + 32], K, V, kv0, ln, blocks, q0, bt, fault, scale)
                Os.append(O)
                ls.append(l)
            O, l = torch.cat(Os, 1), torch.cat(ls, 1)
        else:
            blocks = list(range(0, max(ln, 1), KB))
            if fault == "last_block_dropped" and len(blocks) > 1:
                blocks = blocks[:-1]
            O, l = _walk(c, qr, query, K, V, kv0, ln, blocks, (ln // KB) * KB if ln % KB else None, bt, fault, scale)
        if fault == "rowsum_of_neighbour_query":
            l = l.roll(1, dims=1)
        out[i, :nq] = (O / l).permute(1, 0, 2).reshape(nq, C).to(td)
        if fault == "pad_row_not_zero" and nq < R:
            out[i, nq, 0] = 1.0
    M, ld = n * R, c["ld_out"]
    if fault == "pad_column_written":
        buf[(M // 2) * ld + C] = 0.0
    if fault == "row_past_end_written":
        buf[M * ld + 3] = 0.0
    return buf


_shared = {}


def _ref(c):
    """Operands, reference, bound and live rows of a case: computed once, shared by the tests below, never modified."""
    if c["name"] not in _shared:
        o = S.make_operands(c)
        _shared[c["name"]] = (o,) + S.reference(c, o)
    return _shared[c["name"]]


@pytest.mark.parametrize("c", S.CASES, ids=lambda c: c["name"])
def test_the_checker_passes_the_emulated_kernel_and_fails_every_planted_fault(c):
    o, ref, bound, live = _ref(c)
    assert ref.shape == (c["n"] * c["rows"], c["heads"] * c["d"]) and bool((bound[live] > 0).all()) and bool((bound[~live] == 0).all())
    assert int(live.sum()) == sum(S.live_rows(c, i) for i in range(c["n"]))
    s = S.biased_logits(c, o)
    if c["mode"] == "peaked":
        assert float(s.max()) > 60, float(s.max())
    if c["mode"] == "negative":
        assert float(s.max()) <= -6, float(s.max())
    problems, worst = S.check_output(c, emulate(c, o), ref, bound, live)
    print(f"{c['name']}: emulation err / bound {worst:.3f}")
    assert not problems, problems
    # the headroom of tests/test_attention_cases.py: half the bound on the matrix-core route, 95 % in fp32; a 16-bit result of the exact route
    # has u_P = 0, so a correctly rounded value alone uses up to 1 / 1.02 of its bound
    limit = 0.05 if c["dtype"] == F32 else (0.5 if c["expect"] == "mfma" else 0.99)
    assert worst <= limit, (worst, limit)
    for fault in FAULTS:
        if applicable(c, fault):
            problems, worst = S.check_output(c, emulate(c, o, fault), ref, bound, live)
            assert problems, f"{c['name']}: the checker lets '{fault}' through (worst err / bound {worst:.3g})"


def test_every_fault_is_planted_in_every_cell_it_applies_to():
    """(entry, route, dtype) cells: the matrix-core route exists in 16 bit, the exact one in all three types."""
    def cells(entries, routes=("mfma", "fp32")):
        return {(e, r, dt) for e in entries for r in routes for dt in ((BF16, F16) if r == "mfma" else (F32, BF16, F16))}

    everywhere = cells(ENTRIES)
    want = {f: everywhere for f in FAULTS}
    want["pad_key_unmasked"] = want["ragged_mask_off_by_one"] = cells(("cross", "cross_len", "bias"), ("mfma",))   # the exact kernel stages no key past the length
    want["last_key_dropped"] = cells(("cross", "cross_len", "bias"))
    want["q_map_ignored"] = want["kv_map_ignored"] = cells(S.CROSS)
    want["context_stride_is_len"] = cells(("cross_len",))
    want["len_not_clamped"] = want["len_of_next_sample"] = cells(("cross_len", "bias", "causal"))
    want["bias_index_off_by_one"] = want["bias_of_next_head"] = want["bias_sign_flipped"] = cells(("bias",))
    want["causal_diagonal_masked"] = want["causal_future_key_visible"] = cells(("causal",))
    want["pad_row_not_zero"] = cells(("bias", "causal"))
    assert set(want) == set(FAULTS) and len(FAULTS) == 21
    for fault in FAULTS:
        got = {(c["entry"], c["expect"], c["dtype"]) for c in S.CASES if applicable(c, fault)}
        assert got == want[fault], (fault, got ^ want[fault])


def test_the_off_by_one_mask_hides_in_random_data_and_shows_in_negative_scores():
    """Why the "negative" mode exists: `key > len` where `key >= len` is meant lets one zero-staged key of the ragged block take part.  At
    S = 77 on N(0,1) data it moves a bf16 result by less than the bound (and by 6e-3, under the flat 1.5e-2 of the older tests); against
    scores <= -6 it takes over the softmax."""
    c = S.by_name("cross_mfma_bf16_d64_r64_k77_n2h2_hard_identity_random")
    o, ref, bound, live = _ref(c)
    buf = emulate(c, o, "ragged_mask_off_by_one")
    problems, worst = S.check_output(c, buf, ref, bound, live)
    print(f"random: err / bound {worst:.3f}, max |err| {S.max_abs_err(c, buf, ref, live):.2e} with key 77 unmasked")
    assert not problems and worst < 1.0 and S.max_abs_err(c, buf, ref, live) < 1.5e-2 and applicable(c, "ragged_mask_off_by_one") is False
    c = S.by_name("cross_mfma_bf16_d64_r64_k77_n2h2_hard_identity_negative")
    o, ref, bound, live = _ref(c)
    problems, worst = S.check_output(c, emulate(c, o, "ragged_mask_off_by_one"), ref, bound, live)
    assert problems and worst > 10.0 and applicable(c, "ragged_mask_off_by_one"), worst


# ---- d. the bound ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cross_mfma_bf16_d64_r64_k77_n2h2_hard_identity_random", "cross_fp32_f32_d96_r17_k43_n2h3_odd_out_kv_repeat_random",
                                  "bias_mfma_f16_d64_r65_k65_n3h3_plain_identity_random_len65.1.32", "causal_fp32_bf16_d128_r100_k100_n3h2_plain_identity_random_len100.1.33"])
def test_the_bound_scales_with_v(name):
    """Scaling v by 2^10 scales the reference and everything in the bound but the f16 subnormal floor by exactly 2^10."""
    c = S.by_name(name)
    o = S.make_operands(c)
    ref, bound, live = S.reference(c, o)
    ref2, bound2, _ = S.reference(c, dict(o, v=o["v"] * 1024.0))
    fl = S.FLOOR[c["dtype"]] * live.view(-1, 1)
    assert torch.equal(ref2, ref * 1024.0) and torch.allclose(bound2 - fl, (bound - fl) * 1024.0, rtol=1e-12, atol=0.0)


def test_the_bound_is_a_statement_about_rounding_not_about_magnitude():
    """On "random" data up to d = 64 (and 515 keys) the bound stays below 3 u_out + 2 u_P + 2e-4 (16 bit: + 1e-3) of the result's magnitude w |v| wherever that is at least 0.05."""
    seen = set()
    for c in (c for c in S.CASES if c["mode"] == "random" and c["d"] <= 64):
        o, ref, bound, live = _ref(c)
        mag = torch.zeros_like(ref).view(c["n"], c["rows"], c["heads"], c["d"])
        for i in range(c["n"]):
            q, k, v, s, b, masked = S.sample_scores(c, o, i)
            w = torch.softmax((s + b).masked_fill(masked, float("-inf")), -1)
            mag[i, : q.shape[1]] = (w @ v.abs()).permute(1, 0, 2)
        mag = mag.reshape(ref.shape)
        assert bool((ref.abs() <= mag * (1 + 1e-12)).all())
        u_p = S.U[c["dtype"]] if c["expect"] == "mfma" else 0.0
        big = live.view(-1, 1) & (mag >= 0.05)                # (the absolute subnormal term is no multiple of a tiny w |v|)
        ratio = float(((bound - S.FLOOR[c["dtype"]])[big] / mag[big]).max())
        assert ratio < 3 * S.U_OUT[c["dtype"]] + 2 * u_p + (2e-4 if c["dtype"] == F32 else 1e-3), (c["name"], ratio)
        seen.add((c["entry"], c["expect"], c["dtype"]))
    assert len(seen) == 20
