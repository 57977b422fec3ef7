"""The 3x3 halo-convolution parity cases (tests/conv_halo_cases.py) held to account without a GPU: every case is routed to the kernel it
names, the table covers every instance it claims to, its geometry has the properties it promises, and the checker the GPU test relies on
passes a plain emulation of the kernels and fails each of a list of planted faults.  dc_igemm_variant, dc_igemm_instance (the template
instance and the patch geometry the library itself works out for the launch) and the probes run on the host alone, as in
tests/test_igemm_dispatch.py."""
import ctypes
import itertools
import re

import pytest
import torch

import conv_halo_cases as G
import test_igemm_dispatch as D

FAKE = D.FAKE
F32, BF16, F16 = G.F32, G.BF16, G.F16


def _lib():
    mod = D._load_lib()
    return mod, mod.lib()


def _params(c, mod):
    return mod.IgemmParams(**G.igemm_fields(c, {f: FAKE for f in G.PTR_FIELDS}))


GEOM = ("tw", "th", "ni", "tiles_x", "tiles_y", "hw", "HR", "nxl", "mos", "xbuf", "sws", "lpt", "tiles_m", "grid")      # include/dcamd.h


def _instance(lib, p):
    """(instance string, {geometry field: value}) from the library; the geometry is all -1 where the library wrote none."""
    geom = (ctypes.c_int32 * len(GEOM))(*([-1] * len(GEOM)))
    return lib.dc_igemm_instance(p, geom).decode(), dict(zip(GEOM, geom))


def _halo_key(name):
    """(NW, TAPS, MODE, staggered) of a conv3_halo_kernel instance string without pn, None for every other string."""
    m = re.fullmatch(r"conv3_halo_kernel<\w+,(\d+),(\d+),(\d+)(,stag)?>", name)
    return m and (int(m[1]), int(m[2]), int(m[3]), bool(m[4]))


def _set_env(c, monkeypatch):
    monkeypatch.delenv("DCAMD_HALO_NO_STAG", raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)


# ---- a. routing -------------------------------------------------------------------------------------------------------------------
def test_case_names_are_unique_and_envs_are_the_per_call_switch_only():
    names = [c["name"] for c in G.CASES]
    assert len(names) == len(set(names))
    assert all(set(c["env"]) <= {"DCAMD_HALO_NO_STAG"} for c in G.CASES)
    assert all(c["family"] in G.FAMILIES for c in G.CASES)
    assert all((c["family"] == "halo8_lockstep") == bool(c["env"]) for c in G.CASES)
    fams = [G.by_name(n)["family"] for n in G.REPEAT_CASES]
    assert fams == ["halo4", "halo8", "halo8", "ws_gn", "up4"] and G.geometry(G.by_name(G.REPEAT_CASES[2]))["mosaic"]
    assert max(G.rows(c) for c in G.CASES) <= 2 ** 14 and max(c["Cout"] for c in G.CASES) <= 256
    for c in G.CASES:          # sample maps repeat and reorder, n_src differs from n_img
        o = G.make_operands(c)
        for m, n_in in (("map0", c["n_src"]), ("map1", c["n_src"]), ("map2", c["n_src2"]), ("rowvec_map", c["n_vec"]), ("res_map", c["n_res"])):
            if m in o:
                v = o[m].tolist()
                assert n_in != c["n_img"] and v != list(range(len(v))) and max(v) < n_in, (c["name"], m, v)
                assert len(v) == 2 or (len(set(v)) < len(v) and v != sorted(v)), (c["name"], m, v)       # (two samples cannot do both)
        if "map0" in o and "map1" in o:
            assert o["map0"].tolist() != o["map1"].tolist(), c["name"]


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_every_case_is_routed_to_the_kernel_it_names(c, monkeypatch):
    mod, lib = _lib()
    _set_env(c, monkeypatch)
    p = _params(c, mod)
    assert lib.dc_igemm_variant(p).decode() == c["expect"], c["name"]
    # the instance and the geometry the table claims are the library's own (the ws cases' "+silu" is this table's label, no template argument)
    name, lg = _instance(lib, p)
    assert c["instance"] == G.instance(c) and name == G.instance(c).replace("+silu", ""), (c["name"], name)
    g = G.geometry(c)
    if g["kind"] == "pipe_up4":
        assert set(lg.values()) == {-1}
    else:
        mine = dict({k: g[k] for k in ("tw", "th", "ni", "tiles_x", "tiles_y", "HR", "nxl")}, mos=int(g["mosaic"]), xbuf=int(g["xbuf"]))
        assert {k: lg[k] for k in mine} == mine, (c["name"], lg, mine)
        assert 1 << lg["lpt"] == g["tiles_x"] * g["tiles_y"]
        assert lg["sws"] == {"thin": 0, "ws": 2}.get(g["kind"], min(g["tw"].bit_length() - 1, 4) - 2), (c["name"], lg)
    # the quad-record part count the reference uses is the library's; the mosaic and the tap-gather kernel form none
    kw = G.igemm_fields(c, {f: FAKE for f in G.PTR_FIELDS})
    kw.pop("qstats", None)
    parts = lib.dc_igemm_qstats_parts(mod.IgemmParams(**kw))
    assert parts == G.qparts(c), (c["name"], parts)
    if G.geometry(c)["mosaic"] or G.kind(c) == "pipe_up4":
        assert parts == 0
    if parts:
        pp = G.part_pixels(c)
        assert pp.shape[0] == parts and sorted(pp.flatten().tolist()) == list(range(c["Hout"] * c["Wout"]))


# ---- b. coverage ------------------------------------------------------------------------------------------------------------------
# every instance of conv3_halo_kernel<T, NW, TAPS, MODE, STG> dc_conv3_halo_plan can name without pn_out
ALL_HALO = {(8, 9, m, s) for m in (0, 1, 2) for s in (False, True)} | {(8, 4, m, False) for m in (0, 1, 2)} | \
           {(4, 9, m, False) for m in (0, 1)} | {(4, 4, m, False) for m in (0, 1)}


def test_the_table_reaches_every_instance_or_proves_it_unreachable(monkeypatch):
    mod, lib = _lib()
    for dt in G.DTS:
        mine = [c for c in G.CASES if c["dtype"] == dt]
        reached = set()
        for c in mine:         # what the library says it launches, not what this table derives
            _set_env(c, monkeypatch)
            reached.add(_halo_key(_instance(lib, _params(c, mod))[0]))
        reached -= {None}
        assert reached | set(G.UNREACHABLE) == ALL_HALO and not reached & set(G.UNREACHABLE), (dt, ALL_HALO - reached)
        assert {(c["gn_silu"]) for c in mine if G.kind(c) == "ws"} == {0, 1}
        assert {("gn" in c["use"]) for c in mine if G.kind(c) == "thin"} == {False, True}
        assert any(G.kind(c) == "pipe_up4" for c in mine)
        assert {c["expect"] for c in mine} == {e % G.DTN[dt] for e in ("conv3_halo<%s,4w>", "conv3_halo<%s,8w>", "conv3_ws<%s,gn>", "conv3_thin<%s>",
                                                                       "conv3_up4<%s,4w>", "conv3_up4<%s,8w>", "igemm_pipe_up4<%s,256x128,3st>")}
    # what the table does not reach is out of the launcher's reach: on a probe grid every 4-wave problem gets the buffer-descriptor loaders,
    # and only a source sample of 2 GiB flips it
    monkeypatch.delenv("DCAMD_HALO_NO_STAG", raising=False)
    n = 0
    for dt, (H, W), c0, pad, up4 in itertools.product(G.DTS, [(16, 16), (16, 32), (32, 16), (64, 64), (128, 128), (512, 256), (16, 1024)], (1, 4, 20), (0, 64),
                                                      (0, 1)):
        c = G._case("probe", dt, "up4" if up4 else "halo4", H, W, 1, C0=c0 * G.BKE[dt], ld0_pad=pad, up4=up4, use={"bias"},
                    expect="conv3_up4<%s,4w>" if up4 else "conv3_halo<%s,4w>")
        assert lib.dc_igemm_variant(_params(c, mod)).decode() == c["expect"]
        assert G.halo_instance_key(c) == _halo_key(_instance(lib, _params(c, mod))[0]) == (4, 4 if up4 else 9, 1, False), c
        n += 1
    assert n == 252
    for key, why in G.UNREACHABLE.items():
        assert "2 GiB" in why
        up4 = key[1] == 4
        c = G._case("probe", BF16, "up4" if up4 else "halo4", 4096, 4096, 1, C0=64, up4=up4, use={"bias"},
                    expect="conv3_up4<%s,4w>" if up4 else "conv3_halo<%s,4w>")
        assert 4096 * 4096 * 64 * 2 == 2 ** 31 and G.halo_instance_key(c) == _halo_key(_instance(lib, _params(c, mod))[0]) == key


def test_the_cases_have_the_geometry_they_are_there_for():
    geo = {c["name"]: G.geometry(c) for c in G.CASES}
    halo = [c for c in G.CASES if G.kind(c) in ("halo", "up4")]
    assert {geo[c["name"]]["ni"] for c in halo} == {1, 2, 4, 8, 32}
    for ni in (2, 4, 8, 32):       # a ragged last patch behind a full one
        assert any(geo[c["name"]]["ni"] == ni and c["n_img"] > ni and c["n_img"] % ni for c in halo), ni
    assert any(geo[c["name"]]["mosaic"] and c["n_img"] < 32 for c in halo)
    for fam in G.FAMILIES:
        mine = [c for c in G.CASES if c["family"] == fam]
        for dt in G.DTS:
            md = [c for c in mine if c["dtype"] == dt]
            assert any(c["H"] > c["W"] for c in md) and any(c["H"] < c["W"] for c in md), (fam, dt)
            assert any(geo[c["name"]]["tiles_x"] > 1 for c in md) or fam in ("thin", "up4"), (fam, dt)
            assert any(geo[c["name"]]["tiles_y"] > 1 for c in md), (fam, dt)
            assert any(c["ld0"] > c["C0"] for c in md) and any(c["out_ld"] > c["Cout"] for c in md), (fam, dt)
            assert {c["Cout"] for c in md} >= ({128, 200} if fam != "thin" else {1, 3, 5, 16}), (fam, dt)
            assert any(c["C1"] for c in md) or fam == "up4", (fam, dt)
            if fam not in ("thin", "up4"):
                assert any("residual" in c["use"] and "res_map" in c["use"] and c["res_ld"] > c["Cout"] for c in md), (fam, dt)
                assert any(c["C2"] and c["ld2"] > c["C2"] and "map2" in c["use"] for c in md), (fam, dt)
                assert any(c["C1"] and (c["C0"] // G.BKE[dt]) % 2 == 1 and {"map0", "map1"} & c["use"] for c in md), (fam, dt)
                assert any({"rowvec", "rowvec_map", "bias"} <= c["use"] for c in md), (fam, dt)
            if fam != "thin":
                assert any("qstats" in c["use"] and G.qparts(c) >= 2 for c in md), (fam, dt)
            if dt != F32:
                assert any(c["out_dtype"] == F32 for c in md), (fam, dt)
            if fam.startswith("halo8") or fam == "up4":      # 8x8 images: two per wave, the half-wave form of the quad records
                assert any("qstats" in c["use"] and (c["H"], c["W"]) == (8, 8) for c in md), (fam, dt)
            if fam.startswith("halo8"):
                assert any(geo[c["name"]]["mosaic"] and (c["C0"] + c["C1"]) // G.BKE[dt] == 16 for c in md), (fam, dt)
            if fam == "ws_gn" and dt != F32:
                assert any(c["C0"] + c["C1"] == 512 for c in md)
            if fam == "thin":
                assert all(c["tile_n"] == 32 for c in md)
    # XB = 1 on the 8-wave patch: H >= 64 with W = 8, one and two tiles, staggered and lock-step
    for fam in ("halo8", "halo8_lockstep"):
        assert {geo[c["name"]]["tiles_y"] for c in G.CASES if c["family"] == fam and geo[c["name"]]["xbuf"]} == {1, 2}


# ---- c. the checker checks --------------------------------------------------------------------------------------------------------
HALO_FAMS = {"halo4", "halo8", "halo8_lockstep"}
# fault -> the families in which it must be planted (in all three dtypes)
FAULTS = {
    "tap_dropped_at_border": set(G.FAMILIES),
    "taps_transposed": set(G.FAMILIES),
    "padding_from_previous_image": {"halo8", "halo8_lockstep", "up4"},
    "seam_column_from_wrong_side": set(G.FAMILIES),
    "sample_map_shifted": set(G.FAMILIES),
    "prologue_on_padding": {"ws_gn", "thin"},
    "side_source_left_out_of_second_n_tile": HALO_FAMS | {"ws_gn"},
    "residual_of_next_sample": HALO_FAMS | {"ws_gn"},
    "up4_phases_a_b_swapped": {"up4"},
    "quad_record_part_swapped": HALO_FAMS | {"ws_gn", "up4"},
    "pad_column_written": set(G.FAMILIES),
    "row_past_m_written": set(G.FAMILIES),
}


def applicable(c, fault):
    g, use = G.geometry(c), c["use"]
    return {"tap_dropped_at_border": True, "taps_transposed": True,
            "padding_from_previous_image": g["ni"] > 1 and g["kind"] != "pipe_up4",
            "seam_column_from_wrong_side": g["tiles_x"] > 1 or g["tiles_y"] > 1,
            "sample_map_shifted": True,
            "prologue_on_padding": "gn" in use,
            "side_source_left_out_of_second_n_tile": c["C2"] > 0 and c["Cout"] > 128,
            "residual_of_next_sample": "residual" in use,
            "up4_phases_a_b_swapped": bool(c["up4"]),
            "quad_record_part_swapped": "qstats" in use and G.qparts(c) >= 2,
            "pad_column_written": c["out_ld"] > c["Cout"], "row_past_m_written": True}[fault]


def _conv_input(c, o, shift0=None, prologue_everywhere=False):
    """[n_img, Hin, Win, C] fp32: what the 3x3 taps read — the gathered sources as the compute type holds them, the prologue in fp32 with the
    device's formula on real pixels, upsampled for the four-phase form."""
    x = G.gathered(c, o, torch.float32, shift0)
    if "gn" in c["use"]:
        x = G.prologue_device(c, o, x)
    return G.upsample2(x) if c["up4"] else x


def _finish_rows(c, o, acc, rows_, res_shift=0, drop_side_from=None):
    """The epilogue of rows `rows_` (a LongTensor) in fp32: acc [len, Cout] + side source + bias + row vector + residual."""
    HW = c["Hout"] * c["Wout"]
    x = acc
    if c["C2"]:
        s = G.side_rows(c, o)[rows_] @ o["w2"].t()
        if drop_side_from is not None:
            s[:, drop_side_from:] = 0.0
        x = x + s
    if "bias" in o:
        x = x + o["bias"]
    if "rowvec" in o:
        x = x + G.per_row(c, o, "rowvec", "rowvec_map")[rows_]
    if "residual" in o:
        x = x + G.residual_rows(c, o, res_shift)[rows_]
    return x


def _records(c, val):
    """Quad records of the fp32 values val [M, Cout], plainly (fp64 mean and M2, stored as fp32)."""
    pp = G.part_pixels(c)
    v = val.double().view(c["n_img"], c["Hout"] * c["Wout"], c["Cout"] // 4, 4)[:, pp]
    mean = v.mean((2, 4))
    m2 = ((v - mean[:, :, None, :, None]) ** 2).sum((2, 4))
    return torch.stack([mean, m2], -1).float()


def emulate(c, o):
    """The kernel, plainly: operands as the compute type holds them, the prologue in fp32, fp32 accumulation tap by tap, the epilogue in fp32
    in the documented order.  Returns the pieces the planted faults need: the taps P [M, 9, C], the weights Wm [Cout, 9, C], the conv
    input X and the fp32 output values val [M, Cout]."""
    X = _conv_input(c, o)
    Ct = c["C0"] + c["C1"]
    M = G.rows(c)
    P = G.unfold3(X).view(M, 9, Ct)
    Wm = G.w_matrix(c, o, torch.float32).view(c["Cout"], 9, Ct)
    acc = torch.zeros(M, c["Cout"])
    for tap in range(9):
        acc += P[:, tap] @ Wm[:, tap].t()
    return dict(X=X, P=P, Wm=Wm, val=_finish_rows(c, o, acc, torch.arange(M)))


def to_buffers(c, val):
    """The output rounded into a sentinel-filled buffer, and the quad records likewise where the case has them."""
    M, co, ld = G.rows(c), c["Cout"], c["out_ld"]
    buf = G.new_output(c)
    buf[: M * ld].view(M, ld)[:, :co] = val.to(G.TD[c["out_dtype"]])
    qbuf = None
    if "qstats" in c["use"]:
        qbuf = G.new_qstats(c)
        rec = _records(c, val)
        qbuf[: rec.numel()] = rec.flatten()
    return buf, qbuf


def plant(c, o, em, fault):
    """(buf, qbuf) of the emulation with one fault at one place."""
    g = G.geometry(c)
    Ho, Wo, co, ld = c["Hout"], c["Wout"], c["Cout"], c["out_ld"]
    HW, M = Ho * Wo, G.rows(c)
    up = 2 if c["up4"] else 1
    val = em["val"].clone()
    row_of = lambda n, y, x: n * HW + y * Wo + x

    def redo(row, taps, **kw):         # one row again from its (altered) taps
        acc = torch.zeros(1, co)
        for tap in range(9):
            acc += taps[tap][None] @ em["Wm"][:, tap].t()
        val[row] = _finish_rows(c, o, acc, torch.tensor([row]), **kw)[0]

    if fault == "tap_dropped_at_border":
        row = row_of(0, 0, Wo // 2)
        taps = em["P"][row].clone()
        taps[3] = 0.0                                          # (ky 1, kx 0): a real pixel
        redo(row, taps)
    elif fault == "taps_transposed":
        row = row_of(0, 1, 2)
        redo(row, em["P"][row].view(3, 3, -1).transpose(0, 1).reshape(9, -1))
    elif fault == "padding_from_previous_image":
        x0 = Wo // 2
        row = row_of(1, 0, x0)
        taps = em["P"][row].clone()
        for kx in range(3):
            xx = x0 - 1 + kx
            taps[kx] = em["X"][0, Ho - 1, xx] if 0 <= xx < Wo else 0.0
        redo(row, taps)
    elif fault == "seam_column_from_wrong_side":
        taps3 = None
        if g["tiles_x"] > 1:
            row = row_of(0, 2, up * g["tw"] - 1)
            taps3 = em["P"][row].clone().view(3, 3, -1)
            taps3[:, 2] = taps3[:, 0]                          # the columns of the next tile: the other side's instead
        else:
            row = row_of(0, up * g["th"] - 1, 2)
            taps3 = em["P"][row].clone().view(3, 3, -1)
            taps3[2] = taps3[0]
        redo(row, taps3.reshape(9, -1))
    elif fault == "sample_map_shifted":
        n = min(1, c["n_img"] - 1)
        Xs = _conv_input(c, o, shift0=(n, 1))
        row = row_of(n, 1, 1)
        redo(row, G.unfold3(Xs[n:n + 1]).view(HW, 9, -1)[1 * Wo + 1])
    elif fault == "prologue_on_padding":
        row = row_of(0, 0, 0)
        pv = G.prologue_device(c, o, torch.zeros(c["n_img"], 1, 1, c["C0"] + c["C1"]))[0, 0, 0]       # act(shift) of sample 0
        taps = em["P"][row].clone()
        for tap in (0, 1, 2, 3, 6):                            # the padding taps of the corner pixel
            taps[tap] = pv
        redo(row, taps)
    elif fault == "side_source_left_out_of_second_n_tile":
        row = row_of(0, 1, 1)
        redo(row, em["P"][row], drop_side_from=128)
    elif fault == "residual_of_next_sample":
        row = row_of(0, 1, 1)
        redo(row, em["P"][row], res_shift=1)
    elif fault == "up4_phases_a_b_swapped":
        val[row_of(0, 2, 3)] = em["val"][row_of(0, 3, 2)]      # (a, b) = (0, 1) computed with the taps of (1, 0)
    buf, qbuf = to_buffers(c, val)
    if fault == "quad_record_part_swapped":
        nq = co // 4
        rec = qbuf[: c["n_img"] * G.qparts(c) * nq * 2].view(c["n_img"], G.qparts(c), nq, 2)
        rec[0, 0], rec[0, 1] = rec[0, 1].clone(), rec[0, 0].clone()      # one wave's records (every quad of its N tile) under its neighbour's part
    if fault == "pad_column_written":
        buf[(M // 2) * ld + co] = 0.0
    if fault == "row_past_m_written":
        buf[M * ld + 3] = 0.0
    return buf, qbuf


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_the_checker_passes_the_emulated_kernel_and_fails_every_planted_fault(c):
    o = G.make_operands(c)
    ref, bound, det = G.reference(c, o, detail=True)
    assert ref.shape == (G.rows(c), c["Cout"]) and bool((bound > 0).all())
    em = emulate(c, o)
    buf, qbuf = to_buffers(c, em["val"])
    problems, worst = G.check_output(c, buf, ref, bound, qbuf, det["e"])
    _, worst_out = G.check_output(c, buf, ref, bound)
    print(f"{c['name']} [{c['family']}] {c['instance']}: emulation err / bound {worst_out:.3f} (with quad records {worst:.3f}); flagged inputs "
          f"{100 * det['flagged_share']:.3f} %, largest ambiguity term / output std {det['amb_max'] / det['out_std']:.2e}")
    assert not problems, problems
    # the two caps on the prologue's ambiguity term, on the reference alone
    assert det["flagged_share"] <= 0.02 and det["amb_max"] <= 0.01 * det["out_std"], det
    if "gn" in c["use"] and c["dtype"] != F32:
        assert det["flagged_share"] > 0.0           # the flagging is alive
    for fault in FAULTS:
        if applicable(c, fault):
            fb, fq = plant(c, o, em, fault)
            problems, worst = G.check_output(c, fb, ref, bound, fq, det["e"])
            assert problems, f"{c['name']}: the checker lets '{fault}' through (worst err / bound {worst:.3g})"


@pytest.mark.parametrize("name", ["ws_gn_bf16_16x16_silu_two_maps", "ws_gn_f16_16x16_silu_two_maps", "ws_gn_bf16_8x32_res_map0", "thin_f16_16x16_c3_gn",
                                  "ws_gn_bf16_16x16_silu_c512"])
def test_only_flagged_prologue_elements_round_the_other_way(name):
    """The prologue evaluated in fp32 with the device's formula against the fp64 operand of the reference: they differ only on flagged
    elements, and there by exactly the spacing the bound charges."""
    c = G.by_name(name)
    o = G.make_operands(c)
    a, amb, flagged = G.prologue(c, o, G.gathered(c, o))
    dev = G.prologue_device(c, o, G.gathered(c, o, torch.float32)).double()
    differ = dev != a
    assert not bool((differ & ~flagged).any()), int((differ & ~flagged).sum())
    assert bool(((dev - a).abs()[differ] == amb[differ]).all())
    assert 0 < int(flagged.sum()) <= 0.02 * flagged.numel()


def test_every_fault_is_planted_in_every_family_and_dtype():
    for fault, fams in FAULTS.items():
        cells = {(c["family"], c["dtype"]) for c in G.CASES if applicable(c, fault)}
        assert cells == {(f, dt) for f in fams for dt in G.DTS}, (fault, cells)


def test_the_bound_is_a_statement_about_rounding_not_about_magnitude():
    """A correctly rounded 16-bit output uses most of its bound (the rounding term is tight by nature), fp32 accumulation little of the
    accumulation term: the bound has no slack to hide a fault in.  With the prologue too."""
    for name, lo, hi in (("halo4_bf16_16x16_b0", 0.5, 1.0), ("halo8_bf16_8x8_n11_b0", 0.5, 1.0), ("ws_gn_bf16_16x16_silu_two_maps", 0.5, 1.0),
                         ("halo4_f32_16x16_b0", 0.0, 0.2), ("ws_gn_f32_16x16_silu_two_maps", 0.0, 0.2), ("up4_f32_16x16_4w", 0.0, 0.2)):
        c = G.by_name(name)
        o = G.make_operands(c)
        ref, bound = G.reference(c, o)
        _, worst = G.check_output(c, to_buffers(c, emulate(c, o)["val"])[0], ref, bound)
        assert lo < worst <= hi, (name, worst)
