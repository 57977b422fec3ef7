"""The GroupNorm / LayerNorm parity cases (tests/norm_cases.py) held to account without a GPU: every case is routed to the launch sequence
it names, the table fills every cell it claims to (and what it leaves out cannot exist), K is what torch's own fp32 kernels measure, and
the checker the GPU test relies on passes a plain fp32 emulation of the kernels and fails each of a list of planted faults.
dc_groupnorm_variant / dc_layernorm_variant run on the host alone, as in tests/test_norm_dispatch.py; DCAMD_GN_SPAN / DCAMD_GN_NO_WAVE are
read once per process, so the cases that set one are routed in a child process."""
import collections
import json
import math
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import norm_cases as N
import test_norm_dispatch as D
from norm_cases import BF16, F16, F32

SMALL = [c for c in N.CASES if not c["big"]]


def _variants(cases):
    mod = D._load_lib()
    lib = mod.lib()
    out = []
    for c in cases:
        if c["kind"] == "gn":
            out.append(lib.dc_groupnorm_variant(mod.GroupnormParams(**N.gn_fields(c, N.fake_ptrs(c)))).decode())
        else:
            out.append(lib.dc_layernorm_variant(mod.LayernormParams(**N.ln_fields(c, N.fake_ptrs(c)))).decode())
    return out


def _clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("DCAMD_") or k == "DCAMD_LIB"}


# ---- routing --------------------------------------------------------------------------------------------------------------------
def test_case_names_are_unique_and_envs_are_the_two_switches():
    names = [c["name"] for c in N.CASES]
    assert len(names) == len(set(names))
    assert all(c["env"] in ({}, N.SPAN, N.NO_WAVE) for c in N.CASES)
    assert all(not c["env"] for c in N.LN_CASES)
    for name in N.REPEAT_CASES:
        c = N.by_name(name)
        assert c["HW"] * (c["C"] + c["C1"]) * (4 if c["dtype"] == F32 else 2) >= 1 << 20 and not c["env"], name
    for c in N.GN_CASES:       # only what needs it is large; a map never names the last allocated source sample
        assert c["big"] == (c["HW"] * (c["C"] + c["C1"]) * (4 if c["dtype"] == F32 else 2) > 4 << 20), c["name"]
        if c["use"] & {"map0", "map1"}:
            assert c["n"] > c["n_src"] - 1 >= 2, c["name"]      # more destination samples than sources used


@pytest.mark.parametrize("env", [{}, N.SPAN, N.NO_WAVE], ids=["default", "DCAMD_GN_SPAN", "DCAMD_GN_NO_WAVE"])
def test_every_case_is_routed_to_the_launch_sequence_it_names(env):
    cases = [c for c in N.CASES if c["env"] == env]
    assert cases
    if not env and not [k for k in os.environ if k in N.SWITCHES]:
        got = _variants(cases)
    else:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "variants.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, env=dict(_clean_env(), **env), timeout=600)
            with open(path) as f:
                got = json.load(f)
    bad = [(c["name"], g, c["expect"]) for c, g in zip(cases, got) if g != c["expect"]]
    assert not bad and len(got) == len(cases), bad[:10]
    print(f"{len(cases)} cases routed:", dict(collections.Counter(got)))


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def test_groupnorm_cells_are_all_filled_and_the_missing_ones_cannot_exist():
    have = {(N.family(c), c["dtype"], c["silu"], N.gn_form(c)) for c in N.GN_CASES}
    want = set()
    for fam in N.GN_FAMILIES:
        for dt in N.DTS:
            for silu in ((0,) if fam in N.STATS_ONLY else (0, 1)):
                for form in (N.GN_FORMS if fam in N.GN_PLAIN_ROUTES else ("one", "one_map")):
                    want.add((fam, dt, silu, form))
    assert want <= have, sorted(want - have)
    print(f"{len(want)} GroupNorm cells (route x dtype x SiLU x source form), all filled:")
    for cell in sorted(want):
        print("  ", cell, next(c["name"] for c in N.GN_CASES if (N.family(c), c["dtype"], c["silu"], N.gn_form(c)) == cell))
    # what cannot exist: shown on the variant export
    mod = D._load_lib()
    lib = mod.lib()
    variant = lambda c: lib.dc_groupnorm_variant(mod.GroupnormParams(**N.gn_fields(c, N.fake_ptrs(c)))).decode()
    for dt in N.DTS:
        e = N.EPC[dt]
        for fam in N.GN_QUAD_ROUTES:
            assert (fam, "two") in N.UNREACHABLE
            if not N._gn_cell(fam, dt, 0, "one")["env"]:       # (the switches are not set in this process)
                c = N._gn_cell(fam, dt, 0, "one")
                assert variant(c) == c["expect"]
                two = dict(c, C1=c["C"], use=c["use"] | {"x1"})
                assert variant(two) == "invalid" and "qstats needs one source" in lib.dc_last_error().decode(), (fam, dt)
        # gn_wave_kernel never takes records: the wave cell's problem with records goes to gn_image_kernel
        w = N._gn_cell("wave", dt, 1, "one")
        assert variant(w) == "wave"
        assert variant(dict(w, groups=3, qparts=4, use=w["use"] | {"qstats"})) == "image"
        # the split route with records is qfold+apply
        sa = N._gn("probe", dt, "stats+apply", n=2, HW=8, C=520 * e, groups=10, splits=2)
        assert variant(sa) == "stats+apply" and variant(dict(sa, qparts=2, use=sa["use"] | {"qstats"})) == "qfold+apply"
    assert {k for k in N.UNREACHABLE if k[0] in N.GN_FAMILIES} == {(f, "two") for f in N.GN_QUAD_ROUTES} | {("wave", "qstats"), ("stats+apply", "qstats")}


EDGES = [  # (family, tag) every dtype must have
    ("wave", "nch4"), ("wave", "nch8"), ("wave", "nch16"), ("wave", "nch32"), ("wave", "hw_below_lanes"), ("wave", "cp_limit"), ("wave", "seam"),
    ("image", "hw_below_pl"), ("image", "unroll0"), ("image", "unroll_rem"), ("image", "cp1"), ("image", "cp48"), ("image", "cp512"), ("image", "cpg1"),
    ("image", "groups512"), ("image", "no_wave"), ("image", "seam"), ("image-q", "cp1"), ("image-q", "qparts1"),
    ("stats+apply", "splits7"), ("stats+apply", "splits1"), ("stats+apply", "splits_hw"), ("stats+apply", "above_4mib"),
    ("stats", "groups64"), ("qaffine", "groups_above_64"),
    ("span", "cp1"), ("span", "records_below_2048"), ("span", "records_at_2048"), ("qfold+span", "records_above_2048"), ("span", "qparts1"),
    ("qfold+span", "default_route_1mib"), ("qfold+apply", "qparts1"),
    ("wave", "offset"), ("image", "offset"), ("stats+apply", "offset"), ("image-q", "offset"),
    ("wave", "tiny"), ("image", "tiny"), ("stats+apply", "tiny"), ("image-q", "tiny"), ("stats", "tiny"), ("qaffine", "tiny"), ("span", "tiny"),
    ("qfold+span", "tiny"), ("qfold+apply", "tiny"),
    ("wave", "few"), ("image", "few"), ("stats+apply", "few"), ("image-q", "few"), ("stats", "few"), ("qaffine", "few"), ("span", "few16"), ("qfold+span", "few80"),
]


def test_groupnorm_edges_have_the_properties_they_are_there_for():
    for dt in N.DTS:
        mine = [c for c in N.GN_CASES if c["dtype"] == dt]
        tags = {(N.family(c), c["tag"]) for c in mine}
        assert set(EDGES) <= tags, (dt, sorted(set(EDGES) - tags))
        e = N.EPC[dt]
        cp = lambda c: (c["C"] + c["C1"]) // e
        cpg = lambda c: (c["C"] + c["C1"]) // c["groups"]
        es = 4 if dt == F32 else 2
        tpr = lambda c: 1 << max(0, (cp(c) - 1).bit_length())
        fam = lambda f: [c for c in mine if N.family(c) == f]
        wave = fam("wave")
        # wave: which instance each case runs, all four per dtype; the last workgroup part empty; pixels against pixel lanes; lanes off
        inst = {c["name"]: N.wave_nch(c) for c in wave}
        print(N.DTN[dt], "gn_wave_kernel instances:", inst)
        for nch in (4, 8, 16, 32):
            assert inst[f"gn_wave_nch{nch}_{N.DTN[dt]}"] == nch
        assert {c["n"] % 4 for c in wave} >= {1, 2, 3}
        assert {1, 2, 4} <= {c["HW"] for c in wave if c["HW"] < 64 // tpr(c)}
        assert any(c["HW"] % (64 // tpr(c)) for c in wave) and any(cp(c) == 64 for c in wave)
        assert any(c["C1"] and {"map0", "map1"} <= c["use"] and (c["C"] // e) & (c["C"] // e - 1) for c in wave)
        # image
        img = fam("image") + fam("image-q")
        pl = lambda c: 512 // tpr(c)
        assert any(c["HW"] < pl(c) for c in img) and any(pl(c) <= c["HW"] <= 3 * pl(c) for c in img) and any(c["HW"] > 4 * pl(c) and c["HW"] % (4 * pl(c)) for c in img)
        assert {1, 48, 512} <= {cp(c) for c in img}
        assert {1, 2, 8, 32, 512} <= {c["groups"] for c in img} and any(cpg(c) == 1 for c in img) and any(c["groups"] == 512 and cpg(c) > 1 for c in img)
        assert any(c["C1"] and {"map0", "map1"} <= c["use"] for c in fam("image"))
        # a 16-byte chunk that straddles groups unevenly: cpg neither a multiple nor a divisor of the chunk
        for f in ("wave", "image", "stats+apply"):
            assert any(cpg(c) % e and e % cpg(c) for c in fam(f)), (dt, f)
        # stats+apply
        sa = fam("stats+apply")
        assert any(cp(c) > 512 and (cp(c) + 255) // 256 == 3 for c in sa)
        assert any(c["HW"] % c["splits"] for c in sa) and any(c["splits"] == 1 for c in sa) and any(c["splits"] == c["HW"] > 1 for c in sa)
        assert any(c["C1"] and {"map0", "map1"} <= c["use"] for c in sa)
        big = [c for c in sa if c["HW"] * cp(c) * 16 > 4 << 20]
        assert big and all(c["splits"] == min(64, max(1, c["HW"] // 256)) for c in big)      # dc_groupnorm_splits' own value
        # statistics only
        assert any(c["groups"] == 64 and c["C1"] for c in fam("stats")) and any(c["groups"] > 64 and "map0" in c["use"] for c in fam("qaffine"))
        # records: always with map0 somewhere, CP 1 and 256, around 2048 records, C/4 = 96, one part
        for f in ("image-q", "span", "qfold+span", "qfold+apply", "qaffine"):
            assert any("map0" in c["use"] for c in fam(f)), (dt, f)
        sp = fam("span") + fam("qfold+span")
        rec = lambda c: c["qparts"] * (c["C"] // 4)
        assert {1, 256} <= {cp(c) for c in sp}
        assert any(rec(c) == 2048 for c in fam("span")) and any(1024 < rec(c) < 2048 for c in fam("span")) and any(2048 < rec(c) <= 2560 and c["env"] for c in fam("qfold+span"))
        assert any(c["qparts"] == 1 for c in fam("span")) and any(c["qparts"] == 1 for c in fam("qfold+apply"))
        assert any(256 % (c["C"] // 4) for c in fam("qfold+apply"))
        # data kinds
        for c in mine:
            if c["tag"] == "few":
                assert cpg(c) * c["HW"] <= 8, c["name"]
        assert all(c["HW"] * cp(c) * 16 // es * es >= 1 << 20 for c in fam("qfold+apply"))
    # the cases the issue spells out
    c = N.by_name("gn_wave_f32_group_straddles_seam")
    assert (c["C"], c["C1"], c["groups"]) == (96, 32, 2) and c["C"] % ((c["C"] + c["C1"]) // c["groups"])
    assert N.by_name("gn_wave_bf16_cp48_c384")["C"] == 384 and N.by_name("gn_wave_f32_cp24_c96")["C"] == 96
    c = N.by_name("gn_sa_splits7_f32")
    assert (c["C"], c["HW"], c["groups"], c["splits"]) == (2080, 300, 32, 7)
    assert N.by_name("gn_sa_splits7_bf16")["C"] == 4160


def test_layernorm_cells_are_all_filled_and_fp32_never_takes_two_rows_per_lane_group():
    cells = {(c["expect"], c["dtype"], c["form"], c["rows"]) for c in N.LN_CASES if c["tag"] == "cell"}
    want = {(r, dt, form, rows) for r, dts in N.LN_ROUTES.items() for dt in dts for form in N.LN_FORMS for rows in N.ln_geometries(r).values()}
    assert want <= cells, sorted(want - cells)
    print(f"{len(want)} LayerNorm cells (route x dtype x affine/modulation form x rows), all filled")
    for r, w in N.LN_WG_ROWS.items():
        assert {1, 2, w - 1, w, w + 1} <= set(N.ln_geometries(r).values()) and any(v % 2 and v not in (1, w - 1, w + 1) for v in N.ln_geometries(r).values())
    for r, dts in N.LN_ROUTES.items():
        for dt in dts:
            mine = [c for c in N.LN_CASES if c["expect"] == r and c["dtype"] == dt and "mod" in c["use"]]
            rps = {c["rows_per_sample"] for c in mine}
            assert {1, 32, 64, 16, 5} <= rps, (r, dt, rps)
            assert any(c["rows"] % c["rows_per_sample"] for c in mine) and any(c["mod_ld"] > c["C"] and not c["table6"] for c in mine)
            assert any(c["table6"] and c["mod_ld"] == 6 * c["C"] for c in mine)
            assert any("mod_map" in c["use"] and c["n_samples"] >= 3 for c in mine)       # a map with repeats, out of order (make_operands)
            assert {"offset", "tiny"} <= {c["data"] for c in mine}
    for dt in N.DTS:
        e = N.EPC[dt]
        mine = [c for c in N.LN_CASES if c["dtype"] == dt]
        assert {1, 9, 96, 97, 128, 129, 144, 1280 // e} <= {c["C"] // e for c in mine}
        assert {"mod_ld_not_4", "gamma_misaligned", "mod_misaligned"} <= {c["tag"] for c in mine if c["expect"] == "ln" and c["C"] // e <= 96}
    assert {512, 516} <= {c["C"] for c in N.LN_CASES if c["dtype"] == F32}
    # fp32 ln16x2 cannot exist
    assert ("ln16x2", F32) in N.UNREACHABLE
    got = _variants([N._ln("probe", F32, "?", rows=rows, C=C, form=form, rps=2) for C in (4, 36, 64, 384, 512) for rows in (1, 64) for form in N.LN_FORMS])
    assert set(got) == {"ln16"}, got
    o = N.make_operands(N.by_name("ln_ln16x2_bf16_rps16"))
    assert sorted(o["mod_map"].tolist()) != o["mod_map"].tolist() and len(set(o["mod_map"].tolist())) < len(o["mod_map"])


# ---- K ---------------------------------------------------------------------------------------------------------------------------
def test_k_is_four_times_what_torch_s_fp32_kernels_need():
    worst = {}
    for c in N.CASES:
        r = N.k0_ratio(c, N.make_operands(c))
        if r > worst.get(c["kind"], (0.0, ""))[0]:
            worst[c["kind"]] = (r, c["name"])
    top = max(v[0] for v in worst.values())
    k0 = 2.0 ** math.ceil(math.log2(top))
    print(f"torch fp32 against fp64, largest err / (2^-24 M_e): {worst}; K0 = {k0}, K = {4 * k0}")
    assert N.K == 4 * k0, (worst, k0, N.K)


@pytest.mark.parametrize("fast", [False, True])
def test_the_silu_error_term_holds_against_the_device_formula(fast):
    """e_act("silu") — derived in gemm_tile_cases from the two ~1-ulp hardware ops of silu_fast_f (v_exp_f32, v_rcp_f32) and the roundings
    around them — against the device formula restated in fp32 on the CPU, over the range a normalised value takes."""
    tiny = torch.logspace(-30, -1, 2000)
    x = torch.cat([torch.linspace(-12, 12, 400001), tiny, -tiny, torch.zeros(1)]).float()
    err = (N.G.silu_device(x, fast).double() - torch.nn.functional.silu(x.double())).abs()
    ratio = err / N.G.e_act("silu", x.double(), fast)
    print(f"silu fast={fast}: largest err / e_act {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0


# ---- the checker against an emulated kernel and planted faults ------------------------------------------------------------------
GN_FAULTS = ["eps", "n_minus_1", "affine_shifted", "group_index", "last_pixel", "split_dropped", "map0_ignored", "map1_ignored", "records_map_ignored",
             "silu_skipped", "last_sample_unwritten", "chunk_behind"]
LN_FAULTS = ["eps", "n_minus_1", "affine_shifted", "last_chunk", "mod_map_ignored", "pair_sample", "one_plus_scale", "last_row_unwritten", "chunk_behind"]


def _cpg(c):
    return (c["C"] + c["C1"]) // c["groups"]


def applicable(c, fault):
    u = c["use"]
    if c["kind"] == "gn":
        quad = "qstats" in u
        return {"eps": True, "n_minus_1": True, "affine_shifted": True,
                "group_index": c["groups"] > 1 and _cpg(c) % N.EPC[c["dtype"]] != 0,
                "last_pixel": c["HW"] > 1, "split_dropped": (c["qparts"] if quad else c["splits"]) > 1 and N.family(c) not in ("wave", "image"),
                "map0_ignored": "map0" in u and not (quad and "stats_only" in u), "map1_ignored": "map1" in u, "records_map_ignored": quad and "map0" in u,
                "silu_skipped": bool(c["silu"]) and "stats_only" not in u, "last_sample_unwritten": True, "chunk_behind": True}[fault]
    return {"eps": True, "n_minus_1": True, "affine_shifted": "affine" in u, "last_chunk": c["C"] > N.EPC[c["dtype"]],
            "mod_map_ignored": "mod_map" in u, "pair_sample": "mod" in u and c["expect"] == "ln16x2" and c["rows_per_sample"] % 2 == 1 and c["rows"] > c["rows_per_sample"],
            "one_plus_scale": "mod" in u, "last_row_unwritten": True, "chunk_behind": True}[fault]


def emulate(c, o, fault=None):
    """A correct kernel, plainly: torch fp32 normalisation of the rounded operands (statistics, then the affine the kernels form:
    x * (rstd gamma) + (beta - mean rstd gamma)), the device's SiLU formula for the dtype, the result rounded to the storage type into
    sentinel-filled buffers.  fault: one of GN_FAULTS / LN_FAULTS planted into it."""
    dt = c["dtype"]
    e = N.EPC[dt]
    bufs = N.new_outputs(c)
    eps = c["eps"] if fault != "eps" else (1e-6 if c["eps"] > 5e-6 else 1e-5)
    if c["kind"] == "gn":
        x = N.gn_input(c, o, torch.float32, ignore={"map0_ignored": ("map0",), "map1_ignored": ("map1",)}.get(fault, ()))
        n, HW, Cc = x.shape
        groups, cpg = c["groups"], _cpg(c)
        xs = N.gn_input(c, o, torch.float32, ignore=("map0",)) if fault == "records_map_ignored" else x      # what the statistics are formed on
        if fault == "last_pixel":
            xs = xs[:, :-1]
        if fault == "split_dropped":      # the last split's partial / the last part's records
            k = c["qparts"] if "qstats" in c["use"] else c["splits"]
            xs = xs[:, : HW * (k - 1) // k]
        var, mean = torch.var_mean(xs.reshape(n, -1, groups, cpg), dim=(1, 3), unbiased=fault == "n_minus_1")
        rstd = (var + eps).rsqrt()
        ch = torch.arange(Cc)
        g = ch // cpg
        if fault == "group_index":        # ch / (cpg + 1) in the chunks that straddle two groups
            first, last = (ch // e * e) // cpg, (ch // e * e + e - 1) // cpg
            g = torch.where(first != last, (ch // (cpg + 1)).clamp_max(groups - 1), g)
        gamma, beta = (o["gamma"].roll(1), o["beta"].roll(1)) if fault == "affine_shifted" else (o["gamma"], o["beta"])
        sc = rstd[:, g] * gamma
        sh = beta - mean[:, g] * sc
        if "stats_only" in c["use"]:
            outs = [sc, sh]
        else:
            y = x * sc[:, None] + sh[:, None]
            if c["silu"] and fault != "silu_skipped":
                y = N.G.silu_device(y, dt != F32)
            outs = [y]
        for buf, t in zip(bufs, outs):
            t = t.to(buf.dtype)
            if fault == "last_sample_unwritten":
                t = t[:-1]
            buf[: t.numel()] = t.reshape(-1)
    else:
        x = o["x"]
        rows, C = x.shape
        xs = x[:, :-e] if fault == "last_chunk" else x
        var, mean = torch.var_mean(xs, dim=1, unbiased=fault == "n_minus_1", keepdim=True)
        y = (x - mean) * (var + eps).rsqrt()
        if "gamma" in o:
            gamma, beta = (o["gamma"].roll(1), o["beta"].roll(1)) if fault == "affine_shifted" else (o["gamma"], o["beta"])
            y = y * gamma + beta
        if "scale" in o:
            sc, sh = N.ln_mod_rows(c, o, torch.float32, ignore_map=fault == "mod_map_ignored", pair_fault=fault == "pair_sample")
            y = y * (sc if fault == "one_plus_scale" else 1.0 + sc) + sh
        t = y.to(bufs[0].dtype)
        if fault == "last_row_unwritten":
            t = t[:-1]
        bufs[0][: t.numel()] = t.reshape(-1)
    if fault == "chunk_behind":
        for buf in bufs:
            used = buf.numel() - N.GUARD
            buf[used: used + 16 // buf.element_size()] = 0.0
    return bufs


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c["name"])
def test_the_checker_passes_the_emulated_kernel(c):
    o = N.make_operands(c)
    refs = N.reference(c, o)
    assert all(ref.shape == shape and bool((bound > 0).all()) for (_, ref, bound, _), (_, shape, _) in zip(refs, N.out_shapes(c)))
    problems, worst = N.check_outputs(c, emulate(c, o), refs)
    print(f"{c['name']}: emulation err / bound {worst:.3f}")
    assert not problems, problems


# (fault, route family, dtype) combinations in which no problem of the route can hold the fault, each with the reason
INVISIBLE = {
    # producer statistics need (C / groups) % 4 == 0 (gn_validate): an fp32 chunk of 4 channels never straddles two groups
    **{("group_index", fam, F32): "cpg % 4 == 0: no fp32 chunk straddles groups" for fam in N.GN_QUAD_ROUTES},
}


def _catchers(kind, faults):
    cases = [c for c in SMALL if c["kind"] == kind]
    prepared = {}
    caught = collections.defaultdict(list)
    planted = set()
    for c in cases:
        for fault in faults:
            if not applicable(c, fault):
                continue
            key = (fault, N.family(c), c["dtype"])
            planted.add(key)
            if len(caught[key]) >= 1 and fault not in ("eps", "n_minus_1"):      # one catching case is what is asked for
                continue
            if c["name"] not in prepared:
                o = N.make_operands(c)
                prepared = {c["name"]: (o, N.reference(c, o))}
            o, refs = prepared[c["name"]]
            problems, _ = N.check_outputs(c, emulate(c, o, fault), refs)
            if problems:
                caught[key].append(c["name"])
    return planted, caught


@pytest.mark.parametrize("kind", ["gn", "ln"])
def test_every_planted_fault_fails_in_every_route_family_and_dtype(kind):
    faults = GN_FAULTS if kind == "gn" else LN_FAULTS
    planted, caught = _catchers(kind, faults)
    fams = N.GN_FAMILIES if kind == "gn" else tuple(N.LN_ROUTES)
    missing = []
    for fault in faults:
        for fam in fams:
            for dt in (N.LN_ROUTES[fam] if kind == "ln" else N.DTS):
                key = (fault, fam, dt)
                if kind == "gn":
                    exists = {"split_dropped": fam not in ("wave", "image"), "map0_ignored": fam != "qaffine",      # (qaffine reads map0 for the records only)
                              "map1_ignored": fam in N.GN_PLAIN_ROUTES, "records_map_ignored": fam in N.GN_QUAD_ROUTES,
                              "silu_skipped": fam not in N.STATS_ONLY}.get(fault, True)
                else:
                    exists = fault != "pair_sample" or fam == "ln16x2"
                if not exists:
                    assert key not in planted, key
                    continue
                if key in INVISIBLE:
                    assert not caught.get(key), (key, caught[key])      # the list holds nothing the table does catch
                    print(f"{fault:22s} {fam:12s} {N.DTN[dt]:5s} cannot show: {INVISIBLE[key]}")
                    continue
                if caught.get(key):
                    print(f"{fault:22s} {fam:12s} {N.DTN[dt]:5s} caught by {caught[key][0]}" + (f" (+{len(caught[key]) - 1})" if len(caught[key]) > 1 else ""))
                else:
                    missing.append(key + (("planted, never caught") if key in planted else "never planted",))
    assert not missing, missing


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        env = {k: os.environ[k] for k in N.SWITCHES if k in os.environ}
        with open(sys.argv[2], "w") as f:
            json.dump(_variants([c for c in N.CASES if c["env"] == env]), f)
