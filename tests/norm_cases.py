"""The cases of the GroupNorm / LayerNorm parity tests (every kernel and launch sequence of csrc/norms.hip), their operands, their fp64
reference, the per-element error bound and the checker — one table, two consumers: tests/test_norm_cases.py (host only: routing, coverage,
the checker held against an emulated kernel and planted faults) and tests/test_gpu_norms.py (the kernels themselves).

A case is a dict of the plain fields of dc_groupnorm_params (kind "gn") or dc_layernorm_params (kind "ln") plus
    name    its id
    use     the optional pointers it sets.  gn: "x1", "map0", "map1", "qstats", "stats_only" (y = NULL, out_scale / out_shift set);
            ln: "affine" (gamma / beta), "mod" (scale / shift), "mod_map"
    n_src   gn: samples ALLOCATED per source; a map only ever names the first n_src - 1 of them
    n_vec   ln: rows allocated in the modulation table (one more than mod_map names)
    expect  the exact dc_groupnorm_variant / dc_layernorm_variant string
    env     {}, {"DCAMD_GN_SPAN": "1"} or {"DCAMD_GN_NO_WAVE": "1"} (both are read once per process)
    tag     what it is for: "cell" (one of the route x dtype x ... grid) or the name of the edge
    data    "normal", "offset" (|mean| ~ 1e3 std), "tiny" (variance ~ eps), "probe" (pixel 0 all 0, pixel 1 all 1)
    big     samples of 4 MiB and more (the host test skips its emulation for time)
Plain Python and CPU torch only: nothing here opens a device."""
import math

import torch
import torch.nn.functional as F

import gemm_tile_cases as G
from gemm_tile_cases import BF16, DTN, EPS32, F16, F32, FLOOR, GUARD, LIP, SENTINEL, TD, U_OUT, _bits  # noqa: F401

EPC = {F32: 4, BF16: 8, F16: 8}               # elements of a 16-byte chunk
DTS = (F32, BF16, F16)
SPAN, NO_WAVE = {"DCAMD_GN_SPAN": "1"}, {"DCAMD_GN_NO_WAVE": "1"}
SWITCHES = ("DCAMD_GN_SPAN", "DCAMD_GN_NO_WAVE")

# The constant of the fp32-arithmetic part of the bound, K * 2^-24 * M_e (see `reference`).  Measured against torch's own fp32 CPU
# F.group_norm / F.layer_norm (+ F.silu, + the modulation in fp32) on every case of this table, never against a kernel: the smallest
# power of two for which torch's result lies inside the bound everywhere is
#     K0 = 4: largest err / (2^-24 M_e) 2.02 for GroupNorm (case "gn_stats_tiny_f16", the out_scale / out_shift of a variance ~ eps) and
#             2.64 for LayerNorm (case "ln_ln_bf16_rps64": seven roundings between x - mean and the modulated value)
# and K = 4 * K0 = 16, the margin test_groupnorm_with_large_offsets_f32 gives torch's fp32 error (the kernels sum in another order than
# torch, with the same shifted / centred forms).  tests/test_norm_cases.py recomputes K0 and fails when 4 * K0 != K, and shows that every
# planted fault still fails with this K.
# Largest err / bound on an MI355X per route and dtype (tests/test_gpu_norms.py prints it per case): the table at the end of this file.
K = 16.0


# ---- the tables -----------------------------------------------------------------------------------------------------------------
def _gn(name, dt, route, *, n, HW, C, groups, C1=0, silu=0, splits=1, use=(), qparts=0, env=None, tag="cell", data="normal", big=False,
        n_src=None, eps=1e-5):
    use = set(use) | ({"x1"} if C1 else set())
    assert ("qstats" in use) == (qparts > 0) and ("map1" not in use or C1)
    mapped = bool(use & {"map0", "map1"})
    return dict(kind="gn", name=name, dtype=dt, out_dtype=dt, n=n, HW=HW, C=C, C1=C1, groups=groups, silu=silu, splits=splits, eps=eps,
                qparts=qparts, use=frozenset(use), n_src=(max(3, n - 1) if mapped else n) if n_src is None else n_src, expect=route,
                env=dict(env or {}), tag=tag, data=data, big=big)


GN_FORMS = {"one": (), "one_map": ("map0",), "two": ("x1",), "two_maps": ("x1", "map0", "map1")}
GN_PLAIN_ROUTES = ("wave", "image", "stats+apply", "stats")            # take either source form
GN_QUAD_ROUTES = ("image-q", "span", "qfold+span", "qfold+apply", "qaffine")      # producer statistics: one source (gn_validate)
GN_FAMILIES = GN_PLAIN_ROUTES + GN_QUAD_ROUTES
STATS_ONLY = ("stats", "qaffine")


def _gn_cell(fam, dt, silu, form):
    """The smallest problem of (route family, dtype, SiLU, source form) with channels per group that no 16-byte chunk lines up with
    where the route allows it."""
    e = EPC[dt]
    use = set(GN_FORMS[form])
    two = "x1" in use
    name = f"gn_{fam}_{DTN[dt]}_{'silu' if silu else 'lin'}_{form}"
    kw = dict(silu=silu, use=use)
    if fam in ("wave", "image", "stats"):      # 12 chunks per pixel, cpg = 1.5 chunks; 12 pixels: 3 chunks per lane; 300: 75, more than a wave holds
        c0, c1 = (9 * e, 3 * e) if two else (12 * e, 0)
        if fam == "stats":
            return _gn(name, dt, fam, n=3, HW=20, C=c0, C1=c1, groups=8, splits=3, use=use | {"stats_only"})
        return _gn(name, dt, fam, n=5 if fam == "wave" else 3, HW=12 if fam == "wave" else 300, C=c0, C1=c1, groups=8, **kw)
    if fam == "stats+apply":              # 520 chunks per pixel: more than one workgroup per sample holds; three column passes; cpg = 32.5 chunks
        c0, c1 = (261 * e, 259 * e) if two else (520 * e, 0)
        return _gn(name, dt, fam, n=3, HW=9, C=c0, C1=c1, groups=16, splits=2, **kw)
    q = use | {"qstats"}                  # producer statistics: cpg = 4, half a 16-bit chunk (in fp32 a group is whole chunks by gn_validate)
    if fam == "qaffine":
        return _gn(name, dt, fam, n=4, HW=24, C=8 * e, groups=2 * e, qparts=4, use=q | {"stats_only"})
    if fam == "image-q":
        return _gn(name, dt, "image", n=4, HW=48, C=8 * e, groups=2 * e, qparts=4, silu=silu, use=q)
    if fam == "span":                     # one 16 KiB span per sample
        return _gn(name, dt, fam, n=4, HW=128, C=8 * e, groups=2 * e, qparts=4, silu=silu, use=q, env=SPAN)
    if fam == "qfold+span":               # 4096 quad records per sample: more than gn_span_kernel holds
        qp = 4096 // (4 * e)
        return _gn(name, dt, fam, n=4, HW=qp, C=16 * e, groups=4 * e, qparts=qp, silu=silu, use=q, env=SPAN)
    if fam == "qfold+apply":              # 1 MiB per sample and 48 chunks per pixel (not a power of two: no spans); C/4 does not divide 256
        return _gn(name, dt, fam, n=3, HW=1376, C=48 * e, groups=12 * e, qparts=8, splits=5, silu=silu, use=q, n_src=3)
    raise ValueError(fam)


def gn_cells():
    out = []
    for dt in DTS:
        for fam in GN_FAMILIES:
            for silu in ((0,) if fam in STATS_ONLY else (0, 1)):
                for form in (GN_FORMS if fam in GN_PLAIN_ROUTES else ("one", "one_map")):
                    out.append(_gn_cell(fam, dt, silu, form))
    return out


def gn_edges():
    out = []
    for dt in DTS:
        e, d = EPC[dt], DTN[dt]
        g = lambda name, route, **kw: out.append(_gn(f"gn_{name}_{d}", dt, route, **kw))
        # -- wave: the four NCH instances (8 chunks per pixel: 8 pixel lanes, chunks per lane = ceil(HW / 8)); n % 4 = 1, 2, 3
        for nch, hw, n in ((4, 30, 5), (8, 60, 6), (16, 100, 7), (32, 250, 9)):
            g(f"wave_nch{nch}", "wave", n=n, HW=hw, C=8 * e, groups=4, silu=1, tag=f"nch{nch}")
        for hw in (1, 2, 4):              # fewer pixels than pixel lanes: a 1x1 / 2x2 level
            g(f"wave_hw{hw}", "wave", n=6, HW=hw, C=8 * e, groups=2, silu=1, tag="hw_below_lanes")
        g("wave_cp64", "wave", n=3, HW=7, C=64 * e, groups=32, silu=1, tag="cp_limit")
        g("wave_two_maps_seam_cp0_3", "wave", n=7, HW=10, C=3 * e, C1=5 * e, groups=2, silu=1, use={"map0", "map1"}, tag="seam")
        # -- image
        g("image_hw_below_pl", "image", n=3, HW=3, C=128 * e, groups=32, silu=1, tag="hw_below_pl")              # PL = 4
        g("image_no_unrolled_pass", "image", n=2, HW=11, C=128 * e, groups=8, tag="unroll0")                     # 11 <= 3 PL + 1
        g("image_unroll_remainder", "image", n=2, HW=4 * 64 * 2 + 77, C=8 * e, groups=2, silu=1, tag="unroll_rem")      # PL = 64
        g("image_cp1", "image", n=2, HW=2100, C=e, groups=1, silu=1, tag="cp1")                                  # 33 chunks per lane of a wave
        g("image_cp48", "image", n=3, HW=40, C=48 * e, groups=32, silu=1, use={"map0"}, tag="cp48")              # cpg = 12 / 6: chunks straddle groups
        g("image_cp512", "image", n=2, HW=5, C=512 * e, groups=8, tag="cp512")
        g("image_cpg1", "image", n=2, HW=6, C=512, groups=512, silu=1, env={} if dt == F32 else NO_WAVE, tag="cpg1")      # groups = C
        g("image_groups512", "image", n=2, HW=5, C=2048, groups=512, tag="groups512")
        g("image_no_wave", "image", n=5, HW=12, C=8 * e, groups=4, silu=1, env=NO_WAVE, tag="no_wave")           # the wave cell's problem
        g("image_two_maps_seam", "image", n=4, HW=70, C=5 * e, C1=3 * e, groups=2, silu=1, use={"map0", "map1"}, env=NO_WAVE, tag="seam")
        g("imageq_cp1", "image", n=3, HW=64, C=e, groups=1, qparts=2, silu=1, use={"qstats", "map0"}, tag="cp1")
        g("imageq_qparts1", "image", n=3, HW=20, C=48 * e, groups=6 * e // 4, qparts=1, use={"qstats", "map0"}, tag="qparts1")
        # -- stats+apply: splits that do not divide HW, 1 and HW; a sample above 4 MiB with the engine's own split count
        g("sa_splits7", "stats+apply", n=2, HW=300, C=520 * e, groups=32, splits=7, silu=1, tag="splits7")       # cpg = 65 (f32) / 130
        g("sa_splits1", "stats+apply", n=2, HW=5, C=520 * e, groups=8, splits=1, tag="splits1")
        g("sa_splits_hw", "stats+apply", n=2, HW=5, C=520 * e, groups=8, splits=5, silu=1, tag="splits_hw")
        g("sa_above_4mib", "stats+apply", n=3, HW=16640, C=16 * e, groups=4, splits=64, silu=1, use={"map0"}, tag="above_4mib", big=True)
        # -- statistics only
        g("stats_groups64", "stats", n=3, HW=33, C=64 * e, groups=64, splits=4, use={"stats_only", "x1", "map0", "map1"}, C1=64 * e, tag="groups64")
        g("qaffine_groups128", "qaffine", n=5, HW=6, C=512, groups=128, qparts=3, use={"stats_only", "qstats", "map0"}, tag="groups_above_64")
        # -- span / qfold: CP 1 and 256, records per sample around the 2048 gn_span_kernel holds, one part
        g("span_cp1", "span", n=3, HW=1024, C=e, groups=1, qparts=4, silu=1, use={"qstats", "map0"}, env=SPAN, tag="cp1")
        g("span_cp256_r1536", "span", n=3, HW=12, C=256 * e, groups=32, qparts=(3 if dt != F32 else 6), silu=1, use={"qstats", "map0"}, env=SPAN,
          tag="records_below_2048")
        g("span_cp256_r2048", "span", n=3, HW=(4 if dt != F32 else 8), C=256 * e, groups=32, qparts=(4 if dt != F32 else 8), use={"qstats", "map0"},
          env=SPAN, tag="records_at_2048")
        g("qfspan_cp256_r2560", "qfold+span", n=3, HW=20, C=256 * e, groups=32, qparts=(5 if dt != F32 else 10), silu=1, use={"qstats", "map0"}, env=SPAN,
          tag="records_above_2048")
        g("span_qparts1", "span", n=3, HW=128, C=8 * e, groups=2, qparts=1, use={"qstats", "map0"}, env=SPAN, tag="qparts1")
        g("qfspan_1mib", "qfold+span", n=3, HW=4096, C=32 * e, groups=8, qparts=32, silu=1, use={"qstats", "map0"}, tag="default_route_1mib")
        g("qfapply_qparts1", "qfold+apply", n=3, HW=1376, C=48 * e, groups=4, qparts=1, splits=7, use={"qstats", "map0"}, n_src=3, tag="qparts1")
        # -- across routes: large offset, tiny spread, few values per group (cpg * HW <= 8)
        for data in ("offset", "tiny"):
            g(f"wave_{data}", "wave", n=3, HW=16, C=8 * e, groups=4, silu=1, data=data, tag=data)
            g(f"image_{data}", "image", n=2, HW=300, C=8 * e, groups=4, silu=1, data=data, tag=data)
            g(f"sa_{data}", "stats+apply", n=2, HW=12, C=520 * e, groups=8, splits=3, silu=1, data=data, tag=data)
            g(f"imageq_{data}", "image", n=3, HW=48, C=8 * e, groups=4, qparts=4, silu=1, use={"qstats", "map0"}, data=data, tag=data)
        g("wave_few", "wave", n=5, HW=2, C=8 * e, groups=2 * e, silu=1, tag="few")                              # cpg 4 x 2 pixels
        g("image_few", "image", n=3, HW=4, C=128 * e, groups=64 * e, tag="few")                                 # cpg 2 x 4 pixels
        g("sa_few", "stats+apply", n=3, HW=4, C=1024, groups=1024, splits=2, silu=1, tag="few")                 # more groups than gn_image_kernel takes
        g("imageq_few", "image", n=3, HW=2, C=8 * e, groups=2 * e, qparts=2, use={"qstats", "map0"}, tag="few")
        g("qaffine_few", "qaffine", n=3, HW=2, C=8 * e, groups=2 * e, qparts=1, use={"qstats", "stats_only"}, tag="few")
        g("stats_few", "stats", n=3, HW=2, C=8 * e, groups=2 * e, splits=2, use={"stats_only"}, tag="few")
        # the span routes need whole 16 KiB spans: 16 and 80 values per group are the fewest they admit; qfold+apply starts at 1 MiB
        g("span_few16", "span", n=3, HW=4, C=256 * e, groups=64 * e, qparts=4, silu=1, use={"qstats", "map0"}, env=SPAN, tag="few16")
        g("qfspan_few80", "qfold+span", n=3, HW=20, C=256 * e, groups=64 * e, qparts=(5 if dt != F32 else 10), use={"qstats", "map0"}, env=SPAN, tag="few80")
        for fam in ("stats", "qaffine", "span", "qfold+span", "qfold+apply"):      # variance ~ eps on the routes the list above leaves out
            out.append(dict(_gn_cell(fam, dt, 0 if fam in STATS_ONLY else 1, "one_map"), name=f"gn_{fam}_tiny_{d}", data="tiny", tag="tiny"))
    # the lanes-off cases the issue names, and the group that straddles the two-source seam
    out.append(_gn("gn_wave_bf16_cp48_c384", BF16, "wave", n=6, HW=16, C=384, groups=32, silu=1, tag="cp_not_pow2"))
    out.append(_gn("gn_wave_f32_cp24_c96", F32, "wave", n=6, HW=17, C=96, groups=8, silu=1, tag="cp_not_pow2"))
    out.append(_gn("gn_wave_f32_group_straddles_seam", F32, "wave", n=5, HW=9, C=96, C1=32, groups=2, silu=1, use={"map0", "map1"}, tag="seam_in_group"))
    out.append(_gn("gn_image_bf16_group_straddles_seam", BF16, "image", n=3, HW=40, C=96, C1=32, groups=2, silu=1, use={"map0", "map1"}, env=NO_WAVE,
                   tag="seam_in_group"))
    out.append(_gn("gn_sa_f16_group_straddles_seam", F16, "stats+apply", n=3, HW=6, C=2088, C1=2072, groups=2, splits=3, use={"map0", "map1"},
                   tag="seam_in_group"))
    # gn_image_kernel's affine against gn_qaffine_kernel's from the same records, bit for bit (tests/test_gpu_norms.py): y at a pixel
    # that holds 0 is the shift, at one that holds 1 fl(scale + shift), contracted or not
    out.append(_gn("gn_imageq_f32_affine_probe", F32, "image", n=4, HW=48, C=48, groups=4, qparts=4, use={"qstats", "map0"}, data="probe", tag="probe"))
    out.append(_gn("gn_span_f32_affine_probe", F32, "span", n=4, HW=128, C=32, groups=4, qparts=4, use={"qstats", "map0"}, env=SPAN, data="probe", tag="probe"))
    return out


def _ln(name, dt, route, *, rows, C, form, rps=None, mod_ld=None, table6=False, data="normal", gamma_off=0, mod_off=0, tag="cell", eps=1e-6):
    use = {"none": set(), "affine": {"affine"}, "mod": {"mod"}, "mod_map": {"mod", "mod_map"}, "all": {"affine", "mod", "mod_map"}}[form]
    rps = rows if rps is None else rps
    mod = "mod" in use
    ld = (6 * C if table6 else (C if mod_ld is None else mod_ld)) if mod else 0
    ns = (rows + rps - 1) // rps
    return dict(kind="ln", name=name, dtype=dt, out_dtype=dt, rows=rows, C=C, rows_per_sample=rps, mod_ld=ld, eps=eps, use=frozenset(use), form=form,
                table6=table6 and mod, gamma_off=gamma_off, mod_off=mod_off, n_samples=ns, n_vec=ns + 1, expect=route, env={}, tag=tag, data=data, big=False)


LN_FORMS = ("none", "affine", "mod", "mod_map", "all")
LN_ROUTES = {"ln16x2": (BF16, F16), "ln16": DTS, "ln": DTS}
LN_WG_ROWS = {"ln16x2": 32, "ln16": 16, "ln": 4}


def ln_width(route, dt):
    """A row width of the route: 16-bit ln16 sits between 97 and 128 chunks, ln above 128."""
    e = EPC[dt]
    return {"ln16x2": 9 * e, "ln16": (18 * e if dt == F32 else 100 * e), "ln": 130 * e}[route]


def ln_geometries(route):
    w = LN_WG_ROWS[route]
    return {"rows1": 1, "rows2": 2, "odd": 7, "wg-1": w - 1, "wg": w, "wg+1": w + 1}


def ln_cells():
    out = []
    for route, dts in LN_ROUTES.items():
        for dt in dts:
            for form in LN_FORMS:
                for gname, rows in ln_geometries(route).items():      # 3 rows per sample: pairs of ln16x2 straddle samples
                    out.append(_ln(f"ln_{route}_{DTN[dt]}_{form}_{gname}", dt, route, rows=rows, C=ln_width(route, dt), form=form, rps=3))
    return out


def ln_edges():
    out = []
    route_of = lambda dt, cp: ("ln16x2" if dt != F32 and cp <= 96 else ("ln16" if cp <= 128 else "ln"))
    for route, dts in LN_ROUTES.items():
        for dt in dts:
            d, C = DTN[dt], ln_width(route, dt)
            ln = lambda name, **kw: out.append(_ln(f"ln_{route}_{d}_{name}", dt, route, **kw))
            # samples: one row each; odd; % 16 but not % 32; 32; 48; 64 — two and a half samples, so the last one is partial
            for rps in (1, 5, 16, 32, 48, 64):
                ln(f"rps{rps}", rows=2 * rps + max(1, rps // 2), C=C, form="mod_map" if rps % 2 else "all", rps=rps, table6=rps in (5, 32, 64), tag=f"rps{rps}")
            ln("rps32_mod", rows=96, C=C, form="mod", rps=32, tag="rps32")
            ln("mod_ld_wide", rows=40, C=C, form="mod", rps=16, mod_ld=C + 8, tag="mod_ld_above_c")
            ln("offset", rows=9, C=C, form="all", rps=4, data="offset", tag="offset")
            ln("tiny", rows=9, C=C, form="all", rps=4, data="tiny", tag="tiny")
    for dt in DTS:
        d, e = DTN[dt], EPC[dt]
        for cp in (1, 9, 96, 97, 128, 129, 144, 1280 // e):      # 1280: the widest transformer block the engine builds (UNet), 144 x 8: DiT-XL
            out.append(_ln(f"ln_width_{d}_cp{cp}", dt, route_of(dt, cp), rows=5, C=cp * e, form="all", rps=2, tag=f"cp{cp}"))
        # what forces the one-wave-per-row kernel at a width the register kernels take
        out.append(_ln(f"ln_forced_{d}_mod_ld_odd", dt, "ln", rows=9, C=16 * e, form="all", rps=4, mod_ld=16 * e + 2, tag="mod_ld_not_4"))
        out.append(_ln(f"ln_forced_{d}_gamma_off4", dt, "ln", rows=9, C=16 * e, form="all", rps=4, gamma_off=1, tag="gamma_misaligned"))
        out.append(_ln(f"ln_forced_{d}_mod_off4", dt, "ln", rows=9, C=16 * e, form="mod", rps=4, mod_off=1, tag="mod_misaligned"))
        out.append(_ln(f"ln_forced_{d}_cp1", dt, "ln", rows=6, C=e, form="all", rps=4, gamma_off=1, tag="one_chunk_rows"))
    return out


CASES = gn_cells() + gn_edges() + ln_cells() + ln_edges()
GN_CASES = [c for c in CASES if c["kind"] == "gn"]
LN_CASES = [c for c in CASES if c["kind"] == "ln"]
# the value of a sample must not depend on how many samples share the launch: two cases per route family (one through the sample maps,
# one through plain pointers) and two per LayerNorm route (five rows per sample: the row pairs of ln16x2 shift; sixteen: LDS-staged), per dtype
INDEPENDENT = [f"gn_{fam}_{d}_{'lin' if fam in STATS_ONLY else 'silu'}_{form}" for fam in GN_FAMILIES for d in ("f32", "bf16", "f16")
               for form in (("two", "two_maps") if fam in GN_PLAIN_ROUTES else ("one", "one_map"))] + \
              [f"ln_{r}_{DTN[dt]}_rps{k}" for r, dts in LN_ROUTES.items() for dt in dts for k in (5, 16)]
# launch-to-launch identity at size
REPEAT_CASES = [f"gn_sa_above_4mib_{d}" for d in ("f32", "bf16", "f16")] + ["gn_qfspan_1mib_bf16", "gn_qfold+apply_bf16_silu_one_map"]
# (route family, dtype / form) cells that cannot exist: tests/test_norm_cases.py shows each refused or routed elsewhere
UNREACHABLE = {
    ("ln16x2", F32): "ln_route: two rows per lane group is a 16-bit kernel",
    **{(fam, "two"): "gn_validate: producer statistics need one source" for fam in GN_QUAD_ROUTES},
    ("wave", "qstats"): "gn_route: gn_wave_kernel forms its own statistics",
    ("stats+apply", "qstats"): "gn_route: with records the split route is qfold+apply",
}


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def family(c):
    if c["kind"] == "ln":
        return c["expect"]
    return "image-q" if c["expect"] == "image" and "qstats" in c["use"] else c["expect"]


def gn_form(c):
    u = c["use"]
    return ("two_maps" if "map0" in u else "two") if "x1" in u else ("one_map" if "map0" in u else "one")


def wave_nch(c):
    """The gn_wave_kernel instance (chunks per lane, rounded up to 4 / 8 / 16 / 32) a wave case runs."""
    cp = (c["C"] + c["C1"]) // EPC[c["dtype"]]
    tpr = 1
    while tpr < cp:
        tpr <<= 1
    nch = -(-c["HW"] // (64 // tpr))
    return next(i for i in (4, 8, 16, 32) if nch <= i)


def ws_floats(c):
    return c["n"] * c["groups"] * c["splits"] * 2      # dc_groupnorm_ws_floats


GN_PTRS = ("x", "map0", "x1", "map1", "y", "gamma", "beta", "ws", "out_scale", "out_shift", "qstats")
LN_PTRS = ("x", "y", "gamma", "beta", "scale", "shift", "mod_map")


def gn_fields(c, ptrs, n=None):
    """dc_groupnorm_params fields; ptrs: {pointer field: address} (only those the case uses are taken)."""
    u = c["use"]
    kw = {k: c[k] for k in ("dtype", "out_dtype", "n", "HW", "C", "C1", "groups", "silu", "splits", "eps", "qparts")}
    if n is not None:
        kw["n"] = n
    want = ["x", "gamma", "beta", "ws"] + [f for f in ("map0", "x1", "map1", "qstats") if f in u] + (["out_scale", "out_shift"] if "stats_only" in u else ["y"])
    kw.update({f: ptrs[f] for f in want})
    return kw


def ln_fields(c, ptrs, rows=None):
    u = c["use"]
    kw = {k: c[k] for k in ("dtype", "out_dtype", "rows", "C", "rows_per_sample", "mod_ld", "eps")}
    if rows is not None:
        kw["rows"] = rows
    want = ["x", "y"] + (["gamma", "beta"] if "affine" in u else []) + (["scale", "shift"] if "mod" in u else []) + (["mod_map"] if "mod_map" in u else [])
    kw.update({f: ptrs[f] for f in want})
    return kw


def fake_ptrs(c, base=1 << 20):
    """Addresses with the alignment the real operands have (pointer alignment is part of the LayerNorm route); never dereferenced."""
    if c["kind"] == "gn":
        return {f: base for f in GN_PTRS}
    p = {f: base for f in LN_PTRS}
    p["gamma"] = base + 4 * c["gamma_off"]
    p["shift"] = base + 4 * c["mod_off"]
    p["scale"] = base + 4 * c["mod_off"] + (4 * c["C"] if c["table6"] else 0)
    return p


# ---- operands -------------------------------------------------------------------------------------------------------------------
def gn_map(which, n, n_src):
    """Sample maps over the first n_src - 1 source samples: out of order, with repeats as soon as n > n_src - 1, never the identity."""
    used = n_src - 1
    return torch.tensor([(used - 1 - i) % used if which == "map0" else (i // 2 + 1) % used for i in range(n)], dtype=torch.int32)


def quad_records(x0, qparts):
    """The producer's records as include/dcamd.h documents them, formed in fp64 and rounded to fp32:
    [sample, part, C/4, (mean, M2)] over the 4 * HW / qparts values of a quad of channels in a run of pixels."""
    ns, HW, C = x0.shape
    v = x0.double().view(ns, qparts, HW // qparts, C // 4, 4)
    mean = v.mean(dim=(2, 4))
    m2 = ((v - mean[:, :, None, :, None]) ** 2).sum(dim=(2, 4))
    return torch.stack([mean, m2], -1).float()


def make_operands(c, seed=0):
    """CPU fp32 tensors, x already rounded to the compute type (the kernels' operands are exactly these)."""
    gen = torch.Generator().manual_seed(2000 + seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    q = lambda t: t.to(TD[c["dtype"]]).float()
    if c["kind"] == "gn":
        C0, C1, HW, ns, groups = c["C"], c["C1"], c["HW"], c["n_src"], c["groups"]
        Cc = C0 + C1
        if c["data"] == "offset":         # one offset of ~1e3 standard deviations per group
            off = (rn(groups, 1) * 300 + 1000).expand(groups, Cc // groups).reshape(Cc)
            x = rn(ns, HW, Cc) + off
        elif c["data"] == "tiny":
            x = rn(ns, HW, Cc) * c["eps"] ** 0.5
        else:
            x = rn(ns, HW, Cc) * 2 + 0.5 + 0.5 * rn(Cc)
        if c["data"] == "probe":
            x[:, 0], x[:, 1] = 0.0, 1.0
        o = dict(x0=q(x[..., :C0].contiguous()), gamma=rn(Cc), beta=rn(Cc))
        if C1:
            o["x1"] = q(x[..., C0:].contiguous())
        for m in ("map0", "map1"):
            if m in c["use"]:
                o[m] = gn_map(m, c["n"], ns)
        if "qstats" in c["use"]:
            o["qstats"] = quad_records(o["x0"], c["qparts"])
        return o
    rows, C = c["rows"], c["C"]
    if c["data"] == "offset":
        x = rn(rows, C) + (rn(rows, 1) * 300 + 1000)
    elif c["data"] == "tiny":
        x = rn(rows, C) * c["eps"] ** 0.5
    else:
        x = rn(rows, C) * 3 + 1
    o = dict(x=q(x))
    if "affine" in c["use"]:
        o["gamma"], o["beta"] = rn(C), rn(C)
    if "mod" in c["use"]:
        nv = c["n_vec"] if "mod_map" in c["use"] else c["n_samples"]
        if c["table6"]:                   # adaLN-Zero: shift | scale | gate | ... in one [*, 6 C] table
            o["table"] = rn(nv, 6 * C)
            o["shift"], o["scale"] = o["table"][:, :C], o["table"][:, C:2 * C]
        else:
            o["scale"], o["shift"] = rn(nv, C), rn(nv, C)
        if "mod_map" in c["use"]:
            used = max(1, c["n_samples"] - 1)
            o["mod_map"] = torch.tensor([(used - 1 - i) % used for i in range(c["n_samples"])], dtype=torch.int32)
    return o


def gn_input(c, o, dtype=torch.float64, ignore=()):
    """[n, HW, C0 + C1]: the concatenated input as the maps select it.  ignore: maps to treat as absent (a planted fault)."""
    n = c["n"]
    pick = lambda src, m: src[o[m].long()] if (m in o and m not in ignore) else src[torch.arange(n) % src.shape[0]]
    x = pick(o["x0"], "map0")
    if c["C1"]:
        x = torch.cat([x, pick(o["x1"], "map1")], -1)
    return x.to(dtype)


def ln_mod_rows(c, o, dtype=torch.float64, ignore_map=False, pair_fault=False):
    """(scale, shift) per row [rows, C]."""
    r = torch.arange(c["rows"])
    if pair_fault:                        # the second row of a pair takes the first row's sample
        r = r - r % 2
    s = r // c["rows_per_sample"]
    idx = o["mod_map"].long()[s] if ("mod_map" in o and not ignore_map) else s % o["scale"].shape[0]
    return o["scale"][idx].to(dtype), o["shift"][idx].to(dtype)


# ---- reference and bound --------------------------------------------------------------------------------------------------------
def _stat_units(mean, var, eps):
    """How far fp32 statistics may sit from the exact ones, in units of 2^-24 (before K): the mean by |mean| + std (shifted or plain sums
    round at the magnitude of the values), the variance by var + 2 |mean| std (the fold of per-lane / per-record means squares differences
    of numbers that carry an error of |mean| 2^-24 each), hence rstd relatively by half of that over var + eps."""
    sd = var.sqrt()
    return mean.abs() + sd, 0.5 * (var + 2.0 * mean.abs() * sd) / (var + eps)


def reference(c, o, K_=None):
    """[(label, ref, bound, M_e)] over every output element, ref in fp64 from the rounded operands (F.group_norm / F.layer_norm in double,
    then SiLU, then the modulation).  bound = u_out |ref| + floor + (1 + u_out) (K 2^-24 M_e + e_silu):

        GroupNorm  M_e = L (|x| A + |mean| A + |beta| + dmean A + |x - mean| A drstd),  A = rstd |gamma|, L = SiLU's slope bound or 1
        LayerNorm  M_e = ((|z| |gamma| + |beta|) |1 + scale| + |shift|) + (dmean rstd |gamma| + |z| |gamma| drstd) |1 + scale|,  z = (x - mean) rstd
        out_scale  M_e = A (1 + drstd);   out_shift  M_e = |beta| + |mean| A (1 + drstd) + dmean A

    the sum of the magnitudes that meet in the fp32 affine plus the sensitivity to the fp32 statistics (dmean, drstd: _stat_units).
    e_silu: gemm_tile_cases.e_act, the error of silu_f / silu_fast_f.  Nothing here comes from what a kernel returned."""
    Kc = K if K_ is None else K_
    dt = c["dtype"]
    u, fl = U_OUT[dt], FLOOR[dt]
    if c["kind"] == "gn":
        x = gn_input(c, o)
        n, HW, Cc = x.shape
        groups, eps = c["groups"], c["eps"]
        gamma, beta = o["gamma"].double(), o["beta"].double()
        xg = x.view(n, HW, groups, Cc // groups)
        mean = xg.mean(dim=(1, 3))
        var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
        rstd = (var + eps).rsqrt()
        dm, dr = _stat_units(mean, var, eps)
        per_ch = lambda t: t.repeat_interleave(Cc // groups, 1)              # [n, groups] -> [n, C]
        mean_c, rstd_c, dm_c, dr_c = per_ch(mean), per_ch(rstd), per_ch(dm), per_ch(dr)
        A = rstd_c * gamma.abs()
        if "stats_only" in c["use"]:
            scale = rstd_c * gamma
            shift = beta - mean_c * scale
            Ms = A * (1.0 + dr_c)
            Mh = beta.abs() + mean_c.abs() * A * (1.0 + dr_c) + dm_c * A
            return [("out_scale", scale, Kc * EPS32 * Ms, Ms), ("out_shift", shift, Kc * EPS32 * Mh, Mh)]
        pre = F.group_norm(x.permute(0, 2, 1), groups, gamma, beta, eps).permute(0, 2, 1)
        M = x.abs() * A[:, None] + (mean_c.abs() * A + beta.abs() + dm_c * A)[:, None] + (x - mean_c[:, None]).abs() * (A * dr_c)[:, None]
        if c["silu"]:
            ref, M, extra = F.silu(pre), LIP * M, G.e_act("silu", pre, dt != F32)
        else:
            ref, extra = pre, 0.0
        bound = u * ref.abs() + fl + (1.0 + u) * (Kc * EPS32 * M + extra)
        return [("y", ref, bound, M)]
    x = o["x"].double()
    C, eps = c["C"], c["eps"]
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    dm, dr = _stat_units(mean, var, eps)
    z = (x - mean) * rstd
    g = o["gamma"].double().abs() if "gamma" in o else torch.ones(C, dtype=torch.float64)
    b = o["beta"].double().abs() if "beta" in o else torch.zeros(C, dtype=torch.float64)
    ref = F.layer_norm(x, (C,), o["gamma"].double() if "gamma" in o else None, o["beta"].double() if "beta" in o else None, eps)
    M = z.abs() * g + b
    sens = dm * rstd * g + z.abs() * g * dr
    if "scale" in o:
        sc, sh = ln_mod_rows(c, o)
        ref = ref * (1.0 + sc) + sh
        M, sens = M * (1.0 + sc).abs() + sh.abs(), sens * (1.0 + sc).abs()
    M = M + sens
    return [("y", ref, u * ref.abs() + fl + (1.0 + u) * Kc * EPS32 * M, M)]


def torch_fp32(c, o):
    """torch's own fp32 CPU result of the case, unrounded: what K0 is measured on."""
    if c["kind"] == "gn":
        x = gn_input(c, o, torch.float32)
        if "stats_only" in c["use"]:      # the affine of torch's fp32 statistics
            n, HW, Cc = x.shape
            xg = x.view(n, HW, c["groups"], -1)
            var, mean = torch.var_mean(xg, dim=(1, 3), unbiased=False)
            rstd = (var + c["eps"]).rsqrt().repeat_interleave(Cc // c["groups"], 1)
            scale = rstd * o["gamma"]
            return [scale, o["beta"] - mean.repeat_interleave(Cc // c["groups"], 1) * scale]
        y = F.group_norm(x.permute(0, 2, 1), c["groups"], o["gamma"], o["beta"], c["eps"]).permute(0, 2, 1)
        return [F.silu(y) if c["silu"] else y]
    y = F.layer_norm(o["x"], (c["C"],), o.get("gamma"), o.get("beta"), c["eps"])
    if "scale" in o:
        sc, sh = ln_mod_rows(c, o, torch.float32)
        y = y * (1.0 + sc) + sh
    return [y]


def k0_ratio(c, o):
    """Largest |torch fp32 - fp64| / (2^-24 M_e) over the case's elements (SiLU's own fp32 error, e_act, taken off first)."""
    worst = 0.0
    for (label, ref, _, M), t in zip(reference(c, o), torch_fp32(c, o)):
        err = (t.double() - ref).abs()
        if label == "y" and c["kind"] == "gn" and c["silu"]:
            pre = F.group_norm(gn_input(c, o).permute(0, 2, 1), c["groups"], o["gamma"].double(), o["beta"].double(), c["eps"]).permute(0, 2, 1)
            err = (err - G.e_act("silu", pre, False)).clamp_min(0.0)
        worst = max(worst, float((err / (EPS32 * M)).max()))
    return worst


# ---- the checker ----------------------------------------------------------------------------------------------------------------
def out_shapes(c):
    """[(label, shape, torch dtype)] of the outputs a launch writes."""
    if c["kind"] == "ln":
        return [("y", (c["rows"], c["C"]), TD[c["dtype"]])]
    Cc = c["C"] + c["C1"]
    if "stats_only" in c["use"]:
        return [("out_scale", (c["n"], Cc), torch.float32), ("out_shift", (c["n"], Cc), torch.float32)]
    return [("y", (c["n"], c["HW"], Cc), TD[c["dtype"]])]


def new_outputs(c, device="cpu"):
    """Flat output buffers, the sentinel everywhere: the tensor and a guard region behind it."""
    return [torch.full((math.prod(shape) + GUARD,), SENTINEL, dtype=td, device=device) for _, shape, td in out_shapes(c)]


def guard_intact(buf, used):
    sent = _bits(torch.full((1,), SENTINEL, dtype=buf.dtype))[0]
    return int((_bits(buf[used:]) != sent).sum())


def check_outputs(c, bufs, refs):
    """bufs: the flat buffers (CPU) after the launch; refs: reference(c, o).  Returns (problems, worst err / bound): every element finite
    and inside its bound, everything behind the tensor still the sentinel bit for bit."""
    problems, worst = [], 0.0
    for buf, (label, shape, _), (_, ref, bound, _) in zip(bufs, out_shapes(c), refs):
        used = math.prod(shape)
        bad = guard_intact(buf, used)
        if bad:
            problems.append(f"{label}: {bad} elements behind the tensor were written")
        got = buf[:used].view(shape).double()
        if not bool(torch.isfinite(got).all()):
            problems.append(f"{label}: {int((~torch.isfinite(got)).sum())} non-finite values")
            got = torch.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
        ratio = (got - ref).abs() / bound
        w = float(ratio.max())
        worst = max(worst, w)
        if w > 1.0:
            nbad = int((ratio > 1.0).sum())
            i = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
            problems.append(f"{label}: {nbad} of {used} elements outside the bound, worst err / bound {w:.3g} at {i} (got {float(got[i])!r}, "
                            f"ref {float(ref[i])!r}, bound {float(bound[i]):.3g}); samples / rows hit: {sorted({int(r[0]) for r in (ratio > 1.0).nonzero()[:4096]})[:16]}")
    return problems, worst


# ---- measured -------------------------------------------------------------------------------------------------------------------
# Largest err / bound per route family and dtype on an MI355X, all 666 cases (605 with no switch, 52 under DCAMD_GN_SPAN, 9 under
# DCAMD_GN_NO_WAVE); the module's wall time was 12.9 s.  A 16-bit output rounded to nearest uses its rounding term whole (0.99: the
# term is tight by nature), the fp32 arithmetic little; out_scale / out_shift ("stats", "qaffine") are fp32 whatever the tensor's type.
#     wave          f32 0.119  bf16 0.995  f16 0.991
#     image         f32 0.137  bf16 0.995  f16 0.994
#     image-q       f32 0.090  bf16 0.994  f16 0.981
#     stats+apply   f32 0.135  bf16 0.995  f16 0.993
#     stats         f32 0.083  bf16 0.090  f16 0.098
#     qaffine       f32 0.100  bf16 0.108  f16 0.101
#     span          f32 0.184  bf16 0.994  f16 0.994
#     qfold+span    f32 0.146  bf16 0.996  f16 0.993
#     qfold+apply   f32 0.124  bf16 0.996  f16 0.996
#     ln16x2                   bf16 0.995  f16 0.989
#     ln16          f32 0.118  bf16 0.995  f16 0.996
#     ln            f32 0.127  bf16 0.996  f16 0.995
# Before GnMerge (csrc/norms.hip) summed in fp64, ten 16-bit cases of gn_image_kernel and gn_stats_kernel lay outside: 2.42 on
# "gn_image_cp1_bf16", 2.37 on "gn_sa_f16_group_straddles_seam", 1.09 ... 1.42 on the image cells; the mean of 16800 bf16 values was
# off by 4e-5 where torch's fp32 kernel loses 1e-7.
