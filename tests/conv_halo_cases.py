"""The cases of the 3x3 halo-convolution parity tests (conv3_halo<T,4w|8w> in every instance dc_conv3_halo_plan picks, conv3_ws<T,gn>, conv3_thin<T>,
conv3_up4<T,4w|8w>, igemm_pipe_up4<T,256x128,3st>), their operands, their fp64 reference, the per-element error bound and the checker —
one table, two consumers: tests/test_conv_halo_cases.py (host only: routing, coverage, geometry, the checker held against planted faults)
and tests/test_gpu_conv_halo.py (the kernels themselves).

A case is a dict of dc_igemm's plain fields (the dc_igemm_params names) plus
    name      its id
    family    "halo4", "halo8", "halo8_lockstep", "ws_gn", "thin" or "up4"
    use       the optional pointer fields it sets: "map0", "src1", "map1", "bias", "rowvec", "rowvec_map", "residual", "res_map", "src2", "map2",
              "gn" (gn_scale + gn_shift, made on the host: no GroupNorm kernel is called anywhere in these tests) and "qstats"
    n_src / n_src2 / n_vec / n_res   samples in a source read through map0 / map1, in the side source (map2), rows of the row-vector
              table, samples of the residual (each only where its map is set: a table without a map has n_img rows)
    expect    the exact dc_igemm_variant string
    env       {} or {"DCAMD_HALO_NO_STAG": "1"} — the one switch dc_conv3_halo_plan reads per call
    instance  the template instance the launch takes, from geometry(case) (tests/test_conv_halo_cases.py holds it against dc_igemm_instance)
    H, W      the image the kernel walks (four-phase upsample: the LOW-resolution source; Hin = 2 H)
Not in scope: producer-side GroupNorm (pn_out: tests/test_gpu_ops.py has its tests, and its cross-workgroup waits are no place for a
shape sweep on shared machines), the switches read once per process (DCAMD_WS_PLAIN, DCAMD_NO_MOSAIC, ...), and every kernel that is not
conv3_* / igemm_pipe_up4.  Plain Python and CPU torch only: nothing here opens a device.

"Chunk" below is the dispatcher's K granule of 128 bytes (BKE elements: 32 fp32, 64 bf16 / f16); C0 and C1 are multiples of it.

How much room there is.  The plain emulation of tests/test_conv_halo_cases.py (fp32 accumulation tap by tap, correctly rounded output)
reaches err / bound 0.27 - 0.92 with a bf16 output, 0.04 - 0.69 with an f16 output (at K of a thousand and more the accumulation term
2 (K + 8) 2^-24 |A| |W|^T is of the size of f16's rounding unit), <= 0.003 with fp32 throughout, and <= 0.41 with an fp32 output of a 16-bit
conv (the most where the emulation rounds a flagged prologue element the other way).  Largest err / bound on an MI355X per family
(tests/test_gpu_conv_halo.py prints it per case): RECORDED below."""
import torch
import torch.nn.functional as F

from gemm_tile_cases import BKE, EPS32, FLOOR, GUARD, SENTINEL, TD, U_OUT, _bits, e_act, silu_device

F32, BF16, F16 = 0, 1, 2
DTN = {F32: "f32", BF16: "bf16", F16: "f16"}
DTS = (F32, BF16, F16)
LIP = 1.13                                     # bounds the slope of SiLU (max 1.0998)
MANT = {BF16: 8, F16: 11}                      # significant bits
MIN_EXP = {BF16: -133, F16: -24}               # log2 of the subnormal spacing
FAMILIES = ("halo4", "halo8", "halo8_lockstep", "ws_gn", "thin", "up4")
NO_STAG = {"DCAMD_HALO_NO_STAG": "1"}
# largest err / bound per family on an MI355X (first device run of tests/test_gpu_conv_halo.py; 16-bit outputs set it, the quad records and
# the fp32 outputs stay far below)
RECORDED = {"halo4": 0.912, "halo8": 0.919, "halo8_lockstep": 0.902, "ws_gn": 0.923, "thin": 0.808, "up4": 0.889}


# ---- geometry: halo_geom and the plans of conv3_halo_plan.h, on the host ------------------------------------------------------------------
def _ilog2(v):
    return max(0, (v - 1).bit_length())


def kind(c):
    e = c["expect"]
    return ("pipe_up4" if e.startswith("igemm_pipe_up4") else "up4" if e.startswith("conv3_up4") else "ws" if e.startswith("conv3_ws") else
            "thin" if e.startswith("conv3_thin") else "halo")


def geometry(c):
    """What the launcher works out for the case: tile width / height, images per patch, tiles per image, mosaic, buffer-descriptor
    loaders (xbuf), waves, halo rows and loads per lane (3 <= nxl <= NXL asserted: the launcher returns DC_ERR_SHAPE otherwise)."""
    k, H, W = kind(c), c["H"], c["W"]
    es = 4 if c["dtype"] == F32 else 2
    if k == "pipe_up4":       # tap-gather kernel: no halo patch; the checker still wants image coordinates
        return dict(kind=k, waves=4, tw=W, th=H, ni=1, tiles_x=1, tiles_y=1, mosaic=False, xbuf=False, HR=0, nxl=0, staggered=False)
    if k == "thin":
        waves, pix, nt, nxl_max = 4, 256, 256, 6
    elif k == "ws":
        waves, pix, nt, nxl_max = 8, 256, 256, 6          # two teams of four waves; the loader team fetches the 256-pixel patch
    else:
        waves = 8 if (H <= 8 or W <= 8) else 4
        pix = nt = waves * 64
        nxl_max = 6 if waves == 4 else 7
    tw = min(W, 32)
    th = pix // tw
    if k == "ws":
        assert th <= H, (c["name"], "conv3_ws needs a full 256-pixel tile")
    th = min(th, H)
    ni = pix // (tw * th)
    mosaic = H < 8 or W < 8
    if mosaic:
        assert k in ("halo", "up4") and waves == 8 and tw == W and th == H and ni >= 2, c["name"]
        lmc = (_ilog2(ni) + 1) // 2
        cols = 1 << lmc
        rows = ni // cols
        hw = cols * (tw + 1) + 1
        HR = (rows * (th + 1) + 1) * hw
    else:
        hw = tw + 2
        HR = ni * (th + 2) * hw
    nxl = (HR * 4 + nt - 1) // nt
    assert nxl <= nxl_max and (k == "thin" or nxl >= 3), (c["name"], HR, nxl)
    ldmax = max(c["ld0"] or c["C0"], c["ld1"] or c["C1"], c.get("ld2", 0) or c.get("C2", 0))
    taps = 4 if k == "up4" else 9
    wbytes = (c["Cout"] + 127) // 128 * 128 * (4 if k == "up4" else 1) * taps * (c["C0"] + c["C1"]) * es
    xbuf = k == "ws" or (k != "thin" and ni == 1 and not mosaic and H * W * ldmax * es < 2 ** 31 and wbytes < 2 ** 31)
    stag = k == "halo" and waves == 8 and not c["env"].get("DCAMD_HALO_NO_STAG") and wbytes < 2 ** 31
    return dict(kind=k, waves=waves, tw=tw, th=th, ni=ni, tiles_x=W // tw, tiles_y=H // th, mosaic=mosaic, xbuf=xbuf, HR=HR, nxl=nxl,
                staggered=stag, taps=taps)


def instance(c):
    g, dn = geometry(c), DTN[c["dtype"]]
    k = g["kind"]
    if k == "pipe_up4":
        return f"igemm_pipe_up4<{dn},256x128,3st>"
    if k == "thin":
        return f"conv3_thin_kernel<{dn},{'gn' if 'gn' in c['use'] else 'plain'}>"
    if k == "ws":
        return f"conv3_ws_kernel<{dn},gn>" + ("+silu" if c["gn_silu"] else "")
    mode = 2 if g["mosaic"] else (1 if g["xbuf"] else 0)
    return f"conv3_halo_kernel<{dn},{g['waves']},{g['taps']},{mode}{',stag' if g['staggered'] else ''}>"


def halo_instance_key(c):
    """(NW, TAPS, MODE, staggered) of a conv3_halo / conv3_up4 case, None for the other kernels."""
    g = geometry(c)
    if g["kind"] not in ("halo", "up4"):
        return None
    return (g["waves"], g["taps"], 2 if g["mosaic"] else (1 if g["xbuf"] else 0), g["staggered"])


def qparts(c):
    """dc_igemm_qstats_parts of the case, from its documented rule (the host test compares it with the library's answer)."""
    k = kind(c)
    if k in ("pipe_up4", "thin") or c["H"] < 8 or c["W"] < 8 or c["out_dtype"] != c["dtype"] or c["Cout"] % 8:
        return 0
    lo = c["H"] * c["W"]
    return (4 if k == "up4" else 1) * (lo // 128 if lo >= 128 else 1)


def part_pixels(c):
    """[parts, pixels per part] output-pixel indices (row-major in the output image) of the quad-record parts, as include/dcamd.h
    documents them: a run of 128 consecutive pixels (the whole image below 128 pixels); on images wider than 32 pixels a part is 4 rows of
    a 32-column strip — the image is cut into blocks of 8 rows x 32 columns, blocks in row-major order, upper half before lower half.
    Four-phase upsample: parts [phase * np, (phase + 1) * np) are those of the LOW-resolution image, phase = 2 a + b, and hold the output
    pixels (2 y + a, 2 x + b)."""
    H, W = c["H"], c["W"]
    idx = torch.arange(H * W).view(H, W)
    if H * W < 128:
        lo = idx.reshape(1, -1)
    elif W <= 32:
        lo = idx.reshape(-1, 128)
    else:
        lo = idx.view(H // 8, 2, 4, W // 32, 32).permute(0, 3, 1, 2, 4).reshape(-1, 128)
    if kind(c) != "up4":
        return lo
    y, x = lo // W, lo % W
    return torch.cat([(2 * y + a) * (2 * W) + 2 * x + b for a in (0, 1) for b in (0, 1)], 0)


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _case(name, dt, family, H, W, n_img, *, expect, C0=None, C1=0, Cout=128, use=(), env=None, out_dtype=None, out_pad=0, res_pad=0, ld0_pad=0,
          C2=0, ld2_pad=0, gn_silu=0, tile_n=128, up4=0, n_src=None, n_src2=None, n_vec=None, n_res=None):
    g = BKE[dt]
    C0 = g if C0 is None else C0
    use = set(use) | ({"src1"} if C1 else set()) | ({"src2"} if C2 else set())
    assert ("rowvec" in use or "rowvec_map" not in use) and ("residual" in use or "res_map" not in use) and ("src2" in use or "map2" not in use)
    assert ("src1" in use or "map1" not in use) and ("src2" in use) == (C2 > 0)
    odt = dt if out_dtype is None else out_dtype
    Hin, Win = (2 * H, 2 * W) if up4 else (H, W)
    nin = 3 if n_img == 2 else (2 if n_img <= 5 else 5)          # tables read through a map: never n_img rows, so that the maps repeat
    if n_src is None:
        n_src = nin if "map0" in use or "map1" in use else n_img
    n_src2, n_vec, n_res = (nin if v is None else v for v in (n_src2, n_vec, n_res))
    c = dict(name=name, family=family, dtype=dt, taps=9, stride=1, upsample=up4, up4=up4, n_img=n_img, H=H, W=W, Hin=Hin, Win=Win, Hout=Hin, Wout=Win,
             C0=C0, ld0=C0 + ld0_pad, C1=C1, ld1=C1, Cout=Cout, tile_n=tile_n, act=0, rowvec_ld=Cout, res_dtype=dt, res_ld=Cout + res_pad,
             out_dtype=odt, out_ld=Cout + out_pad, C2=C2, ld2=C2 + ld2_pad if C2 else 0, gn_silu=gn_silu, use=frozenset(use), n_src=n_src,
             n_src2=n_src2, n_vec=n_vec, n_res=n_res, expect=expect % DTN[dt], env=dict(env or {}))
    c["instance"] = instance(c)
    if "qstats" in use:
        assert qparts(c) > 0, name
    return c


def _bundle(i, dt, qs_ok=True):
    """Feature set number i of the plain halo convs; together the six hold what every family / dtype must contain."""
    g = BKE[dt]
    sixteen = dt != F32
    qs = {"qstats"} if qs_ok else set()
    return [
        dict(C1=g, use={"bias", "map0", "map1"} | qs, Cout=128),                                                  # second source, different maps
        dict(C2=g, ld2_pad=8, use={"bias", "map2"} | qs, Cout=200, out_pad=8),   # 1x1 side source, two N tiles, channel tail
        dict(use={"bias", "rowvec", "rowvec_map"} | qs, ld0_pad=8, Cout=128),
        dict(use={"bias", "residual", "res_map", "map0"} | qs, res_pad=8, Cout=200),
        dict(C0=3 * g, C1=g, use={"bias", "rowvec", "map1"}, out_dtype=F32 if sixteen else None, out_pad=8),   # seam after an odd number of chunks
        dict(C1=g, C2=2 * g, ld2_pad=16, ld0_pad=16, res_pad=16, out_pad=16, Cout=200,
             use={"bias", "rowvec", "rowvec_map", "residual", "res_map", "map0", "map1", "map2"} | qs),
    ][i % 6]


def _halo_cases():
    out = []
    for dt in DTS:
        n = DTN[dt]
        g = BKE[dt]
        # conv3_halo<T,4w>: one image per patch, buffer-descriptor loaders
        for i, (H, W, ni) in enumerate([(16, 16, 3), (32, 16, 3), (16, 32, 3), (64, 64, 3), (16, 128, 3), (32, 32, 2)]):
            out.append(_case(f"halo4_{n}_{H}x{W}_b{i}", dt, "halo4", H, W, ni, expect="conv3_halo<%s,4w>", **_bundle(i, dt)))
        # conv3_halo<T,8w>, staggered and (DCAMD_HALO_NO_STAG) lock-step
        shapes8 = [(8, 8, 11), (8, 16, 5), (16, 8, 5), (8, 32, 3), (32, 8, 3), (8, 64, 3), (64, 8, 3), (128, 8, 2), (4, 4, 40), (4, 4, 3)]
        for fam, env in (("halo8", {}), ("halo8_lockstep", NO_STAG)):
            for i, (H, W, ni) in enumerate(shapes8):
                b = _bundle(i + (0 if fam == "halo8" else 3), dt, qs_ok=H >= 8)
                out.append(_case(f"{fam}_{n}_{H}x{W}_n{ni}_b{i}", dt, fam, H, W, ni, expect="conv3_halo<%s,8w>", env=env, **b))
            # deep K on the mosaic: 16 chunks over two sources, two N tiles (the up-path ResNets of the 4x4 level)
            out.append(_case(f"{fam}_{n}_4x4_deep", dt, fam, 4, 4, 33, expect="conv3_halo<%s,8w>", env=env, C0=8 * g, C1=8 * g, Cout=256,
                             use={"bias", "rowvec", "residual"}, n_vec=33, n_res=33))
    return out


def _ws_cases():
    out = []
    for dt in DTS:
        n, g = DTN[dt], BKE[dt]
        w = lambda tag, H, W, ni, **kw: out.append(_case(f"ws_gn_{n}_{H}x{W}_{tag}", dt, "ws_gn", H, W, ni, expect="conv3_ws<%s,gn>",
                                                         use=set(kw.pop("use", ())) | {"gn", "bias"}, **kw))
        w("plain", 16, 16, 3, gn_silu=0, use={"qstats"})
        w("silu_two_maps", 16, 16, 3, gn_silu=1, C0=g, C1=g, use={"map0", "map1"})
        w("silu_side", 8, 32, 3, gn_silu=1, C2=g, ld2_pad=8, use={"map2", "qstats"}, Cout=200, out_pad=8)
        w("res_map0", 8, 32, 3, gn_silu=0, use={"residual", "res_map", "map0", "rowvec", "rowvec_map"}, res_pad=8, ld0_pad=8)
        w("silu_two_ntiles", 32, 32, 2, gn_silu=1, C0=3 * g, C1=g, Cout=200, use={"rowvec"}, n_vec=2, out_dtype=F32 if dt != F32 else None)
        w("silu_tall", 32, 16, 2, gn_silu=1, use={"map1", "qstats"}, C1=g, n_src=3)
        w("silu_wide", 16, 64, 2, gn_silu=1, use={"map0", "residual", "qstats"}, n_res=2, out_pad=8)
        w("plain_wide_side", 16, 64, 2, gn_silu=0, C2=2 * g, use={"residual", "res_map", "map0"}, res_pad=16, ld0_pad=16, Cout=128)
        if dt != F32:         # the affine table exactly fills its LDS slot
            w("silu_c512", 16, 16, 2, gn_silu=1, C0=256, C1=256, use={"map0", "map1"})
    return out


def _thin_cases():
    out = []
    for dt in DTS:
        n, g = DTN[dt], BKE[dt]
        t = lambda tag, H, W, ni, Cout, **kw: out.append(_case(f"thin_{n}_{H}x{W}_c{Cout}_{tag}", dt, "thin", H, W, ni, expect="conv3_thin<%s>",
                                                               Cout=Cout, tile_n=32, use=set(kw.pop("use", ())) | {"bias"}, **kw))
        t("plain", 16, 16, 3, 1)
        t("plain_two", 16, 32, 3, 3, C1=g, use={"map0", "map1"}, out_pad=5)
        t("plain_f32out", 32, 16, 3, 5, out_dtype=F32, ld0_pad=8)
        t("plain_big", 64, 32, 2, 16, C0=2 * g, out_pad=8)
        t("gn", 16, 16, 3, 3, use={"gn"}, gn_silu=0, out_pad=1)
        t("gn_silu_two", 16, 32, 3, 16, use={"gn", "map0", "map1"}, C1=g, gn_silu=1)
        t("gn_silu_f32out", 32, 16, 3, 1, use={"gn"}, gn_silu=1, out_dtype=F32, out_pad=3)
        t("gn_silu_big", 64, 32, 2, 5, use={"gn", "map0"}, gn_silu=1, C0=2 * g, ld0_pad=8)
    return out


def _up4_cases():
    out = []
    for dt in DTS:
        n, g = DTN[dt], BKE[dt]
        u = lambda H, W, ni, expect, tag, **kw: out.append(_case(f"up4_{n}_{H}x{W}_{tag}", dt, "up4", H, W, ni, expect=expect, up4=1,
                                                                 use=set(kw.pop("use", ())) | {"bias"}, **kw))
        u(16, 16, 3, "conv3_up4<%s,4w>", "4w", use={"rowvec", "rowvec_map", "qstats"}, Cout=128)
        u(16, 32, 2, "conv3_up4<%s,4w>", "4w", use={"map0", "qstats"}, Cout=200, out_pad=8)
        u(8, 8, 11, "conv3_up4<%s,8w>", "8w", use={"map0", "rowvec", "qstats"}, Cout=200, n_vec=11)
        u(8, 16, 5, "conv3_up4<%s,8w>", "8w", use={"rowvec", "rowvec_map", "qstats"}, Cout=128, out_pad=8, ld0_pad=8)
        u(16, 8, 5, "conv3_up4<%s,8w>", "8w", use={"map0"}, Cout=128, C0=2 * g, out_dtype=F32 if dt != F32 else None)
        u(64, 8, 2, "conv3_up4<%s,8w>", "8w_one_image", use={"rowvec", "qstats"}, Cout=128, n_vec=2)      # <T,8,4,1>: buffer descriptors
        # 4x4 sources take the mosaic patch of the 8-wave kernel (<T,8,4,2>), not the tap-gather kernel
        u(4, 4, 40, "conv3_up4<%s,8w>", "8w_mosaic", use={"map0", "rowvec", "rowvec_map"}, Cout=200, out_pad=8)
        u(4, 4, 3, "conv3_up4<%s,8w>", "8w_mosaic_n3", Cout=128)
        u(2, 2, 7, "igemm_pipe_up4<%s,256x128,3st>", "pipe", use={"map0", "rowvec", "rowvec_map"}, Cout=200, out_pad=8)
        u(4, 16, 3, "igemm_pipe_up4<%s,256x128,3st>", "pipe", use={"rowvec"}, Cout=128)
        u(2, 8, 5, "igemm_pipe_up4<%s,256x128,3st>", "pipe", use={"map0"}, Cout=128, out_dtype=F32 if dt != F32 else None)
    return out


CASES = _halo_cases() + _ws_cases() + _thin_cases() + _up4_cases()
# launch-to-launch identity, other traffic in between: one case each of halo4, halo8 staggered, the mosaic, ws_gn and conv3_up4<4w>
REPEAT_CASES = ["halo4_bf16_64x64_b3", "halo8_bf16_8x8_n11_b0", "halo8_bf16_4x4_n40_b8", "ws_gn_bf16_8x32_silu_side", "up4_bf16_16x16_4w"]
# (NW, TAPS, MODE, staggered) instances of conv3_halo_kernel without pn_out that no case reaches, and why; tests/test_conv_halo_cases.py
# shows each out of reach on a probe grid
UNREACHABLE = {
    (4, 9, 0, False): "4 waves without buffer descriptors: a source sample of 2 GiB and more",
    (4, 4, 0, False): "4 waves without buffer descriptors: a source sample of 2 GiB and more",
}


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def rows(c):
    return c["n_img"] * c["Hout"] * c["Wout"]


def k_all(c):
    return 9 * (c["C0"] + c["C1"]) + c["C2"]


PTR_FIELDS = ("src0", "W", "out", "map0", "src1", "map1", "bias", "rowvec", "rowvec_map", "residual", "res_map", "src2", "map2", "W2", "gn_scale",
              "gn_shift", "qstats")


def igemm_fields(c, ptrs):
    """The dc_igemm_params fields of a case; ptrs: {pointer field: address}."""
    kw = {k: c[k] for k in ("dtype", "taps", "stride", "upsample", "n_img", "Hin", "Win", "Hout", "Wout", "C0", "ld0", "C1", "ld1", "Cout", "tile_n", "act",
                            "rowvec_ld", "res_dtype", "res_ld", "out_dtype", "out_ld", "C2", "ld2", "gn_silu", "up4")}
    names = {"src0", "W", "out"} | (set(c["use"]) - {"gn"})
    if "gn" in c["use"]:
        names |= {"gn_scale", "gn_shift"}
    if "src2" in c["use"]:
        names.add("W2")
    for f in sorted(names):
        kw[f] = ptrs[f]
    return kw


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def _map(n_out, n_in, kind_):
    """Sample maps that repeat and reorder: three different patterns, none the identity."""
    i = torch.arange(n_out)
    return {"a": (n_in - 1 - i) % n_in, "b": (i // 2 + 1) % n_in, "c": (3 * i + 1 + i // 3) % n_in}[kind_].to(torch.int32)


def make_operands(c, seed=None):
    """CPU fp32 tensors, the MFMA operands and the residual already rounded to the compute type: x0 / x1 [n_src, H, W, C] (activations
    1.5 randn + 0.3: the non-zero mean makes a leaked neighbour pixel show), x2 [n_src2, Hout, Wout, C2], w [Cout, C0 + C1, 3, 3] (four-phase
    cases: on the grid k / 32, |k| <= 31, so that every phase sum of up to four taps is exact in all three types), w2 [Cout, C2], bias,
    tables, maps, and the per-sample GroupNorm affine gn_scale / gn_shift [n_img, C0 + C1] (scale around 1, shift of order 1)."""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"])) if seed is None else seed
    gen = torch.Generator().manual_seed(7000 + seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    q = lambda t: t.to(TD[c["dtype"]]).float()
    use, H, W, Ct = c["use"], c["H"], c["W"], c["C0"] + c["C1"]
    o = dict(x0=q(1.5 * rn(c["n_src"] if "map0" in use else c["n_img"], H, W, c["C0"]) + 0.3))
    if c["C1"]:
        o["x1"] = q(1.5 * rn(c["n_src"] if "map1" in use else c["n_img"], H, W, c["C1"]) + 0.3)
    if c["up4"]:
        o["w"] = torch.randint(-31, 32, (c["Cout"], Ct, 3, 3), generator=gen).float() / 32.0
    else:
        o["w"] = q(rn(c["Cout"], Ct, 3, 3) / (3.0 * Ct ** 0.5))
    if "map0" in use:
        o["map0"] = _map(c["n_img"], c["n_src"], "a")
    if "map1" in use:
        o["map1"] = _map(c["n_img"], c["n_src"], "b")
    if c["C2"]:
        o["x2"] = q(1.5 * rn(c["n_src2"] if "map2" in use else c["n_img"], c["Hout"], c["Wout"], c["C2"]) + 0.3)
        o["w2"] = q(rn(c["Cout"], c["C2"]) / c["C2"] ** 0.5)
        if "map2" in use:
            o["map2"] = _map(c["n_img"], c["n_src2"], "c")
    if "bias" in use:
        o["bias"] = rn(c["Cout"])
    if "rowvec" in use:
        o["rowvec"] = rn(c["n_vec"] if "rowvec_map" in use else c["n_img"], c["Cout"])
        if "rowvec_map" in use:
            o["rowvec_map"] = _map(c["n_img"], c["n_vec"], "c")
    if "residual" in use:
        o["residual"] = q(rn(c["n_res"] if "res_map" in use else c["n_img"], c["Hout"] * c["Wout"], c["Cout"]))
        if "res_map" in use:
            o["res_map"] = _map(c["n_img"], c["n_res"], "b")
    if "gn" in use:
        o["gn_scale"] = 1.0 + 0.25 * rn(c["n_img"], Ct)
        o["gn_shift"] = rn(c["n_img"], Ct)
    return o


def gathered(c, o, dtype=torch.float64, shift0=None):
    """[n_img, H, W, C0 + C1]: the sources read through their maps and concatenated.  shift0 = (sample, d): that output sample reads source
    sample map0 + d instead (a planted fault)."""
    i0 = o["map0"].long() if "map0" in o else torch.arange(c["n_img"])
    if shift0 is not None:
        i0 = i0.clone()
        i0[shift0[0]] = (i0[shift0[0]] + shift0[1]) % o["x0"].shape[0]
    x = o["x0"][i0]
    if c["C1"]:
        x = torch.cat([x, o["x1"][o["map1"].long()] if "map1" in o else o["x1"]], -1)
    return x.to(dtype)


def unfold3(x):
    """[n, H, W, C] -> [n * H * W, 9 * C]: the zero-padded 3x3 patches, k = tap * C + ch, tap = ky * 3 + kx."""
    n, H, W, C = x.shape
    p = F.unfold(x.permute(0, 3, 1, 2), 3, padding=1)
    return p.reshape(n, C, 9, H * W).permute(0, 3, 2, 1).reshape(n * H * W, 9 * C)


def upsample2(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def w_matrix(c, o, dtype=torch.float64):
    """[Cout, 9 * (C0 + C1)], k = tap * C + ch."""
    return o["w"].permute(0, 2, 3, 1).reshape(c["Cout"], -1).to(dtype)


def per_row(c, o, table, tmap):
    t = o[table][o[tmap].long()] if tmap in o else o[table]
    return t.repeat_interleave(c["Hout"] * c["Wout"], 0)


def residual_rows(c, o, shift=0):
    idx = o["res_map"].long() if "res_map" in o else torch.arange(c["n_img"])
    return o["residual"][(idx + shift) % o["residual"].shape[0]].reshape(rows(c), -1)


def side_rows(c, o):
    x2 = o["x2"][o["map2"].long()] if "map2" in o else o["x2"]
    return x2.reshape(rows(c), -1)


# ---- the fused GroupNorm prologue ---------------------------------------------------------------------------------------------------
def ulp_toward(r, y, dt):
    """Spacing of the type's values between r = round(y) and its neighbour on y's side (fp64 tensors)."""
    ar = r.abs()
    m = torch.where(y.abs() >= ar, ar, ar * (1.0 - 2.0 ** -13))           # just below a power of two the spacing halves
    ex = torch.floor(torch.log2(m.clamp_min(2.0 ** -140))) - (MANT[dt] - 1)
    return torch.exp2(ex.clamp_min(MIN_EXP[dt]))


def prologue(c, o, x):
    """x [n_img, H, W, C] fp64 -> (a, amb, flagged): the operand a := act(x * gn_scale[n] + gn_shift[n]) as the MFMA receives it, and how far
    the device's copy of an element may be from it.

    The device (conv3_ws.hip `xform`, conv3_thin_kernel) forms v = x * scale + shift in fp32 — one rounding if the compiler contracts it
    into a fused multiply-add, two if not: |error| <= 1.01 u (|x scale| + |v|), u = 2^-24 — then, with gn_silu, silu_t<T>(v): silu_f (expf,
    IEEE divide) for fp32, silu_fast_f (v_exp_f32 of a rounded argument, v_rcp_f32) for 16-bit types, whose errors e_act states; the
    argument's error passes through SiLU's slope (<= LIP).  The result is rounded ONCE to the compute type (f_to_chunk).  So
      fp32:   a = the fp64 value, amb = that evaluation error e (a forward error of the operand)
      16-bit: a = the fp64 value rounded to the type; the device rounds the other way only where the fp64 value lies within e of a
              rounding tie.  Those elements are flagged, and amb = the spacing of the type there (the device's value is the neighbour)."""
    dt = c["dtype"]
    sc, sh = o["gn_scale"].double()[:, None, None, :], o["gn_shift"].double()[:, None, None, :]
    prod = x * sc
    v = prod + sh
    e = 1.01 * EPS32 * (prod.abs() + v.abs())
    y = v
    if c["gn_silu"]:
        y = F.silu(v)
        e = LIP * e + e_act("silu", v, dt != F32)
    if dt == F32:
        return y, e + EPS32 * y.abs(), torch.zeros_like(y, dtype=torch.bool)
    r = y.to(TD[dt]).double()
    sp = ulp_toward(r, y, dt)
    flagged = (0.5 * sp - (y - r).abs()) <= e
    return r, flagged * sp, flagged


def prologue_device(c, o, x):
    """The same in fp32 with the device's formula (x: fp32, exact in the compute type), rounded to the compute type."""
    v = x * o["gn_scale"][:, None, None, :] + o["gn_shift"][:, None, None, :]
    if c["gn_silu"]:
        v = silu_device(v, c["dtype"] != F32)
    return v.to(TD[c["dtype"]]).float()


# ---- reference and bound ------------------------------------------------------------------------------------------------------------
def reference(c, o, detail=False):
    """(ref, bound): the fp64 result of the documented contract (include/dcamd.h: gather through the maps, zero padding, concat, the
    prologue on real pixels, the 1x1 side source, (+bias)(+rowvec)(+residual)) over every output element [M, Cout], and the bound on
    |got - ref|:

        1.02 u_out |ref| + floor + 2 (K_all + 8) 2^-24 (|A| |W|^T + |A2| |W2|^T + |bias| + |rowvec| + |residual|) + amb |W|^T

    K_all = 9 (C0 + C1) + C2.  (K + 8) 2^-24 is the forward bound of an fp32 dot product of length K in any summation order plus the
    handful of epilogue operations, the factor 2 because the matrix core's internal accumulation is not documented to round every addition
    to nearest; amb is the prologue's term (see `prologue`; zero without it); u_out / floor: the rounding of the stored value.  Nothing here
    comes from what a kernel returned.  detail: also a dict with the forward error e (the bound without the output rounding), the
    largest ambiguity term and the share of flagged inputs."""
    x = gathered(c, o)
    amb = flagged = None
    if "gn" in c["use"]:
        x, amb, flagged = prologue(c, o, x)
    if c["up4"]:
        x = upsample2(x)
    A, Wm = unfold3(x), w_matrix(c, o)
    val, S = A @ Wm.t(), A.abs() @ Wm.abs().t()
    del A
    ambterm = None
    if amb is not None:
        ambterm = unfold3(amb) @ Wm.abs().t()
    if c["C2"]:
        A2, W2 = side_rows(c, o).double(), o["w2"].double()
        val += A2 @ W2.t()
        S += A2.abs() @ W2.abs().t()
    if "bias" in o:
        val += o["bias"].double()
        S += o["bias"].double().abs()
    if "rowvec" in o:
        rv = per_row(c, o, "rowvec", "rowvec_map").double()
        val += rv
        S += rv.abs()
    if "residual" in o:
        r = residual_rows(c, o).double()
        val += r
        S += r.abs()
    e = 2.0 * (k_all(c) + 8) * EPS32 * S
    if ambterm is not None:
        e = e + ambterm
    bound = 1.02 * U_OUT[c["out_dtype"]] * val.abs() + FLOOR[c["out_dtype"]] + e
    if detail:
        return val, bound, dict(e=e, amb_max=0.0 if ambterm is None else float(ambterm.max()),
                                flagged_share=0.0 if flagged is None else float(flagged.double().mean()), out_std=float(val.std()))
    return val, bound


def qstats_reference(c, val, e):
    """(mean, M2, bound_mean, bound_M2), each [n_img, parts, Cout / 4]: the quad records of the fp64 values `val` [M, Cout] before the
    output rounding, per (sample, part, quad of 4 channels) over the part's pixels (part_pixels), and how far the device's records may lie.

    The device holds v' with |v' - v| <= e per element (e: the forward error of `reference`).  Over the count = 4 * pixels values of a
    record: mean' - mean = mean(v' - v), so |.| <= mean(e).  With d = v' - v and the centred values z, z' = z + (d - mean d):
    M2' = M2 + 2 sum z (d - mean d) + sum (d - mean d)^2, and sum (d - mean d)^2 <= sum d^2 <= sum e^2, |sum z (d - mean d)| <=
    sqrt(M2 sum e^2) (Cauchy-Schwarz): |M2' - M2| <= 2 sqrt(M2 sum e^2) + sum e^2.
    The device forms shifted sums in fp32 about a pivot p that is one of the record's own values (igemm_epilogue.h): S = sum (v' - p),
    Q = sum (v' - p)^2, mean = p + S / count, M2 = Q - S^2 / count.  Each sum of `count` fp32 terms carries at most
    gamma = (count + 8) 2^-24 relative to the sum of its terms' magnitudes, the 8 covering the subtraction of the pivot, the square, the
    final fused multiply-adds.  With D = max |v - mean| over the record, |p - mean| <= D: sum |v - p| <= sum |v - mean| + count D <=
    2 count D, so the mean moves by <= gamma 2 D (+ one rounding of the result, 2^-24 |mean|); Q = M2 + count (mean - p)^2 <= M2 + count
    D^2 and S^2 / count = count (mean - p)^2 <= count D^2 (its relative error twice that of S), so M2 moves by <= gamma (M2 + 3 count D^2).
    D and M2 are taken from the reference widened by the element errors (D + max e)."""
    n, HW, Co = c["n_img"], c["Hout"] * c["Wout"], c["Cout"]
    pp = part_pixels(c)
    parts, npx = pp.shape
    count = 4 * npx
    v = val.view(n, HW, Co // 4, 4)[:, pp]                  # [n, parts, npx, quads, 4]
    ee = e.view(n, HW, Co // 4, 4)[:, pp]
    mean = v.mean((2, 4))
    z = v - mean[:, :, None, :, None]
    m2 = (z ** 2).sum((2, 4))
    se2 = (ee ** 2).sum((2, 4))
    D = z.abs().amax((2, 4)) + ee.amax((2, 4))
    gam = (count + 8) * EPS32
    b_mean = ee.mean((2, 4)) + gam * 2.0 * D + EPS32 * mean.abs()
    b_m2 = 2.0 * torch.sqrt(m2 * se2) + se2 + gam * (m2 + se2 + 2.0 * torch.sqrt(m2 * se2) + 3.0 * count * D ** 2)
    return mean, m2, b_mean, b_m2


# ---- the checker --------------------------------------------------------------------------------------------------------------------
def new_output(c, device="cpu"):
    """The flat output buffer of a case, sentinel everywhere: M rows of out_ld elements and a guard region behind them."""
    return torch.full((rows(c) * c["out_ld"] + GUARD,), SENTINEL, dtype=TD[c["out_dtype"]], device=device)


def new_qstats(c, device="cpu"):
    """The flat quad-record buffer [n_img, parts, Cout / 4, 2] fp32 and a guard region behind it, sentinel everywhere."""
    return torch.full((c["n_img"] * qparts(c) * (c["Cout"] // 4) * 2 + GUARD,), SENTINEL, dtype=torch.float32, device=device)


def where(c, row, ch):
    """A failing element in the kernel's own coordinates: (sample, y, x, channel), its patch, its tile and whether it sits on an image
    border or a tile seam."""
    g = geometry(c)
    HW, Wo = c["Hout"] * c["Wout"], c["Wout"]
    n, rem = divmod(int(row), HW)
    y, x = divmod(rem, Wo)
    ly, lx = (y // 2, x // 2) if c["up4"] else (y, x)
    ty, tx = ly // g["th"], lx // g["tw"]
    marks = []
    if y in (0, c["Hout"] - 1) or x in (0, c["Wout"] - 1):
        marks.append("image border")
    if (g["tiles_y"] > 1 and ly % g["th"] in (0, g["th"] - 1)) or (g["tiles_x"] > 1 and lx % g["tw"] in (0, g["tw"] - 1)):
        marks.append("tile seam")
    if g["ni"] > 1 and (n % g["ni"] in (0, g["ni"] - 1)):
        marks.append("patch boundary")
    ph = f" phase ({y % 2},{x % 2})" if c["up4"] else ""
    return f"(sample {n}, y {y}, x {x}, channel {int(ch)}) patch {n // g['ni']} image-in-patch {n % g['ni']} tile (ty {ty}, tx {tx}){ph}" + \
           (" [" + ", ".join(marks) + "]" if marks else "")


def check_output(c, buf, ref, bound, qbuf=None, e=None):
    """buf: the flat output buffer (CPU) after the launch.  Returns (problems, worst err / bound): every element finite and inside its
    bound; the pad columns (out_ld > Cout), and with them everything past row M (the guard region), still the sentinel bit for bit.  With
    qbuf (the flat quad-record buffer; e: the forward error from reference(detail=True)) the records are checked against qstats_reference
    the same way and count into `worst`."""
    M, co, ld = rows(c), c["Cout"], c["out_ld"]
    problems = []
    sent = _bits(torch.full((1,), SENTINEL, dtype=buf.dtype))[0]
    body = buf[: M * ld].view(M, ld)
    if not bool((_bits(buf[M * ld:]) == sent).all()):
        problems.append(f"{int((_bits(buf[M * ld:]) != sent).sum())} elements behind row M were written")
    if ld > co and not bool((_bits(body[:, co:]) == sent).all()):
        bad = (_bits(body[:, co:]) != sent).nonzero()
        problems.append(f"{len(bad)} pad-column elements were written, first at {where(c, bad[0][0], co + int(bad[0][1]))}")
    got = body[:, :co].double()
    if not bool(torch.isfinite(got).all()):
        problems.append(f"{int((~torch.isfinite(got)).sum())} non-finite values, first at {where(c, *(~torch.isfinite(got)).nonzero()[0])}")
        got = torch.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
    ratio = (got - ref).abs() / bound
    worst = float(ratio.max())
    if worst > 1.0:
        bad = (ratio > 1.0).nonzero()
        i, j = (int(v) for v in bad[int(ratio[ratio > 1.0].argmax())])
        first = "; ".join(where(c, r, ch) for r, ch in bad[:6].tolist())
        problems.append(f"{len(bad)} of {M * co} elements outside the bound, worst err / bound {worst:.3g} at {where(c, i, j)} (got {float(got[i, j])!r}, "
                        f"ref {float(ref[i, j])!r}, bound {float(bound[i, j]):.3g}); pixels {len({int(r) for r, _ in bad.tolist()})}; the first: {first}")
    if qbuf is not None:
        n, parts, nq = c["n_img"], qparts(c), co // 4
        nrec = n * parts * nq * 2
        if not bool((_bits(qbuf[nrec:]) == _bits(torch.full((1,), SENTINEL))[0]).all()):
            problems.append("quad records: elements behind the last record were written")
        rec = qbuf[:nrec].view(n, parts, nq, 2).double()
        if not bool(torch.isfinite(rec).all()):
            problems.append(f"quad records: {int((~torch.isfinite(rec)).sum())} non-finite values")
            rec = torch.nan_to_num(rec, nan=1e30, posinf=1e30, neginf=-1e30)
        mean, m2, bm, b2 = qstats_reference(c, ref, e)
        for label, g_, r_, b_ in (("mean", rec[..., 0], mean, bm), ("M2", rec[..., 1], m2, b2)):
            rq = (g_ - r_).abs() / b_
            wq = float(rq.max())
            worst = max(worst, wq)
            if wq > 1.0:
                s, p, qd = (int(v) for v in (rq > 1.0).nonzero()[int(rq[rq > 1.0].argmax())])
                problems.append(f"quad records: {int((rq > 1.0).sum())} of {rq.numel()} {label} values outside the bound, worst {wq:.3g} at (sample {s}, "
                                f"part {p} of {parts}, quad {qd}): got {float(g_[s, p, qd])!r}, ref {float(r_[s, p, qd])!r}, bound {float(b_[s, p, qd]):.3g}")
    return problems, worst
