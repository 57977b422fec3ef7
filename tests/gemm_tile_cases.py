"""The cases of the tile-kernel parity tests (igemm_wide8<256x256>, igemm_pipe<256x128,3st>, igemm_pipe<128x128,2st>), their operands,
their fp64 reference, the per-element error bound and the checker — one table, two consumers: tests/test_gemm_tile_cases.py (host only:
routing, coverage, the checker held against planted faults) and tests/test_gpu_gemm_tiles.py (the kernels themselves).

A case is a dict of dc_igemm's plain fields (the dc_igemm_params names) plus
    name    its id
    use     the optional pointer fields it sets: "map0", "src1", "map1", "bias", "rowvec", "rowvec_map", "gate", "gate_map", "residual", "res_map"
    n_src / n_vec / n_res   samples in the sources (read through map0 / map1), rows of the row-vector / gate tables, samples of the residual
    expect  the exact dc_igemm_variant string
    env     {} or {"DCAMD_PIPE_CHIP_TILES": "0"} — the one switch the dispatcher reads per call
    tag     the epilogue branch: "none", "silu", "geglu", "gelu_tanh" or "gate"
    big     chip-filling (the host test skips its emulation for time)
Plain Python and CPU torch only: nothing here opens a device."""

import torch
import torch.nn.functional as F

F32, BF16, F16 = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_GELU_TANH = 0, 1, 2, 3
TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
DTN = {F32: "f32", BF16: "bf16", F16: "f16"}
BKE = {F32: 32, BF16: 64, F16: 64}            # elements of one K-tile (128 bytes per row)
U_OUT = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}      # round to nearest: 8 / 11 significant bits
FLOOR = {F32: 0.0, BF16: 0.0, F16: 2.0 ** -24}            # f16 subnormal spacing
SENTINEL = 7.0                                # what the output buffer holds before the launch (exact in every type)
GUARD = 4096                                  # elements behind the last row that must keep it
BRANCHES = ["none", "silu", "geglu", "gelu_tanh", "gate"]
TAG_ACT = {"none": ACT_NONE, "silu": ACT_SILU, "geglu": ACT_GEGLU, "gelu_tanh": ACT_GELU_TANH, "gate": ACT_NONE}
WIDE, P256, P128 = "igemm_wide8<%s,256x256>", "igemm_pipe<%s,256x128,3st>", "igemm_pipe<%s,128x128,2st>"


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _case(name, dt, tag, *, n_img, HW=None, H=None, W=None, taps=1, C0, C1=0, Cout, use=(), out_dtype=None, out_pad=0, res_pad=0,
          n_src=None, n_vec=5, n_res=3, expect, env=None, big=False):
    """1 tap: n_img samples of HW rows.  9 taps: the stride-2 3x3 conv of n_img images of H x W."""
    act = TAG_ACT[tag]
    if taps == 1:
        Hin, Win, Ho, Wo, stride = HW, 1, HW, 1, 1
    else:
        Hin, Win, stride = H, W, 2
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    use = set(use) | ({"gate"} if tag == "gate" else set()) | ({"src1"} if C1 else set())
    assert ("rowvec" in use or "rowvec_map" not in use) and ("residual" in use or "res_map" not in use) and ("gate" in use or "gate_map" not in use)
    cout_out = Cout // 2 if act == ACT_GEGLU else Cout
    odt = dt if out_dtype is None else out_dtype
    maps = bool(use & {"map0", "map1"})
    return dict(name=name, dtype=dt, taps=taps, stride=stride, upsample=0, n_img=n_img, Hin=Hin, Win=Win, Hout=Ho, Wout=Wo, C0=C0, ld0=C0, C1=C1, ld1=C1,
                Cout=Cout, tile_n=128, act=act, rowvec_ld=cout_out, gate_ld=cout_out, res_dtype=dt, res_ld=cout_out + res_pad, out_dtype=odt,
                out_ld=cout_out + out_pad, use=frozenset(use), n_src=(4 if maps else n_img) if n_src is None else n_src, n_vec=n_vec, n_res=n_res,
                expect=expect % DTN[dt], env=dict(env or {}), tag=tag, big=big)


def _wide_cases():
    """igemm_wide8 only runs where 256x256 tiles fill the chip (>= 400 of them), so every case is that large.  What each one is for:"""
    w = lambda name, dt, tag, **kw: _case("wide_" + name, dt, tag, expect=WIDE, big=True, **kw)
    return [
        # nk == 4 (the least the dispatcher admits); 402 tiles; the last M tile holds 37 rows (between 32 and 64: X half-tile 1 of wave row 0 part real)
        w("bf16_nk4_ragged37", BF16, "none", n_img=1, HW=200 * 256 + 37, C0=256, Cout=512, use={"bias"}),
        # the same K with an fp32 output; the last tile holds 20 rows (< 32: one X half-tile is all zero page); samples of 2561 rows: a sample
        # boundary inside a wave now and then, mostly one sample per wave (the rv_uni fetch)
        w("bf16_nk4_ragged20_f32out_rowvec", BF16, "none", n_img=20, HW=2561, C0=256, Cout=512, use={"bias", "rowvec"}, out_dtype=F32, n_vec=20),
        # fp32 (K-tile = 32 elements), nk == 4, fp32 residual with res_ld > Cout
        w("f32_nk4_residual", F32, "none", n_img=1, HW=200 * 256 + 37, C0=128, Cout=512, use={"bias", "residual"}, res_pad=8, n_res=1),
        # two sources, an ODD number of K-tiles (3) in the first: the seam falls inside a double-buffer pair; both through different sample
        # maps; 24-row samples (several per 64-row wave: the per-fragment row-vector fetch) with a mapped row vector; Cout = 1000: the channel
        # tail lies inside the second 128-half of the last 256-wide tile; out_ld > Cout; 404 tiles, nk == 5
        w("bf16_seam_tiny_samples_tail1000", BF16, "none", n_img=1069, HW=24, C0=192, C1=128, Cout=1000, out_pad=8,
          use={"bias", "map0", "map1", "rowvec", "rowvec_map"}, n_src=7),
        # K = 3072 (every DiT fc2), 18 MiB of weights: n_fast == 0, M-fastest tile order; 408 tiles
        w("bf16_k3072_mfast", BF16, "none", n_img=34, HW=256, C0=3072, Cout=3072, use={"bias", "residual"}, n_res=34),
        # GEGLU with bias and residual (16-bit needs K > 512 to come here), 800 tiles
        w("bf16_geglu_residual", BF16, "geglu", n_img=25, HW=1024, C0=768, Cout=2048, use={"bias", "residual", "res_map"}, res_pad=16),
        w("f32_geglu", F32, "geglu", n_img=50, HW=1024, C0=128, Cout=1024, use={"bias", "residual"}, n_res=50, out_pad=8),
        w("f16_geglu_odd_nk", F16, "geglu", n_img=1, HW=50 * 256 + 5, C0=576, Cout=2048, use={"bias"}, out_dtype=F32),
        # DiT's adaLN-Zero form: gate through gate_map together with a residual through res_map and a 16-bit output
        w("bf16_gate_residual_maps", BF16, "gate", n_img=50, HW=1024, C0=768, Cout=1536, use={"bias", "gate_map", "residual", "res_map"}, res_pad=8),
        w("f16_gate_residual_f32out", F16, "gate", n_img=67, HW=768, C0=320, Cout=1024, use={"bias", "residual"}, n_res=67, n_vec=67, out_dtype=F32, out_pad=8),
        # fp32 gate on 16-row samples (four per wave), odd nk
        w("f32_gate_tiny_samples", F32, "gate", n_img=3201, HW=16, C0=160, Cout=1024, use={"bias", "gate_map", "rowvec", "rowvec_map"}),
        # tanh-GELU with bias
        w("f16_gelu_tanh", F16, "gelu_tanh", n_img=50, HW=1024, C0=768, Cout=1024, use={"bias"}),
        w("bf16_gelu_tanh_tail", BF16, "gelu_tanh", n_img=1, HW=100 * 256 + 50, C0=320, Cout=1000, use={"bias", "rowvec"}, n_vec=1, out_pad=24, out_dtype=F32),
        w("f32_gelu_tanh", F32, "gelu_tanh", n_img=26, HW=1000, C0=192, Cout=1024, use={"bias", "residual", "res_map"}),
        # f16 plain: output in the compute type (the subnormal floor), 16-row samples with a mapped row vector, residual through res_map, res_ld > Cout
        w("f16_tiny_samples_res_map", F16, "none", n_img=1601, HW=16, C0=320, Cout=1024, use={"bias", "rowvec", "rowvec_map", "residual", "res_map"}, res_pad=8, out_pad=8),
    ]


def _pipe_cell(tile, form, dt, tag):
    """One small case per (tile, form, dtype, epilogue branch) cell of igemm_pipe.  256-row tile: more than 8 K-tiles and the chip-filling rule
    switched off; 128-row tile: what the dispatcher picks for a small problem by itself.  Never more than two N tiles, or 16-bit K <= 512 goes
    to igemm_xreg."""
    g = BKE[dt]
    name = f"pipe{tile}_{form}_{DTN[dt]}_{tag}"
    env = {"DCAMD_PIPE_CHIP_TILES": "0"} if tile == 256 else {}
    expect = P256 if tile == 256 else P128
    cout = 256 if tag == "geglu" else 200             # 200: a channel tail, two N tiles
    extra = {"none": dict(use={"bias", "rowvec", "rowvec_map", "residual", "res_map", "map0"}, out_pad=8, res_pad=16),
             "silu": dict(use={"bias", "rowvec"}, out_dtype=F32, n_vec=5),
             "geglu": dict(use={"bias", "residual"}, out_pad=8, n_res=5),
             "gelu_tanh": dict(use={"bias"}),
             "gate": dict(use={"bias", "gate_map", "residual", "res_map"}, res_pad=8)}[tag]
    if form == "slim":
        K = 10 * g if tile == 256 else 3 * g          # 10 / 3 K-tiles
        two = tag in ("none", "gate")                 # two sources: the seam after 3 (odd) / 1 K-tiles
        c0 = (3 * g if tile == 256 else g) if two else K
        if two:
            extra["use"] = set(extra["use"]) | {"map0", "map1"}
        # 5 samples of 60 / 52 rows: ragged against either tile, several samples per wave
        return _case(name, dt, tag, n_img=5, HW=60 if tile == 256 else 52, C0=c0, C1=K - c0, Cout=cout, expect=expect, env=env, **extra)
    # tap-gather: 3x3 stride 2 on 9x9 images -> 5x5 (25-row samples), 9 or 18 K-tiles
    c1 = g if tag in ("silu", "geglu") else 0
    if extra.get("n_res") == 5:
        extra["n_res"] = 3
    if extra.get("n_vec") == 5 and "rowvec_map" not in extra["use"]:
        extra["n_vec"] = 3
    return _case(name, dt, tag, taps=9, n_img=3, H=9, W=9, C0=g, C1=c1, Cout=cout, expect=expect, env=env, **extra)


def _natural_256_cases():
    """igemm_pipe<256x128,3st> with no switch set: >= 256 tiles, more than 8 K-tiles, an odd number of N tiles (not wide-eligible)."""
    out = []
    for dt in (F32, BF16, F16):
        K = 384 if dt == F32 else 768
        out.append(_case(f"nat256_slim_{DTN[dt]}_silu", dt, "silu", n_img=86, HW=256, C0=K, Cout=384, use={"bias", "rowvec"}, n_vec=86, out_pad=8,
                         expect=P256, big=True))
        out.append(_case(f"nat256_conv_{DTN[dt]}", dt, "none", taps=9, n_img=256, H=32, W=32, C0=64, Cout=128, use={"bias", "residual"}, n_res=256,
                         expect=P256, big=True))
    return out


def all_cases():
    cells = [_pipe_cell(t, f, dt, tag) for t in (128, 256) for f in ("slim", "tap") for dt in (F32, BF16, F16) for tag in BRANCHES]
    return _wide_cases() + cells + _natural_256_cases()


CASES = all_cases()
# launch-to-launch identity at size: one igemm_wide8 case per epilogue variant (bf16) and the two natural 256x128 ones
REPEAT_CASES = ["wide_bf16_nk4_ragged37", "wide_bf16_geglu_residual", "wide_bf16_gelu_tanh_tail", "wide_bf16_gate_residual_maps",
                "nat256_slim_bf16_silu", "nat256_conv_bf16"]
# (kernel family, dtype, branch) cells the dispatcher can never produce; tests/test_gemm_tile_cases.py proves each on a probe grid
UNREACHABLE = {
    # igemm_wide.hip has no SiLU instance: dc_igemm_pipe_shape's `wide_act`
    **{("wide", dt, "silu"): "no SiLU instance of the 256x256 kernel" for dt in (F32, BF16, F16)},
}


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def cout_out(c):
    return c["Cout"] // 2 if c["act"] == ACT_GEGLU else c["Cout"]


def rows(c):
    return c["n_img"] * c["Hout"] * c["Wout"]


def k_total(c):
    return c["taps"] * (c["C0"] + c["C1"])


PTR_FIELDS = ("src0", "W", "out", "map0", "src1", "map1", "bias", "rowvec", "rowvec_map", "gate", "gate_map", "residual", "res_map")


def igemm_fields(c, ptrs):
    """The dc_igemm_params fields of a case; ptrs: {pointer field: address} (src0, W, out and every name in c["use"])."""
    kw = {k: c[k] for k in ("dtype", "taps", "stride", "upsample", "n_img", "Hin", "Win", "Hout", "Wout", "C0", "ld0", "C1", "ld1", "Cout", "tile_n", "act",
                            "rowvec_ld", "gate_ld", "res_dtype", "res_ld", "out_dtype", "out_ld")}
    for f in ("src0", "W", "out") + tuple(sorted(c["use"])):
        kw[f] = ptrs[f]
    return kw


# ---- operands -------------------------------------------------------------------------------------------------------------------
def make_operands(c, seed=0):
    """CPU fp32 tensors, the MFMA operands already rounded to the compute type and the residual to ITS type (the kernel's operands are
    exactly these): x0 / x1 [n_src, Hs, Ws, C] (Hs x Ws = Hin x Win, with `upsample` the source of half those extents), w [Cout, K] with
    k = tap * (C0 + C1) + c (GEGLU: value rows, then gate rows), bias [Cout], tables and maps."""
    gen = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    ri = lambda hi, n: torch.randint(0, hi, (n,), generator=gen, dtype=torch.int32)
    q = lambda t: t.to(TD[c["dtype"]]).float()
    qr = lambda t: t.to(TD[c["res_dtype"]]).float()
    use, K, co = c["use"], k_total(c), cout_out(c)
    Hs, Ws = (c["Hin"] // 2, c["Win"] // 2) if c["upsample"] else (c["Hin"], c["Win"])
    o = dict(x0=q(rn(c["n_src"], Hs, Ws, c["C0"])), w=q(rn(c["Cout"], K) / K ** 0.5))
    if c["C1"]:
        o["x1"] = q(rn(c["n_src"], Hs, Ws, c["C1"]))
    for m in ("map0", "map1"):
        if m in use:
            o[m] = ri(c["n_src"], c["n_img"])
    if "bias" in use:
        o["bias"] = 0.5 * rn(c["Cout"])
    if "rowvec" in use:
        o["rowvec"] = rn(c["n_vec"] if "rowvec_map" in use else c["n_img"], co)
        if "rowvec_map" in use:
            o["rowvec_map"] = ri(c["n_vec"], c["n_img"])
    if "gate" in use:
        o["gate"] = rn(c["n_vec"] if "gate_map" in use else c["n_img"], co)
        if "gate_map" in use:
            o["gate_map"] = ri(c["n_vec"], c["n_img"])
    if "residual" in use:
        o["residual"] = qr(rn(c["n_res"] if "res_map" in use else c["n_img"], c["Hout"] * c["Wout"], co))
        if "res_map" in use:
            o["res_map"] = ri(c["n_res"], c["n_img"])
    return o


def a_matrix(c, o, dtype=torch.float64):
    """The GEMM's A operand [M, K] (the gather through the sample maps, with `upsample` the nearest 2x of the gathered source, and, for
    9 taps, the zero-padded 3x3 patches at the case's stride, k = tap * C + ch)."""
    x = o["x0"][o["map0"].long()] if "map0" in o else o["x0"]
    if c["C1"]:
        x = torch.cat([x, o["x1"][o["map1"].long()] if "map1" in o else o["x1"]], -1)
    x = x.to(dtype)
    if c["upsample"]:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    C = x.shape[-1]
    if c["taps"] == 1:
        return x.reshape(-1, C)
    p = F.unfold(x.permute(0, 3, 1, 2), 3, padding=1, stride=c["stride"])          # [n, C * 9, L], channel-major
    return p.reshape(x.shape[0], C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C)


def per_row(c, o, table, tmap):
    """[M, channels] view of a per-sample table read through its map."""
    t = o[table][o[tmap].long()] if tmap in o else o[table]
    return t.repeat_interleave(c["Hout"] * c["Wout"], 0)


def residual_rows(c, o):
    r = o["residual"][o["res_map"].long()] if "res_map" in o else o["residual"]
    return r.reshape(rows(c), -1)


# ---- the activations as the device functions of csrc/common.h compute them, and how far those may be from the exact ones ------
LIP = 1.13            # bounds the slope of SiLU (max 1.0998) and of both GELUs (max 1.129)
EPS32 = 2.0 ** -24    # unit roundoff of fp32
TINY = 2.0 ** -126    # smallest normal fp32: results below it may be flushed to zero


def silu_device(x, fast):
    """fp32 tensor in, fp32 out: silu_f (expf, IEEE divide) or silu_fast_f (v_exp_f32 on a rounded argument, v_rcp_f32)."""
    if fast:
        return x * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * x)))
    return x / (1.0 + torch.exp(-x))


def gelu_tanh_device(x, fast):
    u = 0.79788456080286535588 * (x + 0.044715 * x * x * x)
    if fast:
        return x * (1.0 / (1.0 + torch.exp2(-2.8853900817779268 * u)))
    return x / (1.0 + torch.exp(-2.0 * u))


def gelu_erf_device(x, fast):
    z = x * 0.70710678118654752440
    az = z.abs()
    t = 1.0 / (1.0 + 0.3275911 * az)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    e = torch.exp2(-1.4426950408889634 * az * az) if fast else torch.exp(-az * az)
    return 0.5 * x * (1.0 + torch.copysign(1.0 - poly * e, z))


def e_act(tag, x, fast):
    """Bound on |device activation(x) - exact activation(x)| for an exact fp32 argument x (fp64 tensor), from the formulas above.

    SiLU = x / (1 + e), e = exp(-x).  A relative error d of e moves 1 + e by at most d * e / (1 + e) <= d relatively.  fp32 instances: expf is
    good to 1 ulp (d = 2 u, u = 2^-24), the add and the IEEE divide round once each: 4 u relative.  16-bit instances: the argument c * x is
    rounded (c itself to 2^-25, the product to u), which moves exp by |x| * 1.5 u relatively, v_exp_f32 and v_rcp_f32 are good to ~1 ulp (2 u
    each), the add and the final multiply round once each: (6 + 1.5 |x|) u relative.
    tanh-GELU = x / (1 + exp(-2 w)), w = k (x + 0.044715 x^3): five roundings and two rounded constants on w, all terms of one sign, so w is
    good to 6 u relatively (7.5 u with the fast form's extra constant and product) and exp(-2 w) to 2 |w| * that, weighted by
    s = e / (1 + e) <= 1 on its way into the result; the rest as for SiLU.
    erf-GELU = 0.5 x (1 + erf(z)), z = x / sqrt 2, erf by Abramowitz-Stegun 7.1.26: |error| <= 1.5e-7 absolute by its own statement, evaluated
    in fp32 as r = 1 - p(t) exp(-z^2), t = 1 / (1 + 0.3275911 z), p a quintic without constant term in Horner form.  Horner's forward bound with
    rounded coefficients is gamma_11 * sum |a_i| t^i <= 11 u * 4.4755 = 49.2 u (t <= 1; the coefficients alternate, so the intermediate
    values exceed the result).  t carries 4 u relatively (product, add, v_rcp_f32) and |t p'(t)| <= 3.44 (its value at z = 0; p = erfc(z)
    exp(z^2) gives t p' = (1.128 - 2 z p) / (0.3276 t), which falls from there): 13.8 u.  exp(-z^2): the argument to 3.5 u relatively with
    the fast form's constant, exp itself to 2 u, weighted by p exp = erfc(z): erfc(z) (3.5 z^2 + 2) u <= 2.7 u.  The product p * exp, the
    subtraction, the rounding of z carried through erf (z erf'(z) <= 0.5) and 1 + erf: one u each or less, 5 u.  Together 71 u, taken as
    72 u absolute on (1 + erf): 0.5 |x| (1.5e-7 + 72 u), and two more roundings (3 u) on the product.
    Everything plus TINY (a result below the normal range may be flushed) and plus |x| 2^-52: the fp64 reference itself forms
    0.5 x (1 + tanh) and 0.5 x (1 + erf) with that cancellation in the negative tail."""
    ax = x.abs()
    if tag == "silu":
        return F.silu(x).abs() * ((6.0 + 1.5 * ax) if fast else 4.0) * EPS32 + TINY + ax * 2.0 ** -52
    if tag == "gelu_tanh":
        w = 0.79788456080286535588 * (x + 0.044715 * x ** 3)
        s = torch.sigmoid(-2.0 * w)
        wrel = 7.5 if fast else 6.0
        return F.gelu(x, approximate="tanh").abs() * (s * (2.0 * w.abs() * wrel + 2.0) + (4.0 if fast else 2.0)) * EPS32 + TINY + ax * 2.0 ** -52
    if tag == "geglu":
        return 0.5 * ax * (1.5e-7 + 72.0 * EPS32) + 3.0 * EPS32 * F.gelu(x).abs() + TINY + ax * 2.0 ** -52
    raise ValueError(tag)


# ---- reference and bound --------------------------------------------------------------------------------------------------------
# How much room there is.  The plain emulation of tests/test_gemm_tile_cases.py (fp32 accumulation one K-tile at a time, correctly rounded
# output) reaches err / bound 0.53 - 0.96 with a 16-bit output (the rounding term is tight by nature) and <= 0.01 with an fp32 output.
# Largest err / bound on an MI355X per kernel family (tests/test_gpu_gemm_tiles.py prints it per case): not recorded yet — the module has
# not run on a device; fill in from its first run.


def reference(c, o, A=None, amb=None, detail=False):
    """(ref, bound): the fp64 result of the documented epilogue  (+bias)(+rowvec) -> act -> (*gate)(+residual)  over every output element
    [M, cout_out], and the per-element bound on |got - ref|:

        1.02 u_out |ref| + floor + 2 e,   e = the forward error of the fp32 evaluation:
        act NONE:    e = (K + 8) 2^-24 ((|A| |W|^T + |bias| + |rowvec|) |gate| + |residual|)
        SiLU / GELU: e = (LIP e_pre + e_act(x)) |gate| (+ (K + 8) 2^-24 |residual|),  e_pre = (K + 8) 2^-24 (|A| |W|^T + |bias| + |rowvec|)
        GEGLU:       e = |gelu(g)| e_pre(u) + |u| (LIP e_pre(g) + e_act(g)) (+ the residual term)

    (K + 8) 2^-24 is the forward bound of an fp32 dot product of length K in any summation order plus the handful of epilogue operations
    (a gate behind an activation is one of them: |act(x)| <= |x|, so its rounding is within 2^-24 of what e_pre already weighs);
    the factor 2 because the matrix core's internal accumulation is not documented to round every addition to nearest.  u_out / floor: the
    rounding of the stored value (U_OUT, FLOOR).  Nothing here comes from what a kernel returned.

    A, amb: a prologue's A operand [M, K] in place of a_matrix(c, o), and how far the device's copy of each of its elements may lie from
    it (tests/gemm_small_cases.py: the fused row LayerNorm).  amb |W|^T then takes the way of e_pre through the epilogue — without the
    factor 2: it is a statement about the operand, not about the accumulation — and joins the bound.  detail: a third value, the dict of
    that term per output element (`amb`) and the forward error (`e`)."""
    A, W = a_matrix(c, o) if A is None else A, o["w"].double()
    K, tag = k_total(c), c["tag"]
    pre, S = A @ W.t(), A.abs() @ W.abs().t()
    del A
    if "bias" in o:
        pre += o["bias"].double()
        S += o["bias"].double().abs()
    if "rowvec" in o and c["act"] != ACT_GEGLU:
        rv = per_row(c, o, "rowvec", "rowvec_map").double()
        pre += rv
        S += rv.abs()
    gam = (K + 8) * EPS32
    e_pre = gam * S
    a_pre = torch.zeros_like(S) if amb is None else amb @ W.abs().t()
    fast = c.get("fast_act", c["dtype"] != F32)      # the tile kernels: v_exp_f32 / v_rcp_f32 forms for 16-bit types; the cases of igemm.hip say otherwise
    if c["act"] == ACT_NONE:
        val, e, a_out = pre, e_pre, a_pre
    elif c["act"] == ACT_SILU:
        val, e, a_out = F.silu(pre), LIP * e_pre + e_act("silu", pre, fast), LIP * a_pre
    elif c["act"] == ACT_GELU_TANH:
        val, e, a_out = F.gelu(pre, approximate="tanh"), LIP * e_pre + e_act("gelu_tanh", pre, fast), LIP * a_pre
    else:
        (u, g), (eu, eg), (au, ag) = pre.chunk(2, dim=-1), e_pre.chunk(2, dim=-1), a_pre.chunk(2, dim=-1)
        gg = F.gelu(g)
        val, e, a_out = u * gg, gg.abs() * eu + u.abs() * (LIP * eg + e_act("geglu", g, fast)), gg.abs() * au + u.abs() * LIP * ag + LIP * au * ag
    if "gate" in o and c["act"] != ACT_GEGLU:
        gt = per_row(c, o, "gate", "gate_map").double()
        val, e, a_out = val * gt, e * gt.abs(), a_out * gt.abs()
    if "residual" in o:
        r = residual_rows(c, o).double()
        val, e = val + r, e + gam * r.abs()
    bound = 1.02 * U_OUT[c["out_dtype"]] * val.abs() + FLOOR[c["out_dtype"]] + 2.0 * e + a_out
    if detail:
        return val, bound, dict(amb=a_out, e=e)
    return val, bound


# ---- the checker ----------------------------------------------------------------------------------------------------------------
def new_output(c, device="cpu"):
    """The flat output buffer of a case, sentinel everywhere: M rows of out_ld elements and a guard region behind them."""
    return torch.full((rows(c) * c["out_ld"] + GUARD,), SENTINEL, dtype=TD[c["out_dtype"]], device=device)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check_output(c, buf, ref, bound):
    """buf: the flat output buffer (CPU) after the launch.  Returns (problems, worst err / bound): every element finite and inside its bound;
    the pad columns (out_ld > channels), and with them everything past row M (the guard region), still the sentinel bit for bit."""
    M, co, ld = rows(c), cout_out(c), c["out_ld"]
    problems = []
    sent = _bits(torch.full((1,), SENTINEL, dtype=buf.dtype))[0]
    body = buf[: M * ld].view(M, ld)
    if not bool((_bits(buf[M * ld:]) == sent).all()):
        problems.append(f"{int((_bits(buf[M * ld:]) != sent).sum())} elements behind row M were written")
    if ld > co and not bool((_bits(body[:, co:]) == sent).all()):
        bad = (_bits(body[:, co:]) != sent).nonzero()
        problems.append(f"{len(bad)} pad-column elements were written, first at row {int(bad[0][0])} column {co + int(bad[0][1])}")
    got = body[:, :co].double()
    if not bool(torch.isfinite(got).all()):
        problems.append(f"{int((~torch.isfinite(got)).sum())} non-finite values")
        got = torch.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
    ratio = (got - ref).abs() / bound
    worst = float(ratio.max())
    if worst > 1.0:
        bad = (ratio > 1.0).nonzero()
        where = sorted({(int(r) % 256, int(ch) % 256) for r, ch in bad[:4096].tolist()})
        i, j = (int(v) for v in bad[int(ratio[ratio > 1.0].argmax())])
        problems.append(f"{len(bad)} of {M * co} elements outside the bound, worst err / bound {worst:.3g} at row {i} channel {j} (got {float(got[i, j])!r}, "
                        f"ref {float(ref[i, j])!r}, bound {float(bound[i, j]):.3g}); rows {len({int(r) for r, _ in bad.tolist()})}, "
                        f"(row % 256, channel % 256) of the first ones: {where[:24]}")
    return problems, worst


def family(c):
    e = c["expect"]
    return "wide" if "wide8" in e else (("pipe256_" if "256x128" in e else "pipe128_") + ("slim" if c["taps"] == 1 else "tap"))
