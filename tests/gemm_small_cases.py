"""The cases of the parity tests of igemm_xreg<T,96xN> (igemm_xreg.hip: the activation-stationary GEMM of every short-K projection, with
its fused row LayerNorm) and of the register-staged igemm<T,128x128> / igemm<T,128x32> (igemm.hip: the fallback with the element-wise
epilogue, and the 32-wide tile of the thin projections), their operands, their fp64 reference, the per-element bound and the checker —
one table, two consumers: tests/test_gemm_small_cases.py (host only: routing, coverage, the checker held against planted faults) and
tests/test_gpu_gemm_small.py (the kernels themselves).  Operands, reference, bound and checker are those of tests/gemm_tile_cases.py.

A case is a dict as gemm_tile_cases describes it, plus
    form      "tap1", "c3s1" (3x3 stride 1), "c3s2" (3x3 stride 2) or "c3up" (nearest 2x upsample, then 3x3: Hin / Win are the upsampled extents)
    tag       also "silu_gate" / "gelu_tanh_gate": an activation followed by a gate
    col0      ld0 > C0: src0 is the column slice [col0, col0 + C0) of a matrix of ld0 columns (how the engine passes q / k / v views)
    out_off / bias_off   bytes by which the output / bias pointer is moved off its 16-byte alignment
    ln        None, or the input of the fused row LayerNorm (ln_eps > 0): "std" (rows of mean 0.5, spread 3), "tiny" (row variance
              about 1e-4 against ln_eps = 1e-5), "offset" (mean 100, spread 1); const_row: one input row is constant
    why       igemm<T,128x128>: the reasons the lane-resident epilogue refuses the problem (REASONS)
    fast_act  False: igemm_epilogue evaluates SiLU / GELU with expf and the IEEE divide in every type
Plain Python and CPU torch only: nothing here opens a device.

How much room there is.  The plain emulation of tests/test_gemm_small_cases.py (fp32 accumulation one K-step at a time, correctly rounded
output) reaches err / bound 0.42 - 0.97 with a bf16 output, 0.09 - 0.94 with an f16 output (the least on the three-channel cases, which
have few elements, and at K of several hundred, where the accumulation term is of the size of f16's rounding unit), <= 0.04 with fp32
throughout, and <= 0.002 with an fp32 output of a 16-bit GEMM — 0.56 where the emulation rounds a flagged LayerNorm element the other
way.  Largest err / bound on an MI355X per family (tests/test_gpu_gemm_small.py prints it per
case): RECORDED below."""
import torch

import gemm_tile_cases as G
from conv_halo_cases import MANT, MIN_EXP, ulp_toward
from gemm_tile_cases import (ACT_GEGLU, ACT_GELU_TANH, ACT_NONE, ACT_SILU, BF16, BKE, DTN, EPS32, F16, F32, FLOOR, GUARD, SENTINEL, TD, U_OUT,  # noqa: F401
                             _bits, a_matrix, check_output, cout_out, e_act, gelu_erf_device, gelu_tanh_device, k_total, new_output, per_row,
                             residual_rows, rows, silu_device)

XREG, REG128, REG32 = "igemm_xreg<%s,96xN>", "igemm<%s,128x128>", "igemm<%s,128x32>"
FORMS = ("tap1", "c3s1", "c3s2", "c3up")
TAG_ACT = dict(G.TAG_ACT, silu_gate=ACT_SILU, gelu_tanh_gate=ACT_GELU_TANH)
LN_EPS = 1e-5
# largest err / bound per family on an MI355X (first device run of tests/test_gpu_gemm_small.py; bf16 outputs set it; an fp32 output of a
# 16-bit GEMM stays below 0.003 without the LayerNorm and reaches 0.56 with it, fp32 throughout 0.043): a record, not a threshold
RECORDED = {"xreg96": 0.971, "xreg64": 0.938, "reg128": 0.968, "reg32": 0.959}


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _case(name, dt, tag, *, expect, n_img, form="tap1", HW=None, H=None, W=None, C0, C1=0, Cout, tile_n=128, use=(), out_dtype=None, res_dtype=None,
          out_pad=0, res_pad=0, rv_pad=0, gate_pad=0, ld0_pad=0, col0=0, out_off=0, bias_off=0, n_src=None, n_vec=3, n_res=3, ln=None, const_row=False, why=(),
          fast_act=None):
    """tap1: n_img samples of HW rows.  c3s1 / c3s2: the 3x3 conv of n_img images of H x W.  c3up: H x W are the UPSAMPLED extents."""
    act = TAG_ACT[tag]
    if form == "tap1":
        Hin, Win, Ho, Wo, taps, stride, ups = HW, 1, HW, 1, 1, 1, 0
    else:
        Hin, Win, taps, stride, ups = H, W, 9, 2 if form == "c3s2" else 1, 1 if form == "c3up" else 0
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        assert not ups or (H % 2 == 0 and W % 2 == 0)
    use = set(use) | ({"gate"} if tag.endswith("gate") else set()) | ({"src1"} if C1 else set())
    assert ("rowvec" in use or "rowvec_map" not in use) and ("residual" in use or "res_map" not in use) and ("gate" in use or "gate_map" not in use)
    assert not (act == ACT_GEGLU and use & {"rowvec", "gate"}) and not (ln and C1) and col0 % 8 == 0 and col0 + C0 <= C0 + ld0_pad
    co = Cout // 2 if act == ACT_GEGLU else Cout
    maps = bool(use & {"map0", "map1"})
    return dict(name=name, form=form, dtype=dt, taps=taps, stride=stride, upsample=ups, n_img=n_img, Hin=Hin, Win=Win, Hout=Ho, Wout=Wo, C0=C0,
                ld0=C0 + ld0_pad, col0=col0, C1=C1, ld1=C1, Cout=Cout, tile_n=tile_n, act=act, rowvec_ld=co + rv_pad, gate_ld=co + gate_pad,
                res_dtype=dt if res_dtype is None else res_dtype, res_ld=co + res_pad, out_dtype=dt if out_dtype is None else out_dtype,
                out_ld=co + out_pad, out_off=out_off, bias_off=bias_off, use=frozenset(use), n_src=(3 if maps else n_img) if n_src is None else n_src,
                n_vec=n_vec, n_res=n_res, ln=ln, const_row=const_row, ln_eps=LN_EPS if ln else 0.0, why=tuple(why), expect=expect % DTN[dt], env={}, tag=tag, big=False,
                fast_act=(dt != F32) if fast_act is None else fast_act)


def _xreg_cases():
    """Layout A: K <= 256, 3 pixel fragments x 8 chunks, 96 rows per workgroup, 48 per wave row.  Layout B: K <= 512, 2 x 16, 64 rows, 32
    per wave row.  Cout = 264: three N tiles (the least the dispatcher admits), the last with 8 real channels."""
    out = []
    for dt in (BF16, F16):
        x = lambda name, tag="none", **kw: out.append(_case(f"xreg_{DTN[dt]}_{name}", dt, tag, expect=XREG, **kw))
        # -- ring and slice counts, ragged M (layout A) --
        # one slice per N tile and Q = 3 = the prefetch distance: nothing is issued inside the loop; one sample of 50 rows: the second wave row holds 2 real rows
        x("a_k64_q3_one_sample_of_50", n_img=1, HW=50, C0=64, Cout=264, use={"bias"})
        # five N tiles of one slice: the prefetch spans three tiles; M = one workgroup + 1
        x("a_k64_q5_m97", n_img=1, HW=97, C0=64, Cout=520, use={"bias", "residual"})
        # the second wave row of the last workgroup lies entirely past M (rows 96..125 are real, 144..191 are not)
        x("a_k128_m126", n_img=1, HW=126, C0=128, Cout=264, use={"bias"}, out_pad=8)
        # -- the row vector of two samples per wave: samples of 48 / 49 / 50 rows --
        x("a_k128_rv48", n_img=5, HW=48, C0=128, Cout=264, use={"bias", "rowvec"})
        x("a_k192_rv49_map", n_img=5, HW=49, C0=192, Cout=264, use={"bias", "rowvec", "rowvec_map"}, out_pad=8)          # an odd slice count per tile
        x("a_k256_rv50_f32out", n_img=5, HW=50, C0=256, Cout=264, use={"rowvec"}, out_dtype=F32)                           # slices per tile = ring slots
        x("a_k256_rv50_map_res_map_c648", n_img=5, HW=50, C0=256, Cout=648, use={"bias", "rowvec", "rowvec_map", "residual", "res_map"}, res_pad=8)
        # -- two sources through different maps, n_src < n_img --
        x("a_two_64_128", n_img=5, HW=40, C0=64, C1=128, Cout=264, use={"bias", "map0", "map1"})
        x("a_two_192_64", n_img=5, HW=52, C0=192, C1=64, Cout=264, use={"bias", "map0", "map1", "residual"}, out_dtype=F32)
        x("a_ld0_slice", n_img=2, HW=70, C0=128, Cout=264, use={"bias"}, ld0_pad=256, col0=128)
        # -- layout B: 5 slices per tile (more than the ring), 7, 8; ragged: 2 real rows in the second wave row, a workgroup + 1, a wave row past M --
        x("b_k320_one_sample_of_34", n_img=1, HW=34, C0=320, Cout=264, use={"bias"})
        x("b_k448_m65", n_img=1, HW=65, C0=448, Cout=264, use={"bias", "residual"})
        x("b_k512_m84_f32out", n_img=1, HW=84, C0=512, Cout=264, use={"bias"}, out_dtype=F32, out_pad=8)
        x("b_k320_rv48", n_img=5, HW=48, C0=320, Cout=264, use={"bias", "rowvec"})
        x("b_k512_rv49_map", n_img=5, HW=49, C0=512, Cout=264, use={"bias", "rowvec", "rowvec_map"})
        x("b_k448_rv50", n_img=5, HW=50, C0=448, Cout=264, use={"rowvec"}, out_pad=8)
        x("b_k320_rv50_map_res_map_c648", n_img=5, HW=50, C0=320, Cout=648, use={"bias", "rowvec", "rowvec_map", "residual", "res_map"}, res_pad=8, out_pad=8)
        x("b_two_256_64", n_img=5, HW=40, C0=256, C1=64, Cout=264, use={"bias", "map0", "map1"})
        x("b_ld0_slice", n_img=2, HW=45, C0=320, Cout=264, use={"bias"}, ld0_pad=64, col0=64)
        # -- GEGLU: hidden width 144 (the last tile holds 16 output channels); with bias (fetched before the K loop) and without --
        x("a_geglu_k64_h144_bias", "geglu", n_img=1, HW=50, C0=64, Cout=288, use={"bias"})
        x("a_geglu_k256_nobias_res", "geglu", n_img=3, HW=65, C0=256, Cout=288, use={"residual", "res_map"}, res_pad=8, out_pad=8)
        x("b_geglu_k512_h144_bias", "geglu", n_img=1, HW=65, C0=512, Cout=288, use={"bias"}, out_dtype=F32)
        x("b_geglu_k320_nobias", "geglu", n_img=2, HW=42, C0=320, Cout=384, use=set())
        # -- the fused row LayerNorm: every instance, a residual, ragged M, tiny variance per layout, a constant row, a large common offset --
        x("a_ln_k256", n_img=2, HW=70, C0=256, Cout=264, use={"bias"}, ln="std", out_dtype=F32)
        x("a_ln_k192_res_const_row", n_img=2, HW=50, C0=192, Cout=264, use={"bias", "residual"}, ln="std", const_row=True)
        x("a_ln_k128_tiny_var", n_img=1, HW=97, C0=128, Cout=264, use={"bias"}, ln="tiny")
        x("a_ln_k256_offset", n_img=2, HW=48, C0=256, Cout=264, use={"bias", "map0"}, ln="offset", out_dtype=F32)
        x("a_ln_geglu_k256", "geglu", n_img=2, HW=50, C0=256, Cout=288, use={"bias"}, ln="std")
        x("b_ln_k512", n_img=2, HW=45, C0=512, Cout=264, use={"bias"}, ln="std", out_dtype=F32)
        x("b_ln_k320_ragged_34", n_img=1, HW=34, C0=320, Cout=264, use={"bias"}, ln="std", out_dtype=F32)
        x("b_ln_k448_tiny_var", n_img=1, HW=65, C0=448, Cout=264, use={"bias"}, ln="tiny", out_dtype=F32)
        x("b_ln_k512_offset_const_row", n_img=2, HW=40, C0=512, Cout=264, use={"bias", "residual", "res_map"}, ln="offset", const_row=True)
        x("b_ln_geglu_k512", "geglu", n_img=1, HW=65, C0=512, Cout=288, use={"bias"}, ln="std", out_dtype=F32)
        x("b_ln_geglu_k320_tiny_var", "geglu", n_img=1, HW=40, C0=320, Cout=288, use={"bias"}, ln="tiny")
        x("a_ln_geglu_k128_tiny_var", "geglu", n_img=1, HW=50, C0=128, Cout=288, use=set(), ln="tiny", out_dtype=F32)
    return out


# why the lane-resident epilogue (igemm.hip `lane_epi_ok`) refuses a problem: reason -> (the compute types it can occur in, the case's fields)
REASONS = {
    "cout_100": ((F32, BF16, F16), dict(Cout=100, use={"bias", "residual", "res_map"})),                       # whole quads, 100 % 8 != 0
    "cout_99_partial_quad": ((F32, BF16, F16), dict(Cout=99, out_pad=1, use={"bias", "rowvec"})),              # out_ld = 100: vector stores and one partial quad
    "out_ld_99": ((F32, BF16, F16), dict(Cout=99, use={"bias", "residual"})),                                  # (out_ld & 3) != 0: scalar stores everywhere
    "out_ld_102": ((F32, BF16, F16), dict(Cout=96, out_pad=6, tag="gelu_tanh", use={"bias", "rowvec", "rowvec_map"})),
    "out_ptr_plus_8": ((F32, BF16, F16), dict(Cout=104, out_off=8, tag="gate", use={"bias", "gate_map"})),
    "bias_ptr_plus_4": ((F32, BF16, F16), dict(Cout=104, bias_off=4, tag="silu", use={"bias"})),
    "rowvec_ld_mod_4": ((F32, BF16, F16), dict(Cout=104, rv_pad=2, use={"bias", "rowvec", "rowvec_map"}, out_pad=8)),
    "res_f32_on_16bit": ((BF16, F16), dict(Cout=104, res_dtype=F32, use={"bias", "residual", "res_map"}, res_pad=8)),
    "res_bf16_on_f32": ((F32,), dict(Cout=104, res_dtype=BF16, use={"bias", "residual", "res_map"}, res_pad=8)),
    "res_f16_on_bf16": ((BF16,), dict(Cout=104, res_dtype=F16, use={"residual"})),
    "out_bf16_of_f32": ((F32,), dict(Cout=104, out_dtype=BF16, use={"bias"})),
    "out_f16_of_f32": ((F32,), dict(Cout=104, out_dtype=F16, use={"bias", "residual"}, tag="gelu_tanh")),
    "out_f16_of_bf16": ((BF16,), dict(Cout=104, out_dtype=F16, use={"bias", "rowvec"})),
    "out_bf16_of_f16": ((F16,), dict(Cout=104, out_dtype=BF16, use={"bias"}, out_pad=8)),
    "silu_gate": ((F32, BF16, F16), dict(Cout=104, tag="silu_gate", use={"bias", "gate_map"})),
    "gelu_tanh_gate": ((F32, BF16, F16), dict(Cout=104, tag="gelu_tanh_gate", use={"bias", "rowvec", "residual"})),
    "geglu_out_ld_84": ((F32, BF16, F16), dict(Cout=160, tag="geglu", out_pad=4, use={"bias"})),              # the second N tile is part empty
}


def _shape(form, dt, variant):
    """Extents and K of a register-staged case.  Images of 5x7 and 6x10: pixel rows wrap inside a 128-row tile and the padding meets every
    border; M = 105 or 300 (3x3 stride 2: 108).  variant 0: one source of one K-tile per tap (tap1: ONE K-step, the main loop's `more`
    is false at once; 3x3: 9); 1: tap1 two K-steps, 3x3 two sources with the seam after one (odd) K-step, 27 in all; 2: two sources
    through different maps, seam after 3 / 1 K-steps."""
    g = BKE[dt]
    kw = {"tap1": dict(n_img=3, HW=35), "c3s1": dict(n_img=3, H=5, W=7), "c3s2": dict(n_img=9, H=5, W=7), "c3up": dict(n_img=5, H=6, W=10)}[form]
    if variant % 3 == 0:
        kw.update(C0=g)
    elif variant % 3 == 1:
        kw.update(C0=2 * g) if form == "tap1" else kw.update(C0=g, C1=2 * g)
    else:
        kw.update(C0=3 * g if form == "tap1" else g, C1=g, maps=True)
    if form == "c3s1" and variant % 2:
        kw.update(n_img=5, H=6, W=10)
    return kw


def _reg128_cases():
    """One case per (reason, dtype); the forms and K variants rotate through them, so that every form meets every dtype."""
    out = []
    for d, dt in enumerate((F32, BF16, F16)):
        i = 0
        for why, (dts, fields) in REASONS.items():
            if dt not in dts:
                continue
            form = FORMS[(i + d) % 4]
            kw = dict(_shape(form, dt, i // 4 + d), **fields)
            tag = kw.pop("tag", "none")
            use = set(kw.pop("use"))
            if kw.pop("maps", False):
                use |= {"map0", "map1"}
            out.append(_case(f"reg128_{DTN[dt]}_{form}_{why}", dt, tag, form=form, expect=REG128, use=use, why=(why,), fast_act=False, **kw))
            i += 1
    # 11 M tiles: the XCD tile map with a non-zero remainder (33 blocks), in both tile orders: M fastest through a 3x3 conv whose padded
    # weights exceed 2 MiB, N fastest through a 1-tap GEMM
    r = lambda name, dt, tag="none", **kw: out.append(_case(f"reg128_{DTN[dt]}_{name}", dt, tag, expect=REG128, fast_act=False, **kw))
    r("c3s1_11_tiles_m_fast", BF16, form="c3s1", n_img=22, H=6, W=10, C0=320, Cout=260, use={"bias", "residual"}, why=("cout_260",))
    r("tap1_11_tiles_n_fast", F16, n_img=38, HW=35, C0=128, Cout=260, use={"bias", "rowvec"}, why=("cout_260",))
    r("tap1_11_tiles_n_fast", F32, n_img=38, HW=35, C0=64, Cout=260, use={"bias"}, why=("cout_260",), out_pad=4)
    return out


def _reg32_cases():
    out = []
    for dt in (F32, BF16, F16):
        g = BKE[dt]
        r = lambda name, tag="none", **kw: out.append(_case(f"reg32_{DTN[dt]}_{name}", dt, tag, expect=REG32, tile_n=32, fast_act=False, **kw))
        # the DiT final projection as the engine states it: Cout = p * p * oc = 32, bias, fp32 output, samples of 50 rows
        for K in ((192, 384) if dt == F32 else (384, 768, 1152)):
            r(f"tap1_dit_final_k{K}", n_img=4, HW=50, C0=K, Cout=32, use={"bias"}, out_dtype=F32)
        # the UNet's conv_out on 8x8 images: two sources, Cout = 4, fp32 output
        r("c3s1_conv_out_8x8", form="c3s1", n_img=3, H=8, W=8, C0=g, C1=g, Cout=4, use={"bias", "map0", "map1"}, out_dtype=F32)
        r("c3s1_cout3_out_ld5", form="c3s1", n_img=3, H=5, W=7, C0=g, Cout=3, use={"bias"}, out_pad=2)
        r("c3s2_cout3_silu", "silu", form="c3s2", n_img=9, H=5, W=7, C0=g, C1=2 * g, Cout=3, use={"bias"})
        # two N tiles, the second with 8 real channels; residual and row vector through sample maps
        r("c3up_cout40_res_maps", form="c3up", n_img=5, H=6, W=10, C0=g, Cout=40, use={"bias", "rowvec", "rowvec_map", "residual", "res_map"}, out_pad=8, res_pad=8)
        r("tap1_cout40_11_tiles", n_img=38, HW=35, C0=2 * g, Cout=40, use={"bias", "residual"})          # 22 blocks, N fastest
        r("tap1_one_kstep_gate", "gate", n_img=3, HW=35, C0=g, Cout=32, use={"bias", "gate_map"})
    return out


CASES = _xreg_cases() + _reg128_cases() + _reg32_cases()


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def family(c):
    e = c["expect"]
    return ("xreg96" if k_total(c) <= 256 else "xreg64") if "xreg" in e else ("reg128" if "128x128" in e else "reg32")


def wave_rows(c):
    """Pixel rows of a wave of igemm_xreg: 48 (K <= 256) or 32."""
    return 48 if k_total(c) <= 256 else 32


def esize(dt):
    return 4 if dt == F32 else 2


PTR_FIELDS = G.PTR_FIELDS


def pointers(c, base):
    """The pointer fields as dc_igemm receives them: base {field: address of the allocation}; src0 moves to its column slice, out and bias
    off their alignment."""
    p = dict(base)
    p["src0"] = base["src0"] + c["col0"] * esize(c["dtype"])
    p["out"] = base["out"] + c["out_off"]
    if "bias" in p:
        p["bias"] = base["bias"] + c["bias_off"]
    return p


def igemm_fields(c, base):
    kw = G.igemm_fields(c, pointers(c, base))
    if c["ln_eps"]:
        kw["ln_eps"] = c["ln_eps"]
    return kw


# ---- operands -----------------------------------------------------------------------------------------------------------------------
def make_operands(c):
    """gemm_tile_cases.make_operands with a seed of the case's own, and the input rows a LayerNorm case is there for."""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"])) % 100003
    o = G.make_operands(c, seed=seed)
    if c["ln"]:
        q = lambda t: t.to(TD[c["dtype"]]).float()
        x = o["x0"]
        o["x0"] = q({"std": 3.0 * x + 0.5, "tiny": 0.01 * x, "offset": 100.0 + x}[c["ln"]])
        if c["const_row"]:
            o["x0"][0, 1, 0, :] = 1.5          # variance 0: the normalised row is exactly 0
    return o


def const_rows(c, o):
    """Output rows whose LayerNorm input is the constant row."""
    if not c["const_row"]:
        return []
    src = o["map0"].long() if "map0" in o else torch.arange(c["n_img"])
    return [int(n) * c["Hout"] * c["Wout"] + 1 for n in (src == 0).nonzero().flatten()]


# ---- the fused row LayerNorm ----------------------------------------------------------------------------------------------------------
def _spacing(m, dt):
    """Spacing of the type's values at magnitude m (fp64 tensor)."""
    ex = torch.floor(torch.log2(m.clamp_min(2.0 ** -140))) - (MANT[dt] - 1)
    return torch.exp2(ex.clamp_min(MIN_EXP[dt]))


def ln_prologue(c, o):
    """(a, amb, flagged), each [M, K]: the A operand as the MFMA receives it — the fp64 LayerNorm (no affine, eps = ln_eps as fp32 holds
    it) of the rounded input row, rounded once to the compute type — and how far the device's copy of an element may lie from it.

    The device (igemm_xreg.hip) holds a row's K values in four lanes — lane lq has elements 8 lq .. 8 lq + 7 of every 32-element chunk —
    and works in fp32 (u = 2^-24):
      sum    each lane adds its K / 4 values one after the other, then (lane 0 + lane 1) + (lane 2 + lane 3) by two xor-shuffles.  Every
             addition rounds its own result: |error| <= u * (the sum of |partial sum| over the K + 3 - 4 additions that round; a lane's
             first addition, to 0, does not), the running error bound of this very order, taken from the fp64 partial sums (`_running`).
             The values of a row are multiples of its smallest element's spacing g in the compute type; where sum |x| <= 2^24 g every
             partial sum in any order is a multiple of g below 2^24 g, hence exact: error 0 (a row around 100).
      mean   sum * (1 / K): the rounded constant and the product, c u |mean| with c = 2 — c = 0 where K is a power of two: the constant
             and the product are then exact.  d_mean := error(sum) / K + c u |mean|.
      var    sum (x - mean')^2 = sum (x - mean)^2 + K d_mean^2 exactly (the cross term vanishes); each term carries the rounding of the
             difference twice and of the square (3 u), the additions their running bound again, * (1 / K) c u, + eps u:
             relative error of v = var + eps:  rel_v <= ((3 u sum t + running(t)) / K + c u var + d_mean^2) / v + u,  t = (x - mean)^2.
      rstd   rsqrtf(v): rel_v / 2, and the instruction itself ~1 ulp, taken as 2 u (the rule e_act uses for v_rcp_f32 / v_exp_f32).
      y      (x - mean') * rstd': the difference is off by d_mean + u |x - mean|, the product rounds once:
             e = 1.01 ((d_mean + u |x - mean|) rstd + |y| (rel_v / 2 + 3 u))      (1.01: the second-order terms)
    The result is rounded ONCE to the compute type (f_to_chunk).  The device rounds the other way only where the fp64 value lies within
    e of a rounding tie: those elements are flagged, and amb = the spacing of the type there (the device's value is the neighbour).
    Where e is not small against the spacing (4 e > spacing: values next to 0, the constant row) the device's value may lie further:
    amb = e + the spacing at |y| + e."""
    dt, K = c["dtype"], c["C0"]
    x = a_matrix(c, o)                                           # [M, K] fp64, exact in the compute type
    u = EPS32
    cK = 0.0 if K & (K - 1) == 0 else 2.0
    eps = float(torch.tensor(c["ln_eps"], dtype=torch.float32))

    def _running(t):
        """[M, 1]: the sum of |partial sum| over the additions of the kernel's order that round (t [M, K] fp64)."""
        part = t.view(-1, K // 32, 4, 8).permute(0, 2, 1, 3).reshape(-1, 4, K // 4).cumsum(2)
        lane = part[:, :, -1]
        s01, s23 = lane[:, 0] + lane[:, 1], lane[:, 2] + lane[:, 3]
        return (part[:, :, 1:].abs().sum((1, 2)) + s01.abs() + s23.abs() + (s01 + s23).abs())[:, None]
    sabs = x.abs().sum(1, keepdim=True)
    grid = torch.where(x == 0, torch.full_like(x, float("inf")), _spacing(x.abs(), dt)).amin(1, keepdim=True)
    e_sum = torch.where(sabs <= 2.0 ** 24 * grid, torch.zeros_like(sabs), u * _running(x))
    mean = x.mean(1, keepdim=True)
    d = x - mean
    t = d * d
    var = t.mean(1, keepdim=True)
    v = var + eps
    rstd = v.rsqrt()
    y = d * rstd
    d_mean = e_sum / K + cK * u * mean.abs()
    rel_v = ((3.0 * u * t.sum(1, keepdim=True) + u * _running(t)) / K + cK * u * var + d_mean ** 2) / v + u
    e = 1.01 * ((d_mean + u * d.abs()) * rstd + y.abs() * (0.5 * rel_v + 3.0 * u))
    r = y.to(TD[dt]).double()
    sp = ulp_toward(r, y, dt)
    flagged = (0.5 * sp - (y - r).abs()) <= e
    amb = torch.where(4.0 * e <= sp, sp, e + _spacing(y.abs() + e, dt)) * flagged
    return r, amb, flagged


def ln_device(c, x, eps=None, mean_shift=0, rounded=True):
    """The same in fp32 as the kernel does it (x [M, K] fp32, exact in the compute type): lane lq of a row holds elements 8 lq .. 8 lq + 7
    of every 32-element chunk and adds them in that order; (lanes 0 + 1) + (lanes 2 + 3); two passes; rounded to the compute type.
    eps / mean_shift / rounded: the planted faults of tests/test_gemm_small_cases.py."""
    M, K = x.shape
    eps = torch.tensor(c["ln_eps"] if eps is None else eps, dtype=torch.float32)
    inv_k = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(K), dtype=torch.float32)
    lanes = x.view(M, K // 32, 4, 8).permute(0, 2, 1, 3).reshape(M, 4, K // 4)

    def lane_sum(t):
        s = torch.zeros(M, 4)
        for i in range(t.shape[2]):
            s = s + t[:, :, i]
        return ((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3]))[:, None]
    mean = lane_sum(lanes) * inv_k
    if mean_shift:
        mean = mean.roll(-mean_shift, 0)
    dl = lanes - mean[:, :, None]
    var = lane_sum(dl * dl)
    rstd = torch.rsqrt(var * inv_k + eps)
    y = (x - mean) * rstd
    return y.to(TD[c["dtype"]]).float() if rounded else y


# ---- reference --------------------------------------------------------------------------------------------------------------------
def reference(c, o, detail=False):
    """gemm_tile_cases.reference; a LayerNorm case's A operand and ambiguity come from ln_prologue.  detail: also a dict with the
    ambiguity term per output element (`amb`), the bound's forward error (`e`) and the share of flagged operand elements."""
    if not c["ln"]:
        return G.reference(c, o, detail=detail)
    a, amb, flagged = ln_prologue(c, o)
    val, bound, d = G.reference(c, o, A=a, amb=amb, detail=True)
    d["flagged_share"] = float(flagged.double().mean())
    return (val, bound, d) if detail else (val, bound)
