"""The cases of the strip-family parity tests: the two attention bodies of csrc/attn_strip.h (attn_strip_run, the matrix-core kernel that
gives one wave 32 queries, and attn_exact_run, the FMA chain) behind their four entry points — dc_cross_attention and
dc_cross_attention_len (attention_cross.hip), dc_attention_bias (t5.hip) and dc_attention_causal (clip.hip) —, their operands, their fp64
reference, the per-element error bound and the checker.  One table, two consumers: tests/test_strip_attention_cases.py (host only: routing,
coverage, the checker held against an emulation of each body and against planted faults) and tests/test_gpu_strip_attention.py (the kernels).

A case is a dict of
    name      its id
    entry     "cross", "cross_len", "bias" or "causal"
    dtype, n, heads, d, scale, ld_out and Lq, S, ld_q, ld_kv, nq, nc (cross entries) or L, ld_qkv (bias, causal): the plain parameter
              fields; rows = Lq or L and keys = S or L name the same numbers for code that serves all four
    expect    the exact *_variant string: "mfma" (attn_strip_run) or "fp32" (attn_exact_run)
    instance  the template instance: ("cross", "mfma", "bf16", 64, True) = attn_cross_kernel<bf16, 64, LEN = true>; ("cross", "fp32", "f16",
              24, False) = attn_cross_f32_kernel<f16, SW = 24, false>; ("bias", "mfma", "f16") = attn_bias_kernel<f16, 64>; ("causal",
              "fp32", "f32") = attn_causal_f32_kernel<f32>
    layout    "hard"       q rows wider than the heads (cross: ld_q = C + 32; bias / causal: one fused tensor), K and V stacked in one
                           tensor with a gap of 8 columns between them and 16 behind, ld_out = C + 8 (the pad columns keep the sentinel)
              "plain"      nothing padded; cross: K and V in two tensors of their own
              "ld_odd"     "hard" with the K / V row stride two elements longer (ld_kv % 8 != 0: no 16-byte loads)
              "q_off"      "hard" with the q tensor (bias / causal: the fused tensor) starting 2 bytes behind a 16-byte boundary
              "odd_out"    "hard" with ld_out = C + 2 (ld_out % 4 != 0: no 8-byte stores)
              In 16 bit the last three are the doors to the exact kernel at a head width the matrix-core kernel serves.  Every element of an
              input tensor that is not a value the kernel may read is NaN: the gaps, K / V rows of a context nobody maps to, rows at or past
              a length, and a guard behind the last row.
    mode      "random" N(0,1); "peaked" q and k times 5 (logits beyond 60; bias: a table of several units that moves the arg max);
              "negative" every score, bias included, <= -6 (a zero-score padded key that is not masked then takes over the softmax)
    lens      the device array of lengths as the caller states it (kv_len per context, kv_len / row_len per sample), None for NULL;
              values outside [1, keys] are there on purpose: the kernels clamp them
    maps      "identity", "many_q" (q_map many-to-one), "kv_repeat" (kv_map with repeats and contexts nobody maps to, one of them directly
              behind a referenced one), "both"; q_map / kv_map hold the lists (None: a NULL pointer)
    why       one line
Plain Python and CPU torch only: nothing here opens a device.

Largest err / bound on an MI355X per entry, route and dtype (tests/test_gpu_strip_attention.py prints it per case), bf16 / f16 on the
"mfma" route and f32 / bf16 / f16 on the "fp32" one (a correctly rounded 16-bit result of the exact route alone uses up to 1 / 1.02):
    cross      mfma 0.39 / 0.31    fp32 0.0060 / 0.89 / 0.65
    cross_len  mfma 0.40 / 0.29    fp32 0.0031 / 0.90 / 0.63
    bias       mfma 0.42 / 0.33    fp32 0.013 / 0.95 / 0.88
    causal     mfma 0.49 / 0.47    fp32 0.014 / 0.95 / 0.90"""

import torch

from attention_cases import BF16, DTN, EPS32, F16, F32, FLOOR, GUARD, SENTINEL, TD, U, U_OUT, _bits

T16 = (BF16, F16)
CROSS = ("cross", "cross_len")
SEQ_KB = 32                                                # keys per block of attn_bias_kernel and attn_causal_kernel
LOG2E = 1.4426950408889634


# ---- what the host code and the kernels derive from a shape ---------------------------------------------------------------------
def cross_kb(d):
    """Keys per block of attn_cross_kernel<T, d>."""
    return 64 if d <= 32 else 32


def is_cross(c):
    return c["entry"] in CROSS


def key_block(c):
    """Keys per step of the route's softmax: KB of the strip kernel, the LDS block of the exact one (from S or L, never from a length)."""
    if c["expect"] == "mfma":
        return cross_kb(c["d"]) if is_cross(c) else SEQ_KB
    return min(c["keys"], 4096 // c["d"])


def exact_sw(c):
    return {96: 24, 160: 20}.get(c["d"], 16) if is_cross(c) else 16


def exact_qt(c):
    """Queries per workgroup of the exact kernels."""
    return 256 // (c["d"] // exact_sw(c))


def q_map(c):
    return c["q_map"] if c.get("q_map") is not None else list(range(c["n"]))


def kv_map(c):
    return c["kv_map"] if c.get("kv_map") is not None else list(range(c["n"]))


def n_lens(c):
    """Entries of the length array: contexts (cross_len) or samples (bias, causal)."""
    return c["nc"] if is_cross(c) else c["n"]


def eff_lens(c, lens="own"):
    """What the kernels make of the lengths: clamped into [1, keys]; NULL (and dc_cross_attention): keys everywhere."""
    lens = c["lens"] if isinstance(lens, str) else lens
    if lens is None:
        return [c["keys"]] * n_lens(c)
    return [min(max(x, 1), c["keys"]) for x in lens]


def sample_len(c, i, eff=None):
    """Keys output sample i attends (its live rows too, for bias and causal)."""
    eff = eff_lens(c) if eff is None else eff
    return eff[kv_map(c)[i]] if is_cross(c) else eff[i]


def live_rows(c, i):
    return c["rows"] if is_cross(c) else sample_len(c, i)


def waves(c):
    """The waves of the strip route, one dict per (sample, 32-query tile) — the heads of a sample share everything here: q0, len, nqt (16-query
    tiles that hold a query; <= 0: the wave stores zeros and leaves), nblk / nplain as cross_view, attn_bias_kernel and attn_causal_kernel
    set them, padded (zero-staged keys the wave holds = nblk KB - len, 0 where that is negative) and live (queries of the wave)."""
    assert c["expect"] == "mfma"
    KB, out = key_block(c), []
    for i in range(c["n"]):
        ln, nq = sample_len(c, i), live_rows(c, i)
        for q0 in range(0, c["rows"], 32):
            nqt = min(2, (nq - q0 + 15) >> 4)
            if c["entry"] == "causal":
                nplain = q0 // KB
                nblk = nplain + 1
            else:
                nblk, nplain = (ln + KB - 1) // KB, ln // KB
            out.append(dict(i=i, q0=q0, len=ln, nqt=nqt, nblk=nblk, nplain=nplain, padded=max(0, nblk * KB - ln), live=max(0, min(32, nq - q0))))
    return out


def items(c):
    """Waves of the strip route's launch, four per workgroup."""
    return c["n"] * c["heads"] * ((c["rows"] + 31) // 32)


def dead_waves(c):
    """Waves of the last workgroup past the last item."""
    return (-items(c)) % 4


def padded_keys(c):
    """The most zero-staged keys a live wave of the case holds (0 on the exact route: it stages the live keys only)."""
    if c["expect"] != "mfma":
        return 0
    return max([w["padded"] for w in waves(c) if w["nqt"] > 0], default=0)


# ---- layouts --------------------------------------------------------------------------------------------------------------------
def geometry(entry, layout, C):
    """Row strides and the element offsets of q, k, v inside their buffers: dict(ld_q, ld_kv, ld_out, bufs, q, k, v) with q / k / v =
    (buffer index, element offset)."""
    hard = layout != "plain"
    off = 1 if layout == "q_off" else 0
    ld_out = {"plain": C, "odd_out": C + 2}.get(layout, C + 8)
    odd = 2 if layout == "ld_odd" else 0
    if entry in CROSS:
        if not hard:
            return dict(ld_q=C, ld_kv=C, ld_out=ld_out, bufs=3, q=(0, 0), k=(1, 0), v=(2, 0))
        return dict(ld_q=C + 32, ld_kv=2 * C + 24 + odd, ld_out=ld_out, bufs=2, q=(0, off), k=(1, 0), v=(1, C + 8))
    if not hard:
        return dict(ld_q=3 * C, ld_kv=3 * C, ld_out=ld_out, bufs=1, q=(0, 0), k=(0, C), v=(0, 2 * C))
    return dict(ld_q=3 * C + 32 + odd, ld_kv=3 * C + 32 + odd, ld_out=ld_out, bufs=1, q=(0, off), k=(0, off + C + 8), v=(0, off + 2 * C + 16))


def case_geometry(c):
    return geometry(c["entry"], c["layout"], c["heads"] * c["d"])


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _maps(kind, n):
    """(q_map, kv_map, nq, nc) of a named pair of maps for n output samples."""
    qm, km, nq, nc = None, None, n, n
    if kind in ("many_q", "both"):
        nq = max(1, (n + 1) // 2)
        qm = [(i // 2) % nq for i in range(n)]
    if kind in ("kv_repeat", "both"):
        nc = 4
        km = [(2, 0, 2, 0, 3)[i % 5] for i in range(n)]       # context 1: nobody maps to it, directly behind context 0
    return qm, km, nq, nc


def _case(entry, route, dt, d, rows, keys=None, n=2, heads=2, layout="hard", mode="random", lens=None, maps="identity", explicit=None, why=""):
    C = heads * d
    keys = rows if keys is None else keys
    g = geometry(entry, layout, C)
    scale = float(torch.tensor(d ** -0.5, dtype=torch.float32))
    c = dict(entry=entry, dtype=dt, n=n, heads=heads, d=d, rows=rows, keys=keys, scale=scale, ld_out=g["ld_out"], expect=route, layout=layout, mode=mode,
             lens=None if lens is None else list(lens), maps=maps, why=why)
    if entry in CROSS:
        qm, km, nq, nc = explicit or _maps(maps, n)
        c.update(Lq=rows, S=keys, ld_q=g["ld_q"], ld_kv=g["ld_kv"], q_map=qm, kv_map=km, nq=nq, nc=nc)
        sw = {96: 24, 160: 20}.get(d, 16)
        c["instance"] = ("cross", route, DTN[dt], d if route == "mfma" else sw, entry == "cross_len")
        assert (entry == "cross_len") == (lens is not None) and (lens is None or len(lens) == nc)
    else:
        c.update(L=rows, ld_qkv=g["ld_q"])
        c["instance"] = (entry, route, DTN[dt])
        assert keys == rows and maps == "identity" and (lens is None or len(lens) == n)
    tag = "" if lens is None else "_len" + ".".join(str(x) for x in lens)
    c["name"] = f"{entry}_{route}_{DTN[dt]}_d{d}_r{rows}_k{keys}_n{n}h{heads}_{layout}_{maps}_{mode}{tag}"
    return c


def _cross_strip_cases():
    """Every (T, D) of attn_cross_kernel, LEN = false and true.  dc_cross_attention: S in {1, KB - 1, KB, KB + 1, 2 KB, 2 KB + 1, 3 KB - 1}
    (only the ragged block; no ragged block; one key in it; odd and even block counts) paired with Lq in {1, 16, 17, 32, 33, 70} (one live
    lane; a tile exactly full; one live query in the second tile; a full wave; a second wave with one query; a third with six) and with item
    counts 6, 5, 3, 4, 10, 9, 12.  dc_cross_attention_len: the same seven values as the lengths of seven referenced contexts of one launch
    (mixed inside a workgroup; 1 and S among them) around a context nobody maps to, and the out-of-range lengths 0, -3 and S + 5."""
    out = []
    for dt in T16:
        for d in (32, 64, 96, 128, 160):
            KB = cross_kb(d)
            Ss = (1, KB - 1, KB, KB + 1, 2 * KB, 2 * KB + 1, 3 * KB - 1)
            Lqs = (1, 16, 17, 32, 33, 70, 33)
            shapes = ((2, 3), (1, 5), (3, 1), (2, 2), (5, 1), (1, 3), (3, 2))
            lays = ("hard", "plain", "hard", "plain", "hard", "hard", "plain")
            maps = ("identity", "identity", "many_q", "kv_repeat", "both", "identity", "kv_repeat")
            for S, Lq, (n, h), lay, mp in zip(Ss, Lqs, shapes, lays, maps):
                out.append(_case("cross", "mfma", dt, d, Lq, S, n, h, lay, maps=mp,
                                 why=f"KB = {KB}: {S // KB} full blocks and {S % KB} keys; {n * h * ((Lq + 31) // 32)} waves"))
            out.append(_case("cross", "mfma", dt, d, 33, 2 * KB + 1, 2, 2, "hard", "peaked", why="row maxima beyond 60, the running max moves between blocks"))
            out.append(_case("cross", "mfma", dt, d, 17, KB + 1, 3, 1, "hard", "negative", maps="kv_repeat", why=f"{KB - 1} zero-staged keys beside one live one in the ragged block"))
            out.append(_case("cross", "mfma", dt, d, 33, 3 * KB - 1, 2, 3, "plain", "negative", why="one zero-staged key in the ragged block against scores <= -6"))
            S = 3 * KB - 1
            lens = [1, KB - 1, KB, KB + 1, 5, 2 * KB, 2 * KB + 1, S]
            out.append(_case("cross_len", "mfma", dt, d, 33, S, 7, 2, "hard", lens=lens, maps="both", explicit=([0, 1, 2, 0, 1, 2, 0], [0, 1, 2, 3, 5, 6, 7], 3, 8),
                             why="seven lengths in one launch, mixed inside a workgroup; context 4 is nobody's, behind a ragged one"))
            out.append(_case("cross_len", "mfma", dt, d, 17, KB + 1, 3, 3, "plain", lens=[0, -3, KB + 6], why="out-of-range lengths behave as 1, 1 and S; 9 waves"))
            out.append(_case("cross_len", "mfma", dt, d, 33, 2 * KB + 1, 2, 2, "hard", "peaked", lens=[2 * KB + 1, KB + 1], why="row maxima beyond 60"))
            out.append(_case("cross_len", "mfma", dt, d, 16, S, 3, 2, "hard", "negative", lens=[KB + 1, 2 * KB - 1, S - 1],
                             why=f"{KB - 1}, 1 and {KB} zero-staged keys against scores <= -6"))
    # the flat bound's blind spot: bf16, d = 64, Lq = 64, 2 x 2 pairs, S = 77 (one zero-staged key left unmasked moves the result by 6e-3)
    for mode in ("random", "negative"):
        out.append(_case("cross", "mfma", BF16, 64, 64, 77, 2, 2, "hard", mode, why="S = 77: the twin pair of the off-by-one test"))
    return out


def _cross_exact_cases():
    """attn_cross_f32_kernel.  f32 at every SW (d = 16 / 32 / 64 / 128: 16; 96: 24; 160: 20) with S in {B, B + 1, 2 B + 3} for the LDS block
    B = 4096 // d and Lq = QT + 1 (a second workgroup with one live query); 16-bit through each door (d = 16, ld_kv % 8 != 0, q 2 bytes off a
    16-byte boundary, ld_out % 4 != 0); lengths on every SW in every type, with B still taken from S."""
    out = []
    qt = lambda d: 256 // (d // {96: 24, 160: 20}.get(d, 16))
    for d in (16, 64, 96, 160):
        B = 4096 // d
        for S, Lq, (n, h), lay in zip((B, B + 1, 2 * B + 3), (5, 17, qt(d) + 1), ((2, 2), (2, 3), (1, 2)), ("plain", "odd_out", "hard")):
            out.append(_case("cross", "fp32", F32, d, Lq, S, n, h, lay, maps="kv_repeat" if S == B + 1 else "identity",
                             why=f"B = {B}: {S // B} full LDS blocks and {S % B} keys, QT = {qt(d)}"))
    for d in (32, 128):
        out.append(_case("cross", "fp32", F32, d, qt(d) + 1, 4096 // d + 1, 2, 2, "hard", maps="many_q", why=f"QT = {qt(d)}: a second query tile with one live query"))
    for d in (64, 96, 160):
        B = 4096 // d
        S = 2 * B + 3
        out.append(_case("cross_len", "fp32", F32, d, qt(d) + 1, S, 6, 2, "hard", lens=[1, B, B + 1, S, 0, S + 5], maps="both",
                         explicit=([0, 1, 2, 0, 1, 2], [1, 0, 2, 3, 5, 4], 3, 6), why=f"lengths around the LDS block B = {B} (from S), clamped ones"))
        out.append(_case("cross", "fp32", F32, d, 17, S, 2, 2, "plain", "peaked", why="row maxima beyond 60 across LDS blocks"))
        out.append(_case("cross_len", "fp32", F32, d, 17, S, 2, 2, "plain", "peaked", lens=[B + 1, S], why="row maxima beyond 60 across LDS blocks"))
    for dt in T16:
        for d, lay, S, Lq in ((16, "plain", 257, 17), (64, "ld_odd", 131, 65), (96, "q_off", 43, 33), (160, "odd_out", 53, 17)):
            out.append(_case("cross", "fp32", dt, d, Lq, S, 2, 2, lay, maps="both" if d == 64 else "identity", why=f"16-bit on the exact kernel: {lay if d > 16 else 'd = 16'}"))
        for d, lay, S in ((16, "hard", 257), (96, "ld_odd", 87), (160, "q_off", 53)):
            B = 4096 // d
            # contexts 0, 2 and 3 are referenced (0 -> 1 key, B + 1: one key in the second LDS block, S + 5 -> S), context 1 is nobody's
            out.append(_case("cross_len", "fp32", dt, d, 17, S, 5, 2, lay, lens=[0, B, B + 1, S + 5], maps="both",
                             why=f"16-bit with lengths on the exact kernel, SW = {dict([(16, 16), (96, 24), (160, 20)])[d]}"))
        out.append(_case("cross", "fp32", dt, 64, 17, 131, 2, 2, "ld_odd", "peaked", why="row maxima beyond 60"))
        out.append(_case("cross_len", "fp32", dt, 96, 17, 87, 2, 2, "ld_odd", "peaked", lens=[43, 87], why="row maxima beyond 60"))
    return out


SEQ_L = (1, 16, 17, 31, 32, 33, 64, 65, 70, 100)


def _third(L, k):
    """The third length of a sample triple (L, 1, third): 31 / 32 / 33 in turn where L allows (33 at L = 100), else L - 1 (L = 1: 1)."""
    if L == 100:
        return 33
    s = [x for x in (31, 32, 33) if x <= L]
    return s[k % len(s)] if s else max(1, L - 1)


def _seq_cases(entry):
    """attn_bias_kernel / attn_causal_kernel (d = 64, 16-bit) at every L of SEQ_L with lengths (L, 1, third), NULL lengths once, L = 512
    once, out-of-range lengths once; the exact kernels in f32 at d = 16 / 32 / 64 / 128 and in 16 bit at d = 16 / 32 / 128 and at d = 64
    through the three doors.  At L = 100 the length 33: the waves at q0 = 64 and 96 are wholly padding and the one at q0 = 32 holds one live query."""
    out = []
    for dt in T16:
        for k, (L, h) in enumerate(zip(SEQ_L, (2, 3, 1, 2, 4, 2, 2, 3, 1, 2))):
            lens = None if L == 70 else (L, 1, _third(L, k))
            out.append(_case(entry, "mfma", dt, 64, L, None, 3, h, "hard" if k % 2 == 0 else "plain", lens=lens,
                             why=f"{3 * h * ((L + 31) // 32)} waves" + (", NULL lengths" if lens is None else f", lengths {lens}")))
        out.append(_case(entry, "mfma", dt, 64, 512, None, 1, 2, "plain", why="the largest table slice and dynamic LDS" if entry == "bias" else "16 diagonal blocks"))
        out.append(_case(entry, "mfma", dt, 64, 33, None, 3, 2, "hard", lens=(0, 38, -3), why="out-of-range lengths behave as 1, L and 1"))
        out.append(_case(entry, "mfma", dt, 64, 70, None, 3, 2, "hard", "peaked", lens=(70, 1, 33), why="row maxima beyond 60"))
        out.append(_case(entry, "mfma", dt, 64, 70, None, 3, 2, "plain", "negative", lens=(70, 33, 31), why="26, 31 and 1 zero-staged keys against scores <= -6"))
    for d, Ls in ((16, (100, 1)), (32, (17, 65)), (64, (65, 31)), (128, (33, 70, 100))):
        for k, L in enumerate(Ls):
            out.append(_case(entry, "fp32", F32, d, L, None, 3, 2, "hard" if k == 0 else "plain", lens=None if (d, k) == (32, 0) else (L, 1, _third(L, k)),
                             why=f"QT = {256 // (d // 16)}, LDS block {min(L, 4096 // d)}"))
    out.append(_case(entry, "fp32", F32, 32, 33, None, 3, 2, "odd_out", lens=(0, 38, -3), why="out-of-range lengths behave as 1, L and 1"))
    out.append(_case(entry, "fp32", F32, 64, 70, None, 3, 2, "hard", "peaked", lens=(70, 1, 33), why="row maxima beyond 60"))
    for dt in T16:
        for d, L, lay in ((16, 16, "hard"), (16, 64, "plain"), (32, 32, "plain"), (32, 70, "hard"), (128, 33, "hard"), (128, 100, "plain"),
                          (64, 65, "ld_odd"), (64, 100, "q_off"), (64, 17, "odd_out")):
            out.append(_case(entry, "fp32", dt, d, L, None, 3, 2, lay, lens=None if (d, L) == (16, 64) else (L, 1, _third(L, d // 16)),
                             why="16-bit on the exact kernel: " + (lay if d == 64 else f"d = {d}")))
        out.append(_case(entry, "fp32", dt, 32, 33, None, 3, 2, "plain", lens=(0, 38, -3), why="out-of-range lengths behave as 1, L and 1"))
        out.append(_case(entry, "fp32", dt, 128, 70, None, 3, 2, "hard", "peaked", lens=(70, 1, 33), why="row maxima beyond 60 across LDS blocks of 32 keys"))
    return out


def all_cases():
    return _cross_strip_cases() + _cross_exact_cases() + _seq_cases("bias") + _seq_cases("causal")


CASES = all_cases()


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def all_instances():
    """The 48 template instances behind the four entry points."""
    inst = {("cross", "mfma", t, d, ln) for t in ("bf16", "f16") for d in (32, 64, 96, 128, 160) for ln in (False, True)}
    inst |= {("cross", "fp32", t, sw, ln) for t in ("f32", "bf16", "f16") for sw in (16, 24, 20) for ln in (False, True)}
    for e in ("bias", "causal"):
        inst |= {(e, "mfma", t) for t in ("bf16", "f16")} | {(e, "fp32", t) for t in ("f32", "bf16", "f16")}
    return inst


# ---- parameters and pointers ----------------------------------------------------------------------------------------------------
PARAMS = {"cross": "CrossAttentionParams", "cross_len": "CrossAttentionLenParams", "bias": "AttentionBiasParams", "causal": "AttentionCausalParams"}
ENTRY = {"cross": "dc_cross_attention", "cross_len": "dc_cross_attention_len", "bias": "dc_attention_bias", "causal": "dc_attention_causal"}


def fields(c, q, k, v, out, lens=None, qm=None, km=None, bias=None):
    """The fields of the entry point's parameter struct for these addresses (lens / qm / km / bias: addresses or None)."""
    f = dict(q=q, k=k, v=v, out=out, dtype=c["dtype"], n=c["n"], heads=c["heads"], d=c["d"], ld_out=c["ld_out"], scale=c["scale"])
    if is_cross(c):
        f.update(q_map=qm, kv_map=km, Lq=c["Lq"], S=c["S"], ld_q=c["ld_q"], ld_kv=c["ld_kv"])
        if c["entry"] == "cross_len":
            f["kv_len"] = lens
    else:
        f.update(L=c["L"], ld_qkv=c["ld_qkv"])
        f["kv_len" if c["entry"] == "bias" else "row_len"] = lens
        if c["entry"] == "bias":
            f["bias"] = bias
    return f


def fake_pointers(c, base=1 << 20):
    """(q, k, v, out, aux) addresses of the alignment the case states, never dereferenced (the *_variant functions read the parameters
    only); aux: an aligned address for whichever of the maps, lengths and table the case passes."""
    es = 4 if c["dtype"] == F32 else 2
    g = case_geometry(c)
    bases = [base + i * (1 << 24) for i in range(g["bufs"])]
    return tuple(bases[i] + o * es for i, o in (g["q"], g["k"], g["v"])) + (base + (1 << 28), base + (1 << 29))


def fake_fields(c, ptrs=None):
    q, k, v, out, aux = ptrs or fake_pointers(c)
    return fields(c, q, k, v, out, lens=None if c["lens"] is None else aux, qm=None if c.get("q_map") is None else aux + 1024,
                  km=None if c.get("kv_map") is None else aux + 2048, bias=aux + 4096)


# ---- operands -------------------------------------------------------------------------------------------------------------------
def make_operands(c, seed=0):
    """q [nq, rows, heads, d], k / v [nc, keys, heads, d] as CPU fp32 tensors already rounded to the compute type (the kernel's operands
    are exactly these), and for dc_attention_bias the fp32 table bias [heads, 2 L - 1]: random per head, asymmetric in the distance."""
    gen = torch.Generator().manual_seed(3000 + seed)
    h, d = c["heads"], c["d"]
    nq, nc = (c["nq"], c["nc"]) if is_cross(c) else (c["n"], c["n"])
    rn = lambda *s: torch.randn(*s, generator=gen)
    q, k, v = rn(nq, c["rows"], h, d), rn(nc, c["keys"], h, d), rn(nc, c["keys"], h, d)
    bias = rn(h, 2 * c["rows"] - 1) if c["entry"] == "bias" else None
    if c["mode"] == "peaked":
        q, k = 5.0 * q, 5.0 * k
        bias = None if bias is None else 4.0 * bias
    elif c["mode"] == "negative":
        # as attention_cases.make_operands, with ONE direction per head for every sample and context (a query meets the keys of any context
        # through the maps): scores -16 + N(0, (2.26 d^-1/4)^2) + a smaller term (+ a unit-normal bias) — all <= -6, asserted by the host test
        u = rn(1, 1, h, d)
        u = u / u.norm(dim=-1, keepdim=True)
        A = (16.0 * d ** 0.5) ** 0.5
        q, k = A * u + 0.4 * q, -A * u + 0.4 * k
    elif c["mode"] != "random":
        raise ValueError(c["mode"])
    r = lambda t: t.to(TD[c["dtype"]]).float()
    o = dict(q=r(q), k=r(k), v=r(v))
    if bias is not None:
        o["bias"] = bias.contiguous()
    return o


def pack(c, o):
    """The CPU tensors a launch reads, in the case's layout and compute type: (buffers, (iq, oq), (ik, ok), (iv, ov)).  Every element that is
    not a value the kernel may read is NaN: the gaps, the leading element of "q_off", K / V rows (bias / causal: q rows too) at or past the
    clamped length, the contexts nobody maps to, and a guard of GUARD elements plus 8 rows behind the last row."""
    g, C, td = case_geometry(c), c["heads"] * c["d"], TD[c["dtype"]]
    eff = eff_lens(c)
    nan = float("nan")
    if is_cross(c):
        qv = o["q"].reshape(c["nq"], c["rows"], C).clone()
        kv_, vv = o["k"].reshape(c["nc"], c["keys"], C).clone(), o["v"].reshape(c["nc"], c["keys"], C).clone()
        for ctx in range(c["nc"]):
            ln = eff[ctx] if ctx in kv_map(c) else 0
            kv_[ctx, ln:] = nan
            vv[ctx, ln:] = nan
    else:
        qv, kv_, vv = (o[x].reshape(c["n"], c["rows"], C).clone() for x in ("q", "k", "v"))
        for i in range(c["n"]):
            for t in (qv, kv_, vv):
                t[i, eff[i]:] = nan
    rows = {"q": qv.reshape(-1, C), "k": kv_.reshape(-1, C), "v": vv.reshape(-1, C)}
    ld = {"q": g["ld_q"], "k": g["ld_kv"], "v": g["ld_kv"]}
    size = [0] * g["bufs"]
    for x in ("q", "k", "v"):
        i, off = g[x]
        size[i] = max(size[i], off + (rows[x].shape[0] + 8) * ld[x] + GUARD)
    bufs = [torch.full((s,), nan, dtype=td) for s in size]
    for x in ("q", "k", "v"):
        i, off = g[x]
        M = rows[x].shape[0]
        bufs[i][off: off + M * ld[x]].view(M, ld[x])[:, :C] = rows[x].to(td)
    return bufs, g["q"], g["k"], g["v"]


# ---- reference and bound --------------------------------------------------------------------------------------------------------
def sample_scores(c, o, i, ln=None):
    """fp64, for output sample i over its first ln keys (default: its clamped length): (q, k, v [heads, *, d], s = scale q.k with the scale
    as the kernel holds it, b = the bias of every (query, key) or zeros, masked = the causal mask)."""
    ln = sample_len(c, i) if ln is None else ln
    R = c["rows"] if is_cross(c) else ln
    q = o["q"][q_map(c)[i], :R].double().permute(1, 0, 2)
    k, v = (o[x][kv_map(c)[i], :ln].double().permute(1, 0, 2) for x in ("k", "v"))
    s = (q @ k.transpose(-1, -2)) * c["scale"]
    qi, ki = torch.arange(R).view(R, 1), torch.arange(ln).view(1, ln)
    b = o["bias"].double()[:, ki - qi + c["rows"] - 1] if c["entry"] == "bias" else torch.zeros_like(s)
    masked = (ki > qi) if c["entry"] == "causal" else torch.zeros(R, ln, dtype=torch.bool)
    return q, k, v, s, b, masked


def reference(c, o):
    """(ref, bound, live): ref and bound [n * rows, heads * d] in fp64, live [n * rows] bool.  A live row is
    ref = softmax(s + b over the keys below the sample's clamped length, and not above the query for causal) v with s = scale q.k, under

        bound = 1.02 u_out |ref| + floor_out + 2 e
        e     = (w |v|) (u_P + 2 delta + (K + 16) 2^-24) + sub,                     w = the softmax weights
        delta = per query, max over its keys of  (d + 4) 2^-24 scale (|q|.|k|)  +  4 2^-24 (|s| + |b|)

    — attention_cases.reference's formula (its docstring argues every term) with L replaced by K, the number of keys the query attends
    (the length; query + 1 for causal: a masked position carries P = 0 exactly and adds nothing to either sum), and with the argument error
    extended by the bias: the strip kernel forms fma(q.k, scale log2 e, b log2 e) - max, the exact one (scale q).k + b - max; the table is
    rounded once when pre-multiplied by log2 e, the rounded constant, the rounding of the FMA and of the difference and the argument
    reduction of the exponential each move the argument by at most 2^-24 of |s|, |b| or the row maximum, which is one of the biased
    scores: 4 2^-24 (|s| + |b|) at the key where that is largest.  u_P: the strip route rounds P to the compute type for P.V and keeps the
    row sum unrounded; 0 on the exact route.  sub: K 2^-25 max |v| on the strip route in f16, K 2^-126 max |v| elsewhere.
    Rows at or past the length (bias, causal) are not live: ref = bound = 0, the checker wants exact zeros there.  Nothing here comes from
    what a kernel returned."""
    n, R, h, d, dt = c["n"], c["rows"], c["heads"], c["d"], c["dtype"]
    strip = c["expect"] == "mfma"
    ref = torch.zeros(n, R, h, d, dtype=torch.float64)
    bound = torch.zeros_like(ref)
    live = torch.zeros(n, R, dtype=torch.bool)
    u_p = U[dt] if strip else 0.0
    for i in range(n):
        q, k, v, s, b, masked = sample_scores(c, o, i)
        rl = q.shape[1]
        w = torch.softmax((s + b).masked_fill(masked, float("-inf")), dim=-1)
        r = w @ v
        mag = w @ v.abs()
        arg = (d + 4) * EPS32 * c["scale"] * (q.abs() @ k.abs().transpose(-1, -2)) + 4 * EPS32 * (s.abs() + b.abs())
        delta = arg.masked_fill(masked, 0.0).amax(-1, keepdim=True)
        K = (~masked).sum(-1).view(1, rl, 1).double()
        sub = K * float(v.abs().max()) * (2.0 ** -25 if (strip and dt == F16) else 2.0 ** -126)
        e = mag * (u_p + 2.0 * delta + (K + 16) * EPS32) + sub
        ref[i, :rl] = r.permute(1, 0, 2)
        bound[i, :rl] = (1.02 * U_OUT[dt] * r.abs() + FLOOR[dt] + 2.0 * e).permute(1, 0, 2)
        live[i, :rl] = True
    return ref.reshape(n * R, h * d), bound.reshape(n * R, h * d), live.reshape(n * R)


def biased_logits(c, o):
    """Every fp64 score the case's softmaxes see, bias included, masked positions left out: one flat tensor."""
    out = []
    for i in range(c["n"]):
        q, k, v, s, b, masked = sample_scores(c, o, i)
        out.append((s + b)[:, ~masked].reshape(-1))
    return torch.cat(out)


# ---- the checker ----------------------------------------------------------------------------------------------------------------
def new_output(c, device="cpu"):
    """The flat output buffer of a case, sentinel everywhere: n * rows rows of ld_out elements and a guard region behind them."""
    return torch.full((c["n"] * c["rows"] * c["ld_out"] + GUARD,), SENTINEL, dtype=TD[c["dtype"]], device=device)


def body(c, buf):
    """[n * rows, heads * d] view of the values inside the flat output buffer."""
    M, ld = c["n"] * c["rows"], c["ld_out"]
    return buf[: M * ld].view(M, ld)[:, : c["heads"] * c["d"]]


def check_output(c, buf, ref, bound, live):
    """buf: the flat output buffer (CPU) after the launch.  Returns (problems, worst err / bound over the live rows): every element of a live
    row finite and inside its bound; every element of a row at or past the length an exact zero; the pad columns (ld_out > heads * d), and
    everything past row n * rows (the guard region), still the sentinel bit for bit."""
    M, C, ld, R, d = c["n"] * c["rows"], c["heads"] * c["d"], c["ld_out"], c["rows"], c["d"]
    problems = []
    sent = _bits(torch.full((1,), SENTINEL, dtype=buf.dtype))[0]
    rows = buf[: M * ld].view(M, ld)
    if not bool((_bits(buf[M * ld:]) == sent).all()):
        bad = (_bits(buf[M * ld:]) != sent).nonzero()
        problems.append(f"{len(bad)} elements behind row n * rows were written, first {int(bad[0][0])} elements behind it")
    if ld > C and not bool((_bits(rows[:, C:]) == sent).all()):
        bad = (_bits(rows[:, C:]) != sent).nonzero()
        problems.append(f"{len(bad)} pad-column elements were written, first at sample {int(bad[0][0]) // R} query {int(bad[0][0]) % R} column {C + int(bad[0][1])}")
    got = rows[:, :C].double()
    pad = got[~live]
    if pad.numel() and not bool((pad == 0).all()):
        bad = (~(got == 0) & ~live.view(M, 1)).nonzero()
        problems.append(f"{len(bad)} elements of rows at or past the length are not zero, first at sample {int(bad[0][0]) // R} query {int(bad[0][0]) % R} "
                        f"column {int(bad[0][1])} (got {float(got[bad[0][0], bad[0][1]])!r})")
    got = torch.where(live.view(M, 1), got, torch.zeros_like(got))
    if not bool(torch.isfinite(got).all()):
        bad = (~torch.isfinite(got)).nonzero()
        problems.append(f"{len(bad)} non-finite values, first at sample {int(bad[0][0]) // R} head {int(bad[0][1]) // d} query {int(bad[0][0]) % R} "
                        f"channel {int(bad[0][1]) % d}")
        got = torch.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
    ratio = torch.where(live.view(M, 1), (got - ref).abs() / bound.clamp_min(1e-300), torch.zeros_like(got))
    worst = float(ratio.max())
    if worst > 1.0:
        bad = (ratio > 1.0).nonzero()
        i, j = (int(x) for x in bad[int(ratio[ratio > 1.0].argmax())])
        where = sorted({(int(r) // R, int(ch) // d, int(r) % R) for r, ch in bad[:4096].tolist()})
        problems.append(f"{len(bad)} of {M * C} elements outside the bound, worst err / bound {worst:.3g} at sample {i // R} head {j // d} query {i % R} "
                        f"channel {j % d} (got {float(got[i, j])!r}, ref {float(ref[i, j])!r}, bound {float(bound[i, j]):.3g}); "
                        f"(sample, head, query) of the first ones: {where[:16]}")
    return problems, worst


def max_abs_err(c, buf, ref, live):
    """max |got - ref| over the live rows (the older tests' flat figure)."""
    got = body(c, buf).double()
    return float(((got - ref).abs() * live.view(-1, 1)).nan_to_num(nan=1e30).max())
