"""The cases of the self-attention parity tests (dc_attention: attn_wave_kernel, attn_mfma_kernel, attn_flash_t_kernel, attn_self_f32_kernel
behind attn_plan of csrc/attention.hip), their operands, their fp64 reference, the per-element error bound and the checker — one table,
two consumers: tests/test_attention_cases.py (host only: routing, coverage, the checker held against an emulation of each route and against
planted faults) and tests/test_gpu_attention.py (the kernels themselves).

A case is a dict of dc_attention_params' plain fields (dtype, n, L, heads, d, ld_qkv, ld_out, scale) plus
    name      its id
    expect    the exact dc_attention_variant string: "wave", "mfma", "flash" or "fp32"
    instance  the kernel instance: ("wave", "bf16", 64, 4) = attn_wave_kernel<bf16, 64, NKT = 4>; ("mfma", "f16", "G2") = attn_mfma_kernel<f16>
              with two pairs per workgroup ("G4": L = 16, "G2": L = 32, "G1", "G4w": L = 64 with d <= 64); ("flash", "bf16", 96) =
              attn_flash_t_kernel<bf16, 96>; ("fp32", "f32", 24, "streamed") = attn_self_f32_kernel<f32, SW = 24> with K / V in blocks ("whole": one block)
    layout    "fused"      one [n, L, 3 heads d] tensor, three offset pointers
              "wide"       fused with ld_qkv = 3 heads d + 8 and ld_out = heads d + 8 (the pad columns of q/k/v hold NaN)
              "split"      three separate tensors, ld_qkv = heads d
              "odd_out"    fused with ld_out = heads d + 2 (the wave and flash kernels store 8 bytes at a time and refuse it);
                           "split_odd_out": the same output behind three separate tensors
              "unaligned"  fused with ld_qkv = 3 heads d + 1 and the 16-bit tensor starting 2 bytes behind a 16-byte boundary
    mode      "random" N(0,1); "peaked" q and k times 5 (logits beyond 60); "negative" every score <= -8 (a zero-score padded key that is not
              masked then takes over the softmax)
    why       one line
Plain Python and CPU torch only: nothing here opens a device.

Largest err / bound on an MI355X per route and dtype (tests/test_gpu_attention.py prints it per case): wave 0.44 (bf16) / 0.33 (f16), mfma
0.42 / 0.34, flash 0.48 / 0.27, fp32 0.0092 (f32) / 0.95 (bf16) / 0.84 (f16)."""

import torch

F32, BF16, F16 = 0, 1, 2
TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
DTN = {F32: "f32", BF16: "bf16", F16: "f16"}
U = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}    # unit roundoff (round to nearest)
U_OUT = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}       # an fp32 result is stored as computed: its rounding is part of e
FLOOR = {F32: 0.0, BF16: 0.0, F16: 2.0 ** -24}             # f16 subnormal spacing
EPS32 = 2.0 ** -24
SENTINEL = 7.0                                             # what the output buffer holds before the launch (exact in every type)
GUARD = 4096                                               # elements behind the last row: NaN in q/k/v, the sentinel in the output
MATRIX_ROUTES = ("wave", "mfma", "flash")                  # they round P to the compute type in front of P.V


# ---- what the dispatcher and the kernels derive from a shape (attn_plan of csrc/attention.hip) ------------------------------------------
def flash_kb(d):
    """Keys per block of attn_flash_t_kernel<T, d>."""
    return 128 if d <= 32 else (64 if d <= 96 else 32)


def fp32_kb(L, d):
    """Keys per LDS block of attn_self_f32_kernel: the whole sequence while 2 L d floats fit 160 KiB, else 8192 / d."""
    return L if 2 * L * d * 4 <= 160 * 1024 else 8192 // d


def fp32_sw(d):
    return 24 if d == 96 else 16


def fp32_qt(d):
    """Queries per workgroup of attn_self_f32_kernel."""
    return 256 // (d // fp32_sw(d))


def mfma_g(L, d):
    """(sample, head) pairs per workgroup of attn_mfma_kernel."""
    if L == 64 and d <= 64:
        return 4
    return 1 if L >= 64 else {32: 2, 16: 4}.get(L, 0)


def mfma_gtag(L, d):
    return "G4w" if (L == 64 and d <= 64) else "G%d" % mfma_g(L, d)


def mfma_lp(L):
    return (L + 31) // 32 * 32


def key_block(c):
    """Keys per step of the route's softmax: the whole (padded) sequence for the two whole-sequence kernels."""
    r = c["expect"]
    return flash_kb(c["d"]) if r == "flash" else (fp32_kb(c["L"], c["d"]) if r == "fp32" else c["L"])


def n_blocks(c):
    kb = key_block(c)
    return (c["L"] + kb - 1) // kb


def padded_keys(c):
    """Keys the kernel holds beyond L (zero rows it has to mask, or whose P it has to zero)."""
    r, L = c["expect"], c["L"]
    if r == "wave":
        return 16 * c["instance"][3] - L
    if r == "mfma":
        return mfma_lp(L) - L
    if r == "flash":
        return n_blocks(c) * key_block(c) - L
    return 0


def pairs(c):
    return c["n"] * c["heads"]


def dead_pair(c):
    """attn_mfma_kernel: the last workgroup holds a pair past n * heads (its waves stage and must not store)."""
    return c["expect"] == "mfma" and pairs(c) % mfma_g(c["L"], c["d"]) != 0


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _case(route, dt, d, L, layout, mode="random", n=2, heads=3, why=""):
    C = heads * d
    ld_qkv = {"fused": 3 * C, "wide": 3 * C + 8, "split": C, "odd_out": 3 * C, "split_odd_out": C, "unaligned": 3 * C + 1}[layout]
    ld_out = {"wide": C + 8, "odd_out": C + 2, "split_odd_out": C + 2}.get(layout, C)
    if route == "wave":
        inst = ("wave", DTN[dt], d, 2 if L <= 32 else 4)
    elif route == "mfma":
        inst = ("mfma", DTN[dt], mfma_gtag(L, d))
    elif route == "flash":
        inst = ("flash", DTN[dt], d)
    else:
        inst = ("fp32", DTN[dt], fp32_sw(d), "whole" if fp32_kb(L, d) == L else "streamed")
    name = f"{route}_{DTN[dt]}_d{d}_L{L}_n{n}h{heads}_{layout}_{mode}"
    return dict(name=name, dtype=dt, n=n, L=L, heads=heads, d=d, ld_qkv=ld_qkv, ld_out=ld_out, scale=float(torch.tensor(d ** -0.5, dtype=torch.float32)),
                expect=route, instance=inst, layout=layout, mode=mode, why=why)


def _wave_cases():
    """All 12 instances.  NKT = 2: L = 1 (one key, fifteen masked in tile 0, tile 1 wholly masked), 16 (tile 1 wholly masked), 17 (one live
    key in tile 1), 32 (nothing masked).  NKT = 4: L = 33 (one live key in tile 2, tile 3 wholly masked), 48 (tile 3 wholly masked), 49, 64.
    Six or five pairs on workgroups of four waves: a ragged last workgroup; one pair alone once per D."""
    out = []
    for dt in (BF16, F16):
        for d in (32, 64, 128):
            for nkt, Ls in ((2, (1, 16, 17, 32)), (4, (33, 48, 49, 64))):
                shapes = [(2, 3), (1, 5), (5, 1), (2, 3)]
                if dt == BF16 and nkt == 2:
                    shapes[2] = (1, 1)                     # one pair: three of the four waves leave at once
                for L, lay, (n, h) in zip(Ls, ("fused", "wide", "split", "fused"), shapes):
                    out.append(_case("wave", dt, d, L, lay, n=n, heads=h, why=f"{16 * nkt - L} of {16 * nkt} staged keys masked, {n * h} pairs"))
                out.append(_case("wave", dt, d, Ls[3], "wide", "peaked", why="row maxima beyond 60"))
                out.append(_case("wave", dt, d, Ls[2], "split", "negative", why=f"{16 * nkt - Ls[2]} zero-score padded keys against scores <= -8"))
                out.append(_case("wave", dt, d, Ls[0], "fused", "negative", n=1, heads=5, why="the fewest live keys of the instance against zero-score padded ones"))
    return out


def _mfma_cases():
    """Both types.  d = 96 (no wave instance) at every G; d = 32 / 64 / 128 at L = 80 ... 128 (G = 1; Lp != L at 80 and 112); the G > 1 forms
    of d = 32 / 64 / 128 through an output the wave kernel refuses (ld_out % 4 != 0).  G > 1 with a dead pair in the last workgroup (3 pairs
    for G = 2, 5 for G = 4) at d = 96 and 32, all pairs live (4) at d = 64 and 128."""
    out = []

    def shape(L, d, alt):
        G = mfma_g(L, d)
        if G == 1:
            return (2, 3)
        if d in (96, 32):
            return ((G + 1, 1) if alt else (1, G + 1))     # G + 1 pairs: 3 for G = 2, 5 for G = 4
        return (2, 2)

    for dt in (BF16, F16):
        alt = dt == F16
        for L, lay in ((16, "wide"), (16, "fused"), (32, "fused"), (32, "split"), (64, "split"), (80, "fused"), (112, "odd_out"), (128, "wide")):
            n, h = shape(L, 96, alt)
            out.append(_case("mfma", dt, 96, L, lay, n=n, heads=h, why=f"G = {mfma_g(L, 96)}, Lp = {mfma_lp(L)}, {n * h} pairs"))
        for d in (32, 64, 128):
            for L, lay in ((80, "fused"), (96, "wide"), (112, "split"), (128, "odd_out")):
                out.append(_case("mfma", dt, d, L, lay, why=f"G = 1, Lp = {mfma_lp(L)}"))
            for L in (16, 32, 64) if d <= 64 else (16, 32):
                n, h = shape(L, d, alt)
                out.append(_case("mfma", dt, d, L, "odd_out", n=n, heads=h, why=f"the wave kernel refuses ld_out % 4 != 0: {mfma_gtag(L, d)}, {n * h} pairs"))
        # peaked once per instance, negative where Lp != L (G4: L = 16; G1: L = 80 and 112)
        out.append(_case("mfma", dt, 96, 16, "fused", "peaked", n=2, heads=4, why="G4, all pairs live, row maxima beyond 60"))
        out.append(_case("mfma", dt, 96, 32, "wide", "peaked", n=2, heads=2, why="G2, all pairs live, row maxima beyond 60"))
        out.append(_case("mfma", dt, 64, 128, "fused", "peaked", why="G1, row maxima beyond 60"))
        out.append(_case("mfma", dt, 32, 64, "split_odd_out", "peaked", n=1, heads=5, why="G4w with a dead pair, row maxima beyond 60"))
        out.append(_case("mfma", dt, 96, 16, "wide", "negative", n=1, heads=5, why="16 zero-padded keys (Lp = 32) against scores <= -8"))
        out.append(_case("mfma", dt, 96, 80, "split", "negative", why="16 zero-padded keys (Lp = 96) against scores <= -8"))
        out.append(_case("mfma", dt, 128, 112, "fused", "negative", why="16 zero-padded keys (Lp = 128) against scores <= -8"))
    return out


def _flash_cases():
    """Both types, all four D.  L = 129: the smallest flash length (the second query block holds one live query, its waves 1 - 3 are wholly
    dead, the ragged key block holds one key); 255: one dead query; 256: no ragged block, an even block count for every KB; 3 KB - 1 (at
    least 129; D = 128: 5 KB - 1 = 159 and 161): an odd block count with a ragged tail of KB - 1 keys (161: of one key behind an odd
    count of full blocks); 300."""
    out = []
    for dt in (BF16, F16):
        for d in (32, 64, 96, 128):
            kb = flash_kb(d)
            odd = (159, 161) if d == 128 else (3 * kb - 1,)
            Ls = (129, 255, 256) + odd + (300,)
            for L, lay in zip(Ls, ("fused", "wide", "split", "fused", "wide", "split")):
                out.append(_case("flash", dt, d, L, lay, why=f"KB = {kb}: {L // kb} full blocks and {L % kb} keys, {(-L) % 128} dead queries in the last query block"))
            out.append(_case("flash", dt, d, 300, "split", "peaked", why="row maxima beyond 60, the running max moves between blocks"))
            out.append(_case("flash", dt, d, odd[0], "wide", "negative", why="one zero-score padded key in the ragged block against scores <= -8"))
            out.append(_case("flash", dt, d, 129, "fused", "negative", why=f"{kb - 129 % kb} zero-score padded keys beside one live one in the ragged block"))
    return out


def _fp32_cases():
    """f32 at every d with L one past the query-tile size QT = 256 / (d / SW) (a second workgroup with one live query); the streamed form at
    its smallest length for every d (d = 96: KB = 85, two full blocks and 44 keys) and the one-block neighbour of two of them; 16-bit inputs
    the matrix-core kernels do not take: d = 16, L % 16 != 0 between 65 and 128, L = 48 at d = 96 (no pairs-per-workgroup form), an output
    the flash kernel refuses at d = 96 (the only way to the streamed SW = 24 form in 16 bit), and q/k/v that are not 16-byte aligned."""
    out = []
    f = lambda *a, **k: out.append(_case("fp32", *a, n=k.pop("n", 2), heads=k.pop("heads", 2), **k))
    for d, L, lay in ((16, 257, "fused"), (32, 129, "wide"), (64, 65, "odd_out"), (96, 65, "fused"), (128, 33, "split")):
        f(F32, d, L, lay, why=f"QT = {fp32_qt(d)}: a second query tile with one live query")
    for d, L, lay in ((128, 161, "wide"), (96, 214, "fused"), (64, 321, "split"), (32, 641, "odd_out"), (16, 1281, "fused")):
        f(F32, d, L, lay, why=f"streamed, KB = {8192 // d}: {L // (8192 // d)} full blocks and {L % (8192 // d)} keys")
    f(F32, 128, 160, "fused", why="the longest one-block length at d = 128")
    f(F32, 96, 213, "wide", why="the longest one-block length at d = 96")
    f(F32, 64, 65, "split", "peaked", why="SW = 16 whole, row maxima beyond 60")
    f(F32, 96, 65, "wide", "peaked", why="SW = 24 whole, row maxima beyond 60")
    f(F32, 64, 321, "fused", "peaked", why="SW = 16 streamed, the running max moves between blocks")
    f(F32, 96, 214, "wide", "peaked", why="SW = 24 streamed, KB = 85")
    for dt in (BF16, F16):
        f(dt, 16, 24, "fused", why="d = 16 has no matrix-core kernel")
        f(dt, 16, 100, "wide", why="d = 16 has no matrix-core kernel")
        f(dt, 64, 100, "split", why="L % 16 != 0 between 65 and 128")
        f(dt, 96, 48, "fused", why="attn_pairs_per_wg(48, 96) == 0 and d = 96 has no wave instance")
        f(dt, 16, 1281, "fused", why="16-bit on the streamed form, KB = 512")
        f(dt, 96, 214, "odd_out", why="the flash kernel refuses ld_out % 4 != 0: 16-bit on the streamed SW = 24 form")
        for L, d in ((64, 64), (96, 32), (128, 96), (300, 64), (214, 96)):
            f(dt, d, L, "unaligned", why="q/k/v 2 bytes behind a 16-byte boundary, ld_qkv odd: no matrix-core kernel reads them")
        f(dt, 64, 100, "fused", "peaked", why="SW = 16 whole, row maxima beyond 60")
        f(dt, 96, 48, "wide", "peaked", why="SW = 24 whole, row maxima beyond 60")
        f(dt, 16, 1281, "wide", "peaked", why="SW = 16 streamed, row maxima beyond 60")
        f(dt, 96, 214, "unaligned", "peaked", why="SW = 24 streamed, row maxima beyond 60")
    return out


def all_cases():
    return _wave_cases() + _mfma_cases() + _flash_cases() + _fp32_cases()


CASES = all_cases()

# Instances that only an output the 8-byte-store kernels refuse (or operands no matrix-core kernel reads) leads to: they never see the
# plain "fused" layout, every other instance does
NO_FUSED = {
    **{("mfma", t, "G4w"): "L = 64 with d <= 64 goes to the wave kernel unless ld_out % 4 != 0" for t in ("bf16", "f16")},
    **{("fp32", t, 24, "streamed"): "d = 96 beyond 213 tokens goes to the flash kernel unless ld_out % 4 != 0 or q/k/v are unaligned" for t in ("bf16", "f16")},
}
# Forms a kernel could run and dc_attention never produces — attn_plan has no such form; tests/test_attention_cases.py proves each on a probe grid
UNREACHABLE = {
    **{("mfma", t, "L>128"): "attn_plan has no whole-sequence form beyond 128 tokens: everything longer goes elsewhere" for t in ("bf16", "f16")},
    **{("flash", t, "L<=128"): "attn_plan has no flash form at or below 128 tokens: the fp32 image of such a sequence always fits 160 KiB" for t in ("bf16", "f16")},
}

# bit-identity whatever the sample's place in the batch: one case per route and dtype (run at n = 1 and at n = 3)
PLACEMENT_CASES = [_case("wave", dt, 64, 49, "fused", n=1, heads=3) for dt in (BF16, F16)] + \
                  [_case("mfma", dt, 96, 32, "fused", n=1, heads=3) for dt in (BF16, F16)] + \
                  [_case("flash", dt, 64, 191, "fused", n=1, heads=3) for dt in (BF16, F16)] + \
                  [_case("fp32", dt, 64, 321, "unaligned" if dt != F32 else "fused", n=1, heads=3) for dt in (F32, BF16, F16)]
# launch-to-launch identity at size: 512 pairs
REPEAT_CASES = [_case("wave", BF16, 64, 64, "fused", n=64, heads=8), _case("mfma", BF16, 64, 128, "fused", n=64, heads=8),
                _case("flash", BF16, 64, 256, "fused", n=64, heads=8), _case("fp32", F32, 64, 256, "fused", n=64, heads=8)]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def elem_offsets(c):
    """Element offsets of q, k, v inside their buffer(s): (buffers, (iq, oq), (ik, ok), (iv, ov)) — buffer index and offset."""
    C = c["heads"] * c["d"]
    if c["layout"].startswith("split"):
        return 3, (0, 0), (1, 0), (2, 0)
    o0 = 1 if c["layout"] == "unaligned" else 0
    return 1, (0, o0), (0, o0 + C), (0, o0 + 2 * C)


def attention_fields(c, q, k, v, out):
    """The dc_attention_params fields of a case for the four addresses."""
    return dict(q=q, k=k, v=v, out=out, **{f: c[f] for f in ("dtype", "n", "L", "heads", "d", "ld_qkv", "ld_out", "scale")})


def fake_pointers(c, base=1 << 20):
    """Addresses of the alignment the case states, never dereferenced (dc_attention_variant reads the parameters only)."""
    es = 4 if c["dtype"] == F32 else 2
    nb, q, k, v = elem_offsets(c)
    bases = [base + i * (1 << 24) for i in range(nb)]
    return tuple(bases[i] + o * es for i, o in (q, k, v)) + (base + (1 << 28),)


# ---- operands -------------------------------------------------------------------------------------------------------------------
def make_operands(c, seed=0):
    """q, k, v [n, L, heads, d] as CPU fp32 tensors already rounded to the compute type (the kernel's operands are exactly these)."""
    gen = torch.Generator().manual_seed(2000 + seed)
    n, L, h, d = c["n"], c["L"], c["heads"], c["d"]
    rn = lambda *s: torch.randn(*s, generator=gen)
    q, k, v = rn(n, L, h, d), rn(n, L, h, d), rn(n, L, h, d)
    if c["mode"] == "peaked":
        q, k = 5.0 * q, 5.0 * k
    elif c["mode"] == "negative":
        # q = A u + 0.4 noise, k = -A u + 0.4 noise for one unit direction u per (sample, head), A^2 = 16 sqrt(d): the scores are
        # -16 + N(0, (2.26 d^-1/4)^2) + a smaller noise.noise term — all <= -8 (asserted on the fp64 logits by the host test), spread enough for a softmax
        u = rn(n, 1, h, d)
        u = u / u.norm(dim=-1, keepdim=True)
        A = (16.0 * d ** 0.5) ** 0.5
        q, k = A * u + 0.4 * q, -A * u + 0.4 * k
    elif c["mode"] != "random":
        raise ValueError(c["mode"])
    r = lambda t: t.to(TD[c["dtype"]]).float()
    return dict(q=r(q), k=r(k), v=r(v))


def pack(c, o):
    """The CPU tensors a launch reads, in the case's layout and compute type: (buffers, (iq, oq), (ik, ok), (iv, ov)).  Every element that is
    not a q/k/v value is NaN: the pad columns of "wide", the odd column of "unaligned", the leading element of "unaligned" and a guard of
    GUARD elements behind the last row."""
    n, L, C, ld = c["n"], c["L"], c["heads"] * c["d"], c["ld_qkv"]
    nb, iq, ik, iv = elem_offsets(c)
    bufs = [torch.full((8 + n * L * ld + GUARD,), float("nan"), dtype=TD[c["dtype"]]) for _ in range(nb)]
    for name, (i, off) in (("q", iq), ("k", ik), ("v", iv)):
        bufs[i][off: off + n * L * ld].view(n * L, ld)[:, :C] = o[name].reshape(n * L, C).to(TD[c["dtype"]])
    return bufs, iq, ik, iv


# ---- reference and bound --------------------------------------------------------------------------------------------------------
def logits(c, o):
    """fp64 scores [n, heads, L, L] with the scale as the kernel holds it (fp32)."""
    q, k = o["q"].double().permute(0, 2, 1, 3), o["k"].double().permute(0, 2, 1, 3)
    return (q @ k.transpose(-1, -2)) * c["scale"]


def reference(c, o):
    """(ref, bound), both [n * L, heads * d] in fp64: ref = softmax(s) v with s = scale q.k, and the per-element bound on |got - ref|

        bound = 1.02 u_out |ref| + floor_out + 2 e
        e     = (w |v|) (u_P + 2 delta + (L + 16) 2^-24) + sub,                     w = softmax(s)
        delta = per query, max over keys of  (d + 4) 2^-24 scale (|q|.|k|)  +  4 2^-24 |s|

    The result is sum_j p_j v_j / sum_j p_j with p_j = exp(s_j - m).  A score carries the forward error of an fp32 dot product of length d in
    any summation order and of the multiply by the scale, (d + 4) 2^-24 scale |q|.|k| (the fp32 kernel scales q first: one more rounding,
    inside the + 4).  The exponent's argument is formed as fma(s, scale log2 e, -m scale log2 e) on the matrix-core routes and as s - m on the
    other: the rounded constant, the rounded product m * const, the rounding of the difference and the argument reduction of v_exp_f32 / expf
    each move it by at most 2^-24 of |s| or |m|, and m is one of the scores: 4 2^-24 max |s|.  An absolute error delta of the argument is a
    relative error delta of p_j; it enters the numerator and the row sum, and since both are sums of positive terms weighted by w the
    quotient moves by at most 2 delta (w |v|).  u_P: the matrix-core routes round p_j to the compute type for the P.V product while the row
    sum keeps the unrounded p_j, so the numerator alone carries one unit roundoff of the compute type; 0 on the fp32 route.  (L + 16) 2^-24:
    the two fp32 sums of L terms in any order (the row sum and P.V, one rounding per addition, to first order L 2^-24 each way of the
    quotient, which the outer factor 2 covers) and the handful of single roundings — the exponential's own ulp, the correction factors of the
    online softmax, the reciprocal and the final product — in the 16.  sub: a weight below the smallest number P can hold is lost —
    L 2^-25 max |v| on the matrix-core routes in f16 (p_j <= 1 and the row sum >= 1, so a weight rounds by at most half the subnormal spacing
    2^-24), L 2^-126 max |v| everywhere else (v_exp_f32 flushes below the normal range of fp32).  The factor 2 because the matrix core's
    internal accumulation is not documented to round every addition to nearest (the convention of tests/gemm_tile_cases.py).  u_out / floor:
    the rounding of the stored value.  Nothing here comes from what a kernel returned."""
    n, L, h, d = c["n"], c["L"], c["heads"], c["d"]
    q, k, v = (o[x].double().permute(0, 2, 1, 3) for x in ("q", "k", "v"))        # [n, h, L, d]
    s = (q @ k.transpose(-1, -2)) * c["scale"]
    w = torch.softmax(s, dim=-1)
    ref = w @ v
    mag = w @ v.abs()
    delta = ((d + 4) * EPS32 * c["scale"] * (q.abs() @ k.abs().transpose(-1, -2)) + 4 * EPS32 * s.abs()).amax(-1, keepdim=True)
    matrix = c["expect"] in MATRIX_ROUTES
    u_p = U[c["dtype"]] if matrix else 0.0
    sub = L * float(v.abs().max()) * (2.0 ** -25 if (matrix and c["dtype"] == F16) else 2.0 ** -126)
    e = mag * (u_p + 2.0 * delta + (L + 16) * EPS32) + sub
    bound = 1.02 * U_OUT[c["dtype"]] * ref.abs() + FLOOR[c["dtype"]] + 2.0 * e
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(n * L, h * d)
    return flat(ref), flat(bound)


# ---- the checker ----------------------------------------------------------------------------------------------------------------
def new_output(c, device="cpu"):
    """The flat output buffer of a case, sentinel everywhere: n * L rows of ld_out elements and a guard region behind them."""
    return torch.full((c["n"] * c["L"] * c["ld_out"] + GUARD,), SENTINEL, dtype=TD[c["dtype"]], device=device)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def body(c, buf):
    """[n * L, heads * d] view of the values inside the flat output buffer."""
    M, ld = c["n"] * c["L"], c["ld_out"]
    return buf[: M * ld].view(M, ld)[:, : c["heads"] * c["d"]]


def check_output(c, buf, ref, bound):
    """buf: the flat output buffer (CPU) after the launch.  Returns (problems, worst err / bound): every element of [n * L, heads * d] finite
    and inside its bound; the pad columns (ld_out > heads * d), and with them everything past row n * L (the guard region), still the
    sentinel bit for bit."""
    M, C, ld, L, d = c["n"] * c["L"], c["heads"] * c["d"], c["ld_out"], c["L"], c["d"]
    problems = []
    sent = _bits(torch.full((1,), SENTINEL, dtype=buf.dtype))[0]
    rows = buf[: M * ld].view(M, ld)
    if not bool((_bits(buf[M * ld:]) == sent).all()):
        bad = (_bits(buf[M * ld:]) != sent).nonzero()
        problems.append(f"{len(bad)} elements behind row n * L were written, first {int(bad[0][0])} elements behind it")
    if ld > C and not bool((_bits(rows[:, C:]) == sent).all()):
        bad = (_bits(rows[:, C:]) != sent).nonzero()
        problems.append(f"{len(bad)} pad-column elements were written, first at sample {int(bad[0][0]) // L} query {int(bad[0][0]) % L} column {C + int(bad[0][1])}")
    got = rows[:, :C].double()
    if not bool(torch.isfinite(got).all()):
        bad = (~torch.isfinite(got)).nonzero()
        problems.append(f"{len(bad)} non-finite values, first at sample {int(bad[0][0]) // L} head {int(bad[0][1]) // d} query {int(bad[0][0]) % L} "
                        f"channel {int(bad[0][1]) % d}")
        got = torch.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
    ratio = (got - ref).abs() / bound
    worst = float(ratio.max())
    if worst > 1.0:
        bad = (ratio > 1.0).nonzero()
        i, j = (int(x) for x in bad[int(ratio[ratio > 1.0].argmax())])
        where = sorted({(int(r) // L, int(ch) // d, int(r) % L) for r, ch in bad[:4096].tolist()})
        problems.append(f"{len(bad)} of {M * C} elements outside the bound, worst err / bound {worst:.3g} at sample {i // L} head {j // d} query {i % L} "
                        f"channel {j % d} (got {float(got[i, j])!r}, ref {float(ref[i, j])!r}, bound {float(bound[i, j]):.3g}); "
                        f"(sample, head, query) of the first ones: {where[:16]}")
    return problems, worst
