"""The cases of the dc_tblock_front parity tests (csrc/tblock.hip: proj_in -> LayerNorm -> q/k/v -> softmax attention -> to_out + bias +
class vector + residual of 64 tokens x 256 channels in ONE launch, q, k, v and p never leaving registers), their operands, their fp64
reference, the expected bits or the bound of every output element, and the checker — one table, two consumers: tests/test_tblock_cases.py
(host only: coverage, preconditions, two CPU emulations, the checker held against planted faults) and tests/test_gpu_tblock.py (the kernel).

A case is a dict of dc_tblock_front_params' plain fields (dtype, n, L, C, heads, ldx, ld_out, rowvec_ld, ln_eps, scale) plus
    name      its id
    kind      "exact" (every output element bit for bit) or "chain" (every element inside a bound)
    mode      exact: "epilogue_exact", "one_hot", "uniform"; chain: "random", "peaked", "attn_dominant", "ln_offset", "ln_flat", "odd_scale"
    why       what the case is there for
    use       the optional pointers it sets, a subset of {"bo", "rowvec", "rowvec_map"}
    n_vec     rows of the row-vector table (n without a map)
    layout    {"ldx", "ld_out", "rowvec_ld"} (the same numbers as the plain fields)
Plain Python and CPU torch only: nothing here opens a device.

Operands are rounded to the compute type first; the reference, the emulations and the device all start from exactly those values.  The
weights are plain [rows][256] matrices (the GPU test packs them with engine.pack_matrix).

EXACT cases.  The operands are small integers or powers of two, so every fp32 accumulation is exact in ANY order and every documented
rounding point but the last receives a value the type holds (test_tblock_cases.py checks these preconditions on the operands); the last
one, the output, is a real rounding of an exact fp32 sum.  The expected bits come from a closed formula, not from a model of the kernel:
    epilogue_exact  Wv = 0, so o = 0 whatever the softmax does: out = round(((0 + bo) + rowvec[map[n]]) + h), h = x Wp^T + bp a multiple
                    of 2^-2 below 32 in magnitude.  Pins the proj_in fragment map, image 1's write and read-back, the epilogue's order and
                    its null branches, the row stores.
    one_hot         Wp = I, x rows are balanced +-1 codes (hn = +-1 exactly: 1 / sqrt(1 + 1e-5) = 0.999995 rounds to 1 in both types),
                    Wk = I, Wq = beta I: a query's score against its own token exceeds every other by more than 160 in log2 units, so p is
                    one-hot, ps = 1 and o_t = v_t: out = round(((v_t Wo^T + bo) + rowvec) + h_t).  A key permuted inside a tile or a head
                    taken from the neighbouring fragment pair returns another token's row.
    uniform         Wq = 0: every score 0, p = 1, ps = 64, Wv = I: o = mean_t hn_t, an integer because the code columns sum to multiples
                    of 64.  A row sum that misses a lane group gives 16, 32 or 48.  (The device's reciprocal of 64 need not be exact for
                    this: o = m (1 + d) with an integer m and |d| of an fp32 ulp rounds back to m, far from any rounding boundary of a
                    16-bit type.  The case is therefore held to bit equality without the relaxation the reciprocal might have asked for.)

CHAIN cases: random operands, every element against
        |got - ref| <= KAPPA u S + 1.02 u |ref| + floor,         S = |o| |Wo|^T + |bo| + |rowvec| + |h|
ref: fp64 with the documented rounding points (h, hn, q, k, v, p and o rounded to the compute type, the row sum over the UNROUNDED p as the
kernel takes it), o and h in S the reference's own intermediates, u the unit roundoff of the compute type (bf16 2^-8, f16 2^-11), the
second and third term the rounding of the stored value.  A worst-case forward bound through LayerNorm and exp is astronomically large and
would hide everything; KAPPA is measured instead.  This module holds two independent CPU emulations that honour the rounding points —
"chunk32": fp32 accumulation in the kernel's k-chunks of 32 with the kernel's own LayerNorm and exp2 formulas, and "plain": fp32
torch.matmul, F.layer_norm and exp — and KAPPA is twice the largest forward error / (u S) of their fp32 value in front of the output
rounding, over all chain cases, rounded up to the next 0.1 (torch.matmul's summation order is the BLAS library's).  They differ from the
reference where an intermediate sat on a rounding boundary of its type and fell the other way; the factor 2 is for what neither samples:
the device's 1-ulp exp2 / rcp / rsqrt and the matrix core's internal order, which move a stored intermediate the same way, only where it
already sits on a boundary.  KAPPA is never adjusted to what a device returned.  RECORDED holds the measured ratios."""
import torch
import torch.nn.functional as F

from gemm_tile_cases import FLOOR, GUARD, SENTINEL, TD, U_OUT, _bits

BF16, F16 = 1, 2
DTN = {BF16: "bf16", F16: "f16"}
DTS = (BF16, F16)
L_TOK, C_CH = 64, 256
LOG2E32 = 1.4426950408889634                     # the kernel's literal, rounded to fp32 where it is used
EXACT_MODES = ("epilogue_exact", "one_hot", "uniform")
CHAIN_MODES = ("random", "peaked", "attn_dominant", "ln_offset", "ln_flat", "odd_scale")
BETA = {32: 128.0, 64: 64.0}                     # one_hot: Wq = beta I per head width
GAP_LOG2 = 160.0                                 # one_hot: score gap in log2 units every other key must exceed

# forward error / (u S) in front of the output rounding.  "emulation": the largest over both CPU emulations per mode, over four operand
# draws of every case with n <= 8 and one of the n = 513 cases (host run of tests/test_tblock_cases.py, which prints them); KAPPA = 2 * their maximum, rounded up to 0.1.  "device": the largest per mode on an MI355X, there with the
# stored (rounded) value: max(0, |got - ref| - output rounding) / (u S) (first device run of tests/test_gpu_tblock.py, which prints it).
RECORDED = {
    "emulation": {"random": 0.888, "peaked": 0.747, "attn_dominant": 0.279, "ln_offset": 1.408, "ln_flat": 0.561, "odd_scale": 1.011},
    "device": {"random": 0.587, "peaked": 0.557, "attn_dominant": 0.202, "ln_offset": 0.529, "ln_flat": 0.010, "odd_scale": 0.365},
}
KAPPA = 3.0          # 2 * 1.5: ln_offset in f16 sets it, where an h of 8 that falls the other way moves the residual by 2 u |h|


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _case(name, dt, heads, kind, mode, why, *, n=3, use=("bo", "rowvec", "rowvec_map"), n_vec=None, ldx=C_CH, ld_out=C_CH, rowvec_ld=C_CH,
          ln_eps=1e-5, scale=None):
    use = frozenset(use)
    assert "rowvec" in use or "rowvec_map" not in use
    assert (kind == "exact" and mode in EXACT_MODES) or (kind == "chain" and mode in CHAIN_MODES)
    d = C_CH // heads
    if "rowvec" not in use:
        n_vec, rowvec_ld = 0, 0                                  # what engine.PlanBuilder.tblock_front passes without a class vector
    elif "rowvec_map" not in use:
        n_vec = n
    elif n_vec is None:
        n_vec = 3
    return dict(name=name, kind=kind, mode=mode, why=why, dtype=dt, n=n, L=L_TOK, C=C_CH, heads=heads, ldx=ldx, ld_out=ld_out, rowvec_ld=rowvec_ld,
                ln_eps=ln_eps, scale=float(d) ** -0.5 if scale is None else scale, use=use, n_vec=n_vec,
                layout=dict(ldx=ldx, ld_out=ld_out, rowvec_ld=rowvec_ld))


def _exact_cases():
    out = []
    for dt in DTS:
        t = DTN[dt]
        e = lambda tag, why, heads=8, **kw: out.append(_case(f"epilogue_exact_{t}_{tag}", dt, heads, "exact", "epilogue_exact", why, **kw))
        e("full", "bias, mapped class vector and residual in the documented order", heads=4)
        e("no_bo", "the null-bo branch", use=("rowvec", "rowvec_map"))
        e("no_rowvec", "the null-rowvec branch: what the engine passes for a block without a class vector", use=("bo",), ldx=264, ld_out=272)
        e("rowvec_no_map", "rowvec without a map: row n of a table of n rows (the engine's per-unit class vector)", use=("bo", "rowvec"), n=5)
        e("map_many_to_one", "a many-to-one, out-of-order map into 3 rows", n=8, n_vec=3)
        e("rowvec_ld260", "a padded row-vector table", rowvec_ld=260, ld_out=264, heads=4)
        e("n1", "one sample: one workgroup", n=1, use=("bo", "rowvec"))
        for heads in (4, 8):
            out.append(_case(f"one_hot_{t}_h{heads}", dt, heads, "exact", "one_hot", "token order of K against Q, key order of P against the swapped-operand V, "
                             "the head slices of both head widths", n=2 if heads == 4 else 3, rowvec_ld=260 if heads == 8 else C_CH,
                             ldx=264 if heads == 4 else C_CH))
            out.append(_case(f"uniform_{t}_h{heads}", dt, heads, "exact", "uniform", "the row sum over all four lane groups and 64 keys", n=2,
                             use=("bo", "rowvec") if heads == 4 else ("bo", "rowvec", "rowvec_map"), ld_out=272 if heads == 8 else C_CH))
    return out


def _chain_cases():
    out = []
    why = dict(random="the whole chain on noise-like data, per element",
               peaked="q and k rows x 3: peaked softmax rows, logits of several tens",
               attn_dominant="Wp and bp scaled so that |h| << |o| |Wo|^T, no rowvec, null bo: softmax and to_out errors are not hidden under h",
               ln_offset="bp + 8: a large row mean against the spread",
               ln_flat="rows of h with a spread of a few ulps and ln_eps = 1e-3: eps decides rstd",
               odd_scale="scale = 0.7 d^-0.5: not the one a hard-coded head width would also produce")
    # the layouts ride on the cross: n = 1, 3 and 8 dense, ldx = 264 with ld_out = 272; the pointer subsets of the engine likewise
    lay = [dict(n=3), dict(n=1), dict(n=8), dict(n=2, ldx=264, ld_out=272, rowvec_ld=260)]
    uses = [("bo", "rowvec", "rowvec_map"), ("bo", "rowvec"), ("bo",), ("bo", "rowvec", "rowvec_map")]
    i = 0
    for mode in CHAIN_MODES:
        for dt in DTS:
            for heads in (4, 8):
                m = i // 4                          # shifted per mode, so that every dtype and head count meets every layout
                kw = dict(lay[(i + m) % 4])
                kw["use"] = uses[(i + 2 * m + m // 2) % 4]
                if mode == "attn_dominant":
                    kw["use"] = ()
                    kw.pop("rowvec_ld", None)
                if "rowvec" not in kw["use"]:
                    kw.pop("rowvec_ld", None)
                if mode == "ln_flat":
                    kw["ln_eps"] = 1e-3
                if mode == "odd_scale":
                    kw["scale"] = 0.7 * float(C_CH // heads) ** -0.5
                out.append(_case(f"{mode}_{DTN[dt]}_h{heads}", dt, heads, "chain", mode, why[mode], **kw))
                i += 1
    for dt, heads in ((BF16, 8), (F16, 4)):
        out.append(_case(f"random_{DTN[dt]}_h{heads}_n513", dt, heads, "chain", "random", "one more than two workgroups on each of 256 CUs",
                         n=513, n_vec=10))
    return out


CASES = _exact_cases() + _chain_cases()
# launch-to-launch identity, other traffic in between: one exact and one peaked case per dtype
REPEAT_CASES = ["one_hot_bf16_h8", "one_hot_f16_h4", "peaked_bf16_h8", "peaked_f16_h4"]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def rows(c):
    return c["n"] * L_TOK


PTR_FIELDS = ("x", "Wp", "bp", "ln_g", "ln_b", "Wqkv", "Wo", "bo", "rowvec", "rowvec_map", "out")


def front_fields(c, ptrs):
    """The dc_tblock_front_params fields of a case; ptrs: {pointer field: address}."""
    kw = {k: c[k] for k in ("dtype", "n", "L", "C", "heads", "ldx", "ld_out", "rowvec_ld", "ln_eps", "scale")}
    for f in PTR_FIELDS:
        if f in ("bo", "rowvec", "rowvec_map") and f not in c["use"]:
            continue
        kw[f] = ptrs[f]
    return kw


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def _rowvec_map(n, n_vec):
    """Many-to-one and out of order for every n >= 3: 2, 0, 2, 1, 0, 1, 0, 2, ... (mod n_vec)."""
    i = torch.arange(n)
    return ((torch.tensor([2, 0, 2, 1])[i % 4] + i // 4) % n_vec).to(torch.int32)


def _sparse_int(gen, rows_, cols, nnz, values):
    """[rows, cols] with nnz entries per row drawn from `values`, elsewhere 0."""
    w = torch.zeros(rows_, cols)
    vals = torch.tensor(values, dtype=torch.float32)
    for r in range(rows_):
        idx = torch.randperm(cols, generator=gen)[:nnz]
        w[r, idx] = vals[torch.randint(0, len(vals), (nnz,), generator=gen)]
    return w


def _balanced_rows(gen, n):
    """[n, 64, 256] of +-1, every row summing to zero."""
    base = torch.cat([torch.ones(C_CH // 2), -torch.ones(C_CH // 2)])
    return torch.stack([torch.stack([base[torch.randperm(C_CH, generator=gen)] for _ in range(L_TOK)]) for _ in range(n)])


def _paired_codes(gen, n):
    """[n, 64, 256] of +-1, every row summing to zero and every column of a sample summing to -64, 0 or 64: columns 0, 4, 8, ... are
    constant (+1 and -1 in turn, one in every 4-channel lane slot of every fragment), the others come in pairs (c, c') at random places,
    column c a random balanced column and c' its negative."""
    x = torch.zeros(n, L_TOK, C_CH)
    const = torch.arange(0, C_CH, 4)
    rest = torch.tensor([c for c in range(C_CH) if c % 4])
    col = torch.cat([torch.ones(L_TOK // 2), -torch.ones(L_TOK // 2)])
    for s in range(n):
        x[s][:, const] = torch.where((const // 4) % 2 == 0, 1.0, -1.0)[None, :].expand(L_TOK, -1)
        perm = rest[torch.randperm(len(rest), generator=gen)]
        for j in range(0, len(perm), 2):
            v = col[torch.randperm(L_TOK, generator=gen)]
            x[s][:, perm[j]] = v
            x[s][:, perm[j + 1]] = -v
    return x


def sc2_of(c):
    """scale * log2 e as the kernel forms it: both fp32, one fp32 product."""
    return float(torch.tensor(c["scale"], dtype=torch.float32) * torch.tensor(LOG2E32, dtype=torch.float32))


def one_hot_gap(c, x):
    """Smallest score gap, in log2 units after scale * log2 e, between a query's own token and every other key, over all samples and heads
    (k = hn = x, q = beta x: scores are beta times the code agreement)."""
    d = C_CH // c["heads"]
    xh = x.view(c["n"], L_TOK, c["heads"], d).transpose(1, 2).double()
    agree = xh @ xh.transpose(-1, -2)                                         # [n, heads, 64, 64], d on the diagonal
    off = agree - 2.0 * d * torch.eye(L_TOK, dtype=torch.float64)           # the diagonal out of the way
    return float((d - off.amax(-1)).min()) * BETA[d] * sc2_of(c)


def make_operands(c, seed=None):
    """CPU fp32 tensors, the MFMA operands already rounded to the compute type: x [n, 64, 256], Wp [256, 256], Wqkv [768, 256] (rows q | k | v),
    Wo [256, 256], bp, ln_g, ln_b, and bo, rowvec [n_vec, 256], rowvec_map [n] where the case uses them."""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"])) if seed is None else seed
    gen = torch.Generator().manual_seed(9000 + seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
    q = lambda t: t.to(TD[c["dtype"]]).float()
    n, mode, d, use = c["n"], c["mode"], C_CH // c["heads"], c["use"]
    eye = torch.eye(C_CH)
    o = {}
    if c["kind"] == "chain":
        o["x"] = q(rn(n, L_TOK, C_CH))
        Wp, Wqkv, Wo = (rn(r, C_CH) / C_CH ** 0.5 for r in (C_CH, 3 * C_CH, C_CH))
        bp, o["ln_g"], o["ln_b"] = 0.1 * rn(C_CH), 1.0 + 0.2 * rn(C_CH), 0.1 * rn(C_CH)
        if mode == "peaked":
            Wqkv[: 2 * C_CH] *= 3.0
        elif mode == "attn_dominant":
            Wp, bp = Wp / 64.0, bp / 64.0
        elif mode == "ln_offset":
            bp = bp + 8.0
        elif mode == "ln_flat":                      # h = 1 + (a few spacings of the type at 1)
            sp = 2.0 * U_OUT[c["dtype"]]
            Wp, bp = Wp * sp, torch.ones(C_CH)
        o.update(Wp=q(Wp), Wqkv=q(Wqkv), Wo=q(Wo), bp=bp)
        bo, rv = 0.1 * rn(C_CH), rn(max(c["n_vec"], 1), C_CH)
    else:
        bo, rv = ri(-512, 512, C_CH) / 256.0, ri(-2048, 2048, max(c["n_vec"], 1), C_CH) / 256.0
        if mode == "epilogue_exact":
            o["x"] = ri(-3, 3, n, L_TOK, C_CH)
            o["Wp"] = _sparse_int(gen, C_CH, C_CH, 8, [-1.0, 1.0])
            o["bp"] = ri(-8, 8, C_CH) / 4.0
            o["ln_g"], o["ln_b"] = 1.0 + 0.2 * rn(C_CH), 0.1 * rn(C_CH)
            o["Wqkv"] = torch.cat([q(rn(2 * C_CH, C_CH) / C_CH ** 0.5), torch.zeros(C_CH, C_CH)])
            o["Wo"] = q(rn(C_CH, C_CH) / C_CH ** 0.5)
        else:
            o["Wp"], o["bp"], o["ln_g"], o["ln_b"] = eye.clone(), torch.zeros(C_CH), torch.ones(C_CH), torch.zeros(C_CH)
            o["Wo"] = _sparse_int(gen, C_CH, C_CH, 4, [-2.0, -1.0, 1.0, 2.0])
            if mode == "one_hot":
                for _ in range(50):                 # redrawn until the gap holds in every head of every sample
                    o["x"] = _balanced_rows(gen, n)
                    if one_hot_gap(c, o["x"]) > GAP_LOG2:
                        break
                assert one_hot_gap(c, o["x"]) > GAP_LOG2, c["name"]
                o["Wqkv"] = torch.cat([BETA[d] * eye, eye, _sparse_int(gen, C_CH, C_CH, 4, [-1.0, 1.0])])
            else:
                o["x"] = _paired_codes(gen, n)
                o["Wqkv"] = torch.cat([torch.zeros(C_CH, C_CH), eye, eye])
    if "bo" in use:
        o["bo"] = bo
    if "rowvec" in use:
        o["rowvec"] = rv
        if "rowvec_map" in use:
            o["rowvec_map"] = _rowvec_map(n, c["n_vec"])
    for k in ("x", "Wp", "Wqkv", "Wo"):
        assert torch.equal(o[k], q(o[k])), (c["name"], k)
    return o


def rowvec_rows(c, o, dtype=torch.float64, unmapped=False):
    """[n, 1, 256]: the class vector of every sample (zeros without one).  unmapped: row n % n_vec instead of map[n] (a planted fault)."""
    if "rowvec" not in o:
        return torch.zeros(c["n"], 1, C_CH, dtype=dtype)
    idx = o["rowvec_map"].long() if "rowvec_map" in o and not unmapped else torch.arange(c["n"]) % o["rowvec"].shape[0]
    return o["rowvec"][idx][:, None, :].to(dtype)


def _heads(t, heads):
    n = t.shape[0]
    return t.view(n, L_TOK, heads, C_CH // heads).transpose(1, 2)


# ---- the fp64 reference, the expected bits, the bound ---------------------------------------------------------------------------------
def reference(c, o):
    """(ref, S, mid): the fp64 result of the documented contract (include/dcamd.h) over every output element [n * 64, 256] with h, hn, q, k,
    v, p and o rounded to the compute type and the row sum over the unrounded p; S = |o| |Wo|^T + |bo| + |rowvec| + |h| from the same
    intermediates; mid: h, hn, o and the logits (scale * q k^T, [n, heads, query, key]) for the preconditions of the host test."""
    td = TD[c["dtype"]]
    r = lambda t: t.to(td).double()
    n, heads = c["n"], c["heads"]
    x, Wp, Wqkv, Wo = (o[k].double() for k in ("x", "Wp", "Wqkv", "Wo"))
    h = r(x @ Wp.t() + o["bp"].double())
    mean = h.mean(-1, keepdim=True)
    var = ((h - mean) ** 2).mean(-1, keepdim=True)
    hn = r((h - mean) / torch.sqrt(var + float(torch.tensor(c["ln_eps"], dtype=torch.float32))) * o["ln_g"].double() + o["ln_b"].double())
    qkv = r(hn @ Wqkv.t())
    qh, kh, vh = (_heads(qkv[..., i * C_CH:(i + 1) * C_CH].contiguous(), heads) for i in range(3))
    logits = (qh @ kh.transpose(-1, -2)) * float(torch.tensor(c["scale"], dtype=torch.float32))
    p = torch.exp(logits - logits.amax(-1, keepdim=True))
    ps = p.sum(-1, keepdim=True)
    ov = r((r(p) @ vh) / ps).transpose(1, 2).reshape(n, L_TOK, C_CH)
    bo = o["bo"].double() if "bo" in o else torch.zeros(C_CH, dtype=torch.float64)
    rv = rowvec_rows(c, o)
    ref = ((ov @ Wo.t() + bo) + rv) + h
    S = ov.abs() @ Wo.abs().t() + bo.abs() + rv.abs() + h.abs()
    return ref.reshape(-1, C_CH), S.reshape(-1, C_CH), dict(h=h, hn=hn, o=ov, logits=logits)


def bound_of(c, ref, S, kappa=None):
    """KAPPA u S + the rounding of the stored value."""
    u = U_OUT[c["dtype"]]
    return (KAPPA if kappa is None else kappa) * u * S + 1.02 * u * ref.abs() + FLOOR[c["dtype"]]


def forward_ratio(c, val, ref, S, stored=False):
    """Largest forward error / (u S) of fp32 values val [M, 256] in front of the output rounding; stored: val is the rounded, stored value,
    and the rounding term of the bound is taken off first."""
    u = U_OUT[c["dtype"]]
    err = (val.double() - ref).abs()
    if stored:
        err = (err - (1.02 * u * ref.abs() + FLOOR[c["dtype"]])).clamp_min(0.0)
    return float((err / (u * S)).max())


def expected_bits(c, o):
    """Exact cases: the bits of every output element [n * 64, 256] from the closed formula of the case's mode, every operation in fp32 and
    exact but the last rounding (the host test checks that against fp64)."""
    assert c["kind"] == "exact"
    f32, f64 = _expected_value(c, o, torch.float32), _expected_value(c, o, torch.float64)
    assert torch.equal(f32.double(), f64), c["name"]                         # every fp32 operation was exact
    return _bits(f32.to(TD[c["dtype"]])).reshape(-1, C_CH)


def _expected_value(c, o, dtype):
    x = o["x"].to(dtype)
    h = x @ o["Wp"].to(dtype).t() + o["bp"].to(dtype)
    if c["mode"] == "epilogue_exact":
        ov = torch.zeros_like(h)
    elif c["mode"] == "one_hot":                     # hn = x, o_t = v_t
        ov = x @ o["Wqkv"][2 * C_CH:].to(dtype).t()
    else:                                            # hn = x, v = hn, o = the mean over the tokens
        ov = (x.sum(1, keepdim=True) / L_TOK).expand(-1, L_TOK, -1)
    bo = o["bo"].to(dtype) if "bo" in o else torch.zeros(C_CH, dtype=dtype)
    return ((ov @ o["Wo"].to(dtype).t() + bo) + rowvec_rows(c, o, dtype)) + h


# ---- two CPU emulations that honour the rounding points ---------------------------------------------------------------------------
FAULTS = ("k_heads_swapped", "scale_other_width", "quarter_max", "sum48", "p_tiles_swapped", "to_out_chunk0_for_7", "rowvec_unmapped",
          "h_shifted_16", "ln_b_dropped", "ln_eps_dropped", "bo_dropped", "v_from_h")
FAULT_HEAD = 1        # the attention faults sit in this head alone, of every sample


def _mm(a, w, how, stale=False):
    """a [..., K] . w [N, K]^T in fp32: "plain" torch.matmul, or "chunk32" accumulated over the kernel's k-chunks of 32.  stale: the last
    chunk takes the weights of chunk 0 (a planted fault)."""
    if how == "plain" and not stale:
        return a @ w.transpose(-1, -2)
    K = a.shape[-1]
    acc = torch.zeros(*a.shape[:-1], w.shape[-2])
    for k0 in range(0, K, 32):
        kw = 0 if stale and k0 == K - 32 else k0
        acc = acc + a[..., k0:k0 + 32] @ w[..., kw:kw + 32].transpose(-1, -2)
    return acc


def emulate(c, o, how, fault=None):
    """The kernel in fp32 on the CPU, rounding where it rounds; returns the fp32 values [n * 64, 256] in front of the output rounding.
    how = "chunk32": k-chunks of 32, the kernel's LayerNorm (sum / 256, two passes, rsqrt), exp2(fma(s, sc2, -max sc2)), o = (P V) * (1 / ps).
    how = "plain": torch.matmul, F.layer_norm, exp(scale (s - max)), o = (P V) / ps.
    fault: one of FAULTS, planted into either."""
    assert how in ("chunk32", "plain") and (fault is None or fault in FAULTS)
    td = TD[c["dtype"]]
    r = lambda t: t.to(td).float()
    n, heads, d = c["n"], c["heads"], C_CH // c["heads"]
    x, Wp, Wqkv, Wo = o["x"], o["Wp"], o["Wqkv"], o["Wo"]
    eps = torch.tensor(0.0 if fault == "ln_eps_dropped" else c["ln_eps"], dtype=torch.float32)
    ln_b = torch.zeros(C_CH) if fault == "ln_b_dropped" else o["ln_b"]
    scale = torch.tensor(c["scale"], dtype=torch.float32)
    if fault == "scale_other_width":
        scale = torch.tensor(float(C_CH // (12 - heads)) ** -0.5 * (c["scale"] / float(d) ** -0.5), dtype=torch.float32)
    h = r(_mm(x, Wp, how) + o["bp"])
    if how == "chunk32":
        mean = h.sum(-1, keepdim=True) / C_CH
        dv = h - mean
        rstd = torch.rsqrt((dv * dv).sum(-1, keepdim=True) / C_CH + eps)
        hn = r(dv * rstd * o["ln_g"] + ln_b)
    else:
        hn = r(F.layer_norm(h, (C_CH,), o["ln_g"], ln_b, float(eps)))
    qkv = r(_mm(hn, Wqkv, how))
    if fault == "v_from_h":
        qkv[..., 2 * C_CH:] = r(_mm(h, Wqkv[2 * C_CH:], how))
    qc, kc, vc = (qkv[..., i * C_CH:(i + 1) * C_CH].contiguous() for i in range(3))
    if fault == "k_heads_swapped":                   # the two 32-channel heads of wave 0, K only
        assert heads == 8
        kc = torch.cat([kc[..., 32:64], kc[..., 0:32], kc[..., 64:]], -1)
    qh, kh, vh = _heads(qc, heads), _heads(kc, heads), _heads(vc, heads)
    s = _mm(qh, kh, how)                                                     # [n, heads, query, key]
    key = torch.arange(L_TOK)
    group = (key % 16) // 4                                                  # the lane group that holds the key in the kernel
    mx = s.amax(-1, keepdim=True)
    if fault == "quarter_max":
        own = torch.stack([s[..., group == g].amax(-1) for g in range(4)], -1)[..., group]
        mx = torch.cat([mx[:, :FAULT_HEAD].expand(-1, -1, -1, L_TOK), own[:, FAULT_HEAD:FAULT_HEAD + 1],
                        mx[:, FAULT_HEAD + 1:].expand(-1, -1, -1, L_TOK)], 1)
    if how == "chunk32":
        sc2 = scale * torch.tensor(LOG2E32, dtype=torch.float32)
        nms = -mx * sc2
        p = torch.exp2((s.double() * sc2.double() + nms.double()).float())   # one rounding: a fused multiply-add
    else:
        p = torch.exp((s - mx) * scale)
    ps = p.sum(-1, keepdim=True)
    if fault == "sum48":
        ps = ps.clone()
        ps[:, FAULT_HEAD] = p[:, FAULT_HEAD][..., group != 3].sum(-1, keepdim=True)
    pr = r(p)
    if fault == "p_tiles_swapped":                   # keys 4 .. 7 of tiles 0 and 1, in P but not in V
        pr = pr.clone()
        a, b = pr[:, FAULT_HEAD, :, 4:8].clone(), pr[:, FAULT_HEAD, :, 20:24].clone()
        pr[:, FAULT_HEAD, :, 4:8], pr[:, FAULT_HEAD, :, 20:24] = b, a
    pv = _mm(pr, vh.transpose(-1, -2), how)
    ov = r(pv * (1.0 / ps) if how == "chunk32" else pv / ps).transpose(1, 2).reshape(n, L_TOK, C_CH)
    acc = _mm(ov, Wo, how, stale=fault == "to_out_chunk0_for_7")
    bo = o["bo"] if "bo" in o and fault != "bo_dropped" else torch.zeros(C_CH)
    hres = torch.roll(h, -16, 1) if fault == "h_shifted_16" else h
    val = ((acc + bo) + rowvec_rows(c, o, torch.float32, unmapped=fault == "rowvec_unmapped")) + hres
    return val.reshape(-1, C_CH)


# ---- operands in memory, the checker ------------------------------------------------------------------------------------------------
def embedded(t, ld, dtype):
    """t [..., C] as rows of `ld` elements inside a NaN-filled flat allocation (CPU): GUARD NaN elements in front and behind, NaN in the
    pad columns.  The operand's first element is element GUARD."""
    C = t.shape[-1]
    r = t.reshape(-1, C)
    flat = torch.full((2 * GUARD + r.shape[0] * ld,), float("nan"), dtype=dtype)
    flat[GUARD: GUARD + r.shape[0] * ld].view(r.shape[0], ld)[:, :C] = r.to(dtype)
    return flat


def extracted(flat, nrows, ld, C=C_CH):
    """The [nrows, C] operand inside an allocation of `embedded`, as a kernel that honours ld and C reads it."""
    return flat[GUARD: GUARD + nrows * ld].view(nrows, ld)[:, :C]


def new_output(c, device="cpu"):
    """The flat output allocation of a case, sentinel everywhere: a guard region, n * 64 rows of ld_out elements, a guard region.  The
    kernel's `out` is element GUARD."""
    return torch.full((2 * GUARD + rows(c) * c["ld_out"],), SENTINEL, dtype=TD[c["dtype"]], device=device)


def to_buffer(c, val):
    """fp32 values [M, 256] rounded into a sentinel-filled allocation, as the kernel would leave it."""
    M, ld = rows(c), c["ld_out"]
    buf = new_output(c)
    buf[GUARD: GUARD + M * ld].view(M, ld)[:, :C_CH] = val.to(TD[c["dtype"]])
    return buf


def where(c, row, ch):
    """A failing element in the kernel's own coordinates."""
    n, t = divmod(int(row), L_TOK)
    ch = int(ch)
    d = C_CH // c["heads"]
    return (f"(sample {n}, token {t}, channel {ch}): wave {ch // 64}, head {ch // d}, channel fragment {ch % 64 // 16}, lane group {ch % 16 // 4}, "
            f"token fragment {t // 16}, lane row {t % 16}")


def ulp_distance(a_bits, b_bits):
    """Distance in representable values between two int16 bit patterns of a 16-bit float type."""
    key = lambda b: torch.where(b.int() < 0, -(b.int() & 0x7FFF), b.int() & 0x7FFF)
    return (key(a_bits) - key(b_bits)).abs()


def check_output(c, buf, ref, bound_or_bits):
    """buf: the flat allocation of new_output (CPU) after the launch.  Returns (problems, worst): every value finite; exact cases: every
    element's bits equal bound_or_bits [M, 256] (int16; ref may be None; worst: the largest distance in representable values); chain cases:
    every element within bound_or_bits of ref (worst: the largest err / bound); the pad columns (ld_out > 256), the guard in front,
    everything behind row n * 64 and the guard behind it still the sentinel bit for bit."""
    M, ld = rows(c), c["ld_out"]
    problems = []
    sent = _bits(torch.full((1,), SENTINEL, dtype=buf.dtype))[0]
    body = buf[GUARD: GUARD + M * ld].view(M, ld)
    for label, region in (("in front of the first row", buf[:GUARD]), (f"behind row {M}", buf[GUARD + M * ld:])):
        if not bool((_bits(region) == sent).all()):
            problems.append(f"{int((_bits(region) != sent).sum())} elements {label} were written")
    if ld > C_CH and not bool((_bits(body[:, C_CH:]) == sent).all()):
        bad = (_bits(body[:, C_CH:]) != sent).nonzero()
        problems.append(f"{len(bad)} pad-column elements were written, first at row {int(bad[0][0])}, column {C_CH + int(bad[0][1])}")
    got = body[:, :C_CH]
    if not bool(torch.isfinite(got.float()).all()):
        nf = (~torch.isfinite(got.float())).nonzero()
        problems.append(f"{len(nf)} non-finite values, first at {where(c, *nf[0])}")
    if c["kind"] == "exact":
        dist = ulp_distance(_bits(got), bound_or_bits)
        worst = float(dist.max())
        if worst > 0:
            bad = (dist > 0).nonzero()
            i, j = (int(v) for v in bad[0])
            want = bound_or_bits[i, j].view(buf.dtype)
            problems.append(f"{len(bad)} of {M * C_CH} elements differ from the expected bits (up to {int(worst)} representable values), in samples "
                            f"{sorted({int(r) // L_TOK for r in bad[:, 0].tolist()})[:8]}, channels {sorted({int(v) for v in bad[:, 1].tolist()})[:8]}...; "
                            f"first at {where(c, i, j)}: got {float(got[i, j])!r}, expected {float(want)!r}")
        return problems, worst
    g64 = torch.nan_to_num(got.double(), nan=1e30, posinf=1e30, neginf=-1e30)
    ratio = (g64 - ref).abs() / bound_or_bits
    worst = float(ratio.max())
    if worst > 1.0:
        bad = (ratio > 1.0).nonzero()
        i, j = (int(v) for v in bad[int(ratio[ratio > 1.0].argmax())])
        problems.append(f"{len(bad)} of {M * C_CH} elements outside the bound, worst err / bound {worst:.3g} at {where(c, i, j)} (got {float(g64[i, j])!r}, "
                        f"ref {float(ref[i, j])!r}, bound {float(bound_or_bits[i, j]):.3g}); the first: " + "; ".join(where(c, a, b) for a, b in bad[:4].tolist()))
    return problems, worst


_REF_CACHE = {}


def prepared(name):
    """(case, operands, ref, S, expected bits or bound) of a case, built once per process."""
    if name not in _REF_CACHE:
        c = by_name(name)
        o = make_operands(c)
        if c["kind"] == "exact":
            _REF_CACHE[name] = (c, o, None, None, expected_bits(c, o))
        else:
            ref, S, _ = reference(c, o)
            _REF_CACHE[name] = (c, o, ref, S, bound_of(c, ref, S))
    return _REF_CACHE[name]
