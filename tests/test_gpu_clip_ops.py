"""GPU: the kernels of the CLIP text encoder path — dc_attention_causal against a float64 reference computed on the device, over every
output element, and dc_layernorm_rows / dc_embed_rows_pos / dc_act_pass against torch in float64.

dc_attention_causal runs on the hard layout of tests/test_gpu_t5_ops.py: q | k | v rows wider than the heads with NaN in the gap, NaN in
every q / k / v row at or past the sample's length, NaN rows behind the last sample, and an output prefilled with NaN — a finite output
with exact zeros in the pad rows proves that nothing past the length was read and that every element was written.
Bounds are the project's for the same arithmetic on unit-normal inputs (tests/test_gpu_cross_attention.py): 2e-5 max abs in f32, 1.5e-2 in
16-bit; dc_layernorm_rows' are those tests/test_gpu_norms.py uses for LayerNorm rows (by output type)."""
import math

import pytest
import torch

from diffusion_classifier_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
NAME = {L.DC_F32: "f32", L.DC_BF16: "bf16", L.DC_F16: "f16"}
BOUND = {L.DC_F32: 2e-5, L.DC_BF16: 1.5e-2, L.DC_F16: 1.5e-2}
LN_BOUND = {L.DC_F32: 2e-5, L.DC_BF16: 5e-2, L.DC_F16: 8e-3}          # tests/test_gpu_norms.py OUTER_LN
NAN = float("nan")


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Case:
    """One dc_attention_causal problem on the hard layout.  q / k / v [n, L, heads * d] clean host copies (rounded to the storage type);
    rows at or past lens[i] are NaN on the device whatever the host copy holds."""

    def __init__(self, dt, q, k, v, lens, heads, d, use_len=True, ld_extra=64):
        self.dt, self.heads, self.d = dt, heads, d
        self.q, self.k, self.v = (t.to(TD[dt]).float() for t in (q, k, v))
        self.n, self.L, self.C = q.shape[0], q.shape[1], heads * d
        self.lens = list(lens)
        n, Lq, Cc = self.n, self.L, self.C
        self.ld = 3 * Cc + ld_extra
        buf = torch.full((n * Lq + 8, self.ld), NAN)                            # 8 NaN rows behind the last sample, NaN in the gap
        for i in range(n):
            r0, ln = i * Lq, self.lens[i]
            buf[r0:r0 + ln, :Cc], buf[r0:r0 + ln, Cc:2 * Cc], buf[r0:r0 + ln, 2 * Cc:3 * Cc] = self.q[i, :ln], self.k[i, :ln], self.v[i, :ln]
        self.buf = buf.to(TD[dt]).to(DEV)
        self.lens_d = torch.tensor(self.lens, dtype=torch.int32, device=DEV) if use_len else None

    def run(self, scale):
        out = torch.full((self.n, self.L, self.C), NAN, dtype=TD[self.dt], device=DEV)
        es, p0 = self.buf.element_size(), self.buf.data_ptr()
        p = L.AttentionCausalParams(q=p0, k=p0 + self.C * es, v=p0 + 2 * self.C * es, out=out.data_ptr(),
                                    row_len=None if self.lens_d is None else self.lens_d.data_ptr(), dtype=self.dt, n=self.n, L=self.L,
                                    heads=self.heads, d=self.d, ld_qkv=self.ld, ld_out=self.C, scale=scale)
        kern = L.lib().dc_attention_causal_variant(p).decode()
        L.check(L.lib().dc_attention_causal(p, L.stream_ptr()), "dc_attention_causal")
        torch.cuda.synchronize()
        return out, kern

    def ref(self, scale):
        """float64 on the device; rows at or past a sample's length are zero."""
        Lq, h, d = self.L, self.heads, self.d
        out = torch.zeros(self.n, Lq, self.C, dtype=torch.float64, device=DEV)
        for i, ln in enumerate(self.lens):
            q, k, v = (t[i, :ln].to(DEV).double().view(ln, h, d).transpose(0, 1) for t in (self.q, self.k, self.v))
            pos = torch.arange(ln, device=DEV)
            s = (q @ k.transpose(-1, -2) * scale).masked_fill(pos[None, :] > pos[:, None], float("-inf"))       # [head, query, key]
            out[i, :ln] = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(ln, self.C)
        return out

    def check(self, out, scale, what):
        got = out.double()
        assert torch.isfinite(got).all(), f"{what}: non-finite output (an unwritten element, or a read at or past the length)"
        for i, ln in enumerate(self.lens):
            assert (out[i, ln:].float() == 0).all(), f"{what}: pad rows of sample {i} are not zero"
        return (got - self.ref(scale)).abs().max().item()


def _straddles(Lq):
    """Lengths of the third sample: 31 / 32 / 33 (around a key-block edge) where L allows; otherwise L - 1, or L itself when L = 1."""
    s = [x for x in (31, 32, 33) if x <= Lq]
    return s or [Lq - 1 if Lq > 1 else Lq]


def _random_case(dt, d, Lq, heads, third, seed=0, **kw):
    torch.manual_seed(10000 * d + 13 * Lq + 101 * heads + third + seed)
    Cc = heads * d
    q, k, v = torch.randn(3, Lq, Cc), torch.randn(3, Lq, Cc), torch.randn(3, Lq, Cc)
    return Case(dt, q, k, v, (Lq, 1, third), heads, d, **kw)


GRID = [(L.DC_F32, 16), (L.DC_F32, 64), (L.DC_BF16, 64), (L.DC_F16, 64)]
GRID_IDS = [f"{NAME[dt]}-d{d}" for dt, d in GRID]
# one query; inside one block; a block edge and one past it; a ragged diagonal block; the real size; an exact multiple; five tiles
L_ALL = [1, 5, 32, 33, 40, 77, 96, 130]


@pytest.mark.parametrize("Lq", L_ALL)
@pytest.mark.parametrize("dt,d", GRID, ids=GRID_IDS)
def test_attention_causal_grid(dt, d, Lq):
    """dtype x head dim x L; heads 2 and 3 (3: a ragged last workgroup of the one-wave-per-tile kernel); n = 3 with lengths (L, 1, a
    value straddling a key-block edge); unit-normal q / k / v with scale d^-1/2."""
    scale = d ** -0.5
    worst = 0.0
    for heads in (2, 3):
        for third in _straddles(Lq):
            c = _random_case(dt, d, Lq, heads, third)
            out, kern = c.run(scale)
            assert kern == ("fp32" if dt == L.DC_F32 else "mfma"), kern
            worst = max(worst, c.check(out, scale, f"{NAME[dt]} d={d} L={Lq} heads={heads} lens=({Lq}, 1, {third})"))
    print(f"dc_attention_causal {NAME[dt]} d={d} L={Lq}: worst max abs err {worst:.2e} (bound {BOUND[dt]:.1e})")
    assert worst < BOUND[dt], worst


@pytest.mark.parametrize("r", [1, 32, 33])
@pytest.mark.parametrize("dt,d", GRID, ids=GRID_IDS)
def test_attention_causal_rows_do_not_depend_on_later_rows(dt, d, r):
    """Causality, bit for bit: output rows < r keep their bits when rows >= r of q, k and v hold other values (every sample at full
    length, row_len = NULL), and when those rows are NaN on the device and the length says r (the prefix of a long prompt's output IS
    the output of the truncated prompt: what lets the encoder ignore the padding mask)."""
    Lq, heads, scale = 77, 3, d ** -0.5
    torch.manual_seed(7 * d + r)
    q, k, v = (torch.randn(2, Lq, heads * d) for _ in range(3))
    full = Case(dt, q, k, v, [Lq, Lq], heads, d, use_len=False)
    a = full.run(scale)[0]
    assert torch.isfinite(a.float()).all()
    q2, k2, v2 = (t.clone() for t in (q, k, v))
    for t in (q2, k2, v2):
        t[:, r:] = 5.0 * torch.randn(2, Lq - r, heads * d) + 1.0
    b = Case(dt, q2, k2, v2, [Lq, Lq], heads, d, use_len=False).run(scale)[0]
    assert torch.equal(_bits(a[:, :r]), _bits(b[:, :r])), "other values in later rows changed earlier rows"
    assert not torch.equal(_bits(a[:, r:]), _bits(b[:, r:]))
    c = Case(dt, q, k, v, [r, Lq], heads, d).run(scale)[0]                      # sample 0: rows >= r are NaN, its length is r
    assert torch.equal(_bits(a[0, :r]), _bits(c[0, :r])) and bool((c[0, r:].float() == 0).all())
    assert torch.equal(_bits(a[1]), _bits(c[1]))


@pytest.mark.parametrize("dt,d", GRID, ids=GRID_IDS)
def test_attention_causal_without_lengths_equals_full_lengths(dt, d):
    """row_len = NULL gives the bits of row_len = L, within the bound of the reference."""
    Lq, heads = 77, 2
    torch.manual_seed(d + 1)
    q, k, v = (torch.randn(3, Lq, heads * d) for _ in range(3))
    c0 = Case(dt, q, k, v, [Lq] * 3, heads, d, use_len=False)
    c1 = Case(dt, q, k, v, [Lq] * 3, heads, d, use_len=True)
    a, b = c0.run(d ** -0.5)[0], c1.run(d ** -0.5)[0]
    err = c0.check(a, d ** -0.5, "row_len = NULL")
    print(f"dc_attention_causal {NAME[dt]} d={d} L={Lq} row_len = NULL: max abs err {err:.2e} (bound {BOUND[dt]:.1e})")
    assert err < BOUND[dt], err
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dt", [L.DC_BF16, L.DC_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("d,ld_extra", [(64, 2), (32, 64)])
def test_attention_causal_exact_route_in_16_bit(dt, d, ld_extra):
    """16-bit operands the matrix-core kernel does not take — rows its 16-byte loads cannot read (ld_qkv % 8 != 0), head width 32 — run
    on the exact kernel, same bound."""
    Lq, heads = 40, 2
    c = _random_case(dt, d, Lq, heads, 33, ld_extra=ld_extra)
    out, kern = c.run(d ** -0.5)
    assert kern == "fp32", kern
    err = c.check(out, d ** -0.5, f"{NAME[dt]} d={d} exact route")
    print(f"dc_attention_causal {NAME[dt]} d={d} ld_qkv={c.ld} on the exact kernel: max abs err {err:.2e} (bound {BOUND[dt]:.1e})")
    assert err < BOUND[dt], err


@pytest.mark.parametrize("dt,d", GRID, ids=GRID_IDS)
def test_attention_causal_is_deterministic_and_permutes_with_its_samples(dt, d):
    """Two launches give identical bits; permuting the samples (rows, lengths) permutes the output bit for bit."""
    Lq, heads = 100, 3
    c = _random_case(dt, d, Lq, heads, 33)
    a, b = c.run(d ** -0.5)[0], c.run(d ** -0.5)[0]
    assert torch.equal(_bits(a), _bits(b))
    perm = [2, 0, 1]
    cp = Case(dt, c.q[perm], c.k[perm], c.v[perm], [c.lens[i] for i in perm], heads, d)
    p = cp.run(d ** -0.5)[0]
    assert torch.isfinite(p.float()).all()
    assert torch.equal(_bits(p), _bits(a[perm]))


# ---- dc_layernorm_rows / dc_embed_rows_pos / dc_act_pass ----------------------------------------------------------------
@pytest.mark.parametrize("C", [128, 768, 1024])
@pytest.mark.parametrize("odt", [L.DC_F32, L.DC_BF16, L.DC_F16], ids=["f32-f32", "f32-bf16", "f32-f16"])
def test_layernorm_rows(odt, C):
    """fp32 rows of C channels, 3 samples of 7 rows, without row_len and with (all, 1, a middle value); rows at or past row_len hold NaN
    and must come out as zeros.  The rows carry an offset so that a skipped mean subtraction cannot pass."""
    torch.manual_seed(C + odt)
    n, rps, eps = 3, 7, 1e-5
    x = torch.randn(n * rps, C) * 1.5 + 0.7
    g = (1.0 + 0.25 * torch.randn(C)).to(DEV)
    b = (0.1 * torch.randn(C)).to(DEV)
    xd64 = x.double()
    want0 = (xd64 - xd64.mean(-1, keepdim=True)) * torch.rsqrt(xd64.var(-1, unbiased=False, keepdim=True) + eps) * g.double().cpu() + b.double().cpu()
    for lens in (None, [7, 1, 4]):
        xin, want = x.clone(), want0.clone()
        if lens is not None:
            for i, ln in enumerate(lens):
                xin[i * rps + ln:(i + 1) * rps] = NAN
                want[i * rps + ln:(i + 1) * rps] = 0
        xd = xin.to(DEV)
        y = torch.full((n * rps + 1, C), NAN, dtype=TD[odt], device=DEV)        # one guard row behind
        ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
        p = L.LayernormRowsParams(x=xd.data_ptr(), y=y.data_ptr(), gamma=g.data_ptr(), beta=b.data_ptr(),
                                  row_len=None if ld is None else ld.data_ptr(), dtype=L.DC_F32, out_dtype=odt, rows=n * rps, C=C,
                                  rows_per_sample=rps, eps=eps)
        L.check(L.lib().dc_layernorm_rows(p, L.stream_ptr()), "dc_layernorm_rows")
        torch.cuda.synchronize()
        got = y.cpu()
        assert torch.isnan(got[-1].float()).all(), "the row behind the last was written"
        got = got[:-1].double()
        assert torch.isfinite(got).all()
        if lens is not None:
            for i, ln in enumerate(lens):
                assert (got[i * rps + ln:(i + 1) * rps] == 0).all()
        err = (got - want).abs().max().item()
        print(f"dc_layernorm_rows f32 -> {NAME[odt]} C={C} row_len={lens}: max abs err {err:.2e} (bound {LN_BOUND[odt]:.1e})")
        assert err < LN_BOUND[odt], err


@pytest.mark.parametrize("odt", [L.DC_F32, L.DC_BF16, L.DC_F16], ids=["f32", "bf16", "f16"])
def test_embed_rows_pos_is_exact_and_clamps(odt):
    torch.manual_seed(5)
    vocab, C, n, Lq = 48, 200, 3, 13
    rows = n * Lq
    table, pos = torch.randn(vocab, C, device=DEV), torch.randn(Lq + 4, C, device=DEV)
    ids = torch.randint(0, vocab, (rows,), device=DEV)
    ids[3], ids[4] = -7, vocab + 100                                            # device data the kernel must not trust: clamped
    out = torch.full((rows + 1, C), NAN, dtype=TD[odt], device=DEV)
    p = L.EmbedRowsPosParams(table=table.data_ptr(), pos=pos.data_ptr(), ids=ids.data_ptr(), out=out.data_ptr(), out_dtype=odt, rows=rows,
                             C=C, vocab=vocab, L=Lq)
    L.check(L.lib().dc_embed_rows_pos(p, L.stream_ptr()), "dc_embed_rows_pos")
    torch.cuda.synchronize()
    want = (table[ids.clamp(0, vocab - 1)] + pos[:Lq].repeat(n, 1)).to(TD[odt])
    assert torch.equal(_bits(out[:rows]), _bits(want))
    assert torch.isnan(out[rows].float()).all()


def _act_ref(x64, kind):
    if kind == L.PASS_QUICK_GELU:
        return x64 * torch.sigmoid(1.702 * x64)
    return 0.5 * x64 * torch.special.erfc(-x64 / math.sqrt(2.0))              # x Phi(x); erfc keeps the negative tail in float64 too


def _ordered(t16):
    """16-bit float patterns as integers in value order (sign-magnitude -> a line; -0 and +0 coincide)."""
    v = _bits(t16).to(torch.int32) & 0xFFFF
    return torch.where(v < 0x8000, v, 0x8000 - v)


@pytest.mark.parametrize("n", [1, 7, 4096 + 3])
@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", [L.PASS_QUICK_GELU, L.PASS_GELU_ERF], ids=["quick_gelu", "gelu_erf"])
def test_act_pass(kind, dt, n):
    """3 x unit normal plus 0, +-inf and NaN; sizes below one chunk and with a tail behind whole chunks; the element behind the last
    stays.  f32: 2e-5 max abs against float64.  16-bit: within one unit in the last place of the float64 value rounded to the storage
    type (one rounding of an fp32 evaluation)."""
    torch.manual_seed(n + 10 * dt + kind)
    x = 3.0 * torch.randn(n + 1)
    if n >= 7:
        x[0], x[1], x[2], x[3] = 0.0, float("inf"), float("-inf"), NAN
    x[-1] = -3.0
    x = x.to(TD[dt])
    want = _act_ref(x[:n].double(), kind)
    xd = x.to(DEV)
    p = L.ActPassParams(x=xd.data_ptr(), n=n, dtype=dt, kind=kind)
    L.check(L.lib().dc_act_pass(p, L.stream_ptr()), "dc_act_pass")
    torch.cuda.synchronize()
    got = xd.cpu()
    assert got[-1].item() == -3.0, "the element behind the last was touched"
    got = got[:n]
    fin = torch.isfinite(want)
    assert torch.equal(torch.isnan(got.float()), torch.isnan(want)), "NaN must stay NaN (and -inf, whose 0 x inf is one, become one)"
    assert torch.equal(got.double()[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)])       # +inf stays +inf
    if dt == L.DC_F32:
        err = (got.double()[fin] - want[fin]).abs().max().item() if fin.any() else 0.0
        print(f"dc_act_pass kind={kind} f32 n={n}: max abs err {err:.2e} (bound 2e-5)")
        assert err < 2e-5, err
    else:
        ulp = (_ordered(got[fin]) - _ordered(want[fin].to(TD[dt]))).abs().max().item() if fin.any() else 0
        print(f"dc_act_pass kind={kind} {NAME[dt]} n={n}: largest distance {ulp} ulp (bound 1)")
        assert ulp <= 1, ulp
