"""GPU: the kernels of the T5 encoder path — dc_attention_bias against a float64 reference computed on the device, over every output
element, and dc_rmsnorm / dc_embed_rows / dc_relu against torch in float64.

dc_attention_bias runs on the hard layout of tests/test_gpu_cross_attention.py: q | k | v rows wider than the heads with NaN in the gap,
NaN in every q / k / v row at or past the sample's length, NaN rows behind the last sample, and an output prefilled with NaN — a finite
output with exact zeros in the pad rows proves that nothing past the length was read and that every element was written.  The table is
random per head and asymmetric in the distance, so a flipped sign of k - q or a wrong head index cannot pass.
Bounds are the project's for the same arithmetic on unit-normal inputs (tests/test_gpu_cross_attention.py): 2e-5 max abs in f32, 1.5e-2 in
16-bit; dc_rmsnorm's are those tests/test_gpu_norms.py uses for LayerNorm rows (by output type)."""
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
    """One dc_attention_bias problem on the hard layout.  q / k / v [n, L, heads * d] clean host copies (rounded to the storage type)."""

    def __init__(self, dt, q, k, v, bias, lens, heads, d, use_len=True, ld_extra=64):
        self.dt, self.heads, self.d = dt, heads, d
        self.q, self.k, self.v = (t.to(TD[dt]).float() for t in (q, k, v))
        self.n, self.L, self.C = q.shape[0], q.shape[1], heads * d
        self.bias, self.lens = bias.float(), list(lens)
        n, Lq, Cc = self.n, self.L, self.C
        self.ld = 3 * Cc + ld_extra
        buf = torch.full((n * Lq + 8, self.ld), NAN)                            # 8 NaN rows behind the last sample, NaN in the gap
        for i in range(n):
            r0, ln = i * Lq, self.lens[i]
            buf[r0:r0 + ln, :Cc], buf[r0:r0 + ln, Cc:2 * Cc], buf[r0:r0 + ln, 2 * Cc:3 * Cc] = self.q[i, :ln], self.k[i, :ln], self.v[i, :ln]
        self.buf = buf.to(TD[dt]).to(DEV)
        self.bias_d = self.bias.to(DEV).contiguous()
        self.lens_d = torch.tensor(self.lens, dtype=torch.int32, device=DEV) if use_len else None

    def run(self, scale):
        out = torch.full((self.n, self.L, self.C), NAN, dtype=TD[self.dt], device=DEV)
        es, p0 = self.buf.element_size(), self.buf.data_ptr()
        p = L.AttentionBiasParams(q=p0, k=p0 + self.C * es, v=p0 + 2 * self.C * es, out=out.data_ptr(), bias=self.bias_d.data_ptr(),
                                  kv_len=None if self.lens_d is None else self.lens_d.data_ptr(), dtype=self.dt, n=self.n, L=self.L,
                                  heads=self.heads, d=self.d, ld_qkv=self.ld, ld_out=self.C, scale=scale)
        kern = L.lib().dc_attention_bias_variant(p).decode()
        L.check(L.lib().dc_attention_bias(p, L.stream_ptr()), "dc_attention_bias")
        torch.cuda.synchronize()
        return out, kern

    def ref(self, scale):
        """float64 on the device; rows at or past a sample's length are zero."""
        Lq, h, d = self.L, self.heads, self.d
        out = torch.zeros(self.n, Lq, self.C, dtype=torch.float64, device=DEV)
        pos = torch.arange(Lq, device=DEV)
        idx = pos[None, :] - pos[:, None] + Lq - 1                              # [query, key] -> k - q + L - 1
        full = self.bias.to(DEV).double()[:, idx]                               # [heads, L, L]
        for i, ln in enumerate(self.lens):
            q, k, v = (t[i, :ln].to(DEV).double().view(ln, h, d).transpose(0, 1) for t in (self.q, self.k, self.v))
            s = q @ k.transpose(-1, -2) * scale + full[:, :ln, :ln]
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
    bias = torch.randn(heads, 2 * Lq - 1)
    return Case(dt, q, k, v, bias, (Lq, 1, third), heads, d, **kw)


GRID = [(L.DC_F32, 16), (L.DC_F32, 64), (L.DC_BF16, 64), (L.DC_F16, 64)]
L_ALL = [1, 5, 16, 33, 64, 100, 130, 512]
WORST = {}


@pytest.mark.parametrize("Lq", L_ALL)
@pytest.mark.parametrize("dt,d", GRID, ids=[f"{NAME[dt]}-d{d}" for dt, d in GRID])
def test_attention_bias_grid(dt, d, Lq):
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
    WORST[(NAME[dt], d)] = max(WORST.get((NAME[dt], d), 0.0), worst)
    print(f"dc_attention_bias {NAME[dt]} d={d} L={Lq}: worst max abs err {worst:.2e} (bound {BOUND[dt]:.1e}); "
          f"worst so far for this type {WORST[(NAME[dt], d)]:.2e}")
    assert worst < BOUND[dt], worst


@pytest.mark.parametrize("dt,d", GRID, ids=[f"{NAME[dt]}-d{d}" for dt, d in GRID])
def test_attention_bias_without_lengths_and_with_unit_scale(dt, d):
    """kv_len = NULL (every sample has L rows), and T5's own call: scale = 1.0 with q pre-scaled by d^-1/2."""
    Lq, heads = 77, 2
    torch.manual_seed(d + 1)
    q, k, v = (torch.randn(3, Lq, heads * d) for _ in range(3))
    c = Case(dt, q, k, v, torch.randn(heads, 2 * Lq - 1), [Lq, Lq, Lq], heads, d, use_len=False)
    out, _ = c.run(d ** -0.5)
    e0 = c.check(out, d ** -0.5, "kv_len = NULL")
    c1 = _random_case(dt, d, Lq, heads, 33, seed=1)
    c1 = Case(dt, c1.q * d ** -0.5, c1.k, c1.v, c1.bias, c1.lens, heads, d)
    out, kern = c1.run(1.0)
    e1 = c1.check(out, 1.0, "scale = 1.0")
    print(f"dc_attention_bias {NAME[dt]} d={d} L={Lq}: kv_len = NULL {e0:.2e}, scale = 1.0 with q pre-scaled {e1:.2e} (bound {BOUND[dt]:.1e}), {kern}")
    assert e0 < BOUND[dt] and e1 < BOUND[dt], (e0, e1)


@pytest.mark.parametrize("dt", [L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("d,ld_extra", [(64, 2), (32, 64), (128, 64)])
def test_attention_bias_exact_route_in_16_bit(dt, d, ld_extra):
    """16-bit operands the matrix-core kernel does not take — rows its 16-byte loads cannot read (ld_qkv % 8 != 0), head widths 32 and
    128 — run on the exact kernel, same bound."""
    Lq, heads = 40, 2
    c = _random_case(dt, d, Lq, heads, 33, ld_extra=ld_extra)
    out, kern = c.run(d ** -0.5)
    assert kern == "fp32", kern
    err = c.check(out, d ** -0.5, f"{NAME[dt]} d={d} exact route")
    print(f"dc_attention_bias {NAME[dt]} d={d} ld_qkv={c.ld} on the exact kernel: max abs err {err:.2e} (bound {BOUND[dt]:.1e})")
    assert err < BOUND[dt], err


@pytest.mark.parametrize("dt,d", GRID, ids=[f"{NAME[dt]}-d{d}" for dt, d in GRID])
def test_attention_bias_is_deterministic_and_permutes_with_its_samples(dt, d):
    """Two launches give identical bits; permuting the samples (rows, lengths) permutes the output bit for bit."""
    Lq, heads = 100, 3
    c = _random_case(dt, d, Lq, heads, 33)
    a, b = c.run(d ** -0.5)[0], c.run(d ** -0.5)[0]
    assert torch.equal(_bits(a), _bits(b))
    perm = [2, 0, 1]
    cp = Case(dt, c.q[perm], c.k[perm], c.v[perm], c.bias, [c.lens[i] for i in perm], heads, d)
    p = cp.run(d ** -0.5)[0]
    assert torch.isfinite(p.float()).all()
    assert torch.equal(_bits(p), _bits(a[perm]))


# ---- dc_rmsnorm / dc_embed_rows / dc_relu -------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 768, 1024])
@pytest.mark.parametrize("dt,odt", [(L.DC_F32, L.DC_BF16), (L.DC_F32, L.DC_F16), (L.DC_F32, L.DC_F32), (L.DC_BF16, L.DC_BF16)],
                         ids=["f32-bf16", "f32-f16", "f32-f32", "bf16-bf16"])
def test_rmsnorm(dt, odt, C):
    """Rows of C channels, 3 samples of 7 rows, with and without row_len; rows at or past row_len hold NaN and must come out as zeros."""
    torch.manual_seed(C + 17 * dt + odt)
    n, rps, eps = 3, 7, 1e-6
    x = torch.randn(n * rps, C).to(TD[dt])
    w = (1.0 + 0.25 * torch.randn(C)).to(DEV)
    ref = lambda t: t.double() * torch.rsqrt(t.double().pow(2).mean(-1, keepdim=True) + eps) * w.double().cpu()
    for lens in (None, [7, 1, 4]):
        xin = x.clone()
        want = ref(x.float())
        if lens is not None:
            for i, ln in enumerate(lens):
                xin[i * rps + ln:(i + 1) * rps] = NAN
                want[i * rps + ln:(i + 1) * rps] = 0
        xd = xin.to(DEV)
        y = torch.full((n * rps + 1, C), NAN, dtype=TD[odt], device=DEV)        # one guard row behind
        ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
        p = L.RmsnormParams(x=xd.data_ptr(), y=y.data_ptr(), weight=w.data_ptr(), row_len=None if ld is None else ld.data_ptr(),
                            dtype=dt, out_dtype=odt, rows=n * rps, C=C, rows_per_sample=rps, eps=eps)
        L.check(L.lib().dc_rmsnorm(p, L.stream_ptr()), "dc_rmsnorm")
        torch.cuda.synchronize()
        got = y.cpu()
        assert torch.isnan(got[-1].float()).all(), "the row behind the last was written"
        got = got[:-1].double()
        assert torch.isfinite(got).all()
        if lens is not None:
            for i, ln in enumerate(lens):
                assert (got[i * rps + ln:(i + 1) * rps] == 0).all()
        err = (got - want).abs().max().item()
        print(f"dc_rmsnorm {NAME[dt]} -> {NAME[odt]} C={C} row_len={lens}: max abs err {err:.2e} (bound {LN_BOUND[odt]:.1e})")
        assert err < LN_BOUND[odt], err


@pytest.mark.parametrize("odt", [L.DC_F32, L.DC_BF16, L.DC_F16], ids=["f32", "bf16", "f16"])
def test_embed_rows_is_exact_and_clamps(odt):
    torch.manual_seed(5)
    vocab, C, rows = 48, 200, 37
    table = torch.randn(vocab, C, device=DEV)
    ids = torch.randint(0, vocab, (rows,), device=DEV)
    ids[3], ids[4] = -7, vocab + 100                                            # device data the kernel must not trust: clamped
    out = torch.full((rows + 1, C), NAN, dtype=TD[odt], device=DEV)
    p = L.EmbedRowsParams(table=table.data_ptr(), ids=ids.data_ptr(), out=out.data_ptr(), out_dtype=odt, rows=rows, C=C, vocab=vocab)
    L.check(L.lib().dc_embed_rows(p, L.stream_ptr()), "dc_embed_rows")
    torch.cuda.synchronize()
    want = table[ids.clamp(0, vocab - 1)].to(TD[odt])
    assert torch.equal(_bits(out[:rows]), _bits(want))
    assert torch.isnan(out[rows].float()).all()


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", [5, 1027, 4096 * 256 * 16 + 3])
def test_relu_is_exact_in_place(dt, n):
    """Sizes below one chunk, with a tail behind whole chunks, and beyond one sweep of the grid; the element behind the last stays."""
    torch.manual_seed(n % 1000)
    x = torch.randn(n + 1).to(TD[dt]).to(DEV)
    x[-1] = -3.0
    want = torch.relu(x[:n].double())
    p = L.ReluParams(x=x.data_ptr(), n=n, dtype=dt)
    L.check(L.lib().dc_relu(p, L.stream_ptr()), "dc_relu")
    torch.cuda.synchronize()
    assert torch.equal(x[:n].double(), want)
    assert x[-1].item() == -3.0
