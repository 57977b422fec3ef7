"""GPU: dc_cross_attention / dc_cross_attention_len at head width 160 (Stable Diffusion 1.x: 1280 channels in 8 heads) against a float64
reference computed on the device, over every output element — the strip kernel's D = 160 instance ("mfma": 16-bit, aligned rows), the
exact kernel at SW = 20 ("fp32"), and the self form that StableDiffusionUNet's attn1 launches (q / k / v the three column offsets of a
fused QKV tensor, Lq = S = L, no maps).

The layout is the hard one of tests/test_gpu_cross_attention.py, restated here: q rows and K | V rows wider than the heads with NaN in the
gap, NaN behind the S-th row of every context (a gap between contexts, NaN rows behind the last), a context nobody maps to made of NaN,
and an output with a sentinel in its row padding and behind its last row — a finite, correct output with the sentinel intact proves that
every element was written, nothing else was, and nothing outside the S rows of the mapped context was read.  Bounds: that file's, the
project's values for every other width on unit-normal inputs — 2e-5 max abs error in f32, 1.5e-2 in 16-bit."""
import pytest
import torch

from diffusion_classifier_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
NAME = {L.DC_F32: "f32", L.DC_BF16: "bf16", L.DC_F16: "f16"}
DTYPES = [L.DC_F32, L.DC_BF16, L.DC_F16]
BOUND = {L.DC_F32: 2e-5, L.DC_BF16: 1.5e-2, L.DC_F16: 1.5e-2}
NAN, SENTINEL = float("nan"), 7.0
D, HEADS, C = 160, 2, 320
LQS, SS = [1, 31, 32, 33, 100], [1, 7, 31, 32, 33, 77, 130]
KB = 32                                  # keys per block of the D = 160 instance (csrc/attention_cross.hip cross_kb)


def _ref64(q, k, v, q_map, kv_map, scale, lens=None):
    """q [nq, Lq, C], k / v [nc, S, C] (f32, already rounded to the storage type) -> float64 attention [n, Lq, C]; lens: keys per context."""
    n, Lq, S = len(kv_map), q.shape[1], k.shape[1]
    qq = q.to(DEV).double()[torch.tensor(q_map)].view(n, Lq, HEADS, D).transpose(1, 2)
    kk = k.to(DEV).double()[torch.tensor(kv_map)].view(n, S, HEADS, D).transpose(1, 2)
    vv = v.to(DEV).double()[torch.tensor(kv_map)].view(n, S, HEADS, D).transpose(1, 2)
    s = qq @ kk.transpose(-1, -2) * scale
    if lens is not None:
        ln = torch.tensor([lens[c] for c in kv_map], device=DEV)
        s = s.masked_fill((torch.arange(S, device=DEV)[None, :] >= ln[:, None])[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ vv).transpose(1, 2).reshape(n, Lq, C).float().cpu()


class Case:
    """Device buffers of one problem on the hard layout; `q`, `k`, `v` are the clean host copies (rounded to the storage type)."""

    def __init__(self, dt, q, k, v, q_map, kv_map, gap_rows=3, lens=None):
        self.dt = dt
        self.q, self.k, self.v = (t.to(TD[dt]).float() for t in (q, k, v))
        nq, Lq, _ = q.shape
        nc, S, _ = k.shape
        self.n, self.Lq, self.S, self.nc = len(kv_map), Lq, S, nc
        self.q_map, self.kv_map = list(q_map), list(kv_map)
        self.ld_q, self.ld_kv, self.ld_out = C + 32, 2 * C + 64, C + 8
        qb = torch.full((nq, Lq, self.ld_q), NAN)
        qb[..., :C] = self.q
        # the kernel's contexts lie S rows apart: NaN "behind the S-th row of every context" is the next context's unmapped rows where
        # there is one (below) and gap_rows NaN rows behind the last
        kvb = torch.full((nc * S + gap_rows, self.ld_kv), NAN)
        kvb[:nc * S, :C] = self.k.reshape(nc * S, C)
        kvb[:nc * S, C:2 * C] = self.v.reshape(nc * S, C)
        for c in set(range(nc)) - set(kv_map):                               # a context nobody maps to: NaN throughout
            kvb[c * S:(c + 1) * S] = NAN
        for c, ln in enumerate(lens or ()):                                  # the pad rows of a short prompt: NaN
            kvb[c * S + ln:(c + 1) * S] = NAN
        self.qd, self.kvd = qb.to(TD[dt]).to(DEV), kvb.to(TD[dt]).to(DEV)
        ident = lambda m: m == list(range(len(m)))
        self.qm = None if ident(self.q_map) and nq == self.n else torch.tensor(self.q_map, dtype=torch.int32, device=DEV)
        self.km = None if ident(self.kv_map) and nc == self.n else torch.tensor(self.kv_map, dtype=torch.int32, device=DEV)

    def _fields(self, out, scale):
        es = self.qd.element_size()
        return dict(q=self.qd.data_ptr(), k=self.kvd.data_ptr(), v=self.kvd.data_ptr() + C * es, out=out.data_ptr(),
                    q_map=None if self.qm is None else self.qm.data_ptr(), kv_map=None if self.km is None else self.km.data_ptr(),
                    dtype=self.dt, n=self.n, Lq=self.Lq, S=self.S, heads=HEADS, d=D, ld_q=self.ld_q, ld_kv=self.ld_kv, ld_out=self.ld_out, scale=scale)

    def run(self, scale=D ** -0.5, lens=None):
        """-> (out [n, Lq, C] in the storage type, the kernel's name); lens: per-context key counts -> dc_cross_attention_len."""
        buf = torch.full((self.n * self.Lq + 4, self.ld_out), SENTINEL, dtype=TD[self.dt], device=DEV)
        lib = L.lib()
        if lens is None:
            p = L.CrossAttentionParams(**self._fields(buf, scale))
            L.check(lib.dc_cross_attention(p, L.stream_ptr()), "dc_cross_attention")
            kern = lib.dc_cross_attention_variant(p).decode()
        else:
            ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
            p = L.CrossAttentionLenParams(**self._fields(buf, scale), kv_len=ld.data_ptr())
            L.check(lib.dc_cross_attention_len(p, L.stream_ptr()), "dc_cross_attention_len")
            kern = lib.dc_cross_attention_len_variant(p).decode()
        torch.cuda.synchronize()
        assert (buf[self.n * self.Lq:] == SENTINEL).all() and (buf[:, C:] == SENTINEL).all(), "a write outside the output's rows"
        return buf[:self.n * self.Lq, :C].reshape(self.n, self.Lq, C).clone(), kern

    def ref(self, scale=D ** -0.5, lens=None):
        return _ref64(self.q, self.k, self.v, self.q_map, self.kv_map, scale, lens)


def _case(dt, Lq, S, maps, seed=0):
    torch.manual_seed(160000 + 131 * Lq + S + seed)
    if maps == "identity":
        nq = nc = 3
        q_map, kv_map = [0, 1, 2], [0, 1, 2]
    else:                      # "shared": one pair's queries read by all three units, the contexts permuted, one (number 1) left out as NaN
        nq, nc = 1, 4
        q_map, kv_map = [0, 0, 0], [3, 0, 2]
    return Case(dt, torch.randn(nq, Lq, C), torch.randn(nc, S, C), torch.randn(nc, S, C), q_map, kv_map)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("maps", ["identity", "shared"])
@pytest.mark.parametrize("dt", DTYPES, ids=[NAME[d] for d in DTYPES])
def test_cross_attention_160_grid(dt, maps):
    """n = 3, 2 heads, every (Lq, S) of the grid: one query, a ragged / whole / just-over 32-query tile, more than one workgroup; one key,
    ragged single key blocks, a whole block, blocks and a ragged tail (S = 130: five blocks)."""
    worst = {}
    for Lq in LQS:
        for S in SS:
            c = _case(dt, Lq, S, maps)
            out, kern = c.run()
            assert kern == ("fp32" if dt == L.DC_F32 else "mfma"), kern
            got = out.float().cpu()
            assert torch.isfinite(got).all(), f"Lq={Lq} S={S}: non-finite output (unwritten element or a read outside the context)"
            worst[(Lq, S)] = (got - c.ref()).abs().max().item()
    top = max(worst, key=worst.get)
    print(f"dc_cross_attention {NAME[dt]} d=160 {maps}: worst max abs err {worst[top]:.2e} at (Lq, S) = {top} (bound {BOUND[dt]:.1e})")
    assert all(e < BOUND[dt] for e in worst.values()), {k: e for k, e in worst.items() if e >= BOUND[dt]}


@pytest.mark.parametrize("S", [33, 77, 130])
@pytest.mark.parametrize("dt", DTYPES, ids=[NAME[d] for d in DTYPES])
def test_cross_attention_len_160_equals_a_launch_of_that_length(dt, S):
    """Per-context lengths {1, S, a mid-block value, an exact block end}: within the bound of the masked float64 reference, and the bits of
    every output are those of dc_cross_attention on a context of exactly that many rows."""
    lens = [1, S, KB + 13 if S > KB + 13 else S - 5, (S // KB) * KB]
    Lq = 33
    torch.manual_seed(1600 + S)
    q, k, v = torch.randn(2, Lq, C), torch.randn(4, S, C), torch.randn(4, S, C)
    q_map, kv_map = [0, 1, 1, 0, 1], [3, 0, 2, 1, 1]
    c = Case(dt, q, k, v, q_map, kv_map, lens=lens)
    out, kern = c.run(lens=lens)
    assert kern == ("fp32" if dt == L.DC_F32 else "mfma")
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    err = (got - c.ref(lens=lens)).abs().max().item()
    print(f"dc_cross_attention_len {NAME[dt]} d=160 S={S} lens={lens}: max abs err {err:.2e} (bound {BOUND[dt]:.1e})")
    assert err < BOUND[dt], err
    for i, (qs, cs) in enumerate(zip(q_map, kv_map)):
        ln = lens[cs]
        one, _ = Case(dt, q[qs:qs + 1], k[cs:cs + 1, :ln], v[cs:cs + 1, :ln], [0], [0]).run()
        assert torch.equal(_bits(out[i]), _bits(one[0])), (i, ln)
    # every length S: the plain launch
    whole = Case(dt, q, k, v, q_map, kv_map)
    assert torch.equal(_bits(whole.run(lens=[S] * 4)[0]), _bits(whole.run()[0]))


@pytest.mark.parametrize("Lseq", [16, 64, 256])
@pytest.mark.parametrize("dt", DTYPES, ids=[NAME[d] for d in DTYPES])
def test_self_attention_160_through_the_fused_qkv_tensor(dt, Lseq):
    """The self form: one [n, L, 3 * 2 * 160] tensor, q / k / v its three column offsets, Lq = S = L, ld_q = ld_kv = 3 C, no maps."""
    n = 3
    torch.manual_seed(16000 + Lseq)
    qkv = torch.randn(n, Lseq, 3 * C).to(TD[dt])
    qkvd = qkv.to(DEV)
    out = torch.full((n * Lseq + 4, C), SENTINEL, dtype=TD[dt], device=DEV)
    es = qkvd.element_size()
    p = L.CrossAttentionParams(q=qkvd.data_ptr(), k=qkvd.data_ptr() + C * es, v=qkvd.data_ptr() + 2 * C * es, out=out.data_ptr(), q_map=None,
                               kv_map=None, dtype=dt, n=n, Lq=Lseq, S=Lseq, heads=HEADS, d=D, ld_q=3 * C, ld_kv=3 * C, ld_out=C, scale=D ** -0.5)
    assert L.lib().dc_cross_attention_variant(p).decode() == ("fp32" if dt == L.DC_F32 else "mfma")
    L.check(L.lib().dc_cross_attention(p, L.stream_ptr()), "dc_cross_attention")
    torch.cuda.synchronize()
    assert (out[n * Lseq:] == SENTINEL).all()
    got = out[:n * Lseq].reshape(n, Lseq, C).float().cpu()
    f = qkv.float()
    ref = _ref64(f[..., :C], f[..., C:2 * C], f[..., 2 * C:], list(range(n)), list(range(n)), D ** -0.5)
    err = (got - ref).abs().max().item()
    print(f"dc_cross_attention {NAME[dt]} d=160 self form L={Lseq}: max abs err {err:.2e} (bound {BOUND[dt]:.1e})")
    assert torch.isfinite(got).all() and err < BOUND[dt], err


@pytest.mark.parametrize("dt", [L.DC_BF16, L.DC_F16], ids=["bf16", "f16"])
def test_cross_attention_160_with_large_logits(dt):
    """As test_cross_attention_with_large_logits: q and k scaled by 5 (logits beyond 60), S = Lq = 256 keys, that test's bounds (the
    softmax is close to one-hot, the error is that of rounding p and v to the storage type: 4e-2 in bf16, 6e-3 in f16)."""
    Lq = 256
    torch.manual_seed(1605)
    c = Case(dt, torch.randn(2, Lq, C) * 5.0, torch.randn(2, Lq, C) * 5.0, torch.randn(2, Lq, C), [0, 1], [0, 1])
    lg = c.q[..., :D] @ c.k[..., :D].transpose(1, 2) * D ** -0.5
    assert lg.amax(-1).max().item() > 60
    out, kern = c.run()
    got = out.float().cpu()
    assert kern == "mfma" and torch.isfinite(got).all()
    err = (got - c.ref()).abs().max().item()
    bound = {L.DC_BF16: 4e-2, L.DC_F16: 6e-3}[dt]
    print(f"dc_cross_attention {NAME[dt]} d=160 Lq=S={Lq}, large logits: max abs err {err:.2e} (bound {bound:.1e})")
    assert err < bound, err


@pytest.mark.parametrize("dt", DTYPES, ids=[NAME[d] for d in DTYPES])
def test_cross_attention_160_is_deterministic_and_placement_free(dt):
    """Two launches give the same bits; the same (query sample, context) gives the same bits as output 0 of a launch of 2 and as output 5
    of a launch of 7 with other contexts around it."""
    Lq, S = 100, 77
    torch.manual_seed(1607)
    q, k, v = torch.randn(3, Lq, C), torch.randn(4, S, C), torch.randn(4, S, C)
    small = Case(dt, q, k, v, [1, 0], [2, 0])
    big = Case(dt, q, k, v, [0, 2, 2, 0, 1, 1, 2], [0, 1, 3, 3, 1, 2, 0])
    a, a2, b = small.run()[0], small.run()[0], big.run()[0]
    assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
    assert torch.equal(_bits(a), _bits(a2))
    assert torch.equal(_bits(a[0]), _bits(b[5]))
