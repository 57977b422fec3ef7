"""GPU: dc_cross_attention_len — cross-attention over prompts of different lengths padded to S rows — over every output element.

The layout is the hard one of tests/test_gpu_cross_attention.py (`Case`: NaN in the gaps of the rows, a NaN context nobody maps to, NaN
rows behind the last context, output prefilled with NaN) and, new here, NaN in the K and V rows at positions >= kv_len[c] of every
context: a finite output proves that no pad row was read.  The reference is attention over the prompt truncated to kv_len[c] keys
(tests/test_prompt_len_host.py shows that this is what a key mask computes): in float64 within the bounds of dc_cross_attention (2e-5
in f32, 1.5e-2 in 16-bit), and bit for bit against dc_cross_attention itself run with S = kv_len[c] on a compact copy of the context —
the kernels skip key blocks past the length and keep the surviving keys in their blocks, so the two must not differ in any bit."""
import pytest
import torch

from diffusion_classifier_amd import _lib as L
from test_gpu_cross_attention import BOUND, DEV, NAME, NAN, TD, Case, _bits, _ref64

pytestmark = pytest.mark.gpu
CASES = [(L.DC_F32, 16), (L.DC_F32, 64), (L.DC_BF16, 32), (L.DC_F16, 64), (L.DC_BF16, 96), (L.DC_F16, 128)]
IDS = [f"{NAME[dt]}-d{d}" for dt, d in CASES]
HEADS = 2


class LenCase(Case):
    """`Case` plus a key count per context; K and V rows at positions >= the (clamped) count are NaN on the device."""

    def __init__(self, dt, q, k, v, q_map, kv_map, heads, dh, kv_len):
        super().__init__(dt, q, k, v, q_map, kv_map, heads, dh)
        nc, S = k.shape[0], k.shape[1]
        assert len(kv_len) == nc
        self.kv_len = list(kv_len)
        self.eff = [min(max(ln, 1), S) for ln in self.kv_len]          # what the kernel is specified to make of a bad length
        rows = self.kvd[:nc * S].view(nc, S, self.ld_kv)
        for c, ln in enumerate(self.eff):
            rows[c, ln:] = NAN
        self.lend = torch.tensor(self.kv_len, dtype=torch.int32, device=DEV)

    def run_len(self, kv_len="own", scale=None):
        """dc_cross_attention_len; kv_len: "own" (this case's lengths), None (a NULL pointer) or an int32 device tensor."""
        scale = self.dh ** -0.5 if scale is None else scale
        kv_len = self.lend if isinstance(kv_len, str) else kv_len
        out = torch.full((self.n, self.Lq, self.C), NAN, dtype=TD[self.dt], device=DEV)
        b = self.params(out, scale)
        p = L.CrossAttentionLenParams(kv_len=None if kv_len is None else kv_len.data_ptr(),
                                      **{name: getattr(b, name) for name, _ in L.CrossAttentionParams._fields_})
        L.check(L.lib().dc_cross_attention_len(p, L.stream_ptr()), "dc_cross_attention_len")
        torch.cuda.synchronize()
        return out, L.lib().dc_cross_attention_len_variant(p).decode()

    def ref_sample(self, i):
        """float64 attention of output sample i over the first kv_len keys of its context -> [Lq, C]."""
        c, ln = self.kv_map[i], self.eff[self.kv_map[i]]
        return _ref64(self.q, self.k[:, :ln], self.v[:, :ln], [self.q_map[i]], [c], self.heads, self.dh, self.dh ** -0.5)[0]

    def compact_sample(self, i):
        """dc_cross_attention with S = kv_len[c] on a compact copy of the context's first kv_len[c] rows (same ld_q, ld_kv) -> [Lq, C]."""
        c, qs = self.kv_map[i], self.q_map[i]
        ln = self.eff[c]
        one = Case(self.dt, self.q[qs:qs + 1], self.k[c:c + 1, :ln], self.v[c:c + 1, :ln], [0], [0], self.heads, self.dh)
        assert one.ld_kv == self.ld_kv and one.ld_q == self.ld_q and one.S == ln
        return one.run()[0][0]


def _expected_kernel(dt):
    return "fp32" if dt == L.DC_F32 else "mfma"


@pytest.mark.parametrize("dt,d", CASES, ids=IDS)
def test_lengths_all_S_and_null_lengths_give_the_bits_of_cross_attention(dt, d):
    """kv_len full of S, and kv_len = NULL, on the buffers of a dc_cross_attention call: the same bits (Lq = 48: one full and one half
    query tile of the matrix-core kernel; S = 77: whole key blocks and a ragged last one)."""
    Lq, S, C = 48, 77, HEADS * d
    torch.manual_seed(100 + d)
    c = LenCase(dt, torch.randn(5, Lq, C), torch.randn(4, S, C), torch.randn(4, S, C), [0, 1, 2, 3, 4], [2, 0, 2, 0, 3], HEADS, d, [S] * 4)
    base, kern = c.run()
    assert kern == _expected_kernel(dt) and torch.isfinite(base.float()).all()
    full, kern_full = c.run_len()
    null, kern_null = c.run_len(None)
    assert kern_full == kern and kern_null == kern
    assert torch.equal(_bits(full), _bits(base)), "kv_len = S everywhere differs from dc_cross_attention"
    assert torch.equal(_bits(null), _bits(base)), "kv_len = NULL differs from dc_cross_attention"


RAGGED = [1, 31, 32, 33, 63, 64, 65, 129, 130]


@pytest.mark.parametrize("Lq", [16, 100])
@pytest.mark.parametrize("dt,d", CASES, ids=IDS)
def test_ragged_lengths(dt, d, Lq):
    """S = 130, contexts of 1 / 31 / 32 / 33 / 63 / 64 / 65 / 129 / 130 keys: one key, a ragged first block, exactly one block and one
    past it, the 32- and 64-key block boundaries from both sides, a ragged last block behind whole ones, the full length.  Context 4 is
    left out of kv_map (NaN throughout), two contexts are used twice, three query samples serve ten outputs."""
    S, C = 130, HEADS * d
    lens = RAGGED[:4] + [77] + RAGGED[4:]                              # context 4: nobody maps to it
    kv_map = [0, 1, 2, 3, 5, 6, 7, 8, 9, 2, 8]
    q_map = [0, 1, 2, 0, 1, 2, 0, 1, 2, 1, 0]
    assert sorted({lens[c] for c in kv_map}) == RAGGED
    torch.manual_seed(1000 * d + Lq)
    c = LenCase(dt, torch.randn(3, Lq, C), torch.randn(10, S, C), torch.randn(10, S, C), q_map, kv_map, HEADS, d, lens)
    out, kern = c.run_len()
    assert kern == _expected_kernel(dt)
    got = out.float().cpu()
    worst = {}
    for i, ctx in enumerate(kv_map):
        ln = lens[ctx]
        assert torch.isfinite(got[i]).all(), f"output {i} (context {ctx}, {ln} keys): non-finite — a pad row was read or an element not written"
        worst[i] = (got[i] - c.ref_sample(i)).abs().max().item()
    print(f"dc_cross_attention_len {NAME[dt]} d={d} Lq={Lq} S={S}: max abs err per output (keys) "
          + ", ".join(f"{lens[kv_map[i]]}: {e:.2e}" for i, e in worst.items()) + f" (bound {BOUND[dt]:.1e})")
    assert all(e < BOUND[dt] for e in worst.values()), worst
    for i, ctx in enumerate(kv_map):
        assert torch.equal(_bits(out[i]), _bits(c.compact_sample(i))), \
            f"output {i} (context {ctx}, {lens[ctx]} keys) differs from dc_cross_attention at S = {lens[ctx]} on the compact context"


@pytest.mark.parametrize("dt,d", CASES, ids=IDS)
def test_out_of_range_lengths_are_clamped(dt, d):
    """0, -3 and S + 5 behave as 1, 1 and S: finite, and the bits of the call with the clamped lengths."""
    Lq, S, C = 48, 77, HEADS * d
    torch.manual_seed(200 + d)
    c = LenCase(dt, torch.randn(3, Lq, C), torch.randn(3, S, C), torch.randn(3, S, C), [0, 1, 2], [0, 1, 2], HEADS, d, [0, -3, S + 5])
    assert c.eff == [1, 1, S]
    bad = c.run_len()[0]
    good = c.run_len(torch.tensor([1, 1, S], dtype=torch.int32, device=DEV))[0]
    assert torch.isfinite(bad.float()).all() and torch.isfinite(good.float()).all()
    assert torch.equal(_bits(bad), _bits(good))
    err = max((good[i].float().cpu() - c.ref_sample(i)).abs().max().item() for i in range(3))
    assert err < BOUND[dt], err


@pytest.mark.parametrize("Lq,S", [(16, 77), (100, 130)])
@pytest.mark.parametrize("dt,d", CASES, ids=IDS)
def test_len_bits_are_deterministic_and_do_not_depend_on_placement(dt, d, Lq, S):
    """Two launches give the same bits; the same (query sample, context, length) gives the same bits as output 0 of a launch of 2 and
    as output 5 of a launch of 7 with other contexts and lengths around it."""
    C = HEADS * d
    torch.manual_seed(d + Lq)
    q, k, v = torch.randn(3, Lq, C), torch.randn(4, S, C), torch.randn(4, S, C)
    lens = [S, 33, 20, 65]
    small = LenCase(dt, q, k, v, [1, 0], [2, 0], HEADS, d, lens)
    big = LenCase(dt, q, k, v, [0, 2, 2, 0, 1, 1, 2], [0, 1, 3, 3, 1, 2, 0], HEADS, d, lens)
    a, b, b2 = small.run_len()[0], big.run_len()[0], big.run_len()[0]
    assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
    assert torch.equal(_bits(b), _bits(b2))
    assert torch.equal(_bits(a[0]), _bits(b[5]))


def test_len_unaligned_rows_take_the_exact_kernel():
    """16-bit rows the 16-byte loads cannot take (ld_kv = 2C + 2) run the exact kernel with lengths, same bound."""
    dt, d, Lq, S, lens = L.DC_BF16, 32, 50, 9, [3, 7]
    torch.manual_seed(3)
    C = HEADS * d
    q, k, v = (torch.randn(2, Lq, C).to(TD[dt]).float(), torch.randn(2, S, C).to(TD[dt]).float(), torch.randn(2, S, C).to(TD[dt]).float())
    ld_kv = 2 * C + 2
    kvb = torch.full((2, S, ld_kv), NAN)
    for c, ln in enumerate(lens):
        kvb[c, :ln, :C], kvb[c, :ln, C:2 * C] = k[c, :ln], v[c, :ln]
    qd, kvd = q.to(TD[dt]).to(DEV), kvb.to(TD[dt]).to(DEV)
    lend = torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = torch.full((2, Lq, C), NAN, dtype=TD[dt], device=DEV)
    p = L.CrossAttentionLenParams(q=qd.data_ptr(), k=kvd.data_ptr(), v=kvd.data_ptr() + 2 * C, out=out.data_ptr(), kv_len=lend.data_ptr(),
                                  dtype=dt, n=2, Lq=Lq, S=S, heads=HEADS, d=d, ld_q=C, ld_kv=ld_kv, ld_out=C, scale=d ** -0.5)
    assert L.lib().dc_cross_attention_len_variant(p) == b"fp32"
    L.check(L.lib().dc_cross_attention_len(p, L.stream_ptr()), "dc_cross_attention_len")
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    for c, ln in enumerate(lens):
        err = (got[c] - _ref64(q, k[:, :ln], v[:, :ln], [c], [c], HEADS, d, d ** -0.5)[0]).abs().max().item()
        assert err < BOUND[dt], (c, ln, err)
