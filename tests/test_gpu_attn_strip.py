"""GPU: what one shared attention body (csrc/attn_strip.h) promises across its three callers, bit for bit.

dc_cross_attention, dc_attention_bias and dc_attention_causal run the same two bodies (the matrix-core strip and the exact FMA chain)
and differ in addressing, bounds, mask and score form alone, so:
  * row q of dc_attention_causal IS dc_cross_attention over the keys 0 .. q of the same rows: the same key blocks, the last of them
    masked at the same positions (key > q there, key >= S = q + 1 here), the same operations in the same order;
  * on the exact route, dc_attention_bias with an all-zero table and full lengths IS dc_cross_attention with S = Lq = L: adding +0.0 to a
    score changes at most the sign of a zero, which exp does not see.
(The matrix-core bias route is NOT claimed equal to cross-attention: its biased score form rounds differently by design.)
Inputs are finite: the causal matrix-core kernel stages the real v rows above the diagonal of its last block, where a non-finite value
would meet P = 0 as 0 x NaN (include/dcamd.h, dc_attention_causal)."""
import pytest
import torch

from diffusion_classifier_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
HEADS, LEN = 2, 70          # three key blocks of 32, the last of them ragged
# the first key; both 16-query tiles of a wave; both sides of each key-block edge; the last row
QUERIES = [0, 15, 16, 31, 32, 63, 64, 69]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Rows:
    """q | k | v rows of one sample, [LEN, 3 * heads * d + ld_extra] in one buffer (the gap holds finite values nobody may need)."""

    def __init__(self, dt, d, ld_extra=0):
        torch.manual_seed(1000 * d + dt + ld_extra)
        self.dt, self.d, self.C = dt, d, HEADS * d
        self.ld = 3 * self.C + ld_extra
        self.buf = torch.randn(LEN, self.ld).to(TD[dt]).to(DEV)
        es, p0 = self.buf.element_size(), self.buf.data_ptr()
        self.q, self.k, self.v = p0, p0 + self.C * es, p0 + 2 * self.C * es
        self.scale = d ** -0.5

    def out(self):
        return torch.full((1, LEN, self.C), float("nan"), dtype=TD[self.dt], device=DEV)

    def causal(self):
        out = self.out()
        p = L.AttentionCausalParams(q=self.q, k=self.k, v=self.v, out=out.data_ptr(), row_len=None, dtype=self.dt, n=1, L=LEN, heads=HEADS,
                                    d=self.d, ld_qkv=self.ld, ld_out=self.C, scale=self.scale)
        kern = L.lib().dc_attention_causal_variant(p).decode()
        L.check(L.lib().dc_attention_causal(p, L.stream_ptr()), "dc_attention_causal")
        return out, kern

    def bias_zero_table(self):
        out = self.out()
        table = torch.zeros(HEADS, 2 * LEN - 1, device=DEV)
        p = L.AttentionBiasParams(q=self.q, k=self.k, v=self.v, out=out.data_ptr(), bias=table.data_ptr(), kv_len=None, dtype=self.dt, n=1,
                                  L=LEN, heads=HEADS, d=self.d, ld_qkv=self.ld, ld_out=self.C, scale=self.scale)
        kern = L.lib().dc_attention_bias_variant(p).decode()
        L.check(L.lib().dc_attention_bias(p, L.stream_ptr()), "dc_attention_bias")
        torch.cuda.synchronize()
        return out, kern

    def cross(self, S):
        """All LEN queries over the keys 0 .. S - 1 of the same rows."""
        out = self.out()
        p = L.CrossAttentionParams(q=self.q, k=self.k, v=self.v, out=out.data_ptr(), q_map=None, kv_map=None, dtype=self.dt, n=1, Lq=LEN, S=S,
                                   heads=HEADS, d=self.d, ld_q=self.ld, ld_kv=self.ld, ld_out=self.C, scale=self.scale)
        kern = L.lib().dc_cross_attention_variant(p).decode()
        L.check(L.lib().dc_cross_attention(p, L.stream_ptr()), "dc_cross_attention")
        return out, kern


def _causal_rows_equal_cross_prefixes(rows, route):
    got, kern = rows.causal()
    assert kern == route, kern
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    for q in QUERIES:
        want, kern = rows.cross(q + 1)
        assert kern == route, kern
        torch.cuda.synchronize()
        assert torch.equal(_bits(got[0, q]), _bits(want[0, q])), f"row {q} of dc_attention_causal differs from dc_cross_attention over {q + 1} keys"


@pytest.mark.parametrize("dt", [L.DC_BF16, L.DC_F16], ids=["bf16", "f16"])
def test_causal_row_is_cross_attention_over_its_prefix(dt):
    """Matrix-core route, d = 64: every row of QUERIES, all three key blocks."""
    _causal_rows_equal_cross_prefixes(Rows(dt, 64), "mfma")


@pytest.mark.parametrize("dt,d,ld_extra", [(L.DC_F32, 16, 0), (L.DC_BF16, 64, 2)], ids=["f32-d16", "bf16-unaligned-ld"])
def test_causal_row_is_cross_attention_over_its_prefix_on_the_exact_route(dt, d, ld_extra):
    """The same statement for the exact kernel: fp32, and 16-bit rows the matrix-core kernel's 16-byte loads cannot take."""
    _causal_rows_equal_cross_prefixes(Rows(dt, d, ld_extra), "fp32")


@pytest.mark.parametrize("d", [16, 32])
def test_bias_with_a_zero_table_is_cross_attention_on_the_exact_route(d):
    rows = Rows(L.DC_F32, d)
    got, kern = rows.bias_zero_table()
    assert kern == "fp32", kern
    want, kern = rows.cross(LEN)
    assert kern == "fp32", kern
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    assert torch.equal(_bits(got), _bits(want))
