"""GPU: dc_cross_attention against a float64 reference computed on the device, over every output element.

Every case runs on the hard layout: q rows and K | V rows wider than the heads with NaN in the gap, an unreferenced context made of NaN
(where the maps leave one out), NaN rows behind the last context, and an output prefilled with NaN — a finite, correct output proves
that every element was written and that nothing outside the S rows of the mapped context was read (the ragged last key block included).
Bounds are those of tests/test_gpu_head_width.py for dc_attention on unit-normal inputs: 1.5e-2 max abs error in 16-bit, 2e-5 in f32."""
import pytest
import torch

from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
NAME = {L.DC_F32: "f32", L.DC_BF16: "bf16", L.DC_F16: "f16"}
LOWP = [L.DC_BF16, L.DC_F16]
BOUND = {L.DC_F32: 2e-5, L.DC_BF16: 1.5e-2, L.DC_F16: 1.5e-2}
NAN = float("nan")


def _ref64(q, k, v, q_map, kv_map, heads, dh, scale):
    """q [nq, Lq, heads*dh], k / v [nc, S, heads*dh] (f32, already rounded to the storage type) -> float64 attention [n, Lq, heads*dh]."""
    n, Lq, S = len(kv_map), q.shape[1], k.shape[1]
    qq = q.to(DEV).double()[torch.tensor(q_map)].view(n, Lq, heads, dh).transpose(1, 2)
    kk = k.to(DEV).double()[torch.tensor(kv_map)].view(n, S, heads, dh).transpose(1, 2)
    vv = v.to(DEV).double()[torch.tensor(kv_map)].view(n, S, heads, dh).transpose(1, 2)
    o = torch.softmax(qq @ kk.transpose(-1, -2) * scale, -1) @ vv
    return o.transpose(1, 2).reshape(n, Lq, heads * dh).float().cpu()


class Case:
    """Device buffers of one problem on the hard layout; `q`, `k`, `v` are the clean host copies (rounded to the storage type)."""

    def __init__(self, dt, q, k, v, q_map, kv_map, heads, dh, gap=True):
        self.dt, self.heads, self.dh = dt, heads, dh
        self.q, self.k, self.v = (t.to(TD[dt]).float() for t in (q, k, v))
        nq, Lq, C = q.shape
        nc, S, _ = k.shape
        self.n, self.Lq, self.S, self.C = len(kv_map), Lq, S, C
        self.q_map, self.kv_map = list(q_map), list(kv_map)
        self.ld_q = C + (32 if gap else 0)
        self.ld_kv = 2 * C + (64 if gap else 0)
        qb = torch.full((nq, Lq, self.ld_q), NAN)
        qb[..., :C] = self.q
        kvb = torch.full((nc * S + 8, self.ld_kv), NAN)                      # 8 NaN rows behind the last context
        kvb[:nc * S, :C] = self.k.reshape(nc * S, C)
        kvb[:nc * S, C:2 * C] = self.v.reshape(nc * S, C)
        for c in set(range(nc)) - set(kv_map):                               # a context nobody maps to: NaN throughout
            kvb[c * S:(c + 1) * S] = NAN
        self.qd, self.kvd = qb.to(TD[dt]).to(DEV), kvb.to(TD[dt]).to(DEV)
        ident = lambda m: m == list(range(len(m)))
        self.qm = None if ident(self.q_map) and nq == self.n else torch.tensor(self.q_map, dtype=torch.int32, device=DEV)
        self.km = None if ident(self.kv_map) and nc == self.n else torch.tensor(self.kv_map, dtype=torch.int32, device=DEV)

    def params(self, out, scale):
        es = self.qd.element_size()
        return L.CrossAttentionParams(q=self.qd.data_ptr(), k=self.kvd.data_ptr(), v=self.kvd.data_ptr() + self.C * es, out=out.data_ptr(),
                                      q_map=None if self.qm is None else self.qm.data_ptr(),
                                      kv_map=None if self.km is None else self.km.data_ptr(), dtype=self.dt, n=self.n, Lq=self.Lq,
                                      S=self.S, heads=self.heads, d=self.dh, ld_q=self.ld_q, ld_kv=self.ld_kv, ld_out=self.C, scale=scale)

    def run(self, scale=None):
        scale = self.dh ** -0.5 if scale is None else scale
        out = torch.full((self.n, self.Lq, self.C), NAN, dtype=TD[self.dt], device=DEV)
        p = self.params(out, scale)
        L.check(L.lib().dc_cross_attention(p, L.stream_ptr()), "dc_cross_attention")
        torch.cuda.synchronize()
        return out, L.lib().dc_cross_attention_variant(p).decode()

    def ref(self, scale=None):
        return _ref64(self.q, self.k, self.v, self.q_map, self.kv_map, self.heads, self.dh, self.dh ** -0.5 if scale is None else scale)


def _random_case(dt, d, Lq, S, maps="identity", heads=2, seed=0):
    torch.manual_seed(1000 * d + 7 * Lq + S + seed)
    if maps == "identity":
        nq = nc = 2
        q_map, kv_map = [0, 1], [0, 1]
    elif maps == "many_to_one_q":            # the class-shared trunk: several units read one pair's queries
        nq, nc = 2, 5
        q_map, kv_map = [0, 0, 1, 1, 0], [0, 1, 2, 3, 4]
    else:                                    # "kv_repeats": contexts reused, one (number 1) left out and made of NaN
        nq, nc = 5, 4
        q_map, kv_map = [0, 1, 2, 3, 4], [2, 0, 2, 0, 3]
    C = heads * d
    return Case(dt, torch.randn(nq, Lq, C), torch.randn(nc, S, C), torch.randn(nc, S, C), q_map, kv_map, heads, d)


GRID = [(dt, d) for dt in (L.DC_F32, L.DC_BF16, L.DC_F16) for d in (32, 64, 96, 128)] + [(L.DC_F32, 16)]
S_ALL = [1, 2, 7, 16, 77, 128, 130, 512]


@pytest.mark.parametrize("Lq", [16, 64, 256, 1000, 4096])
@pytest.mark.parametrize("dt,d", GRID, ids=[f"{NAME[dt]}-d{d}" for dt, d in GRID])
def test_cross_attention_grid(dt, d, Lq):
    """dtype x head dim x query count, every context length S of the grid (1 ... 512: one key, a ragged single block, whole blocks, a
    ragged last block behind whole ones)."""
    worst = {}
    for S in S_ALL:
        c = _random_case(dt, d, Lq, S)
        out, kern = c.run()
        assert kern == ("fp32" if dt == L.DC_F32 else "mfma"), kern
        got = out.float().cpu()
        assert torch.isfinite(got).all(), f"S={S}: non-finite output (unwritten element or a read outside the context)"
        worst[S] = (got - c.ref()).abs().max().item()
    print(f"dc_cross_attention {NAME[dt]} d={d} Lq={Lq}: max abs err per S " + ", ".join(f"{S}: {e:.2e}" for S, e in worst.items())
          + f" (bound {BOUND[dt]:.1e})")
    assert all(e < BOUND[dt] for e in worst.values()), worst


@pytest.mark.parametrize("maps", ["many_to_one_q", "kv_repeats"])
@pytest.mark.parametrize("S", [7, 77, 130])
@pytest.mark.parametrize("dt,d", [(L.DC_F32, 16), (L.DC_F32, 64), (L.DC_BF16, 32), (L.DC_F16, 64), (L.DC_BF16, 96), (L.DC_F16, 128)])
def test_cross_attention_maps(dt, d, S, maps):
    """q_map many-to-one; kv_map with repeats and an unreferenced context filled with NaN (directly behind a referenced one: the rows a
    ragged key block must not read)."""
    for Lq in (16, 100):
        c = _random_case(dt, d, Lq, S, maps)
        got = c.run()[0].float().cpu()
        assert torch.isfinite(got).all()
        err = (got - c.ref()).abs().max().item()
        print(f"dc_cross_attention {NAME[dt]} d={d} Lq={Lq} S={S} {maps}: max abs err {err:.2e} (bound {BOUND[dt]:.1e})")
        assert err < BOUND[dt], err


def test_cross_attention_unaligned_rows_take_the_exact_kernel():
    """16-bit rows the 16-byte loads cannot take (ld_kv not a multiple of 8 elements) run on the exact kernel, same bound."""
    dt, d, heads, Lq, S = L.DC_BF16, 32, 2, 50, 9
    torch.manual_seed(3)
    C = heads * d
    q, k, v = (torch.randn(2, Lq, C).to(TD[dt]).float(), torch.randn(2, S, C).to(TD[dt]).float(), torch.randn(2, S, C).to(TD[dt]).float())
    ld_kv = 2 * C + 2
    kvb = torch.full((2 * S, ld_kv), NAN)
    kvb[:, :C], kvb[:, C:2 * C] = k.reshape(2 * S, C), v.reshape(2 * S, C)
    qd, kvd = q.to(TD[dt]).to(DEV), kvb.to(TD[dt]).to(DEV)
    out = torch.full((2, Lq, C), NAN, dtype=TD[dt], device=DEV)
    p = L.CrossAttentionParams(q=qd.data_ptr(), k=kvd.data_ptr(), v=kvd.data_ptr() + 2 * C, out=out.data_ptr(), dtype=dt, n=2, Lq=Lq, S=S,
                               heads=heads, d=d, ld_q=C, ld_kv=ld_kv, ld_out=C, scale=d ** -0.5)
    assert L.lib().dc_cross_attention_variant(p) == b"fp32"
    L.check(L.lib().dc_cross_attention(p, L.stream_ptr()), "dc_cross_attention")
    torch.cuda.synchronize()
    err = (out.float().cpu() - _ref64(q, k, v, [0, 1], [0, 1], heads, d, d ** -0.5)).abs().max().item()
    assert err < BOUND[dt], err


@pytest.mark.parametrize("dt", LOWP)
@pytest.mark.parametrize("Lq", [256, 1000])
def test_cross_attention_with_large_logits(dt, Lq):
    """As test_flash_head_dim_96_with_large_logits: q and k scaled by 5 (logits beyond 60), S = Lq keys, that test's bounds."""
    d, heads = 96, 2
    torch.manual_seed(960 + Lq)
    C = heads * d
    c = Case(dt, torch.randn(2, Lq, C) * 5.0, torch.randn(2, Lq, C) * 5.0, torch.randn(2, Lq, C), [0, 1], [0, 1], heads, d)
    lg = c.q[..., :d] @ c.k[..., :d].transpose(1, 2) * d ** -0.5
    assert lg.amax(-1).max().item() > 60
    out, kern = c.run()
    got = out.float().cpu()
    assert kern == "mfma" and torch.isfinite(got).all()
    err = (got - c.ref()).abs().max().item()
    bound = {L.DC_BF16: 4e-2, L.DC_F16: 6e-3}[dt]
    print(f"dc_cross_attention {NAME[dt]} d=96 Lq=S={Lq}, large logits: max abs err {err:.2e} (bound {bound:.1e})")
    assert err < bound, err


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dt,d", [(L.DC_F32, 64), (L.DC_BF16, 32), (L.DC_F16, 64), (L.DC_BF16, 96), (L.DC_F16, 128)])
def test_cross_attention_is_deterministic(dt, d):
    """Two launches give the same bits."""
    c = _random_case(dt, d, 1000, 77, "kv_repeats")
    a, b = c.run()[0], c.run()[0]
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dt,d", [(L.DC_F32, 64), (L.DC_F32, 16), (L.DC_BF16, 32), (L.DC_F16, 64), (L.DC_BF16, 96), (L.DC_F16, 128)])
@pytest.mark.parametrize("Lq,S", [(16, 77), (100, 130)])
def test_cross_attention_bits_do_not_depend_on_placement(dt, d, Lq, S):
    """The same (query sample, context) gives the same bits as output 0 of a launch of 2 and as output 5 of a launch of 7 with other
    contexts around it."""
    heads = 2
    C = heads * d
    torch.manual_seed(d + Lq)
    q, k, v = torch.randn(3, Lq, C), torch.randn(4, S, C), torch.randn(4, S, C)
    small = Case(dt, q, k, v, [1, 0], [2, 0], heads, d)
    big = Case(dt, q, k, v, [0, 2, 2, 0, 1, 1, 2], [0, 1, 3, 3, 1, 2, 0], heads, d)
    a, b = small.run()[0], big.run()[0]
    assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
    assert torch.equal(_bits(a[0]), _bits(b[5]))


@pytest.mark.parametrize("dt", [L.DC_F32, L.DC_BF16, L.DC_F16])
@pytest.mark.parametrize("d", [48, 80])
@pytest.mark.parametrize("Lq,S", [(64, 77), (256, 5)])
def test_cross_attention_padded_heads_equal_true_width(dt, d, Lq, S):
    """Heads of 48 / 80 channels zero-padded to 64 / 96 as the packed weights produce them, scale d^-1/2: the real columns are the
    attention at width d, the pad columns exactly 0."""
    dp, heads = E.padded_head_dim(d), 4
    torch.manual_seed(d + Lq + S)
    C, Cp = heads * d, heads * dp
    q, k, v = (t.to(TD[dt]).float() for t in (torch.randn(2, Lq, C), torch.randn(2, S, C), torch.randn(2, S, C)))
    pad = lambda t: E.pad_head_rows(t.reshape(-1, C).t(), d, dp).t().reshape(t.shape[0], t.shape[1], Cp).contiguous()
    c = Case(dt, pad(q), pad(k), pad(v), [0, 1], [0, 1], heads, dp)
    got = c.run(scale=d ** -0.5)[0].float().cpu().reshape(2, Lq, heads, dp)
    assert (got[..., d:] == 0).all()
    err = (got[..., :d].reshape(2, Lq, C) - _ref64(q, k, v, [0, 1], [0, 1], heads, d, d ** -0.5)).abs().max().item()
    print(f"dc_cross_attention {NAME[dt]} d={d} -> {dp} Lq={Lq} S={S}: max abs err {err:.2e} (bound {BOUND[dt]:.1e})")
    assert err < BOUND[dt], err
