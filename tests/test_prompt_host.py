"""CPU: contexts of several tokens — the test-side oracle's sanity properties, the C-ABI of dc_cross_attention (struct order, argument
validation and routing without a GPU) and the host logic of encoder_type='prompt' on a plain nn.Module backbone."""
import os

import pytest
import torch

import diffusion_classifier_amd as dca
import oracle
from diffusion_classifier_amd import _lib as L
from prompt_oracle import PromptOracleClassifier, PromptOracleUNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(pred_param="eps", schedule="cosine", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, n_stages=1,
           evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32", image_size=32, noise_d=32)


def relerr(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _randomise_vectors(m):
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)


def _oracles():
    kw = dca.small_unet_kwargs()
    torch.manual_seed(7)
    stock = oracle.OracleUNetCondition2D(**kw)
    _randomise_vectors(stock)
    po = PromptOracleUNet(**kw)
    po.load_state_dict(stock.state_dict())
    return kw, stock, po


def test_one_token_equals_the_stock_oracle():
    """S = 1: softmax over one key is 1, so the full block equals the stock oracle's shortcut."""
    kw, stock, po = _oracles()
    torch.manual_seed(8)
    x, lam, emb = torch.randn(2, 3, 32, 32) * 0.5, torch.tensor([0.5, -2.0]), torch.randn(2, 1, kw["encoder_hid_dim"])
    with torch.no_grad():
        r = relerr(po(x, lam, encoder_hidden_states=emb), stock(x, lam, encoder_hidden_states=emb))
    print(f"one token vs the stock oracle: rel-L2 {r:.2e} (bound 5e-6)")
    assert r < 5e-6, r


def test_copies_of_one_token_equal_that_token():
    """7 copies of one token: equal keys give a uniform softmax over equal values, i.e. the one-token result."""
    kw, stock, po = _oracles()
    torch.manual_seed(9)
    x, lam, emb = torch.randn(2, 3, 32, 32) * 0.5, torch.tensor([0.5, -2.0]), torch.randn(2, 1, kw["encoder_hid_dim"])
    with torch.no_grad():
        r = relerr(po(x, lam, encoder_hidden_states=emb.expand(2, 7, -1).contiguous()), stock(x, lam, encoder_hidden_states=emb))
    print(f"7 copies of one token vs that token: rel-L2 {r:.2e} (bound 5e-6)")
    assert r < 5e-6, r


def test_cross_attention_struct_matches_header_field_order():
    hdr = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    assert "DC_OP_CROSS_ATTENTION = 9" in hdr and L.OP_CROSS_ATTENTION == 9
    assert {"dc_cross_attention", "dc_cross_attention_variant"} <= set(L.EXPORTS)
    assert L.lib().dc_abi_version() == 5


def _params(**kw):
    ptr = 1 << 20
    base = dict(q=ptr, k=ptr, v=ptr, out=ptr, dtype=L.DC_BF16, n=2, Lq=64, S=77, heads=8, d=32, ld_q=256, ld_kv=512, ld_out=256,
                scale=32 ** -0.5)
    base.update(kw)
    return L.CrossAttentionParams(**base)


def test_cross_attention_validation_and_routes_need_no_gpu():
    lib = L.lib()
    variant = lambda **kw: lib.dc_cross_attention_variant(_params(**kw)).decode()
    for dt in (L.DC_BF16, L.DC_F16):
        for d in (32, 64, 96, 128):
            assert variant(dtype=dt, d=d, ld_q=8 * d, ld_kv=16 * d, ld_out=8 * d) == "mfma"
        assert variant(dtype=dt, d=16) == "fp32"
        assert variant(dtype=dt, q=(1 << 20) + 2) == "fp32"          # rows the 16-byte loads cannot take
        assert variant(dtype=dt, ld_kv=516) == "fp32"
    for d in (16, 32, 64, 96, 128):
        assert variant(dtype=L.DC_F32, d=d, ld_q=8 * d, ld_kv=16 * d, ld_out=8 * d) == "fp32"
    for bad, word, code in ((dict(S=0), b"S=0", -2), (dict(scale=0.0), b"scale", -1), (dict(scale=-1.0), b"scale", -1),
                            (dict(d=48), b"head dim 48", -2), (dict(q=None), b"null", -1), (dict(ld_kv=128), b"ld", -2),
                            (dict(dtype=7), b"dtype", -3), (dict(Lq=0), b"Lq", -2)):
        assert variant(**bad) == "invalid", bad
        assert lib.dc_cross_attention(_params(**bad), None) == code, bad
        assert word in lib.dc_last_error(), (bad, lib.dc_last_error())
    # the plan runner knows the op: a refused cross-attention is reported with its index and kind
    p = _params(S=0)
    import ctypes as C
    ops = (L.Op * 1)()
    ops[0].kind, ops[0].params = L.OP_CROSS_ATTENTION, C.cast(C.pointer(p), C.c_void_p)
    assert lib.dc_run_plan(ops, 1, None) == -2
    assert b"op 0 (kind 9)" in lib.dc_last_error() and b"S=0" in lib.dc_last_error()


def _prompt_pair(S, classes=3):
    kw, _, po = _oracles()
    cfg = dict(CFG, encoder_type="prompt", prompt_tokens=S, classes=classes)
    dc = dca.DiffusionClassifier(po, dca.Config(**cfg))
    oc = PromptOracleClassifier(po, oracle.AttrBag(**cfg))
    oc.encoder.load_state_dict(dc.encoder.state_dict())
    return kw, dc, oc


def test_prompt_encoder_shapes_values_and_checkpoint_name(tmp_path):
    kw, dc, _ = _prompt_pair(5)
    w = dc.encoder.weight
    assert isinstance(w, torch.nn.Parameter) and tuple(w.shape) == (3 + 1, 5, kw["encoder_hid_dim"])
    assert list(dc.encoder.state_dict()) == ["weight"] and dc.null_token == 3
    ids = torch.tensor([2, 0, 3])
    e = dc.encode_text_prompt(ids)
    assert tuple(e.shape) == (3, 5, kw["encoder_hid_dim"]) and torch.equal(e, w[ids])
    dc.save_checkpoint(str(tmp_path))
    dc2 = _prompt_pair(5)[1]
    with torch.no_grad():
        dc2.encoder.weight.zero_()
    dc2.load_checkpoint(str(tmp_path))
    assert torch.equal(dc2.encoder.weight, w)
    with pytest.raises(AssertionError):
        dca.DiffusionClassifier(_oracles()[2], dca.Config(**dict(CFG, encoder_type="prompt", classes=3)))
    with pytest.raises(NotImplementedError, match="prompt"):
        dca.DiffusionClassifier(_oracles()[2], dca.Config(**dict(CFG, encoder_type="t5", classes=3)))


@pytest.mark.parametrize("S", [1, 4])
def test_prompt_classify_on_a_foreign_backbone_reproduces_the_oracle_loop(S):
    """encoder_type='prompt' through _ForeignRunner (a plain nn.Module backbone, eager torch): the errors and labels of the test-side
    oracle's loop, which hands [BS, S, hid] prompts to the backbone as the reference's loop does."""
    kw, dc, oc = _prompt_pair(S)
    torch.manual_seed(11)
    BS, T = 2, 2
    x = torch.rand(BS, 3, 32, 32) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 3, 32, 32)
    ref_l, ref_e = oc.classify(x, t=t, eps=eps, return_errors=True)
    got_l, got_e = dc.classify(x, t=t, eps=eps, return_errors=True)
    assert torch.isfinite(got_e).all()
    torch.testing.assert_close(got_e, ref_e, rtol=1e-6, atol=0)
    assert got_l.tolist() == ref_l.tolist()


def test_multi_token_call_without_a_gpu_raises_dcamd_error():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = dca.UNetCondition2D(**dca.small_unet_kwargs())
    with pytest.raises(L.DcamdError):
        m(torch.zeros(1, 3, 32, 32), torch.zeros(1), encoder_hidden_states=torch.zeros(1, 5, 64))
    with pytest.raises(L.DcamdError):
        m.forward_pair(torch.zeros(1, 3, 32, 32), torch.zeros(1), torch.zeros(1, 5, 64), torch.zeros(1, 5, 64))
    dc = dca.DiffusionClassifier(m, dca.Config(**dict(CFG, encoder_type="prompt", prompt_tokens=5, classes=3)))
    with pytest.raises(L.DcamdError):
        dc.classify(torch.zeros(2, 3, 32, 32))
