"""CPU: prompts of different lengths — the C-ABI of dc_cross_attention_len (struct order, argument validation and routing without a
GPU), the statement that masking keys >= len is attending the truncated prompt (the oracle every length test uses), and the host logic
of a ragged PromptTable (set_prompt / set_lengths, the checkpoint forms, the refusal in front of a foreign backbone)."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import diffusion_classifier_amd as dca
import oracle
from diffusion_classifier_amd import _lib as L
from prompt_oracle import PromptOracleClassifier, PromptOracleUNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(pred_param="eps", schedule="cosine", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, n_stages=1,
           evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32", image_size=32, noise_d=32)


# ------------------------------------------------------------------------------------------------ ABI surface
def test_cross_attention_len_struct_matches_header_field_order():
    hdr = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    names = [n for n, _ in L.CrossAttentionLenParams._fields_]
    # the fields of dc_cross_attention_params in the same order, plus kv_len directly behind kv_map
    base = [n for n, _ in L.CrossAttentionParams._fields_]
    at = base.index("kv_map") + 1
    assert names == base[:at] + ["kv_len"] + base[at:]
    assert "DC_OP_CROSS_ATTENTION_LEN = 10" in hdr and L.OP_CROSS_ATTENTION_LEN == 10
    assert {"dc_cross_attention_len", "dc_cross_attention_len_variant"} <= set(L.EXPORTS)
    lib = L.lib()
    assert lib.dc_cross_attention_len and lib.dc_cross_attention_len_variant
    assert lib.dc_abi_version() == 5 and "#define DC_ABI_VERSION 5" in hdr


def _params(**kw):
    ptr = 1 << 20
    base = dict(q=ptr, k=ptr, v=ptr, out=ptr, kv_len=ptr, dtype=L.DC_BF16, n=2, Lq=64, S=77, heads=8, d=32, ld_q=256, ld_kv=512,
                ld_out=256, scale=32 ** -0.5)
    base.update(kw)
    return L.CrossAttentionLenParams(**base)


@pytest.mark.parametrize("kv_len", [1 << 20, None], ids=["lengths", "null_lengths"])
def test_cross_attention_len_validation_and_routes_need_no_gpu(kv_len):
    """The routing table and the bad-argument cases of test_cross_attention_validation_and_routes_need_no_gpu, through the new entry
    points: same routes, same codes, messages under the new function's name."""
    lib = L.lib()
    variant = lambda **kw: lib.dc_cross_attention_len_variant(_params(kv_len=kv_len, **kw)).decode()
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
        assert lib.dc_cross_attention_len(_params(kv_len=kv_len, **bad), None) == code, bad
        err = lib.dc_last_error()
        assert word in err and err.startswith(b"dc_cross_attention_len:"), (bad, err)
    assert lib.dc_cross_attention_len(None, None) == -1 and lib.dc_cross_attention_len_variant(None) == b"invalid"
    # the plan runner knows the op: a refused call is reported with its index and kind
    p = _params(kv_len=kv_len, S=0)
    ops = (L.Op * 1)()
    ops[0].kind, ops[0].params = L.OP_CROSS_ATTENTION_LEN, C.cast(C.pointer(p), C.c_void_p)
    assert lib.dc_run_plan(ops, 1, None) == -2
    assert b"op 0 (kind 10)" in lib.dc_last_error() and b"S=0" in lib.dc_last_error()


# ------------------------------------------------------------------------------------------------ the oracle: masking = truncation
@pytest.mark.parametrize("S,ln", [(5, 1), (5, 2), (77, 8), (130, 129), (130, 130)])
def test_masking_keys_equals_attending_the_truncated_prompt(S, ln):
    """softmax over keys < len with the rest masked out IS softmax over the truncated keys: exp(-inf) = 0 adds nothing to either sum.
    So `prompt[:len]` through the oracles that exist is the reference of every length test (bound 1e-6 relative)."""
    torch.manual_seed(S + ln)
    q, k, v = torch.randn(2, 4, 19, 16), torch.randn(2, 4, S, 16), torch.randn(2, 4, S, 16)
    mask = (torch.arange(S) < ln)[None, None, None, :].expand(2, 4, 19, S)
    k_bad, v_bad = k.clone(), v.clone()
    k_bad[:, :, ln:], v_bad[:, :, ln:] = 1e4, -1e4                   # what lies in the pad rows is irrelevant under the mask
    masked = F.scaled_dot_product_attention(q, k_bad, v_bad, attn_mask=mask)
    trunc = F.scaled_dot_product_attention(q, k[:, :, :ln], v[:, :, :ln])
    rel = ((masked - trunc).norm() / trunc.norm()).item()
    print(f"S = {S}, len = {ln}: masked vs truncated SDPA rel-L2 {rel:.2e} (bound 1e-6)")
    assert rel < 1e-6, rel


# ------------------------------------------------------------------------------------------------ PromptTable
def _randomise_vectors(m):
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)


def _oracle_unet():
    kw = dca.small_unet_kwargs()
    torch.manual_seed(7)
    po = PromptOracleUNet(**kw)
    _randomise_vectors(po)
    return kw, po


def _prompt_pair(S, classes=3):
    kw, po = _oracle_unet()
    cfg = dict(CFG, encoder_type="prompt", prompt_tokens=S, classes=classes)
    dc = dca.DiffusionClassifier(po, dca.Config(**cfg))
    oc = PromptOracleClassifier(po, oracle.AttrBag(**cfg))
    oc.encoder.load_state_dict(dc.encoder.state_dict())
    return kw, dc, oc


def test_prompt_table_set_prompt_pads_with_zeros_and_records_the_length():
    kw, dc, _ = _prompt_pair(5)
    enc, hid = dc.encoder, kw["encoder_hid_dim"]
    assert enc.lengths.dtype == torch.int64 and enc.lengths.tolist() == [5, 5, 5, 5] and not enc.varlen
    before = enc.weight.detach().clone()
    emb = torch.randn(2, hid)
    enc.set_prompt(1, emb)
    assert torch.equal(enc.weight[1, :2], emb) and (enc.weight[1, 2:] == 0).all()
    assert torch.equal(enc.weight[[0, 2, 3]], before[[0, 2, 3]])
    assert enc.lengths.tolist() == [5, 2, 5, 5] and enc.varlen
    enc.set_prompt(1, torch.randn(5, hid))                            # back to S tokens: the table is uniform again
    assert enc.lengths.tolist() == [5, 5, 5, 5] and not enc.varlen
    enc.set_lengths([5, 1, 3, 2])
    assert enc.lengths.tolist() == [5, 1, 3, 2] and enc.varlen
    assert torch.equal(dc.encode_text_prompt(torch.tensor([2, 0])), enc.weight[[2, 0]])       # unchanged: the padded rows


def test_prompt_table_refuses_lengths_out_of_range():
    kw, dc, _ = _prompt_pair(5)
    enc, hid = dc.encoder, kw["encoder_hid_dim"]
    for bad in (torch.randn(0, hid), torch.randn(6, hid), torch.randn(2, hid + 1), torch.randn(hid)):
        with pytest.raises(ValueError):
            enc.set_prompt(0, bad)
    for bad in ([5, 0, 5, 5], [5, 6, 5, 5], [5, 5, 5], [5.0, 2.0, 1.0, 1.0], [-1, 2, 2, 2]):
        with pytest.raises(ValueError):
            enc.set_lengths(bad)
    assert enc.lengths.tolist() == [5, 5, 5, 5] and not enc.varlen
    with pytest.raises(ValueError):
        enc.load_state_dict({"weight": enc.weight.detach().clone(), "lengths": torch.tensor([5, 9, 5, 5])})


def test_prompt_table_state_dict_and_checkpoint_round_trip(tmp_path):
    from safetensors.torch import load_file, save_file
    kw, dc, _ = _prompt_pair(5)
    hid = kw["encoder_hid_dim"]
    assert list(dc.encoder.state_dict()) == ["weight"]                # uniform: exactly what it saved before lengths existed
    dc.save_checkpoint(str(tmp_path / "uniform"))
    assert list(load_file(str(tmp_path / "uniform" / "model_2.safetensors"))) == ["weight"]
    dc.encoder.set_prompt(3, torch.randn(1, hid))
    dc.encoder.set_prompt(0, torch.randn(3, hid))
    assert list(dc.encoder.state_dict()) == ["weight", "lengths"]
    dc.save_checkpoint(str(tmp_path / "ragged"))
    dc2 = _prompt_pair(5)[1]
    with torch.no_grad():
        dc2.encoder.weight.zero_()
    dc2.load_checkpoint(str(tmp_path / "ragged"))
    assert torch.equal(dc2.encoder.weight, dc.encoder.weight) and dc2.encoder.lengths.tolist() == [3, 5, 5, 1] and dc2.encoder.varlen
    # loading a uniform checkpoint into a ragged table makes it uniform again
    dc2.load_checkpoint(str(tmp_path / "uniform"))
    assert dc2.encoder.lengths.tolist() == [5, 5, 5, 5] and not dc2.encoder.varlen and list(dc2.encoder.state_dict()) == ["weight"]
    # a checkpoint written before lengths existed: model_2.safetensors holds `weight` alone
    old = tmp_path / "old"
    dc.save_checkpoint(str(old))
    w_old = torch.randn(4, 5, hid)
    save_file({"weight": w_old}, str(old / "model_2.safetensors"))
    dc.load_checkpoint(str(old))
    assert torch.equal(dc.encoder.weight, w_old) and dc.encoder.lengths.tolist() == [5, 5, 5, 5] and not dc.encoder.varlen


# ------------------------------------------------------------------------------------------------ foreign backbone
def test_ragged_table_on_a_foreign_backbone_is_refused_and_a_uniform_one_is_not():
    kw, dc, oc = _prompt_pair(4)
    torch.manual_seed(11)
    BS, T = 2, 2
    x = torch.rand(BS, 3, 32, 32) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 3, 32, 32)
    ref_l, ref_e = oc.classify(x, t=t, eps=eps, return_errors=True)
    got_l, got_e = dc.classify(x, t=t, eps=eps, return_errors=True)            # uniform: the oracle loop, as before
    torch.testing.assert_close(got_e, ref_e, rtol=1e-6, atol=0)
    assert got_l.tolist() == ref_l.tolist()
    dc.encoder.set_lengths([4, 2, 4, 1])
    with pytest.raises(NotImplementedError, match="no mask argument"):
        dc.classify(x, t=t, eps=eps)
    dc.config.sampling_steps = 1
    with pytest.raises(NotImplementedError, match="no mask argument"):
        dc.sample(x, torch.tensor([0, 1]), from_t=0.5)
    dc.encoder.set_lengths([4, 4, 4, 4])
    assert torch.equal(dc.classify(x, t=t, eps=eps), got_l)


# ------------------------------------------------------------------------------------------------ no GPU
def test_lengths_without_a_gpu_raise_dcamd_error():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = dca.UNetCondition2D(**dca.small_unet_kwargs())
    with pytest.raises(L.DcamdError):
        m(torch.zeros(1, 3, 32, 32), torch.zeros(1), encoder_hidden_states=torch.zeros(1, 5, 64), encoder_lengths=torch.tensor([2]))
    with pytest.raises(L.DcamdError):
        m.forward_pair(torch.zeros(1, 3, 32, 32), torch.zeros(1), torch.zeros(1, 5, 64), torch.zeros(1, 5, 64),
                       cond_lengths=torch.tensor([3]), null_lengths=torch.tensor([1]))
    dc = dca.DiffusionClassifier(m, dca.Config(**dict(CFG, encoder_type="prompt", prompt_tokens=5, classes=3)))
    dc.encoder.set_lengths([5, 2, 1, 1])
    with pytest.raises(L.DcamdError):
        dc.classify(torch.zeros(2, 3, 32, 32))
