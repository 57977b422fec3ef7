"""CPU: attention heads of any width up to 128.  dc_attention serves 16 / 32 / 64 / 96 / 128; other widths run zero-padded to the next
of them in the packed q/k/v and to_out weights (engine.padded_head_dim, pad_head_rows, pad_head_cols).  Here: the pad rule, the padding
helpers on fp32 matrices before device packing, the float64 equivalence of a padded attention block, and the refusal of heads wider than
128 at construction."""
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import engine as E


@pytest.mark.parametrize("d,dp", [(8, 16), (24, 32), (40, 64), (48, 64), (72, 96), (80, 96), (104, 128), (120, 128), (128, 128),
                                  (16, 16), (32, 32), (64, 64), (96, 96)])
def test_pad_rule(d, dp):
    assert E.padded_head_dim(d) == dp


def test_served_widths_are_not_padded():
    w = torch.randn(3 * 4 * 64, 256)
    assert E.pad_head_rows(w, 64, 64) is w
    assert E.pad_head_cols(w.t(), 64, 64).data_ptr() == w.t().data_ptr()


@pytest.mark.parametrize("heads,d", [(3, 40), (16, 72), (8, 80), (2, 48)])
def test_padding_layout(heads, d):
    """Real rows of head h land at h*dp + i (q | k | v stacked: 3 * heads heads), pad rows and columns are zero, biases alike."""
    dp = E.padded_head_dim(d)
    C = heads * d
    torch.manual_seed(d)
    wqkv, bqkv, wo = torch.randn(3 * C, 64), torch.randn(3 * C), torch.randn(64, C)
    pw, pbias, po = E.pad_head_rows(wqkv, d, dp), E.pad_head_rows(bqkv, d, dp), E.pad_head_cols(wo, d, dp)
    assert pw.shape == (3 * heads * dp, 64) and pbias.shape == (3 * heads * dp,) and po.shape == (64, heads * dp)
    real = torch.zeros(3 * heads * dp, dtype=torch.bool)
    for g in range(3 * heads):                     # g = which * heads + h
        real[g * dp:g * dp + d] = True
        assert torch.equal(pw[g * dp:g * dp + d], wqkv[g * d:(g + 1) * d])
        assert torch.equal(pbias[g * dp:g * dp + d], bqkv[g * d:(g + 1) * d])
    for h in range(heads):
        assert torch.equal(po[:, h * dp:h * dp + d], wo[:, h * d:(h + 1) * d])
    assert (pw[~real] == 0).all() and (pbias[~real] == 0).all()
    assert (po[:, ~real[:heads * dp]] == 0).all()


def _attention_block(x, wqkv, bqkv, wo, bo, heads, dh, d):
    """to_out(softmax(q k^T / sqrt(d)) v) with heads of dh channels (dh >= d: padded) and the scale of the true width d, float64."""
    qkv = x @ wqkv.t() + bqkv
    Cq = heads * dh
    q, k, v = (qkv[:, o:o + Cq].reshape(-1, heads, dh).transpose(0, 1) for o in (0, Cq, 2 * Cq))
    o = torch.softmax(q @ k.transpose(1, 2) * d ** -0.5, -1) @ v
    return o.transpose(0, 1).reshape(-1, Cq), o.transpose(0, 1).reshape(-1, Cq) @ wo.t() + bo


@pytest.mark.parametrize("heads,d", [(3, 40), (16, 72), (8, 80), (8, 48), (4, 24)])
def test_padded_attention_block_equals_unpadded(heads, d):
    dp = E.padded_head_dim(d)
    C, Lq = heads * d, 50
    torch.manual_seed(100 + d)
    x = torch.randn(Lq, C, dtype=torch.float64)
    wqkv, bqkv = torch.randn(3 * C, C, dtype=torch.float64) * C ** -0.5, torch.randn(3 * C, dtype=torch.float64)
    wo, bo = torch.randn(C, C, dtype=torch.float64) * C ** -0.5, torch.randn(C, dtype=torch.float64)
    o_ref, y_ref = _attention_block(x, wqkv, bqkv, wo, bo, heads, d, d)
    o_pad, y_pad = _attention_block(x, E.pad_head_rows(wqkv, d, dp), E.pad_head_rows(bqkv, d, dp), E.pad_head_cols(wo, d, dp), bo,
                                    heads, dp, d)
    o_pad = o_pad.reshape(Lq, heads, dp)
    assert (o_pad[..., d:] == 0).all()
    torch.testing.assert_close(o_pad[..., :d].reshape(Lq, C), o_ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(y_pad, y_ref, rtol=1e-12, atol=1e-12)


def test_heads_wider_than_128_are_refused_at_construction():
    with pytest.raises(NotImplementedError, match="160"):
        dca.DiT(num_attention_heads=4, attention_head_dim=160)
    kw = dict(dca.small_unet_kwargs(), block_out_channels=(64, 640), attention_head_dim=4)
    with pytest.raises(NotImplementedError, match="160"):
        dca.UNetCondition2D(**kw)


def test_padded_widths_construct():
    """The reference DiT defaults (16 heads x 72, DiT-XL/2) and UNet levels of 384 / 640 channels in 8 heads (48 / 80) construct."""
    m = dca.DiT(num_layers=1)
    assert m.D == 1152
    dca.UNetCondition2D(**dict(dca.small_unet_kwargs(), block_out_channels=(64, 384), encoder_hid_dim=32, cross_attention_dim=32))
