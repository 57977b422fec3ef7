"""Weight packing and head padding for the launch plans (plan.py has the plan model).

The packed layouts belong to the C-ABI (include/dcamd.h, "weight packing"): these wrappers only move the fp32 parameter tensor to
the device and call libdcamd's packers — nothing here knows how a packed row is laid out.
"""
import torch

from . import _lib as L
from .plan import TORCH_DT


def f32c(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _packed(rows, cols, dt, device, lead=()):
    return torch.empty(tuple(lead) + (rows, cols), dtype=TORCH_DT[dt], device=device)


def pack_matrix(w2d, dt, device, tile_n=128, kpad=None, col_scale=None):
    """[Cout, K] fp32 (Linear / Conv2d 1x1 weight) -> packed [Cout_pad, kpad or K] in dt (dc_pack_weights_matrix).
    col_scale [K]: a LayerNorm gamma folded into the columns."""
    w = f32c(w2d.reshape(w2d.shape[0], -1), device)
    cout, K = w.shape
    kp = K if kpad is None else kpad
    out = _packed(L.lib().dc_igemm_cout_pad(cout, tile_n), kp, dt, device)
    cs = None if col_scale is None else f32c(col_scale, device)
    L.check(L.lib().dc_pack_weights_matrix(w.data_ptr(), cout, K, kp, None, None if cs is None else cs.data_ptr(), out.data_ptr(), dt, tile_n,
                                           L.stream_ptr()), "dc_pack_weights_matrix")
    return out


def pack_conv3x3(w, dt, device, tile_n=128, kpad=None, c_lo=0, c_hi=None):
    """Conv2d weight [Cout, Cin, 3, 3], input channels [c_lo, c_hi) -> packed [Cout_pad, 9*C (padded to kpad)] (dc_pack_weights_conv3x3)."""
    wd = f32c(w, device)
    cout, cin = wd.shape[0], wd.shape[1]
    c_hi = cin if c_hi is None else c_hi
    kp = 9 * (c_hi - c_lo) if kpad is None else kpad
    out = _packed(L.lib().dc_igemm_cout_pad(cout, tile_n), kp, dt, device)
    L.check(L.lib().dc_pack_weights_conv3x3(wd.data_ptr(), cout, cin, c_lo, c_hi, kp, out.data_ptr(), dt, tile_n, L.stream_ptr()),
            "dc_pack_weights_conv3x3")
    return out


def pack_up4(w, dt, device, tile_n=128):
    """Conv2d weight [Cout, Cin, 3, 3] -> [4, Cout_pad, 4*Cin]: the four-phase form of "nearest-2x upsample, then 3x3 conv"
    (dc_pack_weights_up4 / dc_igemm_params.up4)."""
    wd = f32c(w, device)
    cout, cin = wd.shape[0], wd.shape[1]
    out = _packed(L.lib().dc_igemm_cout_pad(cout, tile_n), 4 * cin, dt, device, lead=(4,))
    L.check(L.lib().dc_pack_weights_up4(wd.data_ptr(), cout, cin, out.data_ptr(), dt, tile_n, L.stream_ptr()), "dc_pack_weights_up4")
    return out


def pack_tail(w, dt, device):
    """Conv2d weight [Co <= 3, 128, 3, 3] -> [32, 128] in dt, row (3 ky + kx) * Co + co, the other rows zero: the A operand of the tail
    fold (dc_pn_tail_params.Wt).  Depends on the weights only."""
    wd = f32c(w, device)
    co, cin = wd.shape[0], wd.shape[1]
    assert 9 * co <= 32 and cin == 128 and tuple(wd.shape[2:]) == (3, 3), tuple(wd.shape)
    out = torch.zeros(32, cin, dtype=TORCH_DT[dt], device=device)
    out[:9 * co] = wd.permute(2, 3, 0, 1).reshape(9 * co, cin).to(TORCH_DT[dt])
    return out


def pack_geglu(w, b, dt, device, ln_gamma=None, ln_beta=None):
    """GEGLU projection [2*n_half, K] + bias -> (packed weight, packed fp32 bias) in the value / gate interleaved row order
    dc_igemm's GEGLU epilogue expects, optionally with a LayerNorm (gamma, beta) folded in (dc_pack_weights_geglu)."""
    wd, bd = f32c(w, device), f32c(b, device)
    cout, K = wd.shape
    out = _packed(L.lib().dc_igemm_cout_pad(cout, 128), K, dt, device)
    ob = torch.empty(cout, dtype=torch.float32, device=device)
    ws = torch.empty(cout, dtype=torch.int32, device=device)
    g = None if ln_gamma is None else f32c(ln_gamma, device)
    be = None if ln_beta is None else f32c(ln_beta, device)
    L.check(L.lib().dc_pack_weights_geglu(wd.data_ptr(), bd.data_ptr(), cout // 2, K, None if g is None else g.data_ptr(),
                                          None if be is None else be.data_ptr(), out.data_ptr(), ob.data_ptr(), ws.data_ptr(), dt,
                                          L.stream_ptr()), "dc_pack_weights_geglu")
    return out, ob


def fold_layernorm_bias(w, bias, ln_beta, device):
    """W beta (+ bias): the bias of a GEMM that absorbed a LayerNorm's beta (dc_fold_layernorm_bias)."""
    wd, be = f32c(w, device), f32c(ln_beta, device)
    bd = None if bias is None else f32c(bias, device)
    out = torch.empty(wd.shape[0], dtype=torch.float32, device=device)
    L.check(L.lib().dc_fold_layernorm_bias(wd.data_ptr(), None if bd is None else bd.data_ptr(), be.data_ptr(), wd.shape[0], wd.shape[1],
                                           out.data_ptr(), L.stream_ptr()), "dc_fold_layernorm_bias")
    return out


def geglu_perm(n_half):
    """Row order of the packed GEGLU projection (what dc_pack_weights_geglu applies): 16-row blocks alternate value / gate halves.
    Kept as the executable statement of that layout for the tests."""
    assert n_half % 16 == 0
    idx = []
    for b in range(n_half // 16):
        idx += list(range(16 * b, 16 * b + 16))
        idx += list(range(n_half + 16 * b, n_half + 16 * b + 16))
    return torch.tensor(idx, dtype=torch.long)


def pad_vec(v, rows):
    if v.shape[0] == rows:
        return v
    out = torch.zeros(rows, dtype=v.dtype, device=v.device)
    out[: v.shape[0]] = v
    return out


# Head widths dc_attention serves.  Heads of another width d <= 128 (DiT-XL/2: 72; UNet levels of 384 / 640 channels in 8 heads:
# 48 / 80) run their attention at dp = padded_head_dim(d): the packed q/k/v weights give each head dp - d zero rows and to_out zero
# input columns at the same positions, so the scores and the real output columns are the same sums.
HEAD_DIMS = (16, 32, 64, 96, 128)


def padded_head_dim(d):
    """The smallest served head width >= d.  Wider heads are refused (NotImplementedError naming the width)."""
    for dp in HEAD_DIMS:
        if dp >= d:
            return dp
    raise NotImplementedError(f"attention head width {d} is not supported (at most {HEAD_DIMS[-1]})")


def pad_head_rows(w, d, dp):
    """[m*d(, K)] rows in consecutive heads of d (q | k | v stacked are 3 * heads of them; a bias too) -> [m*dp(, K)]: head i's row j
    at i*dp + j, rows i*dp + d ... (i+1)*dp - 1 zero."""
    if dp == d:
        return w
    x = w.reshape((-1, d) + tuple(w.shape[1:]))
    out = w.new_zeros((x.shape[0], dp) + tuple(w.shape[1:]))
    out[:, :d] = x
    return out.reshape((-1,) + tuple(w.shape[1:]))


def pad_head_cols(w, d, dp):
    """[N, heads*d] (to_out's weight) -> [N, heads*dp]: zero input columns where pad_head_rows put zero rows."""
    if dp == d:
        return w
    x = w.reshape(w.shape[0], -1, d)
    out = w.new_zeros(w.shape[0], x.shape[1], dp)
    out[..., :d] = x
    return out.reshape(w.shape[0], -1)


def eps_rows(p, C, oc, who="DiT"):
    """Learned-variance outputs (out_channels = 2 * in_channels: eps, then the variance interpolation): the rows of a patch projection
    [p * p * oc, D] that hold eps, row (py * p + px) * oc + c for c < C, in (py, px, c) order — the projection cut to them writes
    features k = (py * p + px) * C + c, what a model with out_channels = C writes and every elementwise kernel reads.
    oc == C: None (every row is one).  Any other width is refused, naming both numbers: nothing here reads such a prediction."""
    if oc == C:
        return None
    if oc != 2 * C:
        raise NotImplementedError(f"{who}: out_channels = {oc} with in_channels = {C} is not served by the scoring and generation plans: "
                                  f"out_channels must be in_channels (eps) or 2 * in_channels = {2 * C} (eps, then a learned variance "
                                  "that is dropped)")
    return (torch.arange(p * p).reshape(-1, 1) * oc + torch.arange(C).reshape(1, -1)).reshape(-1)


class LazyPacks:
    """Base of a weights object whose plans ask for further packed forms on first use.  The object has `P` (key -> packed device
    tensor), `_sd` (the state dict, references only), `dt` and `dev`."""

    def once(self, key, make):
        """P[key], packed on first use.  make() returns that tensor, or a dict of P entries (`key` among them) packed together."""
        if key not in self.P:
            made = make()
            self.P.update(made if isinstance(made, dict) else {key: made})
        return self.P[key]

    def up4(self, key):
        """`<key>.w4`: the four-phase form of an upsampler's conv (pack_up4), packed when a plan first takes that route."""
        return self.once(key + ".w4", lambda: pack_up4(self._sd[key + ".weight"], self.dt, self.dev))
