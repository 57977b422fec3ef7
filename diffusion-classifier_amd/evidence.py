"""Per-pixel class evidence of a classify call: WHERE in the image a class explains the noise worse than the winner.

The scoring loop reduces every (image b, class c, trial j) unit u to one scalar, ||eps_hat_u - eps_bj||^2.  The maps keep what that
reduction throws away.  For pixel (y, x) of the model's [H, W] grid

    v[u, y, x] = sum_ch (eps_hat_u[ch, y, x] - eps_bj[ch, y, x])^2          fp32, ch ascending,

eps_hat formed exactly as the eps-MSE forms it (the v-param conversion, DiT's un-patchified read); under `config.score_loss` "l1" /
"huber" the square is that loss's per-element term (loss.py), so the maps follow the loss the errors use.  All classes of a trial share
(t, eps), so differences between classes are paired by construction, and no backbone forward is added.

Accumulation over trials is FIXED-POINT, hence associative: the same bits for every micro-batch split, launch shape, arrival order
and world size.
    q = (int64) rint((double) v * 2^F),  F = 30,  for a finite v with 0 <= v <= VMAX = 2^14;
any other v (NaN, inf, larger) adds 0 and increments the int32 counter bad[stage, b, c].  classify refuses T > 2^18 with the flag, so
2^(14 + 30 + 18) < 2^63 and the int64 sum cannot overflow.  F and VMAX are csrc's (include/dcamd.h DC_EVIDENCE_*), mirrored below.

Accumulators are kept per stage: acc[s, b, c, y, x] int64 sums the trials of stage s (one extra plane takes the padded slots of a
launch, like the dump cell of `errors`).  Pruning and `stop_margin_z` act at stage ends only, so the trial count n[b, c] of a class is
0 or a stage end, and any prefix the paired difference needs is a sum of whole stage slabs.

`ClassEvidence(mean_map, delta_map, n_trials, invalid)`, tensors on the scoring device; w = the posterior's winner of image b, s_c = the
number of stages class c was scored on:
    mean_map[b, c]   = (sum_{s < s_c} acc[s, b, c]) * 2^-F / n[b, c]                          [BS, C, H, W] f32
    delta_map[b, c]  = (sum_{s < s_c} (acc[s, b, c] - acc[s, b, w])) * 2^-F / n[b, c]         the int64 difference is exact and
                       converted once (double, times 2^-F, divided by n, rounded to f32): delta_map[b, w] is exactly 0 everywhere
    n_trials [BS, C] int32   the posterior's n
    invalid  [BS]    int32   the sum of `bad` over the image's scored cells
Both maps are NaN for a class with n = 0, a cell with bad > 0, and an image whose posterior winner is -1 or has a NaN mean.  (A bad
value in the WINNER's cell leaves the other classes' delta maps finite but short of that contribution: invalid[b] > 0 says so.)
Under `stop_margin_z` each image uses its own t_done[b], exactly as the posterior does.  Summed over the pixels, mean_map[b, c] is the
posterior's mean[b, c] and delta_map[b, c] its delta[b, c], up to fp32 rounding and the quantisation.

`err_map_torch` + `evidence_maps_torch` are the definitions as torch statements: the path of foreign backbones on any device, and the
written form of the kernels `dc_err_map` / `dc_evidence_maps` (csrc/evidence.hip) behind `evidence_maps_hip`.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L
from . import loss as LS

F = L.EVIDENCE_FRAC_BITS          # include/dcamd.h DC_EVIDENCE_FRAC_BITS
VMAX = L.EVIDENCE_VMAX            # include/dcamd.h DC_EVIDENCE_VMAX
T_MAX = 1 << 18                   # 2^(14 + 30 + 18) < 2^63

ClassEvidence = namedtuple("ClassEvidence", ["mean_map", "delta_map", "n_trials", "invalid"])
ClassEvidence.__doc__ = """Per-pixel evidence of a classify call (tensors on the scoring device).
mean_map / delta_map [BS, classes, H, W] f32: the mean per-pixel squared eps-error of a class over its trials, and its paired
difference to the winner over the same trials (exactly 0 for the winner; NaN for a class never scored, a cell with invalid values, an
image without a winner), n_trials [BS, classes] int32, invalid [BS] int32 (values that were NaN, inf or above VMAX and were left out)."""


def check_trials(T):
    if int(T) > T_MAX:
        raise ValueError(f"return_evidence needs T <= 2^18 trials (the int64 fixed-point sums could overflow), got T = {T}")


def new_slabs(n_stages, cells, HW, device):
    """Zeroed per-stage accumulators: acc int64 [n_stages, cells + 1, HW] and bad int32 [n_stages, cells + 1] (the last plane / counter
    takes padded slots)."""
    return (torch.zeros((n_stages, cells + 1, HW), dtype=torch.int64, device=device),
            torch.zeros((n_stages, cells + 1), dtype=torch.int32, device=device))


def err_map_torch(eps_pred, e, cell, acc, bad, loss=L.LOSS_L2, huber_delta=1.0, pixel_w=None, trial_w=None):
    """One batch of units: eps_pred / e [n, C, H, W], cell [n] int64 (the flat (b, class) cell of each unit); adds into acc
    [cells + 1, HW] int64 and bad [cells + 1] int32 of the stage, in place.  loss / huber_delta: the scoring loss (loss.py; a L.LOSS_*
    kind), whose per-element term is summed over the channels.  pixel_w [n, H, W] / trial_w [n] (fp32, the units' own rows; None: no
    such weight): v = ((channel sum) m) w, loss.py's weights, in front of the fixed-point rule."""
    v = LS.term_torch(eps_pred.float() - e.float(), loss, huber_delta).sum(1)      # [n, H, W] fp32
    if pixel_w is not None:
        v = v * pixel_w
    if trial_w is not None:
        v = v * trial_w[:, None, None]
    ok = torch.isfinite(v) & (v >= 0) & (v <= VMAX)
    q = torch.round(torch.where(ok, v, torch.zeros_like(v)).double() * 2.0 ** F).to(torch.int64)
    acc.index_add_(0, cell, q.reshape(q.shape[0], -1))
    bad.index_add_(0, cell, (~ok).reshape(ok.shape[0], -1).sum(1).to(torch.int32))


def _stages_of(n_eval, stage_ends):
    """s_c per cell: 0 for n = 0, s + 1 for n = stage_ends[s], -1 otherwise."""
    sc = torch.where(n_eval == 0, torch.zeros_like(n_eval), torch.full_like(n_eval, -1))
    for s, end in enumerate(stage_ends):
        sc = torch.where(n_eval == int(end), torch.full_like(sc, s + 1), sc)
    return sc


def winner_or_none(winner, means):
    """The posterior's winner as int32 [BS], -1 where it is -1 or its mean is NaN."""
    w = winner.to(torch.int64).view(-1)
    mw = means[torch.arange(w.numel(), device=w.device), w.clamp(min=0)]
    return torch.where((w >= 0) & ~torch.isnan(mw), w, torch.full_like(w, -1)).to(torch.int32)


def evidence_maps_torch(acc, bad, stage_ends, n_eval, winner, H, W):
    """The definitions on acc.device.  acc [n_stages, BS * C + 1, HW] int64, bad [n_stages, BS * C + 1] int32, stage_ends a sequence of
    ints, n_eval [BS, C] int32, winner [BS] int (-1: none)."""
    n_stages, BS, C_ = acc.shape[0], n_eval.shape[0], n_eval.shape[1]
    dev, HW = acc.device, acc.shape[2]
    n_eval = n_eval.to(dev)
    winner = winner.to(dev).to(torch.int64)
    A = acc[:, :BS * C_].view(n_stages, BS, C_, HW)
    Bd = bad[:, :BS * C_].view(n_stages, BS, C_)
    sc = _stages_of(n_eval, stage_ends)                                    # [BS, C]
    has_w = (winner >= 0) & (winner < C_)
    wi = winner.clamp(0, C_ - 1)
    Aw = A[:, torch.arange(BS, device=dev), wi]                            # [n_stages, BS, HW]
    sm = torch.zeros((BS, C_, HW), dtype=torch.int64, device=dev)
    sd = torch.zeros_like(sm)
    nbad = torch.zeros((BS, C_), dtype=torch.int32, device=dev)
    for s in range(n_stages):
        on = (sc > s)
        sm += torch.where(on[:, :, None], A[s], torch.zeros_like(A[s]))
        sd += torch.where(on[:, :, None], A[s] - Aw[s][:, None, :], torch.zeros_like(A[s]))
        nbad += torch.where(on, Bd[s], torch.zeros_like(Bd[s]))
    ok = (sc > 0) & has_w[:, None] & (nbad == 0)
    nd = n_eval.clamp(min=1).double()[:, :, None]
    nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
    mean = torch.where(ok[:, :, None], (sm.double() * 2.0 ** -F / nd).float(), nan)
    delta = torch.where(ok[:, :, None], (sd.double() * 2.0 ** -F / nd).float(), nan)
    invalid = nbad.sum(1).to(torch.int32)
    return ClassEvidence(mean.view(BS, C_, H, W), delta.view(BS, C_, H, W), n_eval.to(torch.int32), invalid)


def evidence_maps_hip(acc, bad, stage_ends, n_eval, winner, H, W):
    """dc_evidence_maps on the current stream.  No synchronisation."""
    lib = L.require_gpu()
    n_stages, BS, C_ = acc.shape[0], n_eval.shape[0], n_eval.shape[1]
    dev = acc.device
    assert acc.is_cuda and acc.is_contiguous() and acc.dtype == torch.int64 and acc.shape[1] == BS * C_ + 1 and acc.shape[2] == H * W
    assert bad.is_contiguous() and bad.dtype == torch.int32 and tuple(bad.shape) == (n_stages, BS * C_ + 1)
    ends = torch.tensor([int(e) for e in stage_ends], dtype=torch.int32).to(dev, non_blocking=True)
    assert ends.numel() == n_stages
    n_eval = n_eval.to(dev, torch.int32).contiguous()
    winner = winner.to(dev, torch.int32).contiguous()
    mean = torch.empty((BS, C_, H, W), dtype=torch.float32, device=dev)
    delta = torch.empty((BS, C_, H, W), dtype=torch.float32, device=dev)
    invalid = torch.empty((BS,), dtype=torch.int32, device=dev)
    p = L.EvidenceMapsParams(acc=acc.data_ptr(), bad=bad.data_ptr(), stage_ends=ends.data_ptr(), n_eval=n_eval.data_ptr(),
                             winner=winner.data_ptr(), mean_map=mean.data_ptr(), delta_map=delta.data_ptr(), invalid=invalid.data_ptr(),
                             n_stages=n_stages, BS=BS, C=C_, HW=H * W)
    L.check(lib.dc_evidence_maps(C.byref(p), L.stream_ptr()), "dc_evidence_maps")
    return ClassEvidence(mean, delta, n_eval, invalid)
