"""The class posterior of a finished classify call: what the errors tensor knows beyond the arg-min label.

Per image, from errors[b] = E [C, T] over the cells j < t_end (+inf = not evaluated, NaN counts as evaluated), every sum fp32,
sequential, j ascending (include/dcamd.h `dc_class_posterior` has the full statement):
  n[c], S[c], mean[c]   evaluated cells of a class, their sum, S / n (+inf for n = 0)
  winner                arg-min of mean over the finalists (n = t_end): NaN last, ties to the lower id — the label's rule; -1: none
  delta[c]              (S[c] - Sw[c]) / n[c], Sw[c] = the winner's errors over the cells class c has: a paired mean difference,
                        because all classes of a trial share (t, eps)
  probs                 softmax_c(-delta / temperature) over classes with n > 0 and a finite delta; 0 elsewhere
  entropy               -sum p ln p (nats)
  runner_up, margin, margin_z
                        the second finalist, the mean of d_j = E[runner, j] - E[winner, j] and that mean over its standard error
                        (two-pass sample variance); no runner: margin = margin_z = +inf
  invalid               NaN cells among the evaluated ones
`class_posterior_hip` is the kernel (csrc/stage.hip), `class_posterior_torch` the same definitions as plain fp32 torch statements on
whatever device the errors live on: the path of foreign backbones, and the written form of the kernel.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L

ClassPosterior = namedtuple("ClassPosterior", ["probs", "entropy", "runner_up", "margin", "margin_z", "n_trials", "invalid"])
ClassPosterior.__doc__ = """Per-image scores of a classify call (tensors on the scoring device).
probs [BS, classes] f32, entropy / margin / margin_z [BS] f32, runner_up [BS] int64 (-1: none), n_trials [BS, classes] int32 (trials a
class was scored on), invalid [BS] int32 (NaN cells: non-zero means the label of that image rests on poisoned scores)."""


def temperature_of(config):
    """config.posterior_temperature (None: 1.0) as a positive float."""
    tau = getattr(config, "posterior_temperature", None)
    tau = 1.0 if tau is None else float(tau)
    if not (tau > 0.0 and tau < float("inf")):
        raise ValueError(f"posterior_temperature must be a positive finite number, got {tau}")
    return tau


def _check(errors, t_end, temperature):
    if errors.dim() != 3 or errors.dtype != torch.float32:
        raise ValueError(f"errors must be float32 [BS, classes, T], got {errors.dtype} {tuple(errors.shape)}")
    if not 1 <= int(t_end) <= errors.shape[2]:
        raise ValueError(f"t_end = {t_end} must lie in [1, T = {errors.shape[2]}]")
    if not (float(temperature) > 0.0 and float(temperature) < float("inf")):
        raise ValueError(f"temperature must be a positive finite number, got {temperature}")


def _argmin_nan_last(mean, cand):
    """Per row: the candidate of smallest mean, NaN after every number, ties to the lower id; -1 where a row has no candidate."""
    C_ = mean.shape[1]
    isnan = torch.isnan(mean)
    tier = torch.where(cand, isnan.to(torch.int64), torch.full_like(isnan, 2, dtype=torch.int64))    # 0 number, 1 NaN, 2 not a candidate
    best_tier = tier.min(dim=1, keepdim=True).values
    pool = tier == best_tier
    val = torch.where(pool & ~isnan, mean, torch.full_like(mean, float("inf")))
    vmin = val.min(dim=1, keepdim=True).values
    ids = torch.arange(C_, device=mean.device).expand_as(mean)
    first = torch.where(pool & ((val == vmin) | isnan), ids, torch.full_like(ids, C_)).min(dim=1).values
    return torch.where(best_tier[:, 0] == 2, torch.full_like(first, -1), first)


def class_posterior_torch(errors, t_end, temperature=1.0, return_parts=False):
    """The definitions in fp32 torch on errors.device.  return_parts: also (winner, means, delta)."""
    _check(errors, t_end, temperature)
    E = errors[:, :, :int(t_end)]
    BS, C_, n_t = E.shape
    f32 = dict(dtype=torch.float32, device=E.device)
    inf, nan = float("inf"), float("nan")
    ev = E != inf
    rows = torch.arange(BS, device=E.device)
    zero = torch.zeros((), **f32)

    n = ev.sum(dim=2).to(torch.int32)
    S = torch.zeros(BS, C_, **f32)
    for j in range(n_t):                                     # sequential, j ascending
        S = S + torch.where(ev[:, :, j], E[:, :, j], zero)
    nf = n.to(torch.float32)
    mean = torch.where(n > 0, S / nf, torch.full_like(S, inf))
    fin = n == n_t
    winner = _argmin_nan_last(mean, fin)
    has_w = winner >= 0
    w = winner.clamp(min=0)
    Ew = E[rows, w]                                          # [BS, t_end]
    runner = _argmin_nan_last(mean, fin & (torch.arange(C_, device=E.device)[None, :] != winner[:, None]))
    runner = torch.where(has_w, runner, torch.full_like(runner, -1))
    has_r = runner >= 0
    Er = E[rows, runner.clamp(min=0)]

    Sw = torch.zeros(BS, C_, **f32)
    for j in range(n_t):
        Sw = Sw + torch.where(ev[:, :, j], Ew[:, j:j + 1].expand(BS, C_), zero)
    delta = (S - Sw) / nf
    delta = torch.where(has_w[:, None], delta, torch.full_like(delta, nan))

    valid = (n > 0) & torch.isfinite(delta)
    a = torch.where(valid, -delta / float(temperature), torch.full_like(delta, -inf))
    mx = a.max(dim=1, keepdim=True).values
    ex = torch.where(valid, torch.exp(a - mx), zero)
    probs = torch.where(valid, ex / ex.sum(dim=1, keepdim=True), zero)
    plogp = torch.where(probs > 0, probs * torch.log(probs.clamp(min=1e-45)), zero)
    entropy = zero - plogp.sum(dim=1)

    sd = torch.zeros(BS, **f32)
    for j in range(n_t):
        sd = sd + (Er[:, j] - Ew[:, j])
    margin = sd / float(n_t)
    ss = torch.zeros(BS, **f32)
    for j in range(n_t):
        d = (Er[:, j] - Ew[:, j]) - margin
        ss = ss + d * d
    var = ss / torch.tensor(float(n_t - 1), **f32)           # t_end = 1: 0 / 0 = NaN
    margin_z = margin / torch.sqrt(var / float(n_t))
    margin = torch.where(has_r, margin, torch.full_like(margin, inf))
    margin_z = torch.where(has_r, margin_z, torch.full_like(margin_z, inf))

    invalid = (torch.isnan(E) & ev).sum(dim=(1, 2)).to(torch.int32)
    mean_w = mean[rows, w]
    bad = ~has_w | torch.isnan(mean_w)
    probs = torch.where(bad[:, None], torch.full_like(probs, nan), probs)
    entropy, margin, margin_z = (torch.where(bad, torch.full_like(v, nan), v) for v in (entropy, margin, margin_z))
    post = ClassPosterior(probs, entropy, runner.to(torch.int64), margin, margin_z, n, invalid)
    return (post, winner.to(torch.int64), mean, delta) if return_parts else post


def class_posterior_hip(errors, t_end, temperature=1.0, return_parts=False):
    """dc_class_posterior on the current stream: errors [BS, classes, T] f32 contiguous on the device.  No synchronisation.
    return_parts: also (winner int32 [BS], means, delta [BS, classes]) — the kernel's optional outputs, for the tests."""
    _check(errors, t_end, temperature)
    lib = L.require_gpu()
    assert errors.is_cuda and errors.is_contiguous()
    BS, C_, T = errors.shape
    dev = errors.device
    # one block for the [BS] statistics: | entropy | margin | margin_z | (f32)   and   | winner | runner | invalid | (int32)
    fstats = torch.empty((3, BS), dtype=torch.float32, device=dev)
    istats = torch.empty((3, BS), dtype=torch.int32, device=dev)
    probs = torch.empty((BS, C_), dtype=torch.float32, device=dev)
    n_eval = torch.empty((BS, C_), dtype=torch.int32, device=dev)
    means = torch.empty((BS, C_), dtype=torch.float32, device=dev) if return_parts else None
    delta = torch.empty((BS, C_), dtype=torch.float32, device=dev) if return_parts else None
    p = L.ClassPosteriorParams(errors=errors.data_ptr(), probs=probs.data_ptr(), entropy=fstats[0].data_ptr(), margin=fstats[1].data_ptr(),
                             margin_z=fstats[2].data_ptr(), winner=istats[0].data_ptr(), runner=istats[1].data_ptr(),
                             invalid=istats[2].data_ptr(), means=means.data_ptr() if return_parts else None,
                             delta=delta.data_ptr() if return_parts else None, n_eval=n_eval.data_ptr(),
                             BS=BS, C=C_, T=T, t_end=int(t_end), temperature=float(temperature), pad_=0)
    L.check(lib.dc_class_posterior(C.byref(p), L.stream_ptr()), "dc_class_posterior")
    post = ClassPosterior(probs, fstats[0], istats[1].to(torch.int64), fstats[1], fstats[2], n_eval, istats[2])
    return (post, istats[0], means, delta) if return_parts else post
