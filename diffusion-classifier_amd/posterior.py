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

Per-image early stopping (config key `stop_margin_z`, include/dcamd.h `dc_stage_stop`): at a stage boundary an image that is still
active stops iff its margin_z over the cells j < t_end is >= the threshold and its winner's mean is not NaN (a NaN margin_z never
stops, no runner-up — margin_z = +inf — does); it keeps label = winner and t_done = t_end.  `stop_rule_torch` is that rule on the
statements above: the path of foreign backbones and the written form of the kernel.  After such a call every image has its own
number of trials: both posterior functions take t_end as an int tensor [BS] and evaluate each image over its own [0, t_end[b]).
The rule looks at the data at every stage boundary, so the threshold is NOT a one-shot significance level: a z of 2 reached at one of
several looks is weaker evidence than a z of 2 at a single, fixed T (sequential testing).
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


def stop_margin_of(config):
    """config.stop_margin_z: None (per-image early stopping off) or a float > 0, +inf allowed ("never stop").  Anything else: ValueError."""
    z = getattr(config, "stop_margin_z", None)
    if z is None:
        return None
    if isinstance(z, bool) or not isinstance(z, (int, float)) or not float(z) > 0.0:
        raise ValueError(f"stop_margin_z must be a number > 0 (+inf: never stop) or None, got {z!r}")
    return float(z)


def _per_image(fn, errors, t_done, temperature, return_parts, t_values):
    """fn at every distinct value of t_done (t_values: the values that can occur, known to the caller — else read from t_done, which
    synchronises), each image's rows taken from the evaluation at its own value: exact, a row select on the device."""
    if t_done.dim() != 1 or t_done.numel() != errors.shape[0] or t_done.dtype.is_floating_point:
        raise ValueError(f"a per-image t_end must be an int tensor [BS = {errors.shape[0]}], got {t_done.dtype} {tuple(t_done.shape)}")
    t_done = t_done.to(errors.device)
    values = sorted(set(int(v) for v in (t_values if t_values is not None else t_done.tolist())))
    out = None
    for v in values:
        res = fn(errors, v, temperature, return_parts=True)
        flat = tuple(res[0]) + tuple(res[1:])
        if out is None:
            out = flat
            continue
        pick = t_done == v
        out = tuple(torch.where(pick.view(-1, *([1] * (a.dim() - 1))), b, a) for a, b in zip(out, flat))
    nf = len(ClassPosterior._fields)
    post = ClassPosterior(*out[:nf])
    return (post,) + out[nf:] if return_parts else post


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


def class_posterior_torch(errors, t_end, temperature=1.0, return_parts=False, t_values=None):
    """The definitions in fp32 torch on errors.device.  return_parts: also (winner, means, delta).
    t_end an int tensor [BS]: each image over its own [0, t_end[b]) (`_per_image`)."""
    if torch.is_tensor(t_end) and t_end.dim() > 0:
        return _per_image(class_posterior_torch, errors, t_end, temperature, return_parts, t_values)
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
    # the square root through float64: torch's vectorised fp32 sqrt on the CPU is not always the correctly rounded one, the square root
    # of an fp32 number taken in fp64 and rounded once more is (53 >= 2 * 24 + 2 bits) — the kernel's, bit for bit
    margin_z = margin / torch.sqrt((var / float(n_t)).double()).float()
    margin = torch.where(has_r, margin, torch.full_like(margin, inf))
    margin_z = torch.where(has_r, margin_z, torch.full_like(margin_z, inf))

    invalid = (torch.isnan(E) & ev).sum(dim=(1, 2)).to(torch.int32)
    mean_w = mean[rows, w]
    bad = ~has_w | torch.isnan(mean_w)
    probs = torch.where(bad[:, None], torch.full_like(probs, nan), probs)
    entropy, margin, margin_z = (torch.where(bad, torch.full_like(v, nan), v) for v in (entropy, margin, margin_z))
    post = ClassPosterior(probs, entropy, runner.to(torch.int64), margin, margin_z, n, invalid)
    return (post, winner.to(torch.int64), mean, delta) if return_parts else post


def stop_rule_torch(errors, t_end, z_stop, t_done, labels):
    """The stop rule at the boundary t_end, in place on t_done [BS] int32 (0 = active) and labels [BS] int64; rows already stopped are
    left alone.  Returns (active_ids [BS] int32: the ids still active, ascending, then -1; n_active [1] int32; margin_z [BS] f32 of
    the rows that were active, NaN elsewhere) on errors.device — what `dc_stage_stop` writes."""
    if not float(z_stop) > 0.0:
        raise ValueError(f"z_stop must be > 0 (+inf: never stop), got {z_stop}")
    post, winner, _, _ = class_posterior_torch(errors, t_end, 1.0, return_parts=True)
    active = t_done == 0
    z = torch.where(active, post.margin_z, torch.full_like(post.margin_z, float("nan")))      # NaN: no winner, a NaN winner mean, t_end = 1
    stop = active & (z >= float(z_stop))                                                       # NaN >= z is false
    labels.copy_(torch.where(stop, winner.to(labels.dtype), labels))
    t_done.copy_(torch.where(stop, torch.full_like(t_done, int(t_end)), t_done))
    ids = torch.nonzero(t_done == 0).view(-1).to(torch.int32)
    active_ids = torch.full((t_done.numel(),), -1, dtype=torch.int32, device=errors.device)
    active_ids[: ids.numel()] = ids
    return active_ids, torch.tensor([ids.numel()], dtype=torch.int32, device=errors.device), z


def stop_rule_hip(errors, t_end, z_stop, t_done, labels, out=None):
    """dc_stage_stop on the current stream, in place on t_done / labels (on the device).  Returns (active_ids, n_active, margin_z) like
    `stop_rule_torch`; active_ids and n_active are views of one int32 [BS + 1] block (`out`, made here when None).  No synchronisation."""
    lib = L.require_gpu()
    BS, C_, T = errors.shape
    assert errors.is_cuda and errors.is_contiguous() and errors.dtype == torch.float32
    assert t_done.dtype == torch.int32 and labels.dtype == torch.int64 and t_done.is_contiguous() and labels.is_contiguous()
    if out is None:
        out = torch.empty(BS + 1, dtype=torch.int32, device=errors.device)
    z = torch.full((BS,), float("nan"), dtype=torch.float32, device=errors.device)
    L.check(lib.dc_stage_stop(errors.data_ptr(), BS, C_, T, int(t_end), float(z_stop), t_done.data_ptr(), labels.data_ptr(), out.data_ptr(),
                              out[BS:].data_ptr(), z.data_ptr(), L.stream_ptr()), "dc_stage_stop")
    return out[:BS], out[BS:], z


def class_posterior_hip(errors, t_end, temperature=1.0, return_parts=False, t_values=None):
    """dc_class_posterior on the current stream: errors [BS, classes, T] f32 contiguous on the device.  No synchronisation.
    return_parts: also (winner int32 [BS], means, delta [BS, classes]) — the kernel's optional outputs, for the tests.
    t_end an int tensor [BS]: one launch per value of t_values and a row select on the device (`_per_image`)."""
    if torch.is_tensor(t_end) and t_end.dim() > 0:
        return _per_image(class_posterior_hip, errors, t_end, temperature, return_parts, t_values)
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
