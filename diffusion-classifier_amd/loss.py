"""The scoring loss of `classify`: which per-element term of d = eps_hat - eps is summed into errors[b, class, j] and into the evidence
maps.  Li et al. evaluate their zero-shot classifier with l1, l2 or Huber; the reference here has l2 only.

With d in fp32 and eps_hat formed as always (the v-param conversion, DiT's un-patchified read), summed over C * H * W — sums, not means:
    "l2" (also None, the default)   sum d^2 through torch.norm(...) ** 2: sqrt, then square — the reference's arithmetic, the same bits as
                                    before the key existed
    "l1"                            sum |d|
    "huber"                         sum h(d), h = 0.5 d^2 for |d| <= delta, else delta (|d| - 0.5 delta): torch's huber_loss, summed;
                                    delta = config.huber_delta (default 1.0) as fp32
l1 and Huber store the sum as it is.  The evidence map's v[y, x] is the channel sum of the same term.  Everything downstream — stage
top-k, arg-min, posterior, `stop_margin_z`, sharding, the maps' finalisation — takes the errors as they come, but their scale follows
the loss: `posterior_temperature` and `stop_margin_z` want re-choosing per loss.

Weights (additive; with none of them in use nothing below runs and no weighted kernel instance is launched).  With t the term above, m
the pixel weight of the unit's image (`classify(..., pixel_weight=m)`, [BS, H, W] on the model's grid) and w the trial weight of
(trial j, image b) (`config.trial_weighting`):
    s = sum_{c, y, x} m[y, x] t(d[c, y, x])       fp32, one multiply per element, the accumulation order of the unweighted kernel on each
                                                  of its three read paths; l2 multiplies (m d) d with the second product fused into the
                                                  sum, as the unweighted kernel's d d is
    l2: r = sqrt(s), r = r r;  l1 / Huber: r = s
    errors = r w                                  one fp32 multiply
    evidence map: v[y, x] = ((sum_c t(d)) m[y, x]) w, then the fixed-point rule of evidence.py with its VMAX unchanged: a weighting that
                                                  pushes v above VMAX makes those cells `invalid`, as any out-of-range v does
so m = 1 and w = 1 give the same bits as no weights, and with trial weights alone errors_weighted == errors_unweighted * w exactly, as an
fp32 product.  The padded units of a launch (the dump slot) take w = 1.  Weights are data: a NaN in m makes the errors of its image
NaN (the posterior counts them as `invalid`), nothing is validated on the device (the one transfer added is the [BS, T] trial weights, host to device once per call); pixel weights are
meant >= 0 (the foreign path's l2 statement folds sqrt(m) into d to keep the reference's norm, exact for ones and for 0/1 masks).
`config.trial_weighting` (read once at construction, `trial_weighting_of`):
    None / "uniform"     no trial weights
    "train"              the weight of the reference's training loss (:331-337): snr = exp(logsnr).clamp(max = config.min_snr_gamma,
                         default 5.0), w = 1 / (1 + snr) for pred_param 'v', 1 / snr for 'eps' — a Monte-Carlo estimate of the objective
                         the checkpoint was trained on, per class
    a callable           f(logsnr) -> weights: logsnr fp32 [T, BS] on the host (the tensor the draws hold), weights of the same shape,
                         finite and >= 0 (checked on the host, where the draws live)
    a 1-D sequence       discrete schedules only: config.train_timesteps numbers, indexed by the DDPM step of the draw
The draws of a call carry the result as `weight` [T, BS] fp32 (`trial_weights`).

`score_loss_of` validates the two config keys; `error_torch` / `term_torch` are the definitions as torch statements: the path of foreign
backbones, and the written form of the kernel instances behind `dc_eps_mse` / `dc_err_map` (include/dcamd.h DC_LOSS_*)."""
import ctypes
import math

import torch

from . import _lib as L

KINDS = {"l2": L.LOSS_L2, "l1": L.LOSS_L1, "huber": L.LOSS_HUBER}


def score_loss_of(config):
    """(config.score_loss, config.huber_delta) -> (kind, delta): kind one of L.LOSS_* (None or key absent: l2), delta a float (1.0 unless
    the kind is Huber and the key is set).  Any other score_loss, a huber_delta that is no finite number > 0, or a huber_delta next to
    another loss: ValueError."""
    name = getattr(config, "score_loss", None)
    delta = getattr(config, "huber_delta", None)
    if name is not None and (not isinstance(name, str) or name not in KINDS):
        raise ValueError(f"score_loss must be None, 'l2', 'l1' or 'huber', got {name!r}")
    kind = KINDS[name or "l2"]
    if delta is None:
        return kind, 1.0
    if kind != L.LOSS_HUBER:
        raise ValueError(f"huber_delta = {delta!r} is set but score_loss = {name!r}: the key belongs to score_loss = 'huber'")
    if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not (float(delta) > 0.0 and math.isfinite(float(delta))):
        raise ValueError(f"huber_delta must be a finite number > 0, got {delta!r}")
    return kind, float(delta)


def term_torch(d, kind, delta):
    """The per-element term of d (fp32 tensor), same shape."""
    if kind == L.LOSS_L1:
        return d.abs()
    if kind == L.LOSS_HUBER:
        return torch.nn.functional.huber_loss(d, torch.zeros_like(d), reduction="none", delta=float(delta))
    return d ** 2


def error_torch(eps_pred, e, kind, delta, pixel_w=None, trial_w=None):
    """errors of one batch of units: eps_pred / e [n, C, H, W] -> [n].  l2 is the reference's statement (:706-711).
    pixel_w [n, H, W] / trial_w [n] (fp32, the units' own rows; None: no such weight): the weighted sums of this module's docstring."""
    n = eps_pred.shape[0]
    d = eps_pred - e
    if kind == L.LOSS_L2:
        if pixel_w is not None:          # the reference's norm kept: sum m d^2 = || sqrt(m) d ||^2
            d = d * torch.sqrt(pixel_w)[:, None]
        r = torch.norm(d.reshape(n, -1), dim=1, p=2) ** 2
    else:
        term = term_torch(d, kind, delta)
        if pixel_w is not None:
            term = term * pixel_w[:, None]
        r = term.reshape(n, -1).sum(dim=1)
    return r if trial_w is None else r * trial_w


# ---- the C ABI of the weights (include/dcamd.h DC_LOSS_WEIGHTED) ----------------------------------------------------------------------
WEIGHTS_BLOCK = [("pixel_w", L.vp), ("trial_w", L.vp), ("w_T", L.i32), ("w_cells", L.i32)]
_weighted = {}


def weighted_params(cls):
    """L.EpsMseParams / L.ErrMapParams -> the ctypes class of the struct WITH the weights block behind it, as dc_eps_mse / dc_err_map
    read it when `loss` carries L.LOSS_WEIGHTED: the struct's own fields, then pixel_w, trial_w, w_T, w_cells at sizeof of the struct.
    The header declares no such struct (its structs are frozen); this flat class has the same layout, checked here."""
    if cls not in _weighted:
        ext = type(cls.__name__ + "Weighted", (ctypes.Structure,), {"_fields_": list(cls._fields_) + WEIGHTS_BLOCK})
        assert ctypes.sizeof(cls) % 8 == 0 and ext.pixel_w.offset == ctypes.sizeof(cls), cls
        _weighted[cls] = ext
    return _weighted[cls]


# ---- config.trial_weighting / classify(pixel_weight=) --------------------------------------------------------------------------------
MIN_SNR_GAMMA = 5.0          # the reference's clamp (:332)


def _gamma_of(value):
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (float(value) > 0.0 and math.isfinite(float(value))):
        raise ValueError(f"min_snr_gamma must be a finite number > 0, got {value!r}")
    return float(value)


def trial_weighting_of(config, train_timesteps=None):
    """(config.trial_weighting, config.min_snr_gamma) -> None (no trial weights) | ("train", gamma) | ("call", f) | ("table", fp32 [N]).
    train_timesteps: N of a discrete schedule, None under the cosine schedules (a table is refused there).  Anything else, a
    min_snr_gamma that is no finite number > 0, or one next to another weighting: ValueError."""
    spec = getattr(config, "trial_weighting", None)
    gamma = getattr(config, "min_snr_gamma", None)
    if gamma is not None and not (isinstance(spec, str) and spec == "train"):
        raise ValueError(f"min_snr_gamma = {gamma!r} is set but trial_weighting = {spec!r}: the key belongs to trial_weighting = 'train'")
    if spec is None or (isinstance(spec, str) and spec == "uniform"):
        return None
    if isinstance(spec, str):
        if spec != "train":
            raise ValueError(f"trial_weighting must be None, 'uniform', 'train', a callable f(logsnr) -> weights or (discrete schedules) a "
                             f"1-D sequence of train_timesteps weights, got {spec!r}")
        return "train", MIN_SNR_GAMMA if gamma is None else _gamma_of(gamma)
    if callable(spec):
        return "call", spec
    if isinstance(spec, (list, tuple, torch.Tensor)) or type(spec).__name__ == "ndarray":
        if train_timesteps is None:
            raise ValueError("trial_weighting as a sequence is indexed by the DDPM step of a draw: it belongs to the discrete schedules "
                             "('scaled_linear', 'ddpm_linear'); under a cosine schedule pass a callable f(logsnr) -> weights")
        try:
            table = torch.as_tensor(spec).detach().to("cpu", torch.float32)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"trial_weighting as a sequence must hold {train_timesteps} numbers, got {spec!r}") from None
        if table.dim() != 1 or table.numel() != train_timesteps:
            raise ValueError(f"trial_weighting as a sequence must be 1-D with train_timesteps = {train_timesteps} entries, got shape "
                             f"{tuple(table.shape)}")
        _check_weights(table, "trial_weighting")
        return "table", table.contiguous()
    raise ValueError(f"trial_weighting must be None, 'uniform', 'train', a callable f(logsnr) -> weights or (discrete schedules) a 1-D "
                     f"sequence of train_timesteps weights, got {spec!r}")


def _check_weights(w, what):
    if not bool((torch.isfinite(w) & (w >= 0)).all()):
        raise ValueError(f"{what}: the weights must be finite and >= 0")


def train_weight(logsnr, pred_param, gamma=MIN_SNR_GAMMA):
    """The reference's statements (:332-336) on a log-SNR tensor: the truncated-SNR weight of its training loss."""
    snr = torch.exp(logsnr).clamp_(max=gamma)
    return 1 / (1 + snr) if pred_param == 'v' else 1 / snr


def trial_weights(spec, pred_param, logsnr, steps=None):
    """The trial weights of one call: spec of `trial_weighting_of`, logsnr fp32 [T, BS] on the host, steps int64 [T, BS] (the DDPM steps
    of the draws; discrete schedules) -> fp32 [T, BS] on the host, or None for no weights.  All of it on the host: no device sync."""
    if spec is None:
        return None
    kind, arg = spec
    if kind == "train":         # one [BS] row per trial, as the reference's loss evaluates it (CPU kernels differ by element position)
        return torch.stack([train_weight(logsnr[j].clone(), pred_param, arg) for j in range(logsnr.shape[0])])
    if kind == "table":
        return arg[steps]
    w = arg(logsnr.clone())
    if not torch.is_tensor(w) or tuple(w.shape) != tuple(logsnr.shape) or not w.dtype.is_floating_point:
        raise ValueError(f"trial_weighting: the callable must return a float tensor of logsnr's shape {tuple(logsnr.shape)}, got "
                         f"{tuple(w.shape) if torch.is_tensor(w) else type(w).__name__}")
    w = w.detach().to("cpu", torch.float32)
    _check_weights(w, "trial_weighting: the callable's result")
    return w


def pixel_weight_of(m, BS, H, W):
    """classify's pixel_weight -> fp32 [BS, H, W], contiguous, on m's device.  m: a float tensor [BS, H, W] or [BS, 1, H, W] on the
    model's grid; anything else ValueError.  The values are data and are not looked at."""
    if not torch.is_tensor(m) or not m.dtype.is_floating_point:
        raise ValueError(f"pixel_weight must be a float tensor [BS, H, W] or [BS, 1, H, W], got "
                         f"{m.dtype if torch.is_tensor(m) else type(m).__name__}")
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() != 3 or tuple(m.shape) != (BS, H, W):
        raise ValueError(f"pixel_weight must be [BS, H, W] or [BS, 1, H, W] on the model's grid, here [{BS}, {H}, {W}] (the latent grid under "
                         f"vae_path / latents=True, the wavelet grid of a DWT model), got {tuple(m.shape)}")
    return m.detach().to(torch.float32).contiguous()
