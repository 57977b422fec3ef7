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

`score_loss_of` validates the two config keys; `error_torch` / `term_torch` are the definitions as torch statements: the path of foreign
backbones, and the written form of the kernel instances behind `dc_eps_mse` / `dc_err_map` (include/dcamd.h DC_LOSS_*)."""
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


def error_torch(eps_pred, e, kind, delta):
    """errors of one batch of units: eps_pred / e [n, ...] -> [n].  l2 is the reference's statement (:706-711)."""
    n = eps_pred.shape[0]
    if kind == L.LOSS_L2:
        return torch.norm((eps_pred - e).view(n, -1), dim=1, p=2) ** 2
    return term_torch((eps_pred - e).view(n, -1), kind, delta).sum(dim=1)
