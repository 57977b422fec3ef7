"""float64 statement of the deterministic samplers and of DDIM inversion (diffusion_classifier_amd/solver.py), used by the tests only.

Everything is evaluated in double: the schedule at the grid points the product visits (the fp32 `linspace` values), the step scalars, the
backbone (a deep copy of the classifier cast to double) and the update expressions.  Nothing here calls the code under test.
"""
import copy
import math

import torch


def scalars64(lams, sampler, direction):
    """[(alpha_t, sigma_t, k1, k2, k3 | None, final)] of the n passes over the n + 1 lambdas `lams`, Python floats computed in double."""
    lam = [float(v) for v in lams]
    n = len(lam) - 1
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))                                  # noqa: E731
    out, h_prev = [], None
    for i in range(n):
        lt, ls = lam[i], lam[i + 1]
        alpha_t, alpha_s, sigma_t, sigma_s = math.sqrt(sig(lt)), math.sqrt(sig(ls)), math.sqrt(sig(-lt)), math.sqrt(sig(-ls))
        h = (ls - lt) / 2
        final = direction == "denoise" and i == n - 1
        second = sampler == "dpmpp_2m" and direction == "denoise" and 1 <= i <= n - 2
        out.append((alpha_t, sigma_t, sigma_s / sigma_t, -alpha_s * math.expm1(-h), 0.5 * h / h_prev if second else None, final))
        h_prev = h
    return out


def pass64(z, pr, sc, x_prev, v_param, clamp=True):
    """One pass on the guided prediction pr: -> (z_s or the final image, x)."""
    alpha_t, sigma_t, k1, k2, k3, final = sc
    x = alpha_t * z - sigma_t * pr if v_param else (z - sigma_t * pr) / alpha_t
    if clamp:
        x = x.clamp(-1, 1)
    D = x if k3 is None else x + k3 * (x - x_prev)
    return (D.clamp(-1, 1) if final else k1 * z + k2 * D), x


def double_of(dc):
    """The classifier in double: backbone, EMA copy and encoder (the config, an attribute bag, is shared, not copied)."""
    dc64 = copy.deepcopy(dc, memo={id(dc.config): dc.config}).double()
    for m in dc64.modules():                 # a backbone that casts its noise labels to fp32 (standin.py) still feeds double layers
        if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d)):
            m.register_forward_pre_hook(lambda mod, args: (args[0].to(mod.weight.dtype),) + tuple(args[1:]))
    return dc64


def grid64(dc64, u_from, u_to):
    steps = torch.linspace(u_from, u_to, dc64.config.sampling_steps + 1).double()       # the product's fp32 grid points
    return [dc64.schedule(steps[j]) for j in range(len(steps))]


def run64(dc64, z, lams, scal, w, lab):
    """The passes `scal` from z (double) under labels `lab` [BS] int64 with guidance w."""
    cond = dc64.encode_text_prompt(lab)
    null = dc64.encode_text_prompt(torch.full_like(lab, dc64.null_token))
    x_prev = None
    for i, sc in enumerate(scal):
        lam_t = lams[i].reshape(1)
        pr = (1 + w) * dc64.ema(z, lam_t, encoder_hidden_states=cond) - w * dc64.ema(z, lam_t, encoder_hidden_states=null)
        z, x_prev = pass64(z, pr, sc, x_prev, dc64.pred_param == "v")
    return z


def decode64(dc, z0, lab, from_t, sampler):
    """n deterministic passes from the latent z0 at from_t down to 0 under labels `lab`."""
    dc64 = double_of(dc)
    lams = grid64(dc64, from_t, 0.0)
    return run64(dc64, z0.double(), lams, scalars64(lams, sampler, "denoise"), float(dc.cfg_w), lab)


def invert64(dc, x, lab, to_t, guidance=0.0):
    """z_{to_t} of x by n first-order passes upwards from alpha(lam(0)) x."""
    dc64 = double_of(dc)
    lams = grid64(dc64, 0.0, to_t)
    z = torch.sqrt(torch.sigmoid(lams[0])) * x.double()
    return run64(dc64, z, lams, scalars64(lams, "ddim", "invert"), float(guidance), lab)


def counterfactual64(dc, z0, cl, from_t, sampler):
    """[BS, K, C, H, W]: the K classes of every image decoded from z0."""
    return torch.stack([decode64(dc, z0, cl[:, k], from_t, sampler) for k in range(cl.shape[1])], dim=1)
