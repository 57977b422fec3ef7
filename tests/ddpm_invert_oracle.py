"""float64 statement of the edit-friendly DDPM inversion and of the decode from its noise maps on a foreign backbone, used by the tests
only.  The draws are passed in; nothing here calls the code under test (the classifier in double and the fp32 grid points come from
solver_oracle.py, another test-side statement).

Grid points i = 0 .. n of linspace(from_t, 0, n + 1), lam_i = schedule(u_i); with c = -expm1(lam_t - lam_s):
  x_i      = alpha_i x + sigma_i e_i
  mu(z; t -> s) = alpha_s (z (1 - c) / alpha_t + c clip(x_hat(z))),  x_hat from the guided prediction (1 + w) pred_c - w pred_u at lam_t
  noise[i] = (x_{i+1} - mu(x_i; i -> i + 1)) / sd_i,   sd_i = sqrt(sigma_{i+1}^2 c_i)
  decode:    z_0 = x_0;  z_{i+1} = mu(z_i; i -> i + 1) + noise[i] sd_i;  result = clip(mu(z_n; n - 1 -> n))   (the sampler's last pass
             repeats the scalars and the lambda of step n - 1)
"""
import math

import torch

from solver_oracle import double_of, grid64


def _sig(v):
    return 1.0 / (1.0 + math.exp(-v))


def scalars64(lam_t, lam_s):
    """(c, alpha_t, sigma_t, alpha_s, sd) of the step lam_t -> lam_s, Python floats computed in double."""
    lt, ls = float(lam_t), float(lam_s)
    c = -math.expm1(lt - ls)
    return c, math.sqrt(_sig(lt)), math.sqrt(_sig(-lt)), math.sqrt(_sig(ls)), math.sqrt(_sig(-ls) * c)


def mean64(dc64, z, lam_t, sc, w, lab):
    c, alpha_t, sigma_t, alpha_s, _ = sc
    cond = dc64.encode_text_prompt(lab)
    null = dc64.encode_text_prompt(torch.full_like(lab, dc64.null_token))
    lam = lam_t.reshape(1)
    pr = (1 + w) * dc64.ema(z, lam, encoder_hidden_states=cond) - w * dc64.ema(z, lam, encoder_hidden_states=null)
    x = alpha_t * z - sigma_t * pr if dc64.pred_param == "v" else (z - sigma_t * pr) / alpha_t
    return alpha_s * (z * (1 - c) / alpha_t + c * x.clamp(-1, 1))


def invert64(dc, x, lab, from_t, w, draws):
    """draws: the n + 1 tensors e_i.  -> (latents [x_0 .. x_n], noise [n maps], sd [n floats]), all double."""
    dc64 = double_of(dc)
    lams = grid64(dc64, from_t, 0.0)
    n = len(lams) - 1
    assert len(draws) == n + 1
    lat = [math.sqrt(_sig(float(lams[i]))) * x.double() + math.sqrt(_sig(-float(lams[i]))) * draws[i].double() for i in range(n + 1)]
    noise, sds = [], []
    for i in range(n):
        sc = scalars64(lams[i], lams[i + 1])
        noise.append((lat[i + 1] - mean64(dc64, lat[i], lams[i], sc, w, lab)) / sc[4])
        sds.append(sc[4])
    return lat, noise, sds


def decode64(dc, start, noise, lab, from_t, w):
    """The ancestral sampler from `start` under labels `lab`, adding noise[i] in step i, and its last pass."""
    dc64 = double_of(dc)
    lams = grid64(dc64, from_t, 0.0)
    n = len(lams) - 1
    z = start.double()
    for i in range(n):
        sc = scalars64(lams[i], lams[i + 1])
        z = mean64(dc64, z, lams[i], sc, w, lab) + noise[i].double() * sc[4]
    return last_pass64(dc, z, lab, from_t, w)


def last_pass64(dc, z, lab, from_t, w):
    """clip(mu) of the sampler's last pass applied to z."""
    dc64 = double_of(dc)
    lams = grid64(dc64, from_t, 0.0)
    sc = scalars64(lams[-2], lams[-1])
    return mean64(dc64, z.double(), lams[-2], sc, w, lab).clamp(-1, 1)


def counterfactual64(dc, start, noise, cl, from_t, w):
    """[BS, K, C, H, W]: every class column of cl decoded from the one start and the one set of maps."""
    return torch.stack([decode64(dc, start, noise, cl[:, k], from_t, w) for k in range(cl.shape[1])], dim=1)
