"""Edit-friendly DDPM inversion (Huberman-Spiegelglas et al., CVPR 2024): the noise maps under which the ancestral sampler decodes an
image back, for `DiffusionClassifier.invert_ddpm` and `counterfactual(start="ddpm_invert")`.

On `sample`'s grid linspace(from_t, 0, sampling_steps + 1), points i = 0 .. n with lam_i = schedule(u_i):
  x_i      = alpha_i x + sigma_i e_i             n + 1 INDEPENDENT draws e_i (not one noise path: that is what makes the maps editable)
  mu_i     = the posterior mean of `ddpm_sampler_step` at (x_i, lam_i -> lam_{i+1}) on the guided prediction pair
  noise[i] = (x_{i+1} - mu_i) / sd_i             sd_i = sqrt(sigma_{i+1}^2 c_i), i = 0 .. n - 1
The ancestral sampler started at x_0 and fed noise[i] in place of its draws lands on x_{i+1} after every step, whatever the number of
steps, the guidance weight and the clip of the data prediction: mu_i is a deterministic function of (x_i, prediction), so the only error
is the rounding of (x_{i+1} - mu_i) / sd_i * sd_i + mu_i.  Under another class the same maps give an edit that keeps the image's
structure.  The sampler's last pass (the clipped mean from x_n) is kept and draws nothing.

`run_eager` is the written statement — two backbone calls per pass and `ddpm_sampler_step` — and the path of a foreign nn.Module.  HIP
backbones run pass i over a `trajectory.Walk` (`run_hip`): one step of a pair session per chunk of images and one `dc_ddpm_noise_map`
(include/dcamd.h) per pass and chunk; nothing is copied to the host inside the loop.  The n passes do not depend on one another: only
two latents are alive at a time.
"""
from collections import namedtuple

import torch

from . import _lib as L
from . import discrete as DG
from . import solver as S
from . import trajectory as TJ

DEFAULT_MAX_BYTES = 2 << 30

DdpmInversion = namedtuple("DdpmInversion", ["start", "noise", "from_t", "guidance"])
DdpmInversion.__doc__ = """Result of `DiffusionClassifier.invert_ddpm` (tensors on the input's device).
start [BS, C, H, W] f32 (x_0, the latent at from_t), noise [sampling_steps, BS, C, H, W] f32 (noise[i]: what the ancestral sampler adds
in step i), from_t (the grid's first point), guidance (the w the maps were solved under)."""


def max_bytes_of(config):
    """config.ddpm_invert_max_bytes: None (2 GiB) or a number >= 0, the largest `noise` buffer `invert_ddpm` allocates."""
    v = config.ddpm_invert_max_bytes
    if v is None:
        return DEFAULT_MAX_BYTES
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0:
        raise ValueError(f"config.ddpm_invert_max_bytes must be a number >= 0 or None, got {v!r}")
    return v


def grid(dc, from_t):
    """(g, scal, alsg): the `trajectory.Grid` of the n + 1 points, (c, alpha_t, sigma_t, alpha_s, sd) of pass i = 0 .. n - 1 and
    (alpha_i, sigma_i) of every point as 0-dim fp32 tensors on the host."""
    g = TJ.grid(dc, from_t, 0.0)
    lams = g.lam
    scal = [dc._sampler_step_scalars(lams[i], lams[i + 1]) for i in range(len(lams) - 1)]
    lam = [v.detach().float().cpu().reshape(()) for v in lams]
    alsg = [(torch.sqrt(torch.sigmoid(v)), torch.sqrt(torch.sigmoid(-v))) for v in lam]
    return g, scal, alsg


def run_eager(dc, x, lab, from_t, w):
    """The statement on any backbone: -> (start, noise).  The draws are `randn_like(x)` in the order i = 0 .. n."""
    if dc.discrete:
        return DG.noise_maps_eager(dc, x, lab, TJ.grid(dc, from_t, 0.0), w)
    dev = x.device
    g, _, alsg = grid(dc, from_t)
    lams = g.lam
    n = len(lams) - 1
    lab_dev = dc.encoder.weight.device if dc.encoder is not None else dev
    cond, null, lens = S.contexts(dc, lab.to(lab_dev), dev, dc.ema.ema_model)
    kc = {"encoder_lengths": lens["cond"]} if lens else {}
    kn = {"encoder_lengths": lens["null"]} if lens else {}
    latent = lambda i: alsg[i][0].to(dev) * x + alsg[i][1].to(dev) * torch.randn_like(x)      # noqa: E731
    noise = torch.empty((n,) + tuple(x.shape), dtype=torch.float32, device=dev)
    start = z = latent(0)
    for i in range(n):
        z_next = latent(i + 1)
        lam_t, lam_s = lams[i].to(dev).unsqueeze(0), lams[i + 1].to(dev).unsqueeze(0)
        label = g.label[i].to(dev).unsqueeze(0)
        pred = dc.ema(z, label, encoder_hidden_states=cond, **kc)
        u_pred = dc.ema(z, label, encoder_hidden_states=null, **kn)
        mu, var = dc.ddpm_sampler_step(z, pred, u_pred, lam_t.clone().detach(), lam_s.clone().detach(), w=w)
        noise[i] = (z_next - mu) / torch.sqrt(var)
        z = z_next
    return start.to(torch.float32), noise


def run_hip(walk, x, scal, alsg, noise):
    """The same on a HIP backbone: image b is the one trajectory of its unit pair in `walk` (trajectory.py), pass i is one session step
    at (x_i, lam_i) and one `dc_ddpm_noise_map` per chunk that writes noise[i] in place.  The latents take draws i = 0 .. n of `noise`."""
    dev = x.device
    n = len(scal)
    alsg = [(a.to(dev), s.to(dev)) for a, s in alsg]
    xf = x.detach().to(torch.float32).contiguous()
    latent = lambda i: (alsg[i][0] * xf + alsg[i][1] * noise(i)).contiguous()              # noqa: E731
    maps = torch.empty((n,) + tuple(x.shape), dtype=torch.float32, device=dev)
    start = z = latent(0)
    for i in range(n):                                                        # no device -> host copy
        z_next = latent(i + 1)
        c, alpha_t, sigma_t, alpha_s, sd = scal[i]
        for _, imgs, f in walk.run(i, z):
            TJ.launch("dc_ddpm_noise_map", L.DdpmNoiseMapParams(
                x_next=z_next[imgs].data_ptr(), out=maps[i, imgs].data_ptr(), alpha_t=alpha_t, sigma_t=sigma_t, alpha_s=alpha_s, c=c, sd=sd, **f))
        z = z_next
    return start, maps


@torch.no_grad()
def invert(dc, x, text, from_t, guidance, rng, seed, name="text"):
    """`DiffusionClassifier.invert_ddpm` (its docstring is the interface).  Every refusal comes before the first draw."""
    from_t, hip = TJ.check_entry(dc, x, from_t, "from_t", "inversion", rng)
    lab = S.label_rows(text, x.shape[0], dc.config.classes, name)
    w = float(dc.cfg_w if guidance is None else guidance)
    n = int(dc.config.sampling_steps)
    size, cap = 4 * n * x.numel(), max_bytes_of(dc.config)
    if size > cap:
        raise ValueError(f"invert_ddpm stores one noise map per step: {n} x {tuple(x.shape)} f32 = {size} bytes, more than "
                         f"config.ddpm_invert_max_bytes = {cap} (fewer sampling_steps, a smaller batch, or raise the key)")
    if hip:
        g, scal, alsg = grid(dc, from_t)
        walk = TJ.Walk(dc, dc.ema.ema_model, x, lab.view(-1, 1), g, w, who="invert_ddpm", noun="fused noise map")
        draws = TJ.NoiseSource(x, rng, seed, n + 1)
        # the discrete grid: the unclipped mean by dc_solver_step and the map in torch (discrete.py); otherwise the fused kernel
        start, noise = DG.noise_maps_hip(walk, x, g, draws) if dc.discrete else run_hip(walk, x, scal, alsg, draws)
    else:
        start, noise = run_eager(dc, x, lab, from_t, w)
    return DdpmInversion(start, noise, from_t, w)
