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

This module is the entry point: the refusals, the size cap and the result.  The loops are ancestral.py's: `noise_maps_eager` is the
written statement — two backbone calls per pass and the step kind's mean — and the path of a foreign nn.Module; HIP backbones run pass
i over a `trajectory.Walk` (`noise_maps_hip`): one step of a pair session per chunk of images and one map per pass and chunk
(`dc_ddpm_noise_map`, include/dcamd.h, on the cosine schedules); nothing is copied to the host inside the loop.
"""
from collections import namedtuple

import torch

from . import ancestral as AN
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


def run_eager(dc, x, lab, from_t, w):
    """The eager statement under its earlier name: `ancestral.noise_maps_eager` on the grid from `from_t` -> (start, noise)."""
    return AN.noise_maps_eager(AN.step_kind(dc, TJ.grid(dc, from_t, 0.0), w), x, lab)


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
    kind = AN.step_kind(dc, TJ.grid(dc, from_t, 0.0), w)
    if hip:
        walk = TJ.Walk(dc, dc.ema.ema_model, x, lab.view(-1, 1), kind.g, w, who="invert_ddpm", noun="fused noise map",
                       variance=kind.variance)
        start, noise = AN.noise_maps_hip(kind, walk, x, TJ.NoiseSource(x, rng, seed, n + 1))
    else:
        start, noise = AN.noise_maps_eager(kind, x, lab)
    return DdpmInversion(start, noise, from_t, w)
