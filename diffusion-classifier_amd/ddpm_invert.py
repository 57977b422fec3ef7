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
backbones run pass i as one step of a pair session per chunk of images and one `dc_ddpm_noise_map` (include/dcamd.h) per pass and chunk;
nothing is copied to the host inside the loop.  The n passes do not depend on one another: only two latents are alive at a time.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L
from . import solver as S

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
    """(lams, scal, alsg): lambda of the n + 1 grid points, (c, alpha_t, sigma_t, alpha_s, sd) of pass i = 0 .. n - 1 and (alpha_i,
    sigma_i) of every point as 0-dim fp32 tensors on the host."""
    lams = S.grid_lams(dc, from_t, 0.0)
    scal = [dc._sampler_step_scalars(lams[i], lams[i + 1]) for i in range(len(lams) - 1)]
    lam = [v.detach().float().cpu().reshape(()) for v in lams]
    alsg = [(torch.sqrt(torch.sigmoid(v)), torch.sqrt(torch.sigmoid(-v))) for v in lam]
    return lams, scal, alsg


def run_eager(dc, x, lab, from_t, w):
    """The statement on any backbone: -> (start, noise).  The draws are `randn_like(x)` in the order i = 0 .. n."""
    dev = x.device
    lams, _, alsg = grid(dc, from_t)
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
        pred = dc.ema(z, lam_t, encoder_hidden_states=cond, **kc)
        u_pred = dc.ema(z, lam_t, encoder_hidden_states=null, **kn)
        mu, var = dc.ddpm_sampler_step(z, pred, u_pred, lam_t.clone().detach(), lam_s.clone().detach(), w=w)
        noise[i] = (z_next - mu) / torch.sqrt(var)
        z = z_next
    return start.to(torch.float32), noise


def run_hip(dc, backbone, x, lab, from_t, w, rng, seed, units):
    """The same on a HIP backbone: image b is one unit pair (class token || null token) of a pair session per chunk of images, pass i is
    one session step at (x_i, lam_i) and one `dc_ddpm_noise_map` per chunk that writes noise[i] in place."""
    from . import counterfactual as CF
    lib = L.require_gpu()
    if not x.is_cuda:
        raise L.DcamdError("invert_ddpm on a HIP backbone needs a CUDA/HIP tensor (as sample does; no CPU fallback)")
    dev = x.device
    BS, Cc, H, W = x.shape
    CHW = Cc * H * W
    patch = int(getattr(backbone.config, "patch_size", 0) or 0)
    oc = int(getattr(backbone.config, "out_channels", Cc) or Cc)
    if oc != Cc:                 # the kernel indexes the prediction with z's channel count as the feature stride
        raise L.DcamdError(f"fused noise map needs out_channels == in_channels (got {oc} vs {Cc})")
    philox = rng == "philox"
    if philox and CHW % 4:
        raise L.DcamdError(f"rng='philox' needs C * H * W to be a multiple of 4, got {CHW}")
    lams, scal, alsg = grid(dc, from_t)
    n = len(lams) - 1
    lam_dev = torch.stack([v.detach().float().reshape(()) for v in lams]).to(dev)
    alsg = [(a.to(dev), s.to(dev)) for a, s in alsg]
    one_plus_w, v_param = float(1.0 + w), int(dc.pred_param == 'v')
    xf = x.detach().to(torch.float32).contiguous()
    if philox:                   # row i * BS + b: counterfactual's convention (row b the start, (step + 1) * BS + b after it)
        row_ids = torch.arange((n + 1) * BS, dtype=torch.int64, device=dev)
        nbuf = torch.empty_like(xf)

    def latent(i):
        if philox:
            L.check(lib.dc_philox_normal(nbuf.data_ptr(), BS, CHW, row_ids[i * BS:(i + 1) * BS].data_ptr(), int(seed), L.stream_ptr()), "dc_philox_normal")
            e = nbuf
        else:
            e = torch.randn_like(x).to(torch.float32)
        return (alsg[i][0] * xf + alsg[i][1] * e).contiguous()

    chunks = CF.image_chunks(BS, 1, units)
    sessions = CF.pair_sessions(dc, backbone, lab.view(-1, 1), chunks, dev)
    noise = torch.empty((n, BS, Cc, H, W), dtype=torch.float32, device=dev)
    start = z = latent(0)
    for i in range(n):                                                        # no device -> host copy
        z_next = latent(i + 1)
        c, alpha_t, sigma_t, alpha_s, sd = scal[i]
        for (b0, b1), ses in zip(chunks, sessions):
            pair = ses.step(z[b0:b1], lam_dev[i:i + 1])
            p = L.DdpmNoiseMapParams(z=z[b0:b1].data_ptr(), pred=pair.data_ptr(), x_next=z_next[b0:b1].data_ptr(),
                                     out=noise[i, b0:b1].data_ptr(), n=b1 - b0, C=Cc, H=H, W=W, ld=pair.shape[-1], patch=patch,
                                     v_param=v_param, w=w, one_plus_w=one_plus_w, alpha_t=alpha_t, sigma_t=sigma_t,
                                     alpha_s=alpha_s, c=c, sd=sd)
            L.check(lib.dc_ddpm_noise_map(C.byref(p), L.stream_ptr()), "dc_ddpm_noise_map")
        z = z_next
    return start, noise


@torch.no_grad()
def invert(dc, x, text, from_t, guidance, rng, seed, units_per_launch, name="text"):
    """`DiffusionClassifier.invert_ddpm` (its docstring is the interface).  Every refusal comes before the first draw."""
    from_t = float(from_t)
    if not 0.0 < from_t <= 1.0:
        raise ValueError(f"from_t must lie in (0, 1], got {from_t}")
    if x.dim() != 4:
        raise ValueError(f"x must be [BS, C, H, W], got {tuple(x.shape)}")
    assert dc.encoder_type is not None, "Encoder must be provided for inversion."
    dc._require_prompts()
    lab = S.label_rows(text, x.shape[0], dc.config.classes, name)
    if rng not in ("reference", "philox"):
        raise ValueError(f"rng must be 'reference' or 'philox', got {rng!r}")
    backbone = dc.ema.ema_model
    hip = hasattr(backbone, "pair_session")
    if not hip:
        if rng == "philox":
            raise L.DcamdError("rng='philox' needs a HIP backbone (UNetCondition2D / DiT)")
        dc._refuse_ragged_on_foreign()
    w = float(dc.cfg_w if guidance is None else guidance)
    n = int(dc.config.sampling_steps)
    size, cap = 4 * n * x.numel(), max_bytes_of(dc.config)
    if size > cap:
        raise ValueError(f"invert_ddpm stores one noise map per step: {n} x {tuple(x.shape)} f32 = {size} bytes, more than "
                         f"config.ddpm_invert_max_bytes = {cap} (fewer sampling_steps, a smaller batch, or raise the key)")
    if hip:
        start, noise = run_hip(dc, backbone, x, lab, from_t, w, rng, seed, units_per_launch(x.shape[2], x.shape[3], 2))
    else:
        start, noise = run_eager(dc, x, lab, from_t, w)
    return DdpmInversion(start, noise, from_t, w)
