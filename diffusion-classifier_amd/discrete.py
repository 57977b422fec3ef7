"""The ancestral sampler and its noise maps on the discrete DDPM grid (config.schedule = 'scaled_linear' with config.timestep_spacing).

A Stable Diffusion UNet works on scaled VAE latents (std about 1, range about +-4), so nothing is clipped here, and the posterior
mean of one step t -> s on the guided prediction pr = (1 + w) pred_c - w pred_u is linear in (z, x):
  x  = alpha_t z - sigma_t pr  (v)   |   (z - sigma_t pr) / alpha_t  (eps)
  mu = a z + b x                     a = alpha_s (1 - c) / alpha_t,  b = alpha_s c,  c = -expm1(lam_t - lam_s)
  z_s = mu + sd noise                sd = sqrt(sigma_s^2 c)
In abar form a = sqrt(abar_t / abar_s) (1 - abar_s) / (1 - abar_t), b = sqrt(abar_s) beta / (1 - abar_t) and
sd^2 = (1 - abar_s) / (1 - abar_t) beta with beta = 1 - abar_t / abar_s: the DDPM posterior.  The mean is one non-final first-order
`dc_solver_step` with clamp = 0, k1 = a, k2 = b (out = k1 z + k2 x), the update and the noise map (x_next - mu) / sd are one torch op
on the walk's buffers: the C ABI has no unclipped ancestral entry (DESIGN §6p says what one would cost).

`mean_eager` / `ancestral_eager` / `noise_maps_eager` are the written statement — two backbone calls per pass and the expressions
above in fp32 torch — and the path of a foreign nn.Module; `decode_hip` / `noise_maps_hip` / `sample_pair` are the same passes on a
HIP backbone.  Both take the scalars from `posterior_scalars`, so the discrete grid has one statement and one operation order.  The
grid itself (`trajectory.Grid`): lam for the scalars, label = float(k_i) for the backbone.  The last pass repeats step n - 1 and keeps
the mean, as on the cosine schedules.
"""
import torch

from . import _lib as L
from . import trajectory as TJ


def posterior_scalars(lam_t, lam_s):
    """(alpha_t, sigma_t, a, b, sd) of one ancestral step as Python floats, from fp32 torch ops on 0-dim host tensors: the expressions
    of `DiffusionClassifier._sampler_step_scalars`, then a = alpha_s (1 - c) / alpha_t and b = alpha_s c."""
    lt, ls = lam_t.detach().float().cpu().reshape(()), lam_s.detach().float().cpu().reshape(())
    c = -torch.special.expm1(lt - ls)
    alpha_t, alpha_s = torch.sqrt(torch.sigmoid(lt)), torch.sqrt(torch.sigmoid(ls))
    sigma_t, sigma_s = torch.sqrt(torch.sigmoid(-lt)), torch.sqrt(torch.sigmoid(-ls))
    a, b = alpha_s * (1 - c) / alpha_t, alpha_s * c
    sd = torch.sqrt((sigma_s ** 2) * c)
    return float(alpha_t), float(sigma_t), float(a), float(b), float(sd)


def pass_scalars(g):
    """`posterior_scalars` of the n + 1 passes of a downward grid: pass n repeats step n - 1."""
    n = len(g.lam) - 1
    scal = [posterior_scalars(g.lam[t], g.lam[t + 1]) for t in range(n)]
    return scal + [scal[-1]]


def mean_eager(dc, z, pred, u_pred, sc, w):
    """mu = a z + b x in torch, the statement of `mean_hip`: the same expressions in the same order."""
    alpha_t, sigma_t, a, b, _ = sc
    pr = (1 + w) * pred - w * u_pred
    x = alpha_t * z - sigma_t * pr if dc.pred_param == 'v' else (z - sigma_t * pr) / alpha_t
    return a * z + b * x


def mean_hip(f, out, sc):
    """The same as one `dc_solver_step` on the step fields `f` (z, pred, n, ld and the common ones): unclipped, no history, not final."""
    alpha_t, sigma_t, a, b, _ = sc
    TJ.launch("dc_solver_step", L.SolverStepParams(xprev=None, xhat=None, out=out.data_ptr(), clamp=0, final_pass=0, alpha_t=alpha_t,
                                                   sigma_t=sigma_t, k1=a, k2=b, k3=0.0, **f))


def ancestral_eager(dc, z0, conds, null, g, lens=None, noise_maps=None):
    """`trajectory.ancestral_eager` on the discrete grid `g`: the same loop, calls and draws; the backbone is fed label_t, the mean
    is `mean_eager`, and nothing is clipped -> the K means of the last pass."""
    dev = z0.device
    kc = {"encoder_lengths": lens["cond"]} if lens else {}
    kn = {"encoder_lengths": lens["null"]} if lens else {}
    n = len(g.lam) - 1
    scal = pass_scalars(g)
    zs = [z0] * len(conds)
    for i in range(n + 1):
        label = g.label[min(i, n - 1)].to(dev).unsqueeze(0)
        mus = []
        for z, cond in zip(zs, conds):
            pred = dc.ema(z, label, encoder_hidden_states=cond, **kc)
            u_pred = dc.ema(z, label, encoder_hidden_states=null, **kn)
            mus.append(mean_eager(dc, z, pred, u_pred, scal[i], dc.cfg_w))
        if i == n:
            return mus
        noise = torch.randn_like(mus[0]) if noise_maps is None else noise_maps[i]
        zs = [torch.add(mu, noise, alpha=scal[i][4]) for mu in mus]


def decode_hip(walk, z0, g, noise):
    """`counterfactual.decode_hip` on the discrete grid: n + 1 passes, per pass and chunk one `mean_hip` and — but for the last pass —
    one in-place add of sd noise(i) [BS, C, H, W], broadcast over the K trajectories of an image -> [BS, K, C, H, W]."""
    n = len(g.lam) - 1
    scal = pass_scalars(g)
    za, zb = walk.buffers(z0)
    for i in range(n + 1):
        e = noise(i) if i < n else None
        for rows, imgs, f in walk.run(min(i, n - 1), za):
            mean_hip(f, zb[rows], scal[i])
            if e is not None:
                zb[rows].view((-1, walk.K) + walk.shape).add_(e[imgs].unsqueeze(1), alpha=scal[i][4])
        za, zb = zb, za
    return walk.view(za)


def sample_pair(dc, backbone, z_t, cond, null, kw, g):
    """`sample`'s ancestral loop on a HIP backbone (one `forward_pair` per pass) on the discrete grid: the draws of the cosine loop
    in its order, `mean_hip` and the add in place of the fused clipped step."""
    dev = z_t.device
    n = len(g.lam) - 1
    scal = pass_scalars(g)
    fields = TJ.step_fields(dc, backbone, z_t.shape, dc.cfg_w)
    for i in range(n + 1):
        pair = backbone.forward_pair(z_t, g.label[min(i, n - 1)].to(dev).unsqueeze(0), cond, null, **kw)
        noise = torch.randn_like(z_t).to(torch.float32) if i < n else None
        z = z_t.detach().to(torch.float32).contiguous()
        out = torch.empty_like(z)
        mean_hip(dict(fields, z=z.data_ptr(), pred=pair.data_ptr(), n=z.shape[0], ld=pair.shape[-1]), out, scal[i])
        z_t = (out if noise is None else out.add_(noise, alpha=scal[i][4])).to(z_t.dtype)
    return z_t


def latent_scalars(g):
    """(alpha_i, sigma_i) of every grid point as 0-dim fp32 tensors on the host (`ddpm_invert.grid`'s third value)."""
    lam = [v.detach().float().cpu().reshape(()) for v in g.lam]
    return [(torch.sqrt(torch.sigmoid(v)), torch.sqrt(torch.sigmoid(-v))) for v in lam]


def noise_maps_eager(dc, x, lab, g, w):
    """`ddpm_invert.run_eager` on the discrete grid: the same latents and draws, noise[i] = (x_{i+1} - mu_i) / sd_i on `mean_eager`."""
    dev = x.device
    n = len(g.lam) - 1
    scal, alsg = pass_scalars(g), latent_scalars(g)
    lab_dev = dc.encoder.weight.device if dc.encoder is not None else dev
    cond, null, lens = TJ.contexts(dc, lab.to(lab_dev), dev, dc.ema.ema_model)
    kc = {"encoder_lengths": lens["cond"]} if lens else {}
    kn = {"encoder_lengths": lens["null"]} if lens else {}
    latent = lambda i: alsg[i][0].to(dev) * x + alsg[i][1].to(dev) * torch.randn_like(x)      # noqa: E731
    noise = torch.empty((n,) + tuple(x.shape), dtype=torch.float32, device=dev)
    start = z = latent(0)
    for i in range(n):
        z_next = latent(i + 1)
        label = g.label[i].to(dev).unsqueeze(0)
        pred = dc.ema(z, label, encoder_hidden_states=cond, **kc)
        u_pred = dc.ema(z, label, encoder_hidden_states=null, **kn)
        noise[i] = (z_next - mean_eager(dc, z, pred, u_pred, scal[i], w)) / scal[i][4]
        z = z_next
    return start.to(torch.float32), noise


def noise_maps_hip(walk, x, g, noise):
    """`ddpm_invert.run_hip` on the discrete grid: per pass and chunk one `mean_hip` into maps[i] and (x_{i+1} - mu) / sd in place —
    the mean the decode's `mean_hip` forms from the same latent."""
    dev = x.device
    n = len(g.lam) - 1
    scal = pass_scalars(g)
    alsg = [(a.to(dev), s.to(dev)) for a, s in latent_scalars(g)]
    xf = x.detach().to(torch.float32).contiguous()
    latent = lambda i: (alsg[i][0] * xf + alsg[i][1] * noise(i)).contiguous()              # noqa: E731
    maps = torch.empty((n,) + tuple(x.shape), dtype=torch.float32, device=dev)
    start = z = latent(0)
    for i in range(n):                                                        # no device -> host copy
        z_next = latent(i + 1)
        for _, imgs, f in walk.run(i, z):
            mu = maps[i, imgs]
            mean_hip(f, mu, scal[i])
            torch.sub(z_next[imgs], mu, out=mu).div_(scal[i][4])
        z = z_next
    return start, maps
