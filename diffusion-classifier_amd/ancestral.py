"""Ancestral generation: the DDPM sampler of `sample` and `counterfactual` and the noise maps of `invert_ddpm`, each loop written once.

One step t -> s of the grid, on the guided prediction pr = (1 + w) pred_c - w pred_u, with c = -expm1(lam_t - lam_s):
  x    = alpha_t z - sigma_t pr  (v)   |   (z - sigma_t pr) / alpha_t  (eps)
  mu   = alpha_s (z (1 - c) / alpha_t + c x)          the posterior mean
  z_s  = mu + sd noise                                sd = sqrt(sigma_s^2 c)
  map  = (x_next - mu) / sd                           the noise under which the step lands on x_next (ddpm_invert.py)
n steps are n + 1 backbone passes: the last pass repeats step n - 1, draws nothing and keeps the mean.

The cosine schedules and the discrete grid differ in the arithmetic of that one step and in nothing else, so the difference is one
object, a step kind, chosen once per call by `step_kind`; the loops below take it and never ask which it is.
  `Clipped`  cosine schedules: x is clipped to [-1, 1], the reference's `ddpm_sampler_step`, and the last pass returns clip(mu).  On
             the device the whole step is one kernel: `dc_ddpm_step_shared` (`sample`: `dc_ddpm_step`), the map `dc_ddpm_noise_map`.
  `Linear`   schedule='scaled_linear': scaled VAE latents are not in [-1, 1], nothing is clipped, and mu = a z + b x with
             a = alpha_s (1 - c) / alpha_t, b = alpha_s c.  In abar form a = sqrt(abar_t / abar_s) (1 - abar_s) / (1 - abar_t),
             b = sqrt(abar_s) beta / (1 - abar_t), sd^2 = (1 - abar_s) / (1 - abar_t) beta with beta = 1 - abar_t / abar_s: the DDPM
             posterior.  On the device the mean is one non-final first-order `dc_solver_step` with clamp = 0, k1 = a, k2 = b, the
             update and the map one in-place torch op on the walk's buffers: the C ABI has no unclipped ancestral entry.
  `LearnedRange`  the discrete grid under config.variance = "learned": `Linear`'s mean, and the deviation of every element from the
             variance channels the model predicts next to eps, sde = exp(0.5 (fr log beta + (1 - fr) log beta~)), fr = (v + 1) / 2.  On
             the device step and map are one kernel each, `dc_ddpm_step_shared` / `dc_ddpm_noise_map` in DC_STEP_LEARNED_RANGE.
The kinds are not harmonised: each keeps its own operation order and its own spelling of the update, bit for bit.

A kind holds the `trajectory.Grid` of the call, the guidance weight, and the host scalars of the n steps (`scalars`: fp32 torch ops on
0-dim host tensors, handed to the kernels as Python floats).  Its eager statement is `mean` / `update` / `last` / `noise_map`, its HIP
form on one chunk `step_hip` / `map_hip`.  The loops: `ancestral_eager` and `noise_maps_eager` are the written statement — two backbone
calls per pass — and the path of a foreign nn.Module; `decode_hip` and `noise_maps_hip` run over a `trajectory.Walk`, one step per pass
and chunk, nothing copied to the host; `sample_pair` is `sample` on a HIP backbone, one `forward_pair` per pass.
"""
import torch

from . import _lib as L
from . import trajectory as TJ


def step_scalars(lam_t, lam_s):
    """(c, alpha_t, sigma_t, alpha_s, sd) of one step as 0-dim fp32 tensors on the host: the expressions of `ddpm_sampler_step` on
    0-dim tensors, sd = sqrt(sigma_s^2 c)."""
    lt, ls = lam_t.detach().float().cpu().reshape(()), lam_s.detach().float().cpu().reshape(())
    c = -torch.special.expm1(lt - ls)
    (alpha_t, sigma_t), (alpha_s, sigma_s) = TJ.point_scalars(lt), TJ.point_scalars(ls)
    return c, alpha_t, sigma_t, alpha_s, torch.sqrt((sigma_s ** 2) * c)


def linear_mean(dc, z, pred, u_pred, sc, w):
    """mu = a z + b x in torch from `Linear.scalars` sc, the statement of `Linear.mean_hip`: the same expressions in the same order."""
    alpha_t, sigma_t, a, b, _ = sc
    pr = (1 + w) * pred - w * u_pred
    x = alpha_t * z - sigma_t * pr if dc.pred_param == 'v' else (z - sigma_t * pr) / alpha_t
    return a * z + b * x


class _Kind:
    variance = False          # does the kind read the backbone's variance channels (pair plans with the full projection)?

    def __init__(self, dc, g, w):
        self.dc, self.g, self.w, self.n = dc, g, w, len(g.lam) - 1
        self.scal = [self.scalars_at(t) for t in range(self.n)]

    def scalars_at(self, t):
        return self.scalars(self.g.lam[t], self.g.lam[t + 1])


class Clipped(_Kind):
    """The cosine schedules' step: clipped data prediction, one fused kernel."""

    @staticmethod
    def scalars(lam_t, lam_s):
        """(c, alpha_t, sigma_t, alpha_s, sd) as Python floats."""
        return tuple(float(v) for v in step_scalars(lam_t, lam_s))

    def mean(self, z, pred, u_pred, t):
        """(mu, var) of `ddpm_sampler_step` at step t, lambda as [1] tensors on z's device as the reference forms them."""
        lam_t, lam_s = self.g.lam[t].to(z.device).unsqueeze(0), self.g.lam[t + 1].to(z.device).unsqueeze(0)
        return self.dc.ddpm_sampler_step(z, pred, u_pred, lam_t.clone().detach(), lam_s.clone().detach(), w=self.w)

    def update(self, mu, noise, var):
        return mu + noise * torch.sqrt(var)

    def last(self, mu):
        return self.dc.clip(mu)

    def noise_map(self, x_next, mu, var):
        return (x_next - mu) / torch.sqrt(var)

    def step_hip(self, f, out, t, e, K=None):
        c, alpha_t, sigma_t, alpha_s, sd = self.scal[t]
        p = dict(noise=None if e is None else e.data_ptr(), out=out.data_ptr(), alpha_t=alpha_t, sigma_t=sigma_t, alpha_s=alpha_s, c=c,
                 sd=sd, **f)
        if K is None:
            TJ.launch("dc_ddpm_step", L.DdpmStepParams(**p))
        else:
            TJ.launch("dc_ddpm_step_shared", L.DdpmStepSharedParams(noise_div=K, pad_=0, **p))

    def map_hip(self, f, x_next, out, t):
        c, alpha_t, sigma_t, alpha_s, sd = self.scal[t]
        TJ.launch("dc_ddpm_noise_map", L.DdpmNoiseMapParams(x_next=x_next.data_ptr(), out=out.data_ptr(), alpha_t=alpha_t, sigma_t=sigma_t,
                                                            alpha_s=alpha_s, c=c, sd=sd, **f))


class Linear(_Kind):
    """The discrete grid's step: mu = a z + b x unclipped, the mean by `dc_solver_step`, update and map in torch."""

    @staticmethod
    def scalars(lam_t, lam_s):
        """(alpha_t, sigma_t, a, b, sd) as Python floats, a and b formed in fp32 from `step_scalars`."""
        c, alpha_t, sigma_t, alpha_s, sd = step_scalars(lam_t, lam_s)
        return float(alpha_t), float(sigma_t), float(alpha_s * (1 - c) / alpha_t), float(alpha_s * c), float(sd)

    def mean(self, z, pred, u_pred, t):
        """(mu, sd) at step t: `linear_mean` on the step's scalars."""
        return linear_mean(self.dc, z, pred, u_pred, self.scal[t], self.w), self.scal[t][4]

    def update(self, mu, noise, sd):
        return torch.add(mu, noise, alpha=sd)

    def last(self, mu):
        return mu

    def noise_map(self, x_next, mu, sd):
        return (x_next - mu) / sd

    def mean_hip(self, f, out, t):
        """One `dc_solver_step` on the step fields `f`: unclipped, no history, not final, out = k1 z + k2 x."""
        alpha_t, sigma_t, a, b, _ = self.scal[t]
        TJ.launch("dc_solver_step", L.SolverStepParams(xprev=None, xhat=None, out=out.data_ptr(), clamp=0, final_pass=0, alpha_t=alpha_t,
                                                       sigma_t=sigma_t, k1=a, k2=b, k3=0.0, **f))

    def step_hip(self, f, out, t, e, K=None):
        self.mean_hip(f, out, t)
        if e is not None:
            out.add_(e, alpha=self.scal[t][4])

    def map_hip(self, f, x_next, out, t):
        self.mean_hip(f, out, t)
        torch.sub(x_next, out, out=out).div_(self.scal[t][4])


class LearnedRange(_Kind):
    """The discrete grid's step of a model that predicts its variance (config.variance = "learned"; diffusers' "learned_range", the
    improved-DDPM sampler of a published DiT): `Linear`'s mean on the eps channels, and per element
    sde = exp(0.5 (fr log_hi + (1 - fr) log_lo)), fr = (v + 1) / 2 on the CONDITIONAL call's variance channels v (guidance mixes eps
    only), log_hi = log beta, log_lo = log of the posterior variance.  On the device step and map are one kernel each:
    `dc_ddpm_step_shared` / `dc_ddpm_noise_map` in DC_STEP_LEARNED_RANGE, on pair plans that keep the variance features."""
    variance = True

    @staticmethod
    def scalars(lam_t, lam_s, abar_t, abar_s):
        """(alpha_t, sigma_t, a, b, log_hi, log_lo) as Python floats: the first four are `Linear.scalars`'; the two logs are formed in
        fp64 from the fp64 abar of the two integer steps and rounded to fp32 once — 1 - abar_t / abar_s cancels at neighbouring steps,
        which the fp32 log-SNRs cannot carry.  The posterior variance is clamped below at 1e-20, as diffusers clamps it."""
        alpha_t, sigma_t, a, b, _ = Linear.scalars(lam_t, lam_s)
        at, as_ = torch.as_tensor(abar_t, dtype=torch.float64), torch.as_tensor(abar_s, dtype=torch.float64)
        beta = 1.0 - at / as_
        post = torch.clamp((1.0 - as_) / (1.0 - at) * beta, min=1e-20)
        return alpha_t, sigma_t, a, b, float(torch.log(beta).to(torch.float32)), float(torch.log(post).to(torch.float32))

    def scalars_at(self, t):
        g, abar = self.g, self.dc.abar
        return self.scalars(g.lam[t], g.lam[t + 1], abar[g.steps[t]], abar[g.steps[t + 1]])

    def mean(self, z, pred, u_pred, t):
        """(mu, sde) at step t from the two calls' 2C-channel outputs: `linear_mean` on their eps halves, sde [BS, C, H, W] from the
        conditional call's variance half."""
        Cc = z.shape[1]
        if pred.shape[1] != 2 * Cc or u_pred.shape[1] != 2 * Cc:
            raise ValueError(f"config.variance = 'learned' needs a backbone that returns {2 * Cc} channels (eps and variance) for "
                             f"{Cc}-channel latents, got {pred.shape[1]}")
        alpha_t, sigma_t, a, b, log_hi, log_lo = self.scal[t]
        mu = linear_mean(self.dc, z, pred[:, :Cc], u_pred[:, :Cc], (alpha_t, sigma_t, a, b, None), self.w)
        fr = 0.5 * pred[:, Cc:] + 0.5
        return mu, torch.exp(0.5 * (fr * log_hi + (1.0 - fr) * log_lo))

    def update(self, mu, noise, sde):
        return mu + noise * sde

    def last(self, mu):
        return mu

    def noise_map(self, x_next, mu, sde):
        return (x_next - mu) / sde

    def _step_scalars(self, t):
        """The scalar fields of both structs at step t; alpha_s, c and sd are not read in this mode."""
        alpha_t, sigma_t, a, b, log_hi, log_lo = self.scal[t]
        return dict(alpha_t=alpha_t, sigma_t=sigma_t, alpha_s=0.0, c=0.0, sd=0.0, k1=a, k2=b, log_hi=log_hi, log_lo=log_lo)

    def step_hip(self, f, out, t, e, K=None):
        """One `dc_ddpm_step_shared` on the step fields `f` (which carry the mode block's flag, mode and fstride), the block behind
        the struct: unshared noise is noise_div = 1."""
        p = TJ.mode_params(L.DdpmStepSharedParams)(noise=None if e is None else e.data_ptr(), out=out.data_ptr(),
                                                   noise_div=1 if K is None else K, pad_=0, **self._step_scalars(t), **f)
        TJ.launch("dc_ddpm_step_shared", p, L.DdpmStepSharedParams)

    def map_hip(self, f, x_next, out, t):
        p = TJ.mode_params(L.DdpmNoiseMapParams)(x_next=x_next.data_ptr(), out=out.data_ptr(), **self._step_scalars(t), **f)
        TJ.launch("dc_ddpm_noise_map", p, L.DdpmNoiseMapParams)


def step_kind(dc, g, w):
    """The step kind of a call on the grid `g` under guidance weight w: the one place that asks which schedule the classifier has and
    whether its variance is learned (config.variance, refused at construction off the discrete grid)."""
    if getattr(dc, "variance", None) == "learned":
        return LearnedRange(dc, g, w)
    return (Linear if dc.discrete else Clipped)(dc, g, w)


def ancestral_eager(kind, z0, conds, null, lens=None, noise_maps=None):
    """The reference's ancestral loop from z0 under the K label columns `conds`: per pass and column one guided pair at z0's batch
    and the kind's mean, every column adding the pass's one `randn_like` (or noise_maps[i] in its place) — op for op what K calls of
    `sample` with the seed reset in front of each compute -> the K means of the last pass (`kind.last`).
    lens: `contexts`' token counts for a ragged table (K = 1)."""
    dc, g, n = kind.dc, kind.g, kind.n
    zs = [z0] * len(conds)
    for i in range(n + 1):                                                    # the last pass repeats step n-1 and keeps the mean
        t = min(i, n - 1)
        label = g.label[t].to(z0.device).unsqueeze(0)
        steps = [kind.mean(z, *TJ.guided_pair(dc, z, label, cond, null, lens), t) for z, cond in zip(zs, conds)]
        if i == n:
            return [kind.last(mu) for mu, _ in steps]
        noise = torch.randn_like(steps[0][0]) if noise_maps is None else noise_maps[i]
        zs = [kind.update(mu, noise, spread) for mu, spread in steps]


def decode_hip(kind, walk, z0, noise):
    """The ancestral decode of all trajectories of `walk` from z0 [BS, C, H, W]: n + 1 passes, one `kind.step_hip` per pass and chunk;
    pass i < n adds noise(i) [BS, C, H, W] f32, shared by the K trajectories of an image; the last pass takes none and keeps the mean
    -> [BS, K, C, H, W]."""
    n = kind.n
    za, zb = walk.buffers(z0)
    for i in range(n + 1):
        t = min(i, n - 1)
        e = noise(i) if i < n else None
        for rows, imgs, f in walk.run(t, za):
            kind.step_hip(f, zb[rows].view((-1, walk.K) + walk.shape), t, None if e is None else e[imgs].unsqueeze(1), walk.K)
        za, zb = zb, za
    return walk.view(za)


def sample_pair(kind, backbone, z_t, cond, null, lens):
    """`sample`'s loop on a HIP backbone: one `forward_pair` (class token || null token, one batch-2 plan launch) and one
    `kind.step_hip` per pass, one `randn_like` per pass but the last, in the reference's order."""
    dc, g, n = kind.dc, kind.g, kind.n
    kw = {"cond_lengths": lens["cond"], "null_lengths": lens["null"]} if lens else {}
    if kind.variance:
        kw["variance"] = True                                                 # the pair plan that keeps the variance features
    fields = TJ.step_fields(dc, backbone, z_t.shape, dc.cfg_w, variance=kind.variance)
    for i in range(n + 1):
        t = min(i, n - 1)
        pair = backbone.forward_pair(z_t, g.label[t].to(z_t.device).unsqueeze(0), cond, null, **kw)
        noise = torch.randn_like(z_t).to(torch.float32).contiguous() if i < n else None
        z = z_t.detach().to(torch.float32).contiguous()
        out = torch.empty_like(z)
        kind.step_hip(dict(fields, z=z.data_ptr(), pred=pair.data_ptr(), n=z.shape[0], ld=pair.shape[-1]), out, t, noise)
        z_t = out.to(z_t.dtype)
    return z_t


def sample(dc, x, text, from_t):
    """`DiffusionClassifier.sample` under the ancestral sampler, before any decoding: the start, the contexts, then `sample_pair` on
    a HIP backbone with labels and `ancestral_eager` on everything else."""
    z_t = TJ.initial_latent(dc, x, from_t)
    backbone = dc.ema.ema_model
    cond, null, lens = TJ.contexts(dc, text, x.device, backbone)              # lens: the rows' token counts of a ragged prompt table
    kind = step_kind(dc, TJ.grid(dc, from_t, 0.0), dc.cfg_w)
    if hasattr(backbone, "forward_pair") and cond is not None and z_t.is_cuda:
        return sample_pair(kind, backbone, z_t, cond, null, lens)
    return ancestral_eager(kind, z_t, [cond], null, lens)[0]


def noise_maps_eager(kind, x, lab):
    """`invert_ddpm` on any backbone, the written statement: the latents x_i = alpha_i x + sigma_i e_i from `randn_like(x)` draws in
    the order i = 0 .. n, noise[i] = `kind.noise_map` of x_{i+1} on the mean at x_i -> (start, noise)."""
    dc, g, n, dev = kind.dc, kind.g, kind.n, x.device
    alsg = [TJ.point_scalars(v) for v in g.lam]
    cond, null, lens = TJ.contexts(dc, lab.to(TJ.label_device(dc, dev)), dev, dc.ema.ema_model)
    latent = lambda i: alsg[i][0].to(dev) * x + alsg[i][1].to(dev) * torch.randn_like(x)      # noqa: E731
    noise = torch.empty((n,) + tuple(x.shape), dtype=torch.float32, device=dev)
    start = z = latent(0)
    for i in range(n):
        z_next = latent(i + 1)
        label = g.label[i].to(dev).unsqueeze(0)
        mu, spread = kind.mean(z, *TJ.guided_pair(dc, z, label, cond, null, lens), i)
        noise[i] = kind.noise_map(z_next, mu, spread)
        z = z_next
    return start.to(torch.float32), noise


def noise_maps_hip(kind, walk, x, noise):
    """The same on a HIP backbone: image b is the one trajectory of its unit pair in `walk`, pass i is one session step at
    (x_i, label_i) and one `kind.map_hip` per chunk that writes noise[i] in place.  The latents take draws i = 0 .. n of `noise`; the n
    passes do not depend on one another, so only two latents are alive at a time."""
    n, dev = kind.n, x.device
    alsg = [tuple(v.to(dev) for v in TJ.point_scalars(lam)) for lam in kind.g.lam]
    xf = x.detach().to(torch.float32).contiguous()
    latent = lambda i: (alsg[i][0] * xf + alsg[i][1] * noise(i)).contiguous()              # noqa: E731
    maps = torch.empty((n,) + tuple(x.shape), dtype=torch.float32, device=dev)
    start = z = latent(0)
    for i in range(n):                                                        # no device -> host copy
        z_next = latent(i + 1)
        for _, imgs, f in walk.run(i, z):
            kind.map_hip(f, z_next[imgs], maps[i, imgs], i)
        z = z_next
    return start, maps
