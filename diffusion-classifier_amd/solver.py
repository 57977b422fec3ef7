"""Deterministic samplers and DDIM inversion for `sample`, `counterfactual` and `invert` (config.sampler = "ddim" | "dpmpp_2m").

The schedule is a log-SNR schedule, so the half-log-SNR step of the data-prediction solvers is exact: h = (lam_s - lam_t) / 2.  One pass
from grid point t to grid point s, on the guided prediction pr = (1 + w) pred_c - w pred_u:
  x   = alpha_t z - sigma_t pr  (v)   |   (z - sigma_t pr) / alpha_t  (eps);   x = clip(x, -1, 1)
  D   = x                            first order: DDIM, z_s = alpha_s x + sigma_s (z - alpha_t x) / sigma_t, in either direction
      = x + k3 (x - x_prev)          second order: DPM-Solver++(2M), k3 = h / (2 h_prev)
  z_s = k1 z + k2 D                  k1 = sigma_s / sigma_t, k2 = -alpha_s expm1(-h) (= alpha_s - alpha_t sigma_s / sigma_t)
The last denoising pass returns clip(x) at the last grid point, so n steps are n backbone passes (ancestral DDPM makes n + 1).
Inversion walks the grid upwards (h < 0), first order throughout, and starts from z = alpha(lam(0)) x.
On the discrete grid (schedule='scaled_linear' with config.timestep_spacing; `trajectory.Grid`) the backbone is fed the step float(k_i),
nothing is clipped (scaled VAE latents are not in [-1, 1]) and the last pass is an ordinary first-order pass with k1 = 0, k2 = 1: its
output 0 z + 1 D is the unclipped data prediction, still one backbone pass.

`eager_pass` / `run_eager` are the written statement — two backbone calls per pass and the expressions above in fp32 torch — and the
path of a foreign nn.Module.  HIP backbones run the same passes as `run_walk` over a `trajectory.Walk`, one `dc_solver_step` per step and
chunk: the decode of `sample` (K = 1) and `counterfactual`, and DDIM inversion — the same loop on the upward grid with "invert" scalars.
"""
import torch

from . import _lib as L
from . import trajectory as TJ
from .trajectory import contexts, initial_latent      # noqa: F401  (shared with `sample`; importable here as ever)

SAMPLERS = ("ddim", "dpmpp_2m")


def sampler_of(config):
    """config.sampler -> None (unset or "ddpm": the ancestral path, untouched) | "ddim" | "dpmpp_2m"; anything else: ValueError."""
    s = config.sampler
    if s is None or s == "ddpm":
        return None
    if isinstance(s, str) and s in SAMPLERS:
        return s
    raise ValueError(f"config.sampler must be one of 'ddpm', 'ddim', 'dpmpp_2m' (unset: 'ddpm'), got {s!r}")


def grid_lams(dc, u_from, u_to):
    """lambda at the points of the call's grid (`trajectory.grid`, which also says what the backbone is fed there): 0-dim tensors."""
    return TJ.grid(dc, u_from, u_to).lam


def step_scalars(lams, sampler, direction, clip=True):
    """The per-pass scalars of a walk over the grid `lams` (n + 1 lambdas in the order they are visited) as Python floats, from fp32
    torch ops on 0-dim tensors on the host: [(alpha_t, sigma_t, k1, k2, k3 | None, final)] of n passes.
      direction "denoise": pass 0 is first order (k3 None); with "dpmpp_2m" passes 1 .. n-2 are second order; pass n-1 is `final` (first
                           order, it returns the clipped data prediction)
      direction "invert":  first order throughout, no final pass
      clip False (the discrete grid): the last denoising pass is (alpha_t, sigma_t, 0, 1, None, not final) — k1 z + k2 D = D unclipped"""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    if direction not in ("denoise", "invert"):
        raise ValueError(f"direction must be 'denoise' or 'invert', got {direction!r}")
    lam = [v.detach().float().cpu().reshape(()) for v in lams]
    n = len(lam) - 1
    out, h_prev = [], None
    for i in range(n):
        lt, ls = lam[i], lam[i + 1]
        (alpha_t, sigma_t), (alpha_s, sigma_s) = TJ.point_scalars(lt), TJ.point_scalars(ls)
        h = (ls - lt) / 2
        k1 = sigma_s / sigma_t
        k2 = -alpha_s * torch.special.expm1(-h)
        final = direction == "denoise" and i == n - 1
        second = sampler == "dpmpp_2m" and direction == "denoise" and 1 <= i <= n - 2
        k3 = float(0.5 * h / h_prev) if second else None
        if final and not clip:
            out.append((float(alpha_t), float(sigma_t), 0.0, 1.0, None, False))
            break
        out.append((float(alpha_t), float(sigma_t), float(k1), float(k2), k3, final))
        h_prev = h
    return out


def denoise_scalars(dc, g, sampler):
    """`step_scalars` of a decode down the grid `g`: the one place that says the discrete grid clips nothing."""
    return step_scalars(g.lam, sampler, "denoise", clip=not dc.discrete)


def eager_pass(dc, z, pred, u_pred, w, sc, x_prev, clamp=True):
    """One pass in torch, the statement of `dc_solver_step`: -> (z_s or the final image, x for the next pass's history)."""
    alpha_t, sigma_t, k1, k2, k3, final = sc
    pr = (1 + w) * pred - w * u_pred
    x = alpha_t * z - sigma_t * pr if dc.pred_param == 'v' else (z - sigma_t * pr) / alpha_t
    if clamp:
        x = dc.clip(x)
    D = x + k3 * (x - x_prev) if k3 is not None else x
    return (dc.clip(D) if final else k1 * z + k2 * D), x


def run_eager(dc, z, g, scal, w, cond, null, lens=None):
    """The passes `scal` from z on the grid `g`: per pass one conditional and one null backbone call at z's batch, fed g.label."""
    x_prev = None
    for i, sc in enumerate(scal):
        pred, u_pred = TJ.guided_pair(dc, z, g.label[i].to(z.device).unsqueeze(0), cond, null, lens)
        z, x_prev = eager_pass(dc, z, pred, u_pred, w, sc, x_prev, clamp=not dc.discrete)
    return z


def decode_eager(dc, z, text, from_t, sampler):
    """The latent z at from_t decoded under the labels `text` in eager torch on any backbone: n passes on the grid from from_t
    down to 0 with config.cfg_w."""
    cond, null, lens = contexts(dc, text, z.device, dc.ema.ema_model)
    g = TJ.grid(dc, from_t, 0.0)
    return run_eager(dc, z, g, denoise_scalars(dc, g, sampler), dc.cfg_w, cond, null, lens)


def sample_eager(dc, x, text, from_t, sampler):
    """`sample` under a deterministic sampler in eager torch: the start as ever, then `decode_eager`."""
    return decode_eager(dc, initial_latent(dc, x, from_t), text, from_t, sampler)


def run_walk(walk, z0, scal):
    """The passes `scal` of all trajectories of `walk` (trajectory.py) from z0 [BS, C, H, W]: one `dc_solver_step` per pass and chunk,
    no draw, one history buffer of data predictions for the second-order passes -> [BS, K, C, H, W].  The direction is in the scalars
    and in the grid the walk was built on: the deterministic decode, or DDIM inversion on the upward grid."""
    za, zb = walk.buffers(z0)
    hist = torch.empty_like(za) if any(sc[4] is not None for sc in scal) else None       # x of the pass before
    for t, (alpha_t, sigma_t, k1, k2, k3, final) in enumerate(scal):
        for rows, _, f in walk.run(t, za):
            # 2M: pass 0 writes the history, a second-order pass reads its element and writes it again; the final pass needs none
            hc = None if hist is None or final else hist[rows].data_ptr()
            TJ.launch("dc_solver_step", L.SolverStepParams(
                xprev=hc if k3 is not None else None, xhat=hc, out=zb[rows].data_ptr(), clamp=walk.clamp, final_pass=int(final), alpha_t=alpha_t,
                sigma_t=sigma_t, k1=k1, k2=k2, k3=0.0 if k3 is None else k3, **f))
        za, zb = zb, za
    return walk.view(za)


def sample(dc, x, text, from_t, sampler):
    """`DiffusionClassifier.sample` with config.sampler set.  A HIP backbone with labels runs the trajectories as a walk with one
    class per image; everything else takes the eager form."""
    backbone = dc.ema.ema_model
    if hasattr(backbone, "pair_session") and text is not None and dc.encoder_type is not None and x.is_cuda:
        g = TJ.grid(dc, from_t, 0.0)
        walk = TJ.Walk(dc, backbone, x, text.detach().cpu().reshape(-1, 1).to(torch.int64), g, dc.cfg_w)
        return run_walk(walk, initial_latent(dc, x, from_t), denoise_scalars(dc, g, sampler))[:, 0]
    return sample_eager(dc, x, text, from_t, sampler)


def label_rows(text, BS, n_classes, name):
    """An int tensor [BS] of class ids (None: the null token, id n_classes) -> int64 [BS] on the CPU, validated."""
    if text is None:
        return torch.full((BS,), n_classes, dtype=torch.int64)
    lab = torch.as_tensor(text).detach().cpu()
    if lab.dtype.is_floating_point or lab.dtype == torch.bool or lab.dim() != 1 or lab.numel() != BS:
        raise ValueError(f"{name} must be None or an int tensor [{BS}] of class ids, got {lab.dtype} {tuple(lab.shape)}")
    lab = lab.to(torch.int64).contiguous()
    if int(lab.min()) < 0 or int(lab.max()) > n_classes:
        raise ValueError(f"{name}: class ids must lie in [0, {n_classes}] ({n_classes}: the null token), got {lab.tolist()}")
    return lab


def invert_eager(dc, x, lab, to_t, guidance):
    """DDIM inversion in eager torch: z = alpha(lam(0)) x, then n first-order passes up the grid from 0 to to_t."""
    dev = x.device
    g = TJ.grid(dc, 0.0, to_t)
    lams = g.lam
    z = torch.sqrt(torch.sigmoid(lams[0])).to(dev) * x
    cond, null, lens = contexts(dc, lab.to(TJ.label_device(dc, dev)), dev, dc.ema.ema_model)
    return run_eager(dc, z, g, step_scalars(lams, "ddim", "invert"), float(guidance), cond, null, lens)


@torch.no_grad()
def invert(dc, x, text, to_t, guidance):
    """`DiffusionClassifier.invert` (its docstring is the interface)."""
    to_t, hip = TJ.check_entry(dc, x, to_t, "to_t", "inversion")
    lab = label_rows(text, x.shape[0], dc.config.classes, "text")
    if not hip:
        return invert_eager(dc, x, lab, to_t, guidance).to(torch.float32)
    g = TJ.grid(dc, 0.0, to_t)
    walk = TJ.Walk(dc, dc.ema.ema_model, x, lab.view(-1, 1), g, guidance)
    return run_walk(walk, torch.sqrt(torch.sigmoid(g.lam[0])).to(x.device) * x, step_scalars(g.lam, "ddim", "invert"))[:, 0]
