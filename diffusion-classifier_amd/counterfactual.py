"""Counterfactual explanations: one image denoised under every class label from shared noise, and where the results differ.

The reference's procedure (experiments/ipmsa/explain.py) noises an image to `from_t`, runs `sample` once per class label with the seed
reset in front of each run, and compares the generated images.  `DiffusionClassifier.counterfactual` is that procedure as one call:
  samples [BS, K, C, H, W]   samples[b, k] = what `sample(x, classes[:, k], from_t)` returns for image b; the K trajectories of an image
                             start from one z_{from_t} and add one noise draw per step (common random numbers by construction)
  maps [BS, K, H', W']       maps[b, k] = sum_c |samples[b, k, c] - base[b, c]|, c ascending, fp32; base = the input image or the
                             trajectory of one of the classes
HIP backbones run all BS x K trajectories as the units of one pair session per chunk of images (`run_hip`: the prompts are projected
once per call, the step scalars are formed before the loop, nothing is copied to the host inside it; `dc_ddpm_step_shared`,
`dc_abs_diff_map`).  A foreign nn.Module takes the reference's own form in eager torch (`run_foreign`): it is the written statement.
With config.sampler = "ddim" | "dpmpp_2m" (solver.py) the trajectories are deterministic after their start (`dc_solver_step`), and
start="invert" takes that start from DDIM inversion of the image instead of from noise.  Under the ancestral sampler
start="ddpm_invert" takes the start AND the noise of every step from the image's edit-friendly DDPM inversion (ddpm_invert.py): the
decode under the inversion's class is the image again, and the loop draws nothing.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L
from . import ddpm_invert as DI
from . import solver as S

Counterfactuals = namedtuple("Counterfactuals", ["samples", "classes", "maps"])
Counterfactuals.__doc__ = """Result of `DiffusionClassifier.counterfactual` (tensors on the input's device).
samples [BS, K, C, H, W] f32 (pixel_space: [BS, K, C / 4, 2H, 2W]), classes [BS, K] int64 (the label of every trajectory),
maps [BS, K, H', W'] f32 (the channel-summed absolute difference to the base image, at the resolution of `samples`)."""


def class_table(classes, BS, n_classes):
    """`classes` (None: all; [K]: the same for every image; [BS, K]) -> int64 [BS, K] on the CPU, validated."""
    if classes is None:
        return torch.arange(n_classes).repeat(BS, 1)
    cl = torch.as_tensor(classes).detach().cpu()
    if cl.dtype.is_floating_point or cl.dtype == torch.bool:
        raise ValueError(f"classes must be an int tensor, got {cl.dtype}")
    if cl.dim() == 1:
        cl = cl.unsqueeze(0).expand(BS, -1)
    if cl.dim() != 2 or cl.shape[0] != BS or cl.shape[1] < 1:
        raise ValueError(f"classes must be [K] or [{BS}, K] with K >= 1, got {tuple(cl.shape)}")
    cl = cl.to(torch.int64).contiguous()
    if int(cl.min()) < 0 or int(cl.max()) >= n_classes:
        raise ValueError(f"class ids must lie in [0, {n_classes}), got {cl.tolist()}")
    return cl


def base_rows(against, cl):
    """against = class ids [BS]: for every trajectory b * K + k the trajectory it is compared with, b * K + (the first column of image b
    that holds against[b]) -> int64 [BS * K].  ValueError when an image's class list does not hold its id."""
    BS, K = cl.shape
    ag = torch.as_tensor(against).detach().cpu()
    if ag.dim() != 1 or ag.numel() != BS or ag.dtype.is_floating_point or ag.dtype == torch.bool:
        raise ValueError(f"against must be 'input' or an int tensor [{BS}] of class ids, got {ag.dtype} {tuple(ag.shape)}")
    hit = cl == ag.to(torch.int64).view(-1, 1)
    if not bool(hit.any(dim=1).all()):
        bad = [b for b in range(BS) if not bool(hit[b].any())]
        raise ValueError(f"against[b] must be one of classes[b]: image(s) {bad} have {ag[bad].tolist()} outside {cl[bad].tolist()}")
    col = hit.to(torch.int64).argmax(dim=1)                     # the first column that holds the id
    return (torch.arange(BS) * K + col).repeat_interleave(K)


def abs_diff_map_torch(a, r, r_of_a):
    """The statement of `dc_abs_diff_map` in fp32 torch: a [n, C, H, W], r [m, C, H, W], r_of_a [n] -> [n, H, W], c ascending."""
    ref = r[r_of_a.to(r.device)]
    out = torch.zeros((a.shape[0],) + tuple(a.shape[2:]), dtype=torch.float32, device=a.device)
    for c in range(a.shape[1]):
        out = out + (a[:, c] - ref[:, c]).abs()
    return out


def abs_diff_map_hip(a, r, r_of_a):
    """dc_abs_diff_map on the current stream: a, r fp32 contiguous on the device, r_of_a any int tensor [n]."""
    lib = L.require_gpu()
    assert a.is_cuda and r.is_cuda and a.dtype == r.dtype == torch.float32 and a.is_contiguous() and r.is_contiguous()
    assert a.dim() == 4 and r.dim() == 4 and a.shape[1:] == r.shape[1:] and r_of_a.numel() == a.shape[0]
    n, Cc, H, W = a.shape
    idx = r_of_a.to(a.device, torch.int32).contiguous()
    out = torch.empty((n, H, W), dtype=torch.float32, device=a.device)
    p = L.AbsDiffMapParams(a=a.data_ptr(), r=r.data_ptr(), r_of_a=idx.data_ptr(), out=out.data_ptr(), n=n, m=r.shape[0], C=Cc, H=H, W=W, pad_=0)
    L.check(lib.dc_abs_diff_map(C.byref(p), L.stream_ptr()), "dc_abs_diff_map")
    return out


def image_chunks(BS, K, units):
    """Whole images per launch: 2 * K units an image, at most `units` a launch (one image at least), in equal chunks -> [(b0, b1)]."""
    per = max(1, int(units) // (2 * K))
    n_chunks = -(-BS // per)
    per = -(-BS // n_chunks)
    return [(b0, min(BS, b0 + per)) for b0 in range(0, BS, per)]


def pair_sessions(dc, backbone, cl, chunks, dev):
    """One pair session per chunk (b0, b1) of images for the labels cl [BS, K]: unit pair b * K + k is class token cl[b, k] || null
    token; contexts, lengths and the context plan once per call and chunk, session ci in slot ci."""
    table = dc.encoder is not None
    lab_dev = dc.encoder.weight.device if table else dev
    ln = dc.encoder.lengths.cpu() if dc._ragged_table() else None
    sessions = []
    for ci, (b0, b1) in enumerate(chunks):
        lab = cl[b0:b1].reshape(-1)
        nul = torch.full_like(lab, dc.null_token)
        cond, null = dc.encode_text_prompt(lab.to(lab_dev)).to(dev), dc.encode_text_prompt(nul.to(lab_dev)).to(dev)
        kw = dict(cond_lengths=ln[lab], null_lengths=ln[nul]) if ln is not None else {}
        sessions.append(backbone.pair_session(lab.numel(), dev, cond, null, slot=ci, **kw))
    return sessions


def run_foreign(dc, backbone, x, cl, from_t, sampler=None, z0=None, noise_maps=None):
    """The reference's form: per step and class one conditional and one null call at batch BS and `ddpm_sampler_step`, every class
    adding the step's one `randn_like` — op for op what K calls of `sample` with the seed reset in front of each compute.
    sampler "ddim" / "dpmpp_2m": the K classes by `solver.run_eager` from the one start instead, no draw after it; z0 [BS, C, H, W]:
    that start (an inverted latent) in place of the noised image, no draw at all.  noise_maps [n, BS, C, H, W] (ancestral sampler, with
    z0; ddpm_invert.py): step i adds noise_maps[i] in place of its draw."""
    dev = x.device
    BS, K = cl.shape
    if z0 is not None:
        pass
    elif from_t == 1:
        z0 = torch.randn(x.shape).to(dev)
    else:
        lam = dc.schedule(torch.ones(BS) * from_t).to(dev)
        z0, _ = dc.diffuse(x, torch.sqrt(torch.sigmoid(lam)).view(-1, 1, 1, 1), torch.sqrt(torch.sigmoid(-lam)).view(-1, 1, 1, 1))
    lab_dev = dc.encoder.weight.device if dc.encoder is not None else dev
    labs = [cl[:, k].to(lab_dev) for k in range(K)]
    conds = [dc.encode_text_prompt(lab).to(dev) for lab in labs]
    null = dc.encode_text_prompt(torch.full_like(labs[0], dc.null_token)).to(dev)
    if sampler is not None:
        lams = S.grid_lams(dc, from_t, 0.0)
        scal = S.step_scalars(lams, sampler, "denoise")
        return torch.stack([S.run_eager(dc, z0, lams, scal, dc.cfg_w, cond, null) for cond in conds], dim=1).to(torch.float32)
    steps = torch.linspace(from_t, 0.0, dc.config.sampling_steps + 1)
    n = len(steps) - 1
    zs = [z0] * K
    for i in range(n + 1):                                                    # the last pass repeats step n-1 and keeps the mean
        u_t, u_s = (steps[i], steps[i + 1]) if i < n else (steps[-2], steps[-1])
        lam_t, lam_s = dc.schedule(u_t).to(dev).unsqueeze(0), dc.schedule(u_s).to(dev).unsqueeze(0)
        mus, var = [], None
        for k in range(K):
            pred = dc.ema(zs[k], lam_t, encoder_hidden_states=conds[k])
            u_pred = dc.ema(zs[k], lam_t, encoder_hidden_states=null)
            mu, var = dc.ddpm_sampler_step(zs[k], pred, u_pred, lam_t.clone().detach(), lam_s.clone().detach())
            mus.append(mu)
        if i == n:
            return torch.stack([dc.clip(mu) for mu in mus], dim=1).to(torch.float32)
        noise = torch.randn_like(mus[0]) if noise_maps is None else noise_maps[i]
        zs = [mu + noise * torch.sqrt(var) for mu in mus]


def run_hip(dc, backbone, x, cl, from_t, rng, seed, units, sampler=None, z0=None, invert=False, w=None, noise_maps=None):
    """All BS x K trajectories on a HIP backbone: trajectory b * K + k is one image of a pair session (unit pair: class token || null
    token), the loop is step-major and chunk-minor, the noise of a step is drawn for the whole batch and read by the K trajectories
    of an image through `dc_ddpm_step_shared`.
    sampler "ddim" / "dpmpp_2m" (solver.py): sampling_steps deterministic passes, one `dc_solver_step` per step and chunk, no draw
    after the start, one history buffer of data predictions for the second-order passes.  z0 [BS, C, H, W]: the start, in place of the
    noised image (no draw at all).  invert: the grid is walked upwards from z = alpha(lam(0)) x to `from_t` (DDIM inversion; K = 1,
    the labels are cl[:, 0]).  w: the guidance weight, config.cfg_w when None.  noise_maps [n, BS, C, H, W] f32 on the device (ancestral
    sampler, with z0; ddpm_invert.py): step i reads noise_maps[i] in place of a draw, so the loop draws nothing."""
    lib = L.require_gpu()
    if not x.is_cuda:
        raise L.DcamdError("counterfactual on a HIP backbone needs a CUDA/HIP tensor (as sample does; no CPU fallback)")
    dev = x.device
    BS, K = cl.shape
    _, Cc, H, W = x.shape
    CHW = Cc * H * W
    patch = int(getattr(backbone.config, "patch_size", 0) or 0)
    oc = int(getattr(backbone.config, "out_channels", Cc) or Cc)
    if oc != Cc:                 # the step kernel indexes the prediction with z's channel count as the feature stride
        raise L.DcamdError(f"fused sampler step needs out_channels == in_channels (got {oc} vs {Cc})")
    philox = rng == "philox"
    if philox and CHW % 4:
        raise L.DcamdError(f"rng='philox' needs C * H * W to be a multiple of 4, got {CHW}")
    steps = torch.linspace(0.0, from_t, dc.config.sampling_steps + 1) if invert else torch.linspace(from_t, 0.0, dc.config.sampling_steps + 1)
    n = len(steps) - 1

    # ---- before the loop: lambda of every grid point (0-dim evaluations, as `sample` forms them), the scalars of every pass ----
    lams = [dc.schedule(steps[j]) for j in range(n + 1)]
    lam_dev = torch.stack([v.detach().float().reshape(()) for v in lams]).to(dev)
    if sampler is None:
        passes = [(i, i + 1) if i < n else (n - 1, n) for i in range(n + 1)]
        scal = [dc._sampler_step_scalars(lams[t], lams[s]) for t, s in passes]
    else:
        passes = [(i, i + 1) for i in range(n)]
        scal = S.step_scalars(lams, sampler, "invert" if invert else "denoise")
    w = float(dc.cfg_w) if w is None else float(w)
    one_plus_w, v_param = float(1.0 + w), int(dc.pred_param == 'v')

    # ---- noise: torch's generators in `sample`'s order, or Philox rows b (initial) and (step + 1) * BS + b ----
    if philox:
        row_ids = torch.arange((n + 1) * BS, dtype=torch.int64, device=dev)
        nbuf = torch.empty((BS, Cc, H, W), dtype=torch.float32, device=dev)

        def draw(row0):
            L.check(lib.dc_philox_normal(nbuf.data_ptr(), BS, CHW, row_ids[row0:row0 + BS].data_ptr(), int(seed), L.stream_ptr()), "dc_philox_normal")
            return nbuf
    if z0 is not None:
        pass
    elif invert:
        z0 = torch.sqrt(torch.sigmoid(lams[0])).to(dev) * x
    elif from_t == 1:
        z0 = draw(0).clone() if philox else torch.randn(x.shape).to(dev)
    else:
        lam = dc.schedule(torch.ones(BS) * from_t).to(dev)
        al, sg = torch.sqrt(torch.sigmoid(lam)).view(-1, 1, 1, 1), torch.sqrt(torch.sigmoid(-lam)).view(-1, 1, 1, 1)
        z0 = al * x + sg * draw(0) if philox else dc.diffuse(x, al, sg)[0]
    za = z0.detach().to(torch.float32).repeat_interleave(K, dim=0).contiguous()          # trajectory b * K + k starts from z0[b]
    zb = torch.empty_like(za)
    hist = torch.empty_like(za) if sampler is not None and any(sc[4] is not None for sc in scal) else None   # x of the pass before

    # ---- once per call and chunk: contexts, lengths, the context plan ----
    chunks = image_chunks(BS, K, units)
    sessions = pair_sessions(dc, backbone, cl, chunks, dev)

    # ---- the loop: step-major, chunk-minor; no device -> host copy ----
    for i, (t, _s) in enumerate(passes):
        noise = None
        if sampler is None:
            c, alpha_t, sigma_t, alpha_s, sd = scal[i]
            if i < n and noise_maps is not None:
                noise = noise_maps[i]
            elif i < n:
                noise = draw((i + 1) * BS) if philox else torch.randn_like(z0).to(torch.float32).contiguous()
        else:
            alpha_t, sigma_t, k1, k2, k3, final = scal[i]
        for (b0, b1), ses in zip(chunks, sessions):
            zc = za[b0 * K:b1 * K]
            pair = ses.step(zc, lam_dev[t:t + 1])
            if sampler is not None:
                # 2M: pass 0 writes the history, a second-order pass reads its element and writes it again; the final pass needs none
                hc = None if hist is None or final else hist[b0 * K:b1 * K].data_ptr()
                p = L.SolverStepParams(z=zc.data_ptr(), pred=pair.data_ptr(), xprev=hc if k3 is not None else None, xhat=hc,
                                       out=zb[b0 * K:b1 * K].data_ptr(), n=(b1 - b0) * K, C=Cc, H=H, W=W, ld=pair.shape[-1], patch=patch,
                                       v_param=v_param, clamp=1, final_pass=int(final), w=w, one_plus_w=one_plus_w, alpha_t=alpha_t,
                                       sigma_t=sigma_t, k1=k1, k2=k2, k3=0.0 if k3 is None else k3)
                L.check(lib.dc_solver_step(C.byref(p), L.stream_ptr()), "dc_solver_step")
                continue
            p = L.DdpmStepSharedParams(z=zc.data_ptr(), pred=pair.data_ptr(), noise=None if noise is None else noise[b0:b1].data_ptr(),
                                       out=zb[b0 * K:b1 * K].data_ptr(), n=(b1 - b0) * K, C=Cc, H=H, W=W, ld=pair.shape[-1], patch=patch,
                                       v_param=v_param, noise_div=K, w=w, alpha_t=alpha_t, sigma_t=sigma_t, alpha_s=alpha_s, c=c, sd=sd,
                                       one_plus_w=one_plus_w, pad_=0)
            L.check(lib.dc_ddpm_step_shared(C.byref(p), L.stream_ptr()), "dc_ddpm_step_shared")
        za, zb = zb, za
    return za.view(BS, K, Cc, H, W)


@torch.no_grad()
def run(dc, x, classes, from_t, against, rng, seed, pixel_space, units_per_launch, start="noise", invert_class=None):
    """`DiffusionClassifier.counterfactual` (its docstring is the interface); units_per_launch(H, W, k) is classify's launch-size rule."""
    sampler = S.sampler_of(dc.config)
    if start not in ("noise", "invert", "ddpm_invert"):
        raise ValueError(f"start must be 'noise', 'invert' or 'ddpm_invert', got {start!r}")
    if start == "invert" and sampler is None:
        raise ValueError("start='invert' needs a deterministic config.sampler ('ddim' or 'dpmpp_2m'): ancestral DDPM adds fresh noise to "
                         "the inverted latent at every step, which defeats the inversion")
    if start == "ddpm_invert" and sampler is not None:
        raise ValueError(f"start='ddpm_invert' needs the ancestral sampler (config.sampler unset or 'ddpm'), got config.sampler = "
                         f"{sampler!r}: its noise maps stand in for the ancestral sampler's draws, a deterministic sampler takes none")
    if start == "noise" and invert_class is not None:
        raise ValueError("invert_class belongs to start='invert' / 'ddpm_invert'")
    if rng not in ("reference", "philox"):
        raise ValueError(f"rng must be 'reference' or 'philox', got {rng!r}")
    from_t = float(from_t)
    if not 0.0 < from_t <= 1.0:
        raise ValueError(f"from_t must lie in (0, 1], got {from_t}")
    if x.dim() != 4:
        raise ValueError(f"x must be [BS, C, H, W], got {tuple(x.shape)}")
    assert dc.encoder_type is not None, "Encoder must be provided for counterfactual sampling."
    dc._require_prompts()
    BS = x.shape[0]
    cl = class_table(classes, BS, dc.config.classes)
    K = cl.shape[1]
    if isinstance(against, str):
        if against != "input":
            raise ValueError(f"against must be 'input' or an int tensor [{BS}] of class ids, got {against!r}")
        base = None
    else:
        base = base_rows(against, cl)
    backbone = dc.ema.ema_model
    hip = hasattr(backbone, "pair_session")
    if not hip:
        if rng == "philox":
            raise L.DcamdError("rng='philox' needs a HIP backbone (UNetCondition2D / DiT)")
        dc._refuse_ragged_on_foreign()
    z0 = nmaps = None
    if start == "invert":
        inv = S.label_rows(invert_class, BS, dc.config.classes, "invert_class")
        z0 = S.invert(dc, x, inv, from_t, 0.0, units_per_launch)         # z_{from_t} of the image itself: no noise is drawn
    elif start == "ddpm_invert":
        # rng and seed govern the inversion's draws; the decode reads its noise from the maps and draws nothing
        inv = DI.invert(dc, x, invert_class, from_t, None, rng, seed, units_per_launch, name="invert_class")
        z0, nmaps, rng = inv.start, inv.noise, "reference"
    if hip:
        samples = run_hip(dc, backbone, x, cl, from_t, rng, seed, units_per_launch(x.shape[2], x.shape[3], 2 * K), sampler=sampler, z0=z0,
                          noise_maps=nmaps)
    else:
        samples = run_foreign(dc, backbone, x, cl, from_t, sampler=sampler, z0=z0, noise_maps=nmaps)
    flat = samples.reshape((BS * K,) + tuple(samples.shape[2:])).contiguous()
    xb = x.detach().to(torch.float32).contiguous()
    if pixel_space:
        # models trained on wavelet_dec_2(image) / 2: back to the image, as the reference's plotters do before they look at a sample
        from .utils.wavelet import wavelet_enc_2
        flat, xb = wavelet_enc_2(flat * 2), wavelet_enc_2(xb * 2)
    r, r_of_a = (xb, torch.arange(BS).repeat_interleave(K)) if base is None else (flat, base)
    maps = abs_diff_map_hip(flat, r, r_of_a) if hip else abs_diff_map_torch(flat, r, r_of_a)
    return Counterfactuals(flat.view((BS, K) + tuple(flat.shape[1:])), cl.to(x.device), maps.view((BS, K) + tuple(maps.shape[1:])))
