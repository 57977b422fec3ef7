"""Counterfactual explanations: one image denoised under every class label from shared noise, and where the results differ.

The reference's procedure (experiments/ipmsa/explain.py) noises an image to `from_t`, runs `sample` once per class label with the seed
reset in front of each run, and compares the generated images.  `DiffusionClassifier.counterfactual` is that procedure as one call:
  samples [BS, K, C, H, W]   samples[b, k] = what `sample(x, classes[:, k], from_t)` returns for image b; the K trajectories of an image
                             start from one z_{from_t} and add one noise draw per step (common random numbers by construction)
  maps [BS, K, H', W']       maps[b, k] = sum_c |samples[b, k, c] - base[b, c]|, c ascending, fp32; base = the input image or the
                             trajectory of one of the classes
HIP backbones run all BS x K trajectories as the units of one pair session per chunk of images (a `trajectory.Walk`: the prompts are
projected once per call, the step scalars are formed before the loop, nothing is copied to the host inside it); the ancestral loop on
it is `ancestral.decode_hip` (`dc_ddpm_step_shared` on the cosine schedules), the maps are `dc_abs_diff_map`.  A foreign nn.Module takes
the reference's own form in eager torch (`run_foreign`, `run_foreign_solver`): it is the written statement.
With config.sampler = "ddim" | "dpmpp_2m" the trajectories are deterministic after their start (`solver.run_walk`), and
start="invert" takes that start from DDIM inversion of the image instead of from noise.  Under the ancestral sampler
start="ddpm_invert" takes the start AND the noise of every step from the image's edit-friendly DDPM inversion (ddpm_invert.py): the
decode under the inversion's class is the image again, and the loop draws nothing: `run` hands the decode the maps as its noise.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L
from . import ancestral as AN
from . import ddpm_invert as DI
from . import solver as S
from . import trajectory as TJ
from .trajectory import image_chunks      # noqa: F401  (its home is the walk; importable here as ever)

Counterfactuals = namedtuple("Counterfactuals", ["samples", "classes", "maps"])
Counterfactuals.__doc__ = """Result of `DiffusionClassifier.counterfactual` (tensors on the input's device).
samples [BS, K, C, H, W] f32 (pixel_space: [BS, K, C / 4, 2H, 2W]; decode: [BS, K, out_channels, f H, f W], images), classes [BS, K] int64 (the label of every trajectory),
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


def column_contexts(dc, cl, dev):
    """(conds, null) of a foreign module: the encoded labels of every column of cl [BS, K] and the encoded null token, at batch BS."""
    labs = [cl[:, k].to(TJ.label_device(dc, dev)) for k in range(cl.shape[1])]
    return [dc.encode_text_prompt(lab).to(dev) for lab in labs], dc.encode_text_prompt(torch.full_like(labs[0], dc.null_token)).to(dev)


def run_foreign(dc, z0, cl, from_t, noise_maps=None):
    """The reference's form from the start z0 [BS, C, H, W]: `ancestral.ancestral_eager` over the K columns of cl, every class adding
    the step's one `randn_like` — or, with noise_maps [n, BS, C, H, W] (ddpm_invert.py), noise_maps[i] in place of the draw."""
    conds, null = column_contexts(dc, cl, z0.device)
    kind = AN.step_kind(dc, TJ.grid(dc, from_t, 0.0), dc.cfg_w)
    return torch.stack(AN.ancestral_eager(kind, z0, conds, null, noise_maps=noise_maps), dim=1).to(torch.float32)


def run_foreign_solver(dc, z0, cl, from_t, sampler):
    """The same under "ddim" / "dpmpp_2m": the K classes by `solver.run_eager` from the one start, no draw after it."""
    conds, null = column_contexts(dc, cl, z0.device)
    g = TJ.grid(dc, from_t, 0.0)
    scal = S.denoise_scalars(dc, g, sampler)
    return torch.stack([S.run_eager(dc, z0, g, scal, dc.cfg_w, cond, null) for cond in conds], dim=1).to(torch.float32)


@torch.no_grad()
def run(dc, x, classes, from_t, against, rng, seed, pixel_space, start="noise", invert_class=None, decode=False):
    """`DiffusionClassifier.counterfactual` (its docstring is the interface)."""
    TJ.check_decode(dc, decode, pixel_space)
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
    from_t, hip = TJ.check_entry(dc, x, from_t, "from_t", "counterfactual sampling", rng)
    BS = x.shape[0]
    cl = class_table(classes, BS, dc.config.classes)
    K = cl.shape[1]
    if isinstance(against, str):
        if against != "input":
            raise ValueError(f"against must be 'input' or an int tensor [{BS}] of class ids, got {against!r}")
        base = None
    else:
        base = base_rows(against, cl)
    z0 = nmaps = None
    if start == "invert":
        inv = S.label_rows(invert_class, BS, dc.config.classes, "invert_class")
        z0 = S.invert(dc, x, inv, from_t, 0.0)                           # z_{from_t} of the image itself: no noise is drawn
    elif start == "ddpm_invert":
        # rng and seed govern the inversion's draws; the decode reads its noise from the maps and draws nothing
        inv = DI.invert(dc, x, invert_class, from_t, None, rng, seed, name="invert_class")
        z0, nmaps = inv.start, inv.noise
    if hip:
        # the walk's refusals before the first draw here; its sessions open at its first pass, after the inversions' (the same slots)
        g = TJ.grid(dc, from_t, 0.0)
        kind = None if sampler is not None else AN.step_kind(dc, g, dc.cfg_w)
        walk = TJ.Walk(dc, dc.ema.ema_model, x, cl, g, dc.cfg_w, variance=kind is not None and kind.variance)
        noise = TJ.NoiseSource(x, rng, seed, len(g.lam))
        if z0 is None:
            z0 = S.initial_latent(dc, x, from_t, noise)
        if sampler is not None:
            samples = S.run_walk(walk, z0, S.denoise_scalars(dc, g, sampler))
        else:
            noise.like = z0                                              # the steps draw in the start's dtype, as `sample` does
            draw = nmaps.__getitem__ if nmaps is not None else lambda i: noise(i + 1)
            samples = AN.decode_hip(kind, walk, z0, draw)
    else:
        z0 = S.initial_latent(dc, x, from_t) if z0 is None else z0
        samples = run_foreign(dc, z0, cl, from_t, nmaps) if sampler is None else run_foreign_solver(dc, z0, cl, from_t, sampler)
    flat = samples.reshape((BS * K,) + tuple(samples.shape[2:])).contiguous()
    xb = x.detach().to(torch.float32).contiguous()
    if pixel_space:
        # models trained on wavelet_dec_2(image) / 2: back to the image, as the reference's plotters do before they look at a sample
        from .utils.wavelet import wavelet_enc_2
        flat, xb = wavelet_enc_2(flat * 2), wavelet_enc_2(xb * 2)
    if decode:
        # latents -> images (config.vae_path); against="input": the base is the VAE's own reconstruction of x, so the map holds the
        # label's effect and no reconstruction error
        flat = dc.decode_latents(flat)
        xb = dc.decode_latents(xb) if base is None else xb
    r, r_of_a = (xb, torch.arange(BS).repeat_interleave(K)) if base is None else (flat, base)
    maps = abs_diff_map_hip(flat, r, r_of_a) if hip else abs_diff_map_torch(flat, r, r_of_a)
    return Counterfactuals(flat.view((BS, K) + tuple(flat.shape[1:])), cl.to(x.device), maps.view((BS, K) + tuple(maps.shape[1:])))
