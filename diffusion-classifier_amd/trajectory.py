"""What `sample`, `counterfactual`, `invert` and `invert_ddpm` share: the entry checks, the grid of a call (`Grid`: the log-SNR of every
point and what the backbone is fed there; `discrete_steps`: the integer DDPM grid), alpha and sigma of a grid point, the start latent,
the contexts, the eager guided prediction pair, the step kernels' geometry, the noise of a call, and the walk of all trajectories of a
call over a HIP backbone.

The loops themselves live with their arithmetic and none takes a mode flag: the solver walk in solver.py (`run_walk`: the deterministic
decode and, on the upward grid, DDIM inversion) and the ancestral loops in ancestral.py (decode, `sample`'s pair loop, noise maps; each
once in eager torch and once on HIP).  A HIP loop is `for pass: for chunk in walk.run(t, z): one step`.  What the cosine schedules and
the discrete grid do differently in an ancestral step — and a learned variance from a fixed one — is an `ancestral.step_kind`, chosen
once per call; the loops never ask which.  A kind that reads the variance channels says so (`kind.variance`), and the `Walk` then opens
pair sessions whose plans keep them.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L


def units_per_launch(config, H, W, k):
    """Work units one plan launch should hold (k: the units that must stay together); config.units_per_launch overrides the rule."""
    u = config.units_per_launch
    if u is None:
        # ~8M output pixel rows per launch at full resolution (measured on cfg2: 1M -> 4M = +13 %, 4M -> 8M = +2.4 %), but never fewer than 192
        # units: the deep levels of a 256x256 UNet see only units x 64 rows, and 64-unit launches left their GEMMs at
        # 0.2-0.35 PF (IPMSA: 1.14 -> 1.27 img/s; ~200 MB of arena per unit, far inside 288 GB)
        u = max(192, (1 << 23) // (H * W))
    return max(k, int(u))


def check_entry(dc, x, t, name, purpose, rng="reference"):
    """The refusals of an entry point, all before its first draw: the range of `t` (`name`: "from_t" / "to_t"), x's rank, the encoder
    (`purpose` ends the assertion's sentence), the prompt table, the value of `rng`, and Philox or a ragged table in front of a foreign
    module -> (float(t), is the backbone a HIP one)."""
    t = float(t)
    if not 0.0 < t <= 1.0:
        raise ValueError(f"{name} must lie in (0, 1], got {t}")
    if x.dim() != 4:
        raise ValueError(f"x must be [BS, C, H, W], got {tuple(x.shape)}")
    assert dc.encoder_type is not None, f"Encoder must be provided for {purpose}."
    dc._require_prompts()
    if rng not in ("reference", "philox"):
        raise ValueError(f"rng must be 'reference' or 'philox', got {rng!r}")
    hip = hasattr(dc.ema.ema_model, "pair_session")
    if not hip:
        if rng == "philox":
            raise L.DcamdError("rng='philox' needs a HIP backbone (UNetCondition2D / DiT)")
        dc._refuse_ragged_on_foreign()
    return t, hip


def check_decode(dc, decode, pixel_space=False):
    """The refusals of `decode=True` (sample / counterfactual), before the first draw: it needs config.vae_path, and the wavelet form of
    `pixel_space` belongs to models trained on wavelet coefficients, not on VAE latents."""
    if not decode:
        return
    if dc.vae is None:
        raise ValueError("decode=True needs config.vae_path: a LOCAL diffusers AutoencoderKL directory whose decoder turns the latents into images")
    if pixel_space:
        raise ValueError("decode=True cannot be combined with pixel_space=True: a model on VAE latents is not one on wavelet coefficients")


Grid = namedtuple("Grid", ["lam", "label", "steps"])
Grid.__doc__ = """The grid of one call, n + 1 points in the order they are visited.  lam[i]: the log-SNR, a 0-dim fp32 tensor on the host —
every step scalar is a function of two of them.  label[i]: what the backbone is fed at the point — the same tensor on the cosine
schedules, float(k_i) on the discrete grid.  steps: the DDPM steps k_i as Python ints (None on the cosine schedules)."""


def discrete_steps(dc, from_t):
    """schedule='scaled_linear': the DDPM steps k_0 > k_1 > ... > k_n = 0 of a downward walk from `from_t` in n = sampling_steps
    passes, in Python integers only (the floor of an fp32 linspace value times N is off by one unpredictably).  With
    k_top = ddpm_step(from_t), classify's map, and M = k_top + 1:
      config.timestep_spacing = "trailing":  k_i = (M (n - i)) // n - 1                  i < n
                                "leading":   k_i = (n - 1 - i) (M // n) + steps_offset   i < n
    and k_n = 0 in both (abar_0: the published set_alpha_to_one = false).  A grid that is not strictly decreasing down to k_{n-1} >= 1
    or that starts above N - 1 is refused: equal neighbours give c = 0 and sd = 0, and a noise map divides by sd."""
    N, spacing, off = dc.train_timesteps, dc.timestep_spacing, dc.steps_offset
    n = dc.config.sampling_steps
    from_t = float(from_t)
    if not 0.0 < from_t <= 1.0:
        raise ValueError(f"from_t must lie in (0, 1], got {from_t}")
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"config.sampling_steps must be an int >= 1, got {n!r}")
    M = int(dc.ddpm_step(from_t)) + 1
    if spacing == "trailing":
        ks = [(M * (n - i)) // n - 1 for i in range(n)]
    elif spacing == "leading":
        ks = [(n - 1 - i) * (M // n) + off for i in range(n)]
    else:
        raise ValueError(f"the discrete grid needs config.timestep_spacing = 'trailing' | 'leading', got {spacing!r}")
    ks.append(0)
    if ks[0] > N - 1 or ks[n - 1] < 1 or any(a <= b for a, b in zip(ks, ks[1:])):
        raise ValueError(f"sampling_steps = {n} from from_t = {from_t} on N = {N} train steps with timestep_spacing = {spacing!r}"
                         f"{f' (steps_offset = {off})' if spacing == 'leading' else ''} gives the steps {ks}: they must decrease strictly "
                         f"from at most {N - 1} down to k_(n-1) >= 1 and end at 0 (fewer sampling_steps, a larger from_t, or for "
                         "'leading' steps_offset = 1)")
    return ks


def grid(dc, u_from, u_to):
    """The `Grid` of a call from u_from to u_to.  Cosine schedules: the schedule at the points of linspace(u_from, u_to,
    sampling_steps + 1), 0-dim evaluations as `sample` forms them, lam and label the same tensors.  schedule='scaled_linear':
    `discrete_steps` from max(u_from, u_to), reversed for an upward walk (inversion visits the points the decode visits),
    lam = ddpm_logsnr[k_i] and label = float(k_i)."""
    if not dc.discrete:
        pts = torch.linspace(u_from, u_to, dc.config.sampling_steps + 1)
        lam = [dc.schedule(pts[j]) for j in range(len(pts))]
        return Grid(lam, lam, None)
    ks = discrete_steps(dc, max(u_from, u_to))
    if u_from < u_to:
        ks = ks[::-1]
    return Grid([dc.ddpm_logsnr[k] for k in ks], [torch.tensor(float(k), dtype=torch.float32) for k in ks], ks)


def point_scalars(lam):
    """(alpha, sigma) of the grid point with log-SNR `lam`: 0-dim fp32 tensors on the host, the fp32 torch ops every step scalar and
    every latent alpha_i x + sigma_i e_i is formed from."""
    v = lam.detach().float().cpu().reshape(())
    return torch.sqrt(torch.sigmoid(v)), torch.sqrt(torch.sigmoid(-v))


def initial_latent(dc, x, from_t, noise=None):
    """`sample`'s start: randn for from_t == 1, else diffuse(x) to from_t — one draw from torch's generator, or draw 0 of a Philox
    `NoiseSource` (cloned out of its buffer when it is the start itself).  On the discrete grid x is diffused to grid point 0, which
    under 'leading' spacing is not the step from_t falls into."""
    dev = x.device
    philox = noise is not None and noise.philox
    if from_t == 1:
        return noise(0).clone() if philox else torch.randn(x.shape).to(dev)
    if dc.discrete:
        lam = grid(dc, from_t, 0.0).lam[0].expand(x.shape[0]).to(dev)
    else:
        lam = dc.schedule(torch.ones(x.shape[0]) * from_t).to(dev)
    al, sg = torch.sqrt(torch.sigmoid(lam)).view(-1, 1, 1, 1), torch.sqrt(torch.sigmoid(-lam)).view(-1, 1, 1, 1)
    return al * x + sg * noise(0) if philox else dc.diffuse(x, al, sg)[0]


def contexts(dc, text, dev, backbone):
    """(cond, null, lens) of `sample`: the encoded labels, the encoded null token and, for a ragged prompt table, the rows' token counts."""
    cond = null = None
    lens = None
    if text is not None and dc.encoder_type is not None:
        cond = dc.encode_text_prompt(text).to(dev)
        null = dc.encode_text_prompt(torch.full_like(text, dc.null_token)).to(dev)
        if dc._ragged_table():
            if not hasattr(backbone, "make_plan"):
                dc._refuse_ragged_on_foreign()
            ln = dc.encoder.lengths.cpu()
            lens = dict(cond=ln[text.detach().cpu()], null=ln[torch.full_like(text, dc.null_token).cpu()])
    return cond, null, lens


def label_device(dc, dev):
    """Where class ids must live to be encoded: the prompt table's device, else `dev`."""
    return dc.encoder.weight.device if dc.encoder is not None else dev


def guided_pair(dc, z, label, cond, null, lens=None):
    """(pred, u_pred) in eager torch: one conditional and one null backbone call at (z, label), in that order.
    lens: `contexts`' token counts for a ragged table."""
    kc = {"encoder_lengths": lens["cond"]} if lens else {}
    kn = {"encoder_lengths": lens["null"]} if lens else {}
    return dc.ema(z, label, encoder_hidden_states=cond, **kc), dc.ema(z, label, encoder_hidden_states=null, **kn)


def step_fields(dc, backbone, shape, w, noun="fused sampler step", variance=False):
    """The fields every step struct shares but n and ld, for latents of `shape` [*, C, H, W] under guidance weight w.  `patch` is the
    backbone's; the kernels index the prediction with z's channel count as the feature stride, so the prediction must hold C channels:
    out_channels == C, or a backbone whose pair plans project the eps rows only (`eps_rows_only`: DiT) with out_channels == 2 C — the
    learned variance is then not computed at all: these kinds step with the fixed posterior variance.
    variance (the step kind's: `ancestral.LearnedRange`): the kernels read the variance features too, from pair plans that keep the full
    projection (`variance_pair_plans`: DiT) — the fields gain the mode block's mode = DC_STEP_LEARNED_RANGE and fstride =
    out_channels, which must be 2 C, and `v_param` the flag that announces the block (DC_STEP_MODE_BLOCK)."""
    _, Cc, H, W = shape
    oc = int(getattr(backbone.config, "out_channels", Cc) or Cc)
    w = float(w)
    f = dict(C=Cc, H=H, W=W, patch=int(getattr(backbone.config, "patch_size", 0) or 0), v_param=int(dc.pred_param == 'v'),
             w=w, one_plus_w=float(1.0 + w))
    if variance:
        if oc != 2 * Cc:
            raise L.DcamdError(f"{noun} with a learned variance needs out_channels == 2 * in_channels (got {oc} vs 2 * {Cc} = {2 * Cc})")
        if not getattr(backbone, "variance_pair_plans", False):
            raise L.DcamdError(f"{noun} with a learned variance needs a backbone whose pair plans keep the variance features (DiT); "
                               f"{type(backbone).__name__} has none")
        return dict(f, v_param=f["v_param"] | L.STEP_MODE_BLOCK, mode=L.STEP_LEARNED_RANGE, fstride=oc)
    if oc != Cc and not (oc == 2 * Cc and getattr(backbone, "eps_rows_only", False)):
        raise L.DcamdError(f"{noun} needs out_channels == in_channels (got {oc} vs {Cc})")
    return f


class NoiseSource:
    """noise(i): draw i of a call on a HIP backbone, [BS, C, H, W] f32 contiguous on x's device.
    "reference": `torch.randn_like(like)` in call order (like: x until the caller sets another, its dtype is the draw's).
    "philox": `dc_philox_normal` rows i * BS + b keyed by `seed` into ONE reused buffer — row b the start, (step + 1) * BS + b after it."""

    def __init__(self, x, rng, seed, n_draws):
        self.like, self.philox, self.seed = x, rng == "philox", int(seed)
        self.BS, self.CHW = x.shape[0], x[0].numel()
        if self.philox:
            if self.CHW % 4:
                raise L.DcamdError(f"rng='philox' needs C * H * W to be a multiple of 4, got {self.CHW}")
            self.rows = torch.arange(n_draws * self.BS, dtype=torch.int64, device=x.device)
            self.buf = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)

    def __call__(self, i):
        if not self.philox:
            return torch.randn_like(self.like).to(torch.float32).contiguous()
        rows = self.rows[i * self.BS:(i + 1) * self.BS]
        L.check(L.lib().dc_philox_normal(self.buf.data_ptr(), self.BS, self.CHW, rows.data_ptr(), self.seed, L.stream_ptr()), "dc_philox_normal")
        return self.buf


def image_chunks(BS, K, units):
    """Whole images per launch: 2 * K units an image, at most `units` a launch (one image at least), in equal chunks -> [(b0, b1)]."""
    per = max(1, int(units) // (2 * K))
    n_chunks = -(-BS // per)
    per = -(-BS // n_chunks)
    return [(b0, min(BS, b0 + per)) for b0 in range(0, BS, per)]


def pair_sessions(dc, backbone, cl, chunks, dev, variance=False):
    """One pair session per chunk (b0, b1) of images for the labels cl [BS, K]: unit pair b * K + k is class token cl[b, k] || null
    token; contexts, lengths and the context plan once per call and chunk, session ci in slot ci.
    variance: the sessions' plans keep the variance features (the backbone's `pair_session(..., variance=True)`)."""
    lab_dev = label_device(dc, dev)
    ln = dc.encoder.lengths.cpu() if dc._ragged_table() else None
    sessions = []
    for ci, (b0, b1) in enumerate(chunks):
        lab = cl[b0:b1].reshape(-1)
        nul = torch.full_like(lab, dc.null_token)
        cond, null = dc.encode_text_prompt(lab.to(lab_dev)).to(dev), dc.encode_text_prompt(nul.to(lab_dev)).to(dev)
        kw = dict(cond_lengths=ln[lab], null_lengths=ln[nul]) if ln is not None else {}
        if variance:
            kw["variance"] = True
        sessions.append(backbone.pair_session(lab.numel(), dev, cond, null, slot=ci, **kw))
    return sessions


class Walk:
    """The BS x K trajectories of one call on a HIP backbone: trajectory b * K + k is image b under label cl[b, k], one unit pair
    (class token || null token) of a pair session.  Built once per call — the images cut into chunks by classify's launch-size rule,
    one pair session per chunk (the prompts projected once), lambda and the backbone's time input of the `Grid` on the device, the
    step structs' common fields
    — and walked step-major, chunk-minor by the caller's loop; nothing is copied to the host inside it.
    who / noun: the caller's words in the two refusals.  variance: the step kind's `variance` — the sessions' plans then keep the
    variance features and the step fields carry mode and fstride (`step_fields`)."""

    def __init__(self, dc, backbone, x, cl, grid, w, who="counterfactual", noun="fused sampler step", variance=False):
        L.require_gpu()
        if not x.is_cuda:
            raise L.DcamdError(f"{who} on a HIP backbone needs a CUDA/HIP tensor (as sample does; no CPU fallback)")
        self.BS, self.K = cl.shape
        self.shape = tuple(x.shape[1:])
        self.fields = step_fields(dc, backbone, x.shape, w, noun, variance=variance)
        self.chunks = image_chunks(self.BS, self.K, units_per_launch(dc.config, x.shape[2], x.shape[3], 2 * self.K))
        self.lam = torch.stack([v.detach().float().reshape(()) for v in grid.lam]).to(x.device)
        # the cosine schedules feed the backbone the log-SNR itself: one tensor, as ever
        self.label = self.lam if grid.label is grid.lam else torch.stack([v.detach().float().reshape(()) for v in grid.label]).to(x.device)
        self.clamp = int(not dc.discrete)                                     # dc_solver_step's clamp: nothing is clipped on the discrete grid
        # opened at the first pass, behind the caller's draws and blocking host-to-device copies: the context plans then run on the
        # device while the host prepares pass 0, instead of being waited for by the next such copy
        self.sessions, self._open = None, lambda: pair_sessions(dc, backbone, cl, self.chunks, x.device, variance)

    def buffers(self, z0):
        """(za, zb): the trajectories' latents, trajectory b * K + k starting from z0[b], and the buffer the first pass writes."""
        za = z0.detach().to(torch.float32).repeat_interleave(self.K, dim=0).contiguous()
        return za, torch.empty_like(za)

    def view(self, z):
        return z.view((self.BS, self.K) + self.shape)

    def run(self, t, z):
        """Pass t over z [BS * K, C, H, W]: per chunk one session step at (z[rows], label_t), then -> (rows: the chunk's trajectories,
        imgs: its images, f: the step struct's fields z, pred, n, ld and the common ones) for the caller's one kernel."""
        if self.sessions is None:
            self.sessions = self._open()
        for (b0, b1), ses in zip(self.chunks, self.sessions):
            rows = slice(b0 * self.K, b1 * self.K)
            pair = ses.step(z[rows], self.label[t:t + 1])
            yield rows, slice(b0, b1), dict(self.fields, z=z[rows].data_ptr(), pred=pair.data_ptr(), n=(b1 - b0) * self.K, ld=pair.shape[-1])


# ---- the C ABI of the step mode (include/dcamd.h DC_STEP_MODE_BLOCK) ------------------------------------------------------------------
MODE_BLOCK = [("mode", L.i32), ("fstride", L.i32), ("k1", L.f32), ("k2", L.f32), ("log_hi", L.f32), ("log_lo", L.f32)]
_with_mode = {}


def mode_params(cls):
    """L.DdpmStepSharedParams / L.DdpmNoiseMapParams -> the ctypes class of the struct WITH the mode block behind it, as the two entries
    read it when `v_param` carries L.STEP_MODE_BLOCK: the struct's own fields, then mode, fstride, k1, k2, log_hi, log_lo at sizeof of
    the struct.  The header declares no such struct (its structs are frozen); this flat class has the same layout, checked here."""
    if cls not in _with_mode:
        ext = type(cls.__name__ + "Mode", (C.Structure,), {"_fields_": list(cls._fields_) + MODE_BLOCK})
        assert C.sizeof(cls) % 8 == 0 and ext.mode.offset == C.sizeof(cls) and C.sizeof(ext) == C.sizeof(cls) + 24, cls
        _with_mode[cls] = ext
    return _with_mode[cls]


def launch(entry, params, base=None):
    """One step kernel on the current stream: entry "dc_solver_step" | "dc_ddpm_step_shared" | "dc_ddpm_noise_map".
    base: the entry's own struct class when `params` is that struct with the mode block behind it (`mode_params`)."""
    ref = C.byref(params) if base is None else C.cast(C.pointer(params), C.POINTER(base))
    L.check(getattr(L.lib(), entry)(ref, L.stream_ptr()), entry)
