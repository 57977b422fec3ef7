"""MI355X-native drop-in for the scoring API of reference `diffusion/diffusion_classifier.py`.

Kept surface (same names, argument meaning, assertions and return types):
  DiffusionClassifier(backbone, config)                         reference :17-81
  .classify(x, text=None, fast=False) -> LongTensor[BS]         reference :657-725
  .evaluate(val_dataloader, stop_idx, metrics, classification)  reference :532-578
  .loss(x, text=None)                                           reference :295-344, forward only (training is not part of this project)
  .encode_text_prompt / .diffuse / .logsnr_schedule_cosine(_shifted)  :83-161
`config.encoder_type`: 'nn' and 'DiT' as in the reference; 'prompt' (additive, with `config.prompt_tokens = S`) conditions on a table of
per-class prompts [classes + 1, S, hid] — the [B, S, hid] the reference's text encoder hands to the backbone (:93-98), without fetching one.
't5' (with `config.t5_path`, a LOCAL Hugging Face directory, and `config.prompt_tokens = S`) runs the T5 encoder on the device
(nets/t5.py) and fills the same table: `set_class_prompts(input_ids, attention_mask)`, then everything is the 'prompt' path.
'clip' (additive, with `config.clip_path` and `config.prompt_tokens = S`) does the same with a CLIP text transformer (nets/clip.py).
'clip_dual' (additive, with `config.clip_path`, `config.clip2_path`, optionally `config.clip2_variant` and `config.add_time_ids`) is the
conditioning of a StableDiffusionXLUNet: both CLIP text encoders read at their penultimate layer fill the table side by side, the second
one's projected pooled output fills `pooled_table` next to it, and six size numbers shared by all classes go with them
(`set_class_prompts(ids, mask, input_ids_2=, attention_mask_2=)`, `set_pooled`); scoring only — `sample`, `counterfactual`, `invert` and
`invert_ddpm` raise NotImplementedError under it.
`config.schedule`: 'cosine' and 'shifted_cosine' as in the reference; 'scaled_linear' (additive) is the discrete DDPM schedule a Stable
Diffusion UNet is trained on — `train_timesteps` (1000) steps, `beta_start` / `beta_end` (0.00085 / 0.012), optionally read from
`scheduler_path` (a local diffusers scheduler_config.json); 'ddpm_linear' (additive) is the DDPM paper's grid a published DiT is trained
on, betas = linspace(beta_start, beta_end) (1e-4 / 0.02), diffusers' beta_schedule = "linear", and everything below holds for it as for
'scaled_linear'.  `schedule(t)` is then the log-SNR of the step t falls into, and the backbone
is fed `noise_labels(t)`, that step as a float, instead of the log-SNR.  Generation on that grid is opt-in: with
`config.timestep_spacing` = "trailing" | "leading" (additive; diffusers' two integer spacings, `steps_offset` an additive int read from
`scheduler_path` too) `sample`, `counterfactual`, `invert` and `invert_ddpm` walk the integer steps k_0 > ... > k_n = 0 of
`trajectory.discrete_steps`, feed the backbone float(k_i), take every scalar from the step's log-SNR and clip nothing (scaled VAE latents
are not in [-1, 1]); without the key they raise NotImplementedError under this schedule, with it under a cosine schedule ValueError.
`config` is the reference's attribute bag (missing keys read as None).  Additive keys read
here: `compute_dtype` ("bf16" default | "f16" | "f32"), `units_per_launch`, `score_plan_cache` (launch plans kept, LRU;
default 6), `dwt_on_device` (True: `inference` applies `wavelet_dec_2(images) / 2` on the device to the batches its loader yields, on the
prefetch stream), `shard_grid` (opt-in: True
shards the (trial, image) grid of ONE replicated batch over the default process group),
`simulate_rank` ((r, N), bench.py only: time rank r's share of an N-rank sharded call on one GPU),
`stop_margin_z` (opt-in per-image early stopping, see below; None: off, none of its code runs),
`score_loss` (None | "l2" | "l1" | "huber": the per-element term summed into classify's errors and evidence maps, with `huber_delta`
(default 1.0) for "huber"; read once at construction; None / "l2": the reference's squared error, bit for bit; loss.py),
`trial_weighting` (None | "uniform" | "train" | a callable f(logsnr [T, BS]) -> weights | under the discrete schedules a 1-D sequence of
`train_timesteps` weights: a weight per (trial, image) on classify's errors and evidence maps, "train" being the truncated-SNR weight of
the reference's training loss with its clamp `min_snr_gamma`, default 5.0; read once at construction; with `simulate_rank` ValueError;
None / "uniform": nothing changes, bit for bit; loss.py), `pixel_weight_key` (`evaluate` / `inference` in classification mode hand
batch[key] to `classify(..., pixel_weight=)`),
`vae_path` (a LOCAL diffusers AutoencoderKL directory: `classify` encodes images to latents on the device first, nets/vae.py;
`vae_dtype` its compute dtype, default the backbone's; `encode_latents(x)`; `classify(..., latents=True)` takes latents as they are;
`decode_latents(z)` is the way back through the same directory's decoder, loaded at its first call, at most `vae_decode_batch` (default 8)
images per launch plan; `sample(..., decode=True)` and `counterfactual(..., decode=True)` return images instead of latents).

What differs is HOW classify runs: the (image, trial, class) grid is flattened into micro-batches of work units, one native call each,
with the stage ends on the device — scoring.py (`_HipRunner`; a foreign `nn.Module` backbone takes `_ForeignRunner`, eager torch).

Per-image early stopping (`config.stop_margin_z` = a float > 0; +inf: never stop; anything else, or the key together with
`simulate_rank`, raises ValueError): stage pruning drops classes, never images — with two classes every image pays all T trials.
With the key set, the stages are checkpoints: after stage i < n_stages - 1 (and after its top-k pruning) every image still active
stops iff the posterior's margin_z over its cells j < t_end is >= stop_margin_z (posterior.py has the rule).  A stopped image keeps label = winner and t_done = t_end, its cells j >= t_done stay +inf for good, and it is in no
later stage's pairs: the work of a batch is sum_b t_done[b] (trial, image) pairs instead of BS * T.  The last stage ends as always,
the images that got there take its label and t_done = T; if no image is left after a checkpoint the remaining stages are skipped.
With +inf labels, errors and posterior are bit-identical to the key unset.  `stop_margin_z` is NOT a one-shot significance level
(sequential testing, posterior.py): calibrate the threshold on held-out data.  How and at what price the device decides: scoring.py.

Extra keyword-only arguments (defaults keep the reference behaviour):
  t, eps         inject the per-trial draws ([T,BS] and [T,BS,C,H,W]) — parity tests
  fast_select    inject the `randint` draw of fast mode
  return_errors  also return errors[BS, classes, T] (copied to the CPU; with the multi-GPU gather's host leg under gloo
                 the only device -> host copies of a classify call)
  return_posterior  also return a `ClassPosterior` (posterior.py): class probabilities softmax(-delta / config.posterior_temperature) on the
                 paired mean differences to the winner, their entropy, the runner-up with the paired margin and its z-score, trials per
                 class and the NaN-cell count, computed after the last stage end from the gathered errors (`dc_class_posterior` for the
                 HIP backbones, the same definitions in torch for a foreign one), left on the scoring device: no host synchronisation,
                 identical on every rank.  argmax probs is the label.  Returns (labels, post), with return_errors (labels, errors, post).
                 With stop_margin_z every image is evaluated over its own [0, t_done[b]) (one launch per stage end that was reached
                 and a row select on the device); `n_trials` then reports the trials each image used
  return_evidence  also return a `ClassEvidence` (evidence.py): per-pixel maps [BS, classes, H, W] of the mean squared eps-error of every
                 class and of its paired difference to the posterior's winner (the spatial form of the posterior's delta; exactly 0 for
                 the winner), from the predictions the scoring loop already holds — one more elementwise op per launch (`dc_err_map`:
                 fixed-point int64 sums, the same bits for every micro-batch split and world size), one `dc_evidence_maps` at the end
                 and, under grid sharding, one int64 all-reduce per call; no backbone forward is added.  Placed after the posterior and
                 before t_done in the returned tuple.  T <= 2^18; with `simulate_rank` ValueError.  Models trained on
                 `wavelet_dec_2(image) / 2`: the maps live on the wavelet grid
  pixel_weight   a float tensor [BS, H, W] or [BS, 1, H, W] on the model's grid: the per-pixel weight of every term in the errors and the
                 evidence maps (a 0/1 mask scores a region; loss.py); None: nothing changes, bit for bit
  return_trials  also return t_done, int32 [BS] on the scoring device, as the LAST element of the tuple: the trials each image was
                 scored on (T everywhere when stop_margin_z is unset)
  rng            "reference": draw rand(BS) / randn_like(x) per trial in the reference's order;
                 "philox":   t from the CPU generator, eps on device from Philox keyed by
                             (seed, image, trial) — no eps traffic, world-size independent
  group          a torch.distributed process group: shard the (trial, image) grid of THIS batch over its
                 ranks (every rank must pass the identical x; checked).  Default (None, `shard_grid`
                 unset): no grid sharding — under `accelerate launch` each rank scores its own images,
                 exactly like the reference (:615-617).

Additive: `.counterfactual(x, classes, from_t, ...)` — every class from shared noise in one call, with difference maps (the
reference's experiments/ipmsa/explain.py procedure; counterfactual.py).  `config.sampler` ("ddim" | "dpmpp_2m"; unset or "ddpm": the
ancestral sampler) makes `sample` and `counterfactual` deterministic after their start, `.invert(x, text, to_t)` is DDIM inversion and
`counterfactual(..., start="invert")` decodes every class from the image's own inverted latent (solver.py).
`.invert_ddpm(x, text, from_t)` is the edit-friendly DDPM inversion — a start and one noise map per step under which the ancestral sampler
decodes the image back exactly — and `counterfactual(..., start="ddpm_invert")` decodes every class from it (ddpm_invert.py;
`ddpm_invert_max_bytes` caps the maps' buffer, default 2 GiB).
`config.variance` (None | "fixed" | "learned"; read once at construction) chooses the deviation of an ancestral step on the discrete
grid: "learned" takes it, per element, from the variance channels a model with out_channels = 2 * in_channels predicts next to eps
(a published DiT; diffusers' variance_type = "learned_range") in `sample`, `counterfactual` and `invert_ddpm`; `classify` and `invert`
do not read it.  None / "fixed": the fixed posterior variance, everything as before, bit for bit.
"""
import math
import os

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ancestral as AN
from .. import dist as D
from .. import counterfactual as CF
from .. import ddpm_invert as DI
from .. import posterior as P
from .. import evidence as EV
from .. import loss as LS
from .. import solver as S
from .. import trajectory as TJ
from ..scoring import _ForeignRunner, _HipRunner      # (tests and tools reach the runners through this module)
from .._ema import EMA


def log(t, eps=1e-20):
    return torch.log(t.clamp(min=eps))


class PromptTable(nn.Module):
    """encoder_type='prompt': one prompt of S token embeddings per class, `weight` [classes + 1, S, encoder_hid_dim] (the last row is the
    null prompt, as for 'nn').  The place for per-class text embeddings computed offline (T5, CLIP, a learned soft prompt): copy them
    into `weight`; the parameter keeps the name `weight`, so a checkpoint carries it as `model_2.safetensors` like nn.Embedding's.

    Prompts of different lengths: `lengths` [rows] int64 (a buffer; S everywhere by default) says how many of a row's S tokens are
    attended, the rest being padding whose content is never read — `set_prompt(row, emb)` for one prompt, or copy a text encoder's
    padded output into `weight` and hand the token counts to `set_lengths`.  A table whose lengths are all S saves exactly
    `["weight"]`, as before; a ragged one adds `"lengths"`; loading takes both forms (no `"lengths"`: all S)."""

    def __init__(self, rows, tokens, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(rows, tokens, dim))
        self.register_buffer("lengths", torch.full((rows,), tokens, dtype=torch.int64))
        self._ragged = False         # host copy of `(lengths != S).any()`: asked per plan lookup, must not synchronise with the device

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if not self._ragged:
            destination.pop(prefix + "lengths", None)

    def _load_from_state_dict(self, state_dict, prefix, *args):
        ln = state_dict.get(prefix + "lengths")
        if ln is None:
            ln = state_dict[prefix + "lengths"] = torch.full_like(self.lengths, self.weight.shape[1])
        self._check(ln.cpu())
        self._ragged = bool((ln != self.weight.shape[1]).any())
        super()._load_from_state_dict(state_dict, prefix, *args)

    def _check(self, ln):
        rows, S = self.weight.shape[0], self.weight.shape[1]
        if ln.dim() != 1 or ln.numel() != rows or ln.dtype.is_floating_point or ln.dtype == torch.bool:
            raise ValueError(f"prompt lengths must be an int sequence of {rows} entries, got {ln.dtype} {tuple(ln.shape)}")
        if int(ln.min()) < 1 or int(ln.max()) > S:
            raise ValueError(f"prompt lengths must lie in [1, {S}], got {ln.tolist()}")

    @property
    def varlen(self):
        """Does any prompt have fewer than S tokens (known on the host: no device read)?"""
        return self._ragged

    @torch.no_grad()
    def set_lengths(self, seq):
        """Token counts of all rows (1 <= len <= S), for a `weight` filled with padded text-encoder output."""
        ln = torch.as_tensor(seq).detach().cpu()
        self._check(ln)
        self.lengths.copy_(ln.to(torch.int64))
        self._ragged = bool((ln != self.weight.shape[1]).any())

    @torch.no_grad()
    def set_prompt(self, row, emb):
        """Prompt `row` := emb [len, hid] with 1 <= len <= S: writes its tokens, zeroes the pad rows and records the length."""
        S, hid = self.weight.shape[1], self.weight.shape[2]
        emb = torch.as_tensor(emb)
        if emb.dim() != 2 or emb.shape[1] != hid or not 1 <= emb.shape[0] <= S:
            raise ValueError(f"a prompt must be [len, {hid}] with 1 <= len <= {S}, got {tuple(emb.shape)}")
        n = int(emb.shape[0])
        self.weight[row, :n] = emb.to(self.weight.device, self.weight.dtype)
        self.weight[row, n:] = 0
        self.lengths[row] = n
        self._ragged = bool((self.lengths.cpu() != S).any())

    def forward(self, ids):
        return self.weight[ids]


class DiffusionClassifier(nn.Module):
    def __init__(self, backbone: nn.Module, config):
        super().__init__()
        self.config = config
        pred_param = self.config.pred_param
        assert pred_param in ['v', 'eps'], "Invalid prediction parameterization. Must be 'v' or 'eps'"
        self.pred_param = pred_param
        self.score_loss = LS.score_loss_of(self.config)      # (kind, huber delta) of classify's errors and maps; ValueError for bad keys
        schedule = self.config.schedule
        assert schedule in ['cosine', 'shifted_cosine', 'scaled_linear', 'ddpm_linear'], \
            "Invalid schedule. Must be 'cosine', 'shifted_cosine', 'scaled_linear' or 'ddpm_linear'"
        self.discrete = schedule in self.DISCRETE      # the backbone's time input is then the DDPM step, not the log-SNR (noise_labels)
        spacing = self.config.timestep_spacing
        if spacing not in (None, "trailing", "leading"):
            raise ValueError(f"config.timestep_spacing must be None, 'trailing' or 'leading', got {spacing!r}")
        if spacing is not None and not self.discrete:
            raise ValueError(f"config.timestep_spacing = {spacing!r} belongs to the discrete grid of schedule='scaled_linear' / 'ddpm_linear', "
                             f"not to schedule={schedule!r}: the cosine schedules generate on linspace(from_t, 0, sampling_steps + 1)")
        self.timestep_spacing = spacing
        if self.discrete:
            self._init_discrete(schedule)
            self.schedule = self.logsnr_schedule_discrete
        else:
            self.schedule = self.logsnr_schedule_cosine if schedule == 'cosine' else self.logsnr_schedule_cosine_shifted
        # the per-trial weights of classify's errors and maps (loss.py): None, or what `trial_weights` turns into `weight` per call
        self.trial_weighting = LS.trial_weighting_of(self.config, self.train_timesteps if self.discrete else None)
        self.noise_d = self.config.noise_d
        self.image_d = self.config.image_size
        self.cfg_w = self.config.cfg_w
        assert isinstance(backbone, nn.Module), "Model must be an instance of torch.nn.Module."
        self.variance = self._variance_of(backbone)      # None | "learned": which ancestral step kind generation takes (ancestral.py)
        self.model = backbone
        self.ema = EMA(self.model, beta=config.ema_beta, update_after_step=config.ema_warmup,
                       update_every=config.ema_update_freq)
        self.encoder_type = self.config.encoder_type
        if self.encoder_type == 't5' and self.config.t5_path is None:
            raise NotImplementedError("encoder_type='t5' fetches t5-base over the network; not part of the scoring path. Text embeddings "
                                      "computed offline run through encoder_type='prompt' (config.prompt_tokens = S; copy them into "
                                      "encoder.weight [classes + 1, S, encoder_hid_dim])")
        elif self.encoder_type == 't5':
            # the reference's T5EncoderModel (:59-74), from a local directory; its output for one prompt per class (and the null prompt) fills
            # the table 'prompt' uses — the reference's own 't5' loop hands integer class ids to the tokenizer (:695-698), which cannot classify
            from ..nets.t5 import T5Encoder
            S = self.config.prompt_tokens
            assert isinstance(S, int) and S >= 1, "encoder_type='t5' needs config.prompt_tokens = S >= 1"
            hid = getattr(backbone.config, "encoder_hid_dim", None)
            if hid is None:
                raise NotImplementedError("encoder_type='t5' needs a backbone with a projected context (config.encoder_hid_dim: UNetCondition2D)")
            self.text_encoder = T5Encoder.from_directory(self.config.t5_path)
            if self.text_encoder.config.d_model != hid:
                raise ValueError(f"backbone.config.encoder_hid_dim = {hid} but the T5 encoder under {self.config.t5_path} has "
                                 f"d_model = {self.text_encoder.config.d_model}")
            self.encoder = PromptTable(self.config.classes + 1, S, hid)      # model_2.safetensors stays the table: no T5 weights in a checkpoint
            self.tokenizer = None
            self.null_token = self.config.classes
            self._prompts_set = False
        elif self.encoder_type == 'clip':
            # a CLIP text transformer from a local directory (Stable Diffusion's text_encoder/, openai/clip-vit-*): its last_hidden_state
            # for one prompt per class (and the null prompt) fills the table 'prompt' uses, exactly as 't5' does
            if self.config.clip_path is None:
                raise NotImplementedError("encoder_type='clip' needs config.clip_path: a LOCAL Hugging Face directory (config.json + "
                                          "model.safetensors of a CLIP text model; nothing is fetched). Text embeddings computed offline "
                                          "run through encoder_type='prompt' (config.prompt_tokens = S; copy them into encoder.weight "
                                          "[classes + 1, S, encoder_hid_dim])")
            from ..nets.clip import CLIPTextEncoder
            S = self.config.prompt_tokens
            assert isinstance(S, int) and S >= 1, "encoder_type='clip' needs config.prompt_tokens = S >= 1"
            hid = getattr(backbone.config, "encoder_hid_dim", None)
            if hid is None:
                raise NotImplementedError("encoder_type='clip' needs a backbone with a projected context (config.encoder_hid_dim: UNetCondition2D)")
            self.text_encoder = CLIPTextEncoder.from_directory(self.config.clip_path)
            if self.text_encoder.config.hidden_size != hid:
                raise ValueError(f"backbone.config.encoder_hid_dim = {hid} but the CLIP text encoder under {self.config.clip_path} has "
                                 f"hidden_size = {self.text_encoder.config.hidden_size}")
            self.encoder = PromptTable(self.config.classes + 1, S, hid)      # model_2.safetensors stays the table: no CLIP weights in a checkpoint
            self.tokenizer = None
            self.null_token = self.config.classes
            self._prompts_set = False
        elif self.encoder_type == 'clip_dual':
            self._init_clip_dual(backbone)
        elif self.encoder_type == 'prompt':
            S = self.config.prompt_tokens
            assert isinstance(S, int) and S >= 1, "encoder_type='prompt' needs config.prompt_tokens = S >= 1"
            hid = getattr(backbone.config, "encoder_hid_dim", None)
            if hid is None:
                raise NotImplementedError("encoder_type='prompt' needs a backbone with a projected context (config.encoder_hid_dim: UNetCondition2D)")
            self.encoder = PromptTable(self.config.classes + 1, S, hid)
            self.tokenizer = None
            self.null_token = self.config.classes
        elif self.encoder_type == 'nn':
            self.encoder = nn.Embedding(self.config.classes + 1, backbone.config.encoder_hid_dim)
            self.tokenizer = None
            self.null_token = self.config.classes
        elif self.encoder_type == 'DiT':
            self.tokenizer = None
            self.encoder = None
            self.null_token = self.config.classes
        print(f"Parameter count: {sum(p.numel() for p in self.model.parameters())}")
        # latent-space backbones (additive key vae_path): the encoder half of an AutoencoderKL from a local diffusers directory, in front
        # of classify; a submodule, so it moves with the classifier.  Without the key nothing below exists
        self.vae = None
        if self.config.vae_path is not None:
            from ..nets.vae import VAEEncoder
            self.vae = VAEEncoder.from_directory(self.config.vae_path)
            self.vae.set_compute_dtype(self.config.vae_dtype or self.config.compute_dtype or "bf16")
            zc, ic = self.vae.config.latent_channels, getattr(backbone.config, "in_channels", None)
            if ic != zc:
                raise ValueError(f"backbone.config.in_channels = {ic} but the VAE under {self.config.vae_path} has latent_channels = {zc}")
        object.__setattr__(self, "_vae_decoder", None)      # decode_latents loads it; never a submodule: state_dict stays as it is
        self._score_plans = {}
        self._timed_sink = None      # bench.py: list collecting (plan, per-op event ms) instead of plain runs

    # ---- encoder_type='clip_dual' (additive): the conditioning of a Stable Diffusion XL UNet ----
    def _init_clip_dual(self, backbone):
        """Two CLIP text encoders from LOCAL directories: config.clip_path (SDXL's text_encoder/, a CLIPTextEncoder) and
        config.clip2_path (text_encoder_2/, a CLIPTextEncoderWithProjection; config.clip2_variant = "fp16" reads model.fp16.safetensors),
        both read at layer=-2, the second also pooled.  The prompt table [classes + 1, S, hidden_1 + hidden_2] holds the two
        penultimate states side by side, encoder 1 first, as diffusers concatenates them; next to it `pooled_table`
        [classes + 1, projection_dim], a buffer registered under this encoder type only.  config.add_time_ids: diffusers' six numbers
        (original_h, original_w, crop_top, crop_left, target_h, target_w), one set for all classes and images; None: (s, s, 0, 0, s, s)
        with s = config.image_size."""
        cfg = self.config
        for key in ("clip_path", "clip2_path"):
            if getattr(cfg, key) is None:
                raise NotImplementedError(f"encoder_type='clip_dual' needs config.{key}: LOCAL Hugging Face directories of the two CLIP text "
                                          "models of a Stable Diffusion XL pipeline (clip_path: text_encoder/, clip2_path: text_encoder_2/; "
                                          "nothing is fetched)")
        from ..nets.clip import CLIPTextEncoder, CLIPTextEncoderWithProjection
        S = cfg.prompt_tokens
        assert isinstance(S, int) and S >= 2, "encoder_type='clip_dual' needs config.prompt_tokens = S >= 2"
        self.text_encoder = CLIPTextEncoder.from_directory(cfg.clip_path)
        self.text_encoder_2 = CLIPTextEncoderWithProjection.from_directory(cfg.clip2_path, variant=cfg.clip2_variant)
        h1, h2, P_ = self.text_encoder.config.hidden_size, self.text_encoder_2.config.hidden_size, self.text_encoder_2.config.projection_dim
        bc = backbone.config
        xdim = getattr(bc, "cross_attention_dim", None)
        if h1 + h2 != xdim:
            raise ValueError(f"the two CLIP text encoders are {h1} + {h2} = {h1 + h2} wide but backbone.config.cross_attention_dim = {xdim}")
        dim, pcid = getattr(bc, "addition_time_embed_dim", None), getattr(bc, "projection_class_embeddings_input_dim", None)
        if dim is None or pcid is None or P_ + 6 * dim != pcid:
            raise ValueError(f"projection_dim + 6 * addition_time_embed_dim = {P_} + 6 * {dim} but "
                             f"backbone.config.projection_class_embeddings_input_dim = {pcid}")
        ids = cfg.add_time_ids
        if ids is None:
            s = float(cfg.image_size)
            ids = (s, s, 0.0, 0.0, s, s)
        ids = torch.as_tensor(ids, dtype=torch.float32).reshape(-1)
        if ids.numel() != 6:
            raise ValueError(f"config.add_time_ids must be six numbers (original_h, original_w, crop_top, crop_left, target_h, target_w), "
                             f"got {ids.numel()}")
        self.add_time_ids = ids                          # plain attribute: host data, one set for every class and image
        self.encoder = PromptTable(cfg.classes + 1, S, h1 + h2)
        self.register_buffer("pooled_table", torch.zeros(cfg.classes + 1, P_))
        self.tokenizer = None
        self.null_token = cfg.classes
        self._prompts_set = False
        self._pooled_rows = set()                        # rows given through set_pooled: a table filled by hand needs all of them

    @torch.no_grad()
    def set_pooled(self, row, vec):
        """encoder_type='clip_dual': pooled row `row` := vec [projection_dim], the way PromptTable.set_prompt sets a prompt row (for
        text embeddings computed offline; `set_class_prompts` fills both tables from token ids)."""
        if self.encoder_type != 'clip_dual':
            raise RuntimeError(f"set_pooled belongs to encoder_type='clip_dual' (this classifier has {self.encoder_type!r})")
        vec = torch.as_tensor(vec)
        P_ = self.pooled_table.shape[1]
        if vec.dim() != 1 or vec.shape[0] != P_:
            raise ValueError(f"the pooled vector of row {row} must be [{P_}], got {tuple(vec.shape)}")
        self.pooled_table[row] = vec.to(self.pooled_table.device, self.pooled_table.dtype)
        self._pooled_rows.add(int(row) % self.pooled_table.shape[0])

    def added_cond(self, labels):
        """What a foreign backbone is called with next to encoder_hidden_states: {} unless encoder_type='clip_dual', then
        added_cond_kwargs = {"text_embeds": the pooled rows of `labels`, "time_ids": config.add_time_ids per row} (diffusers' names)."""
        if self.encoder_type != 'clip_dual':
            return {}
        te = self.pooled_table[labels.to(self.pooled_table.device)]
        return {"added_cond_kwargs": {"text_embeds": te, "time_ids": self.add_time_ids.to(te.device).expand(te.shape[0], 6)}}

    def _refuse_sdxl_generation(self, what):
        if self.encoder_type == 'clip_dual':
            raise NotImplementedError(f"{what}: generation with an SDXL backbone (encoder_type='clip_dual') is not built: scoring only — "
                                      "classify, evaluate / inference in classification mode, and the backbone's forward")

    # ---- small reference-identical helpers (host side, fp32 torch like the reference) -------
    def encode_text_prompt(self, text):
        if self.encoder_type == 'nn':
            embeddings = self.encoder(text)
            embeddings.unsqueeze_(1)
        elif self._table_mode():
            self._require_prompts()
            embeddings = self.encoder(text)              # [B, S, hid], what the reference's text encoder returns (:93-98)
        elif self.encoder_type == 'DiT':
            embeddings = text
        else:
            raise NotImplementedError(self.encoder_type)
        return embeddings

    def _table_mode(self):
        """Is the conditioning a PromptTable row per class ('prompt', and 't5' / 'clip' whose encoder fills the same table)?"""
        return self.encoder_type in ('prompt', 't5', 'clip', 'clip_dual')

    def _ragged_table(self):
        return self._table_mode() and self.encoder.varlen

    def _require_prompts(self):
        if self.encoder_type == 'clip_dual' and not self._prompts_set and len(self._pooled_rows) < self.pooled_table.shape[0]:
            raise RuntimeError("encoder_type='clip_dual': call set_class_prompts(input_ids, attention_mask, input_ids_2=..., "
                               "attention_mask_2=...) before classify, or fill both tables by hand (encoder.set_prompt and set_pooled for "
                               "every row)")
        if self.encoder_type in ('t5', 'clip') and not self._prompts_set:
            raise RuntimeError(f"encoder_type={self.encoder_type!r}: call set_class_prompts(input_ids, attention_mask) before classify / "
                               "sample (the prompt table is still empty)")

    @torch.no_grad()
    def set_class_prompts(self, input_ids, attention_mask=None, *, input_ids_2=None, attention_mask_2=None):
        """encoder_type='t5' / 'clip': token ids [classes + 1, L <= S] of one prompt per class, the last row the null prompt (tokenising
        is the caller's job), and their right-padded attention mask.  Runs the text encoder on the device (its compute dtype is
        config.compute_dtype), writes weight[:, :L], zeroes the rest and records the token counts as the table's lengths (without a
        mask every row is a real state and the lengths are L: what Stable Diffusion feeds its UNet from CLIP).
        encoder_type='clip_dual': input_ids / attention_mask are the first tokenizer's, input_ids_2 / attention_mask_2 (required) the
        second's — the two differ in their pad token and may differ in L, but the token counts must agree row by row (the table has
        one length per row; ValueError naming the first row that differs).  Both encoders are read at layer=-2, their states written
        side by side (encoder 1 first), the second's pooled output into `pooled_table`.  The null row is encoded like any other."""
        if self.encoder_type == 'clip_dual':
            return self._set_class_prompts_dual(input_ids, attention_mask, input_ids_2, attention_mask_2)
        if input_ids_2 is not None or attention_mask_2 is not None:
            raise ValueError(f"input_ids_2 / attention_mask_2 belong to encoder_type='clip_dual' (this classifier has {self.encoder_type!r})")
        if self.encoder_type not in ('t5', 'clip'):
            raise RuntimeError(f"set_class_prompts belongs to encoder_type='t5' / 'clip' (this classifier has {self.encoder_type!r})")
        rows, S = self.encoder.weight.shape[0], self.encoder.weight.shape[1]
        ids = torch.as_tensor(input_ids)
        if ids.dim() != 2 or ids.shape[0] != rows or not 1 <= ids.shape[1] <= S:
            raise ValueError(f"input_ids must be [{rows}, L <= {S}] (one prompt per class and the null prompt), got {tuple(ids.shape)}")
        dev = self.encoder.weight.device
        from ..engine_t5 import lengths_of_mask
        lens = lengths_of_mask(attention_mask, ids.shape)
        dt = self.config.compute_dtype or "bf16"
        if self.text_encoder.compute_dtype != dt:
            self.text_encoder.set_compute_dtype(dt)
        emb = self.text_encoder(ids.to(dev), None if attention_mask is None else torch.as_tensor(attention_mask).to(dev))
        self.encoder.weight.zero_()
        self.encoder.weight[:, :ids.shape[1]] = emb.to(self.encoder.weight.dtype)
        self.encoder.set_lengths(lens)
        self._prompts_set = True

    def _set_class_prompts_dual(self, ids1, mask1, ids2, mask2):
        if ids2 is None:
            raise ValueError("encoder_type='clip_dual' needs input_ids_2 (and attention_mask_2): the token ids of the second tokenizer")
        rows, S = self.encoder.weight.shape[0], self.encoder.weight.shape[1]
        ids1, ids2 = torch.as_tensor(ids1), torch.as_tensor(ids2)
        for name, ids in (("input_ids", ids1), ("input_ids_2", ids2)):
            if ids.dim() != 2 or ids.shape[0] != rows or not 1 <= ids.shape[1] <= S:
                raise ValueError(f"{name} must be [{rows}, L <= {S}] (one prompt per class and the null prompt), got {tuple(ids.shape)}")
        from ..engine_t5 import lengths_of_mask
        len1, len2 = lengths_of_mask(mask1, ids1.shape), lengths_of_mask(mask2, ids2.shape)
        differ = (len1 != len2).nonzero().reshape(-1).tolist()
        if differ:
            b = differ[0]
            raise ValueError(f"the two tokenizers' token counts must agree row by row: row {b} has {int(len1[b])} tokens for the first "
                             f"encoder and {int(len2[b])} for the second")
        dev = self.encoder.weight.device
        dt = self.config.compute_dtype or "bf16"
        for enc in (self.text_encoder, self.text_encoder_2):
            if enc.compute_dtype != dt:
                enc.set_compute_dtype(dt)
        on = lambda t: None if t is None else torch.as_tensor(t).to(dev)
        h1 = self.text_encoder.hidden_state(ids1.to(dev), on(mask1), layer=-2)
        h2, pooled = self.text_encoder_2(ids2.to(dev), on(mask2), layer=-2, pooled=True)
        L1, L2, H1 = ids1.shape[1], ids2.shape[1], h1.shape[2]
        self.encoder.weight.zero_()
        self.encoder.weight[:, :L1, :H1] = h1.to(self.encoder.weight.dtype)
        self.encoder.weight[:, :L2, H1:] = h2.to(self.encoder.weight.dtype)
        self.encoder.set_lengths(len1)
        self.pooled_table.copy_(pooled.to(self.pooled_table.dtype))
        self._prompts_set = True

    def _refuse_ragged_on_foreign(self):
        if self._ragged_table():
            raise NotImplementedError("prompts of different lengths need a HIP backbone (UNetCondition2D): the reference's backbone "
                                      "signature (x, noise_labels, encoder_hidden_states) has no mask argument, so a foreign nn.Module "
                                      "would attend the pad rows")

    def diffuse(self, x, alpha_t, sigma_t):
        eps_t = torch.randn_like(x)
        return alpha_t * x + sigma_t * eps_t, eps_t

    def logsnr_schedule_cosine(self, t, logsnr_min=-15, logsnr_max=15):
        logsnr_max = logsnr_max + math.log(self.noise_d / self.image_d)
        logsnr_min = logsnr_min + math.log(self.noise_d / self.image_d)
        t_min = math.atan(math.exp(-0.5 * logsnr_max))
        t_max = math.atan(math.exp(-0.5 * logsnr_min))
        return -2 * log(torch.tan((t_min + t * (t_max - t_min)).clone().detach()))

    def logsnr_schedule_cosine_shifted(self, t):
        return self.logsnr_schedule_cosine(t) + 2 * math.log(self.noise_d / self.image_d)

    # ---- the discrete DDPM schedules (additive: config.schedule = 'scaled_linear' | 'ddpm_linear') ----
    # name -> (diffusers' beta_schedule, default beta_start, default beta_end, the betas of N steps in fp64)
    DISCRETE = {
        "scaled_linear": ("scaled_linear", 0.00085, 0.012, lambda b0, b1, N: torch.linspace(b0 ** 0.5, b1 ** 0.5, N, dtype=torch.float64) ** 2),
        "ddpm_linear": ("linear", 1e-4, 0.02, lambda b0, b1, N: torch.linspace(b0, b1, N, dtype=torch.float64)),
    }

    def _init_discrete(self, schedule):
        """N = config.train_timesteps (1000) steps of betas — 'scaled_linear' (Stable Diffusion): linspace(sqrt(beta_start),
        sqrt(beta_end), N)^2 (0.00085, 0.012); 'ddpm_linear' (DiT, the DDPM paper's grid): linspace(beta_start, beta_end, N) (1e-4, 0.02) ->
        `self.ddpm_logsnr` [N] fp32, log(abar_k / (1 - abar_k)) with abar = cumprod(1 - betas) in fp64, once, on the host.
        config.scheduler_path: a local diffusers scheduler_config.json that supplies num_train_timesteps / beta_start / beta_end (keys of
        the config win over it where both are given), must name the schedule's own beta_schedule ("scaled_linear", and "linear" for
        'ddpm_linear') and must agree with config.pred_param."""
        cfg = self.config
        beta_schedule, d0, d1, betas_of = self.DISCRETE[schedule]
        sched = {}
        if cfg.scheduler_path is not None:
            import json
            path = cfg.scheduler_path
            if os.path.isdir(path):
                path = os.path.join(path, "scheduler_config.json")
            with open(path) as fh:
                sched = json.load(fh)
            if sched.get("beta_schedule", beta_schedule) != beta_schedule:
                other = [k for k, v in self.DISCRETE.items() if v[0] == sched["beta_schedule"]]
                raise ValueError(f"{path}: beta_schedule = {sched['beta_schedule']!r}, but schedule={schedule!r} is built from beta_schedule = "
                                 f"{beta_schedule!r}" + (f" (that file belongs to schedule={other[0]!r})" if other else
                                                         f" (the discrete schedules built here: {sorted(self.DISCRETE)})"))
            want = {"epsilon": "eps", "v_prediction": "v"}.get(sched.get("prediction_type", "epsilon"))
            if want != self.pred_param:
                raise ValueError(f"{path}: prediction_type = {sched.get('prediction_type')!r} but config.pred_param = {self.pred_param!r}")
        pick = lambda own, key, default: own if own is not None else sched.get(key, default)
        N = int(pick(cfg.train_timesteps, "num_train_timesteps", 1000))
        b0, b1 = float(pick(cfg.beta_start, "beta_start", d0)), float(pick(cfg.beta_end, "beta_end", d1))
        if N < 1 or not 0.0 < b0 <= b1 < 1.0:
            raise ValueError(f"schedule={schedule!r} needs train_timesteps >= 1 and 0 < beta_start <= beta_end < 1, got {N}, {b0}, {b1}")
        betas = betas_of(b0, b1, N)
        abar = torch.cumprod(1.0 - betas, 0)
        self.train_timesteps = N
        off = pick(cfg.steps_offset, "steps_offset", 0)
        if isinstance(off, bool) or not isinstance(off, int):
            raise ValueError(f"steps_offset must be an int, got {off!r}")
        self.steps_offset = off                                                  # added to every 'leading' step of the generation grid
        self.ddpm_logsnr = torch.log(abar / (1.0 - abar)).to(torch.float32)      # plain attribute: host data, never part of a checkpoint
        self.abar = abar                                 # the fp64 table itself, likewise: the learned-range step's two log variances

    def ddpm_step(self, t):
        """t in [0, 1] as the reference draws it -> the DDPM step k = min(floor(t N), N - 1) (int64; the product in fp64)."""
        N = self.train_timesteps
        t = torch.as_tensor(t)
        return torch.clamp(torch.floor(t.detach().to("cpu", torch.float64) * N), 0, N - 1).to(torch.int64)

    def logsnr_schedule_discrete(self, t):
        """log-SNR of the step t falls into, fp32 (on t's device)."""
        return self.ddpm_logsnr[self.ddpm_step(t)].to(torch.as_tensor(t).device)

    logsnr_schedule_scaled_linear = logsnr_schedule_discrete      # the earlier name

    def noise_labels(self, t):
        """What the backbone is fed as its time input at t: the log-SNR `schedule(t)` for the cosine schedules (the reference's
        models), the DDPM step as fp32 for the discrete schedules (a Stable Diffusion UNet and a published DiT embed the integer step)."""
        if self.discrete:
            return self.ddpm_step(t).to(torch.float32).to(torch.as_tensor(t).device)
        return self.schedule(t)

    def _refuse_discrete(self, what, from_t):
        """Generation under a discrete schedule ('scaled_linear', 'ddpm_linear') is opt-in: without config.timestep_spacing there is no map from
        linspace(from_t, 0, sampling_steps + 1) to DDPM steps.  With the key, the grid of this call is built once here so that an
        impossible one (trajectory.discrete_steps) is refused before any draw."""
        if not self.discrete:
            return
        if self.timestep_spacing is None:
            raise NotImplementedError(f"{what} under schedule={self.config.schedule!r} needs config.timestep_spacing = 'trailing' | 'leading': "
                                      "how sampling_steps are laid on the discrete DDPM grid is the caller's choice (unset: classify only)")
        TJ.discrete_steps(self, from_t)

    def _variance_of(self, backbone):
        """config.variance (additive, read once here): None / "fixed" -> None, every ancestral step adds the fixed posterior deviation
        as ever; "learned" -> "learned", the step takes its deviation from the variance channels the backbone predicts next to eps
        (diffusers' variance_type = "learned_range", the improved-DDPM sampler a published DiT is trained for; ancestral.LearnedRange).
        "learned" needs a discrete schedule, a backbone with out_channels == 2 * in_channels and the ancestral sampler: ValueError
        otherwise, as for any other value."""
        v = getattr(self.config, "variance", None)
        if v is None or v == "fixed":
            return None
        if v != "learned":
            raise ValueError(f"config.variance must be None, 'fixed' or 'learned', got {v!r}")
        if not self.discrete:
            raise ValueError(f"config.variance = 'learned' belongs to the discrete DDPM grid (schedule='scaled_linear' / 'ddpm_linear'): "
                             f"its two bounds are log beta and the log posterior variance of integer steps, which "
                             f"schedule={self.config.schedule!r} does not have")
        ic, oc = getattr(backbone.config, "in_channels", None), getattr(backbone.config, "out_channels", None)
        if ic is None or oc is None or oc != 2 * ic:
            raise ValueError(f"config.variance = 'learned' needs a backbone that predicts the variance next to eps: "
                             f"out_channels == 2 * in_channels, got out_channels = {oc} and in_channels = {ic}")
        self._refuse_learned_under_solver()
        return v

    def _refuse_learned_under_solver(self):
        """config.sampler is read per call, so `sample` and `counterfactual` ask again: a deterministic sampler adds no noise, the
        learned variance would do nothing there."""
        sampler = S.sampler_of(self.config)
        if sampler is not None:
            raise ValueError(f"config.variance = 'learned' needs the ancestral sampler (config.sampler unset or 'ddpm'), got "
                             f"config.sampler = {sampler!r}: a deterministic sampler adds no noise, the key would do nothing there")

    @torch.no_grad()
    def encode_latents(self, x):
        """config.vae_path set: images [B, C, H, W] in [-1, 1] -> the latents [B, latent_channels, H / f, W / f] fp32 the backbone is
        trained on, (posterior mean - shift_factor) * scaling_factor, on the VAE's device (nets/vae.py: all of it in libdcamd; x is moved
        there if it is elsewhere).  The mean, not a posterior sample: the same image always gives the same latents."""
        if self.vae is None:
            raise RuntimeError("encode_latents needs config.vae_path: a LOCAL diffusers AutoencoderKL directory")
        return self.vae(x.to(device=self.vae.encoder.conv_in.weight.device, dtype=torch.float32))

    @torch.no_grad()
    def decode_latents(self, z):
        """config.vae_path set: latents [B, latent_channels, h, w] as `encode_latents` returns them (scaled) -> images
        [B, out_channels, f h, f w] fp32, `AutoencoderKL.decode(z / scaling_factor + shift_factor).sample`, unclamped, on the VAE's device
        (nets/vae.py VAEDecoder: all of it in libdcamd).  The decoder is read from config.vae_path at the first call, at config.vae_dtype
        (a directory that holds the encoder only is refused then, by the first key it lacks); at most config.vae_decode_batch (additive,
        default 8) images go through one launch plan, plans are kept per chunk size.  fp16 is known to overflow in published VAE
        decoders (upstream's `force_upcast`): prefer bf16, the default, or f32."""
        if self.vae is None:
            raise RuntimeError("decode_latents needs config.vae_path: a LOCAL diffusers AutoencoderKL directory")
        dev = self.vae.encoder.conv_in.weight.device
        dec = self._vae_decoder
        if dec is None:
            from ..nets.vae import VAEDecoder
            dec = VAEDecoder.from_directory(self.config.vae_path)
            object.__setattr__(self, "_vae_decoder", dec)
        if dec.compute_dtype != self.vae.compute_dtype:        # follows the encoder's at every call (plans are kept per dtype)
            dec.set_compute_dtype(self.vae.compute_dtype)
        if dec.decoder.conv_in.weight.device != dev:
            dec.to(dev)
        step = self.config.vae_decode_batch
        step = 8 if step is None else int(step)
        if step < 1:
            raise ValueError(f"config.vae_decode_batch must be an int >= 1, got {self.config.vae_decode_batch!r}")
        z = z.to(device=dev, dtype=torch.float32)
        dec.check_latent_shape(z.shape)
        out = [dec(z[i:i + step].contiguous()) for i in range(0, z.shape[0], step)]
        return out[0] if len(out) == 1 else torch.cat(out, 0)

    # ---- the hot path ---------------------------------------------------------------------
    @torch.no_grad()
    def classify(self, x, text=None, fast=False, *, t=None, eps=None, fast_select=None, return_errors=False,
                 rng="reference", seed=0, group=None, return_posterior=False, return_trials=False, return_evidence=False, latents=False,
                 pixel_weight=None):
        """latents (additive; config.vae_path only): True says x already holds latents (`encode_latents`); otherwise x is an image
        batch and is encoded first — t / eps, the evidence maps and everything else then live on the latent grid.
        pixel_weight (additive): a float tensor [BS, H, W] or [BS, 1, H, W] on the model's grid (x's own after the VAE encoder: the latent
        grid under config.vae_path, the wavelet grid of a DWT model, DiT's un-patchified [H, W]) that weights every pixel's term in the
        errors and the evidence maps (loss.py); a 0/1 mask scores a region.  Its values are data (NaN propagates and is counted by the
        posterior's `invalid`); under grid sharding every rank passes the identical tensor.
        config.variance is not read: scoring compares eps alone."""
        if self.vae is not None and not latents:
            x = self.encode_latents(x)
        cfg = self.config
        if pixel_weight is not None:
            pixel_weight = LS.pixel_weight_of(pixel_weight, x.shape[0], x.shape[2], x.shape[3])
        z_stop = P.stop_margin_of(cfg)           # None: no per-image early stopping, none of its code runs
        if z_stop is not None and cfg.simulate_rank:
            raise ValueError("stop_margin_z cannot be combined with simulate_rank: one rank's share of the errors decides nothing")
        if self.trial_weighting is not None and cfg.simulate_rank:
            raise ValueError("trial_weighting cannot be combined with simulate_rank: the measurement key times the unweighted kernels")
        tau = P.temperature_of(cfg) if return_posterior else None
        if return_evidence and cfg.simulate_rank:
            raise ValueError("return_evidence cannot be combined with simulate_rank: one rank's share of the grid explains nothing")
        assert self.encoder_type is not None, "Encoder must be provided for classification."
        self._require_prompts()
        assert len(cfg.evaluation_per_stage) == cfg.n_stages, "Number of evaluations per stage must match the number of stages."
        assert len(cfg.n_keep_per_stage) == cfg.n_stages, "Number of classes to keep per stage must match the number of stages."
        assert cfg.n_keep_per_stage[-1] == 1, "Only one class should be selected at the end of the classification process."
        assert cfg.n_fast_classes <= cfg.classes and cfg.n_fast_classes >= 2, "Number of fast classes must be less than or equal to the total number of classes. Must be at least 2."
        assert rng in ("reference", "philox")
        backbone = self.ema.ema_model
        ends = [0] + list(cfg.evaluation_per_stage)
        T = ends[-1]
        BS = x.shape[0]
        if return_evidence:
            EV.check_trials(T)
        # grid sharding is opt-in: the reference shards the DATALOADER over ranks, so an initialised process group alone
        # must not make ranks mix the errors of different images
        shard = group is not None or cfg.shard_grid is True
        rank, ws = D.world(group) if shard else (0, 1)
        # bench.py --simulate-rank r/N (measurement only): score exactly rank r's share of an N-rank grid-sharded call on this one
        # GPU, without a process group — no replication check, no gather, so the labels of such a call mean nothing
        sim = cfg.simulate_rank
        if sim:
            rank, ws = int(sim[0]), int(sim[1])
        elif ws > 1:
            D.assert_replicated(x, group, also=pixel_weight)

        classes = self._candidate_classes(text, fast, fast_select, BS)
        draws = self._trial_draws(x, T, t, eps, rng, seed)
        weights = {} if pixel_weight is None else {"pixel_w": pixel_weight}      # (the trial weights travel in the draws)
        if hasattr(backbone, "make_plan"):
            runner = _HipRunner(self, backbone, x, T, draws, **weights)           # libdcamd; raises without GPU / library
        else:
            runner = _ForeignRunner(self, backbone, x, T, draws, **weights)       # user-supplied nn.Module, eager torch
        # per-image early stopping (config.stop_margin_z): t_done[b] = 0 while image b is undecided, else the trials it was decided on;
        # `rows` = the undecided images (ascending ids; None: all of them, the plain path), the same list on every rank
        t_done = frozen = rows = None
        if z_stop is not None:
            t_done, frozen = runner.stop_state()
        if return_evidence:
            runner.evidence_begin(cfg.n_stages)      # per-stage int64 accumulators; the plans of this call carry the map op
        for i in range(cfg.n_stages):
            last = i == cfg.n_stages - 1
            if return_evidence:
                runner.ev_stage = i
            pairs = D.local_pairs(ends[i], ends[i + 1], BS, rank, ws) if rows is None else D.local_pairs_rows(ends[i], ends[i + 1], rows, rank, ws)
            runner.run_stage(pairs, classes, stage=(ends[i], rank, ws), rows=rows)
            errors = runner.errors()
            if not sim:
                D.gather_stage_errors(errors, ends[i], ends[i + 1], rank, ws, group=group,
                                      **({} if rows is None else {"rows": runner.rows_on_device(rows)}))
            # stage end (:718-721), identically on every rank: mean over the trials so far, the k smallest classes per image (HIP
            # backbones: on the device, scoring.py).  (A stopped image's cells past t_done stay +inf: its class list is meaningless
            # from then on and never used.)
            classes = runner.stage_end(errors, ends[i + 1], cfg.n_keep_per_stage[i], last=last)
            if z_stop is not None and not last:
                active = runner.stage_stop(errors, ends[i + 1], z_stop, t_done, frozen)
                rows = None if len(active) == BS else active
                if not active:
                    break                        # every image is decided: the remaining stages have nothing to score
        if z_stop is None or last:
            assert classes.shape[1] == 1, "Only one class should be selected at the end of the classification process."
        if z_stop is None:
            out = classes[:, 0].to(device=x.device, dtype=torch.int64)
        elif last:                               # the images that ran to T take the last stage's label, the others keep theirs
            out = torch.where(t_done == 0, classes[:, 0].to(device=frozen.device, dtype=torch.int64), frozen).to(x.device)
            t_done = torch.where(t_done == 0, torch.full_like(t_done, T), t_done)
        else:
            out = frozen.to(x.device)
        # the posterior reads the errors every rank holds after the last gather: the same bits everywhere
        post = evid = None
        t_end, t_values = (T, None) if z_stop is None else (t_done, ends[1:i + 2])
        if return_evidence:
            # the maps are paired to the posterior's winner over the posterior's trial counts: its parts are computed either way
            post, winner, means, _ = runner.posterior(errors, t_end, 1.0 if tau is None else tau, t_values=t_values, return_parts=True)
            acc, bad = runner.ev
            if ws > 1:
                D.reduce_evidence(acc, bad, ws, group=group)     # exact integer sums: the same bits on every rank and for every world size
            evid = runner.evidence(ends[1:], post.n_trials, EV.winner_or_none(winner, means))
        elif return_posterior:
            post = runner.posterior(errors, t_end, tau, t_values=t_values)
        res = (out,)
        if return_errors:
            res += (errors.cpu(),)               # (synchronises: the cheap moment to look at the device-side failure counter)
            self.check_device_errors()
        if return_posterior:
            res += (post,)
        if return_evidence:
            res += (evid,)
        if return_trials:
            res += (t_done if t_done is not None else torch.full((BS,), T, dtype=torch.int32, device=errors.device),)
        return res if len(res) > 1 else out

    def _candidate_classes(self, text, fast, fast_select, BS):
        """Candidate classes per image (host, exactly the reference's ops :671-679)."""
        cfg, ncls = self.config, self.config.classes
        if fast:
            text_c = text.detach().cpu().view(-1, 1)
            classes = torch.arange(ncls).repeat(BS, 1)
            wrong = classes[(classes == text_c) == False].view(BS, -1)  # noqa: E712
            sel = fast_select.cpu() if fast_select is not None else torch.randint(0, wrong.shape[1], (BS, cfg.n_fast_classes - 1))
            return torch.cat((text_c, torch.gather(wrong, 1, sel)), dim=1)
        return torch.arange(ncls).repeat(BS, 1)

    def _trial_draws(self, x, T, t, eps, rng, seed):
        """Per-trial draws.  reference order: t = rand(BS) then eps = randn_like(x), trial by trial (:688-692, :113)."""
        BS = x.shape[0]
        eps_of = {}
        if t is not None:
            t_all = torch.as_tensor(t, dtype=torch.float32).cpu().reshape(T, BS)
        elif rng == "reference":
            t_rows = []
            for j in range(T):
                t_rows.append(torch.rand(BS))
                if eps is None:
                    eps_of[j] = torch.randn_like(x)
            t_all = torch.stack(t_rows)
        else:
            t_all = torch.rand(T, BS)
        if eps is not None:
            eps_of = {j: eps[j] for j in range(T)}
        elif rng == "reference" and not eps_of:
            eps_of = {j: torch.randn_like(x) for j in range(T)}
        # fp32 on the host, one [BS] vector per trial exactly like the reference (:689-691): torch's CPU
        # kernels take different (vector / scalar-tail) code paths by element position, so evaluating the
        # whole [T,BS] grid at once would differ from the reference in the last bit.
        if rng == "philox" and t is None:
            # throughput mode draws its own t anyway: one vectorised evaluation (last-bit differences from the
            # per-trial form are irrelevant here and ~2 ms of host time per call are not)
            logsnr = self.schedule(t_all)
            alpha_all, sigma_all = torch.sqrt(torch.sigmoid(logsnr)), torch.sqrt(torch.sigmoid(-logsnr))
        else:
            logsnr = torch.stack([self.schedule(t_all[j].clone()) for j in range(T)])
            alpha_all = torch.stack([torch.sqrt(torch.sigmoid(logsnr[j].clone())) for j in range(T)])
            sigma_all = torch.stack([torch.sqrt(torch.sigmoid(-logsnr[j].clone())) for j in range(T)])
        # `label`: the backbone's time input per (trial, image) — the log-SNR tensor itself unless the schedule is discrete
        label = torch.stack([self.noise_labels(t_all[j].clone()) for j in range(T)]) if self.discrete else logsnr
        draws = dict(logsnr=logsnr, alpha=alpha_all, sigma=sigma_all, label=label,
                     eps_of=eps_of, philox=(rng == "philox" and eps is None), seed=int(seed))
        if self.trial_weighting is not None:     # config.trial_weighting: `weight` [T, BS] fp32 on the host (loss.py); absent otherwise
            steps = self.ddpm_step(t_all) if self.discrete else None
            draws["weight"] = LS.trial_weights(self.trial_weighting, self.pred_param, logsnr, steps)
        return draws

    @torch.no_grad()
    def loss(self, x, text=None, *, t=None, eps=None, ema=False):
        """The reference's `loss` (:295-344) as a forward-only evaluation — the validation loss people log; TRAINING IS NOT PART OF THIS
        PROJECT, no autograd graph is built and nothing can be back-propagated through the result.  mean over the batch and C * H * W of
        w(logsnr) (eps_hat - eps)^2 with the truncated-SNR weight of :331-337 (loss.py `train_weight`: config.trial_weighting = "train"'s
        weight with its min_snr_gamma, whatever trial_weighting is set to), at one draw per image in the reference's order (t = rand(BS),
        then eps = randn_like(x)); `t` [BS] and `eps` (x's shape) inject the draws.  Returns a 0-dim fp32 tensor on the scoring device.
        HIP backbones: one trial and one class column (`text`, class ids [BS]; None raises ValueError) through the scoring plans — the
        weighted dc_eps_mse, so the per-image sums go through its sqrt-then-square; ema=False scores `self.model` as the reference does,
        True the EMA model `classify` scores.  A foreign backbone: the reference's statements in eager torch."""
        if self.vae is not None:
            x = self.encode_latents(x)
        BS = x.shape[0]
        tw = self.trial_weighting
        gamma = tw[1] if tw is not None and tw[0] == "train" else LS.MIN_SNR_GAMMA
        backbone = self.ema.ema_model if ema else self.model
        t = torch.rand(BS) if t is None else torch.as_tensor(t, dtype=torch.float32).cpu().reshape(BS)
        if not hasattr(backbone, "make_plan"):
            text_embeddings = None
            if text is not None and self.encoder_type is not None:
                text_embeddings = self.encode_text_prompt(text).to(x.device)
            logsnr_t = self.schedule(t).to(x.device)
            alpha_t = torch.sqrt(torch.sigmoid(logsnr_t)).view(-1, 1, 1, 1).to(x.device)
            sigma_t = torch.sqrt(torch.sigmoid(-logsnr_t)).view(-1, 1, 1, 1).to(x.device)
            eps_t = torch.randn_like(x) if eps is None else eps.to(x.device).reshape(x.shape)
            z_t = alpha_t * x + sigma_t * eps_t
            pred = backbone(x=z_t, noise_labels=self.noise_labels(t).to(x.device), encoder_hidden_states=text_embeddings,
                            **({} if text is None else self.added_cond(text)))
            eps_pred = sigma_t * z_t + alpha_t * pred if self.pred_param == 'v' else pred
            minsnr_weight = LS.train_weight(logsnr_t, self.pred_param, gamma).view(-1, 1, 1, 1)
            return torch.mean(minsnr_weight * (eps_pred - eps_t) ** 2).to(torch.float32)
        if text is None:
            raise ValueError("loss on a HIP backbone scores one class column: pass text, the class id of every image ([BS])")
        self._require_prompts()
        labels = torch.as_tensor(text).detach().cpu().reshape(-1).to(torch.int64)
        if labels.numel() != BS or int(labels.min()) < 0 or int(labels.max()) >= self.config.classes:
            raise ValueError(f"loss: text must hold one class id in [0, {self.config.classes}) per image, got {labels.tolist()}")
        eps_t = torch.randn_like(x) if eps is None else eps.reshape(x.shape)
        logsnr = self.schedule(t.clone()).reshape(1, BS)
        draws = dict(logsnr=logsnr, alpha=torch.sqrt(torch.sigmoid(logsnr.clone())), sigma=torch.sqrt(torch.sigmoid(-logsnr.clone())),
                     label=self.noise_labels(t.clone()).reshape(1, BS), eps_of={0: eps_t}, philox=False, seed=0,
                     weight=LS.trial_weights(("train", gamma), self.pred_param, logsnr))
        runner = _HipRunner(self, backbone, x, 1, draws)
        runner.score_loss = (L.LOSS_L2, 1.0)             # the training loss is the squared error, whatever config.score_loss scores with
        runner.run_stage(D.local_pairs(0, 1, BS, 0, 1), labels.view(BS, 1), stage=(0, 0, 1))
        err = runner.errors()[torch.arange(BS, device=runner.dev), labels.to(runner.dev), 0]      # w_b * sum over C H W, per image
        return err.sum() / float(BS * x.shape[1] * x.shape[2] * x.shape[3])

    def check_device_errors(self):
        """Raise if a producer-side-GroupNorm launch (csrc/epi_pn.h) gave up waiting for the other workgroups of a sample since the last
        check: its outputs were NaN-poisoned, so the scores of that call are invalid.  Synchronises with the device; called where the
        host synchronises anyway — `classify(return_errors=True)`, the end of `evaluate`, bench.py, the smoke test."""
        if torch.cuda.is_available() and hasattr(self.ema.ema_model, "make_plan"):
            n = int(L.lib().dc_pn_timeouts())
            if n:
                raise L.DcamdError(f"{n} wave(s) timed out inside a producer-side GroupNorm launch: the results of this call are invalid")

    # ---- callers of the hot path (reference :532-578) ----------------------------------------
    @torch.no_grad()
    def evaluate(self, val_dataloader, stop_idx=None, metrics=None, classification=False, from_t=1):
        val_samples, batches = [], []
        for idx, batch in enumerate(val_dataloader):
            batch = {k: v for k, v in batch.items()}
            x = batch["images"]
            p = batch["prompt"] if "prompt" in batch.keys() else None
            # a metric with `wants_posterior = True` (utils/metrics.py AUROC, SelectiveAccuracy) is fed (labels, batch, ClassPosterior)
            want_post = classification and metrics is not None and any(getattr(m, "wants_posterior", False) for m in metrics)
            post = None
            # config.pixel_weight_key (additive): batch[key] is the call's pixel_weight, on the model's grid as it is (dwt_on_device
            # transforms "images" only)
            key = self.config.pixel_weight_key if classification else None      # (sampling mode never looks for the mask)
            pw = {} if key is None else {"pixel_weight": batch[key]}
            if want_post:
                sample, post = self.classify(x, p, fast=self.config.fast_classification, return_posterior=True, **pw)
            else:
                sample = self.classify(x, p, fast=self.config.fast_classification, **pw) if classification else self.sample(x, p, from_t)
            if metrics is not None:
                for metric in metrics:
                    if post is not None and getattr(metric, "wants_posterior", False):
                        metric.update((sample, batch, post))
                    else:
                        metric.update((sample, batch))
            val_samples.append(sample)
            batches.append(batch)
            if stop_idx is not None and idx == stop_idx:
                break
        self.check_device_errors()
        return val_samples, batches, metrics

    def prefetch_to_device(self, loader, dev):
        """The batches of `loader` on `dev`, one batch AHEAD of the consumer: while batch i is being scored on the
        current stream, batch i+1 is copied host -> HBM on a side stream (pinned staging, non_blocking) and — with the additive config
        key `dwt_on_device=True`, for loaders that yield the RAW [-1, 1] images — transformed there by the HIP Haar kernel,
        `images := wavelet_dec_2(images) / 2`, what reference dataset/chexpert.py:146-147 does per item on the host before
        `evaluate` (:555-563) sees the batch.  The consumer's stream waits on the batch's event, so results are those of the
        unpipelined loop.  `self._prefetch_log` keeps (copy start, copy end, handed over) events per batch for the tests."""
        from ..utils.wavelet import wavelet_dec_2
        side = torch.cuda.Stream(device=dev)
        dwt = self.config.dwt_on_device is True
        self._prefetch_log = []

        def stage(batch):
            out = {}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                e0.record(side)
                for k, v in batch.items():
                    if not torch.is_tensor(v):
                        out[k] = v
                        continue
                    d = v if v.is_cuda else (v if v.is_pinned() else v.pin_memory()).to(dev, non_blocking=True)
                    if dwt and k == "images":
                        d = wavelet_dec_2(d, scale=0.5)          # enqueued on the side stream (L.stream_ptr() = the current stream)
                    out[k] = d
                e1.record(side)
            return out, e0, e1

        it = iter(loader)
        first = next(it, None)
        nxt = stage(first) if first is not None else None
        while nxt is not None:
            cur, e0, e1 = nxt
            following = next(it, None)
            nxt = stage(following) if following is not None else None     # batch i+1 starts moving before batch i is handed over
            main = torch.cuda.current_stream(dev)
            main.wait_event(e1)
            for v in cur.values():
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(main)
            eh = torch.cuda.Event(enable_timing=True)
            eh.record(main)
            self._prefetch_log.append((e0, e1, eh))
            yield cur

    # ---- generation (reference :163-293) ---------------------------------------------------
    # HIP backbones: ONE batch-2 plan launch per step (class token || null token, the class-independent layers once per
    # image) and ONE fused sampler-step kernel (`dc_ddpm_step`); a foreign nn.Module takes the reference's two eager calls
    # and its elementwise torch expressions (`ddpm_sampler_step`, kept for that path and as the fused kernel's statement).
    # The loops are ancestral.py's; `clip` and `ddpm_sampler_step` stay here as the reference's surface.
    def clip(self, x):
        return torch.clamp(x, -1, 1)

    @torch.no_grad()
    def ddpm_sampler_step(self, z_t, pred, u_pred, logsnr_t, logsnr_s, w=None):
        """(mu, var) of one ancestral step; w: the guidance weight, config.cfg_w when None (`invert_ddpm` passes its own)."""
        c = -torch.special.expm1(logsnr_t - logsnr_s)
        alpha_t, alpha_s = torch.sqrt(torch.sigmoid(logsnr_t)), torch.sqrt(torch.sigmoid(logsnr_s))
        sigma_t, sigma_s = torch.sqrt(torch.sigmoid(-logsnr_t)), torch.sqrt(torch.sigmoid(-logsnr_s))
        w = self.cfg_w if w is None else w
        pred = (1 + w) * pred - w * u_pred                                   # classifier-free guidance mix
        x_pred = alpha_t * z_t - sigma_t * pred if self.pred_param == 'v' else (z_t - sigma_t * pred) / alpha_t
        x_pred = self.clip(x_pred)
        mu = alpha_s * (z_t * (1 - c) / alpha_t + c * x_pred)
        return mu, (sigma_s ** 2) * c

    _sampler_step_scalars = staticmethod(AN.Clipped.scalars)                  # the earlier name of the clipped step's host scalars

    @torch.no_grad()
    def sample(self, x, text=None, from_t=1, decode=False):
        """Ancestral DDPM sampling with classifier-free guidance (reference :210-293), same RNG consumption order as the reference.
        config.sampler = "ddim" | "dpmpp_2m" (additive; unset or "ddpm": the ancestral loop, untouched): the start is drawn as ever, then
        sampling_steps deterministic passes on linspace(from_t, 0, sampling_steps + 1) (solver.py) — only the initial draw is taken
        from torch's generator.
        With config.vae_path, x and the result are LATENTS (`encode_latents`), unless decode=True (additive; ValueError without
        config.vae_path): the result is then `decode_latents` of those latents, images [BS, out_channels, f H, f W].
        schedule='scaled_linear' (needs config.timestep_spacing): the grid is the integer steps of `trajectory.discrete_steps`, x is
        diffused to its first point k_0, the backbone is fed float(k_i), and nothing is clipped — the ancestral mean is a z + b x
        (ancestral.py), the last deterministic pass returns the data prediction as it is.
        config.variance = "learned" (additive; a discrete schedule, out_channels == 2 * in_channels, the ancestral sampler): every pass but
        the last adds noise * exp(0.5 (fr log beta + (1 - fr) log beta~)) per element, fr = (v + 1) / 2 from the variance channels of the
        CONDITIONAL prediction — diffusers' "learned_range" — in place of the fixed posterior deviation; the mean is unchanged.  HIP DiT:
        one pair plan that keeps the variance features and one `dc_ddpm_step_shared` in DC_STEP_LEARNED_RANGE per pass; a foreign
        nn.Module: the same expressions in torch on its 2C-channel outputs.  Under a deterministic config.sampler ValueError."""
        self._refuse_sdxl_generation("sample")
        self._refuse_discrete("sample", from_t)
        if self.variance is not None:
            self._refuse_learned_under_solver()
        TJ.check_decode(self, decode)
        sampler = S.sampler_of(self.config)
        z = AN.sample(self, x, text, from_t) if sampler is None else S.sample(self, x, text, from_t, sampler)
        return self.decode_latents(z) if decode else z

    @torch.no_grad()
    def counterfactual(self, x, classes=None, from_t=0.5, *, against="input", rng="reference", seed=0, pixel_space=False,
                       start="noise", invert_class=None, decode=False):
        """Every class from shared noise in one call (reference experiments/ipmsa/explain.py: noise to `from_t`, denoise once per label
        with the seed reset in front of each run, look at where the results differ) -> `Counterfactuals(samples, classes, maps)`.
          classes      None: all config.classes; an int tensor [K] (the same for every image) or [BS, K]; K >= 1, duplicates allowed
          samples      [BS, K, C, H, W] f32 on x.device; samples[b, k] is the image `sample(x, classes[:, k], from_t)` returns for image
                       b: the K trajectories of an image start from one z_{from_t} (from_t in (0, 1]; 1: pure noise) and add the same
                       noise at every step
          rng          "reference": torch's generators in the order of ONE `sample` call (the initial draw, then one randn_like
                       [BS, C, H, W] per step), each draw shared by the K classes — K calls of `sample` with `torch.manual_seed(s)`
                       in front of each are the written statement of this function;
                       "philox": all noise from Philox on the device keyed by (seed, row), row = b for the initial draw and
                       (step + 1) * BS + b after it; no torch generator is touched, the result is the same bits from call to call.
                       HIP backbones only
          maps         [BS, K, H', W'] f32: sum over channels (ascending, fp32) of |samples[b, k] - base[b]|; against="input": base is
                       x[b]; against = an int tensor [BS] of class ids (the label `classify` returned, say): base is that class's
                       trajectory of the same image, which must be among classes[b]
          pixel_space  models trained on `wavelet_dec_2(image) / 2`: samples and base go through `wavelet_enc_2(. * 2)` on the device
                       before the maps are taken, and the returned samples are [BS, K, C / 4, 2H, 2W]
        HIP backbones: the BS x K trajectories are the images of pair sessions (nets/unet.py PairSession: prompts projected once per
        call), cut into chunks of whole images by classify's launch-size rule (config.units_per_launch), step-major and chunk-minor, one
        `dc_ddpm_step_shared` per step and chunk, the maps by `dc_abs_diff_map`; nothing is copied to the host inside the loop.  A
        foreign nn.Module takes the reference's eager form at batch BS and is bit-identical to the K reseeded `sample` calls.
        config.sampler = "ddim" | "dpmpp_2m" (additive; unset or "ddpm": all of the above, untouched): the K trajectories are
        deterministic after their start — sampling_steps passes, one `dc_solver_step` per step and chunk, no draw per step.
          start        "noise": the start is drawn as above (torch, or Philox row b);
                       "invert": the start is `invert(x, invert_class, from_t)`, the image's own z_{from_t} — no noise at all, the call
                       touches no generator and returns the same bits every time; needs a deterministic config.sampler (ValueError
                       otherwise: noise added to an inverted latent defeats it);
                       "ddpm_invert": see below
          invert_class an int tensor [BS] of class ids to invert under (the label `classify` returned, say); None: the null token
        start="ddpm_invert" (the ancestral sampler only: config.sampler unset or "ddpm"; ValueError under a deterministic one): the
        start and the noise of every step come from `invert_ddpm(x, invert_class, from_t, rng=rng, seed=seed)` — the K trajectories of
        image b start from its x_0 and step i adds its noise map i through `dc_ddpm_step_shared`, then `sample`'s last pass, the clipped
        mean, as ever.  Under invert_class itself every step lands on the inversion's next latent again (fp32 rounding is the only
        error, at any sampling_steps and cfg_w), so that class's sample is the last pass applied to the image's own x_n and its map
        holds no solver error; another class's map is the label's effect.  rng / seed govern the inversion's n + 1 draws; the decode
        draws nothing.  Costs one more backbone pass per step and the maps' memory (config.ddpm_invert_max_bytes)
        With config.vae_path, x, the samples and the maps are LATENTS (`encode_latents`), unless
          decode       True (config.vae_path only; ValueError without it or together with pixel_space): samples are the decoded images
                       [BS, K, out_channels, f H, f W] (`decode_latents`) and maps [BS, K, f H, f W] are taken on them by
                       `dc_abs_diff_map`; against="input": the base is `decode_latents(x)`, the VAE's own reconstruction, so the map
                       holds no reconstruction error; class ids: the base is that class's decoded trajectory.  False: nothing changes
        schedule='scaled_linear' (needs config.timestep_spacing): all of the above on the integer grid of `sample`, unclipped — the
        ancestral passes are one unclamped `dc_solver_step` (the posterior mean) and one torch add of the shared noise per pass and
        chunk (ancestral.py)
        config.variance = "learned" (see `sample`): the ancestral passes add the learned deviation — the K trajectories of an image share
        their noise draw, each scales it by its own per-element deviation (its own class's variance channels); one `dc_ddpm_step_shared`
        in DC_STEP_LEARNED_RANGE per pass and chunk, starts "noise" and "ddpm_invert", `against` and decode=True as ever; start="invert"
        needs a deterministic sampler, which the key refuses (ValueError)"""
        self._refuse_sdxl_generation("counterfactual")
        self._refuse_discrete("counterfactual", from_t)
        if self.variance is not None:
            self._refuse_learned_under_solver()
        return CF.run(self, x, classes, from_t, against, rng, seed, pixel_space, start=start, invert_class=invert_class, decode=decode)

    @torch.no_grad()
    def invert(self, x, text=None, to_t=0.5, *, guidance=0.0):
        """DDIM inversion: the latent z_{to_t} [BS, C, H, W] f32 that the deterministic sampler decodes back to x (up to the solver's
        error, which shrinks as 1 / sampling_steps and is not small at few steps).  The grid is linspace(0, to_t, sampling_steps + 1),
        the start z = alpha(lam(0)) x, then sampling_steps first-order passes upwards with the data prediction clipped.
          text      an int tensor [BS] of class ids to condition on; None: the null token
          guidance  the w of the inversion only (config.cfg_w is not read).  0, the default, is the conditional prediction alone: guided
                    inversion is known to be unstable
        Works whatever config.sampler says (always DDIM).  HIP backbones run a pair session per chunk of images and one `dc_solver_step`
        per step and chunk; a foreign nn.Module takes the eager form (solver.py).
        With config.vae_path, x and the result are LATENTS (`encode_latents` / `decode_latents`).
        schedule='scaled_linear' (needs config.timestep_spacing): the grid is `sample`'s integer steps from to_t in reverse, so inversion
        and decode visit the same points; the data prediction is not clipped.
        config.variance is not read: DDIM inversion adds no noise (a HIP DiT runs its eps-only pair plans here as ever)."""
        self._refuse_sdxl_generation("invert")
        self._refuse_discrete("invert", to_t)
        return S.invert(self, x, text, to_t, guidance)

    @torch.no_grad()
    def invert_ddpm(self, x, text=None, from_t=0.5, *, guidance=None, rng="reference", seed=0):
        """Edit-friendly DDPM inversion (Huberman-Spiegelglas et al., CVPR 2024) -> `DdpmInversion(start, noise, from_t, guidance)`: the
        noise maps under which the ANCESTRAL sampler decodes x back.  On `sample`'s grid linspace(from_t, 0, sampling_steps + 1), points
        i = 0 .. n: the latents x_i = alpha_i x + sigma_i e_i are drawn independently, and noise[i] = (x_{i+1} - mu_i) / sd_i with mu_i,
        sd_i the posterior mean and deviation of `ddpm_sampler_step` at (x_i, lam_i -> lam_{i+1}).  The sampler started at `start` = x_0
        and fed noise[i] in place of its draws lands on x_{i+1} after every step — exactly up to fp32 rounding, at any sampling_steps
        and any guidance, the clip of the data prediction included — and ends with its usual last pass from x_n.
          start     [BS, C, H, W] f32;  noise [sampling_steps, BS, C, H, W] f32 on x.device: 4 * sampling_steps * x.numel() bytes, refused
                    with a ValueError above config.ddpm_invert_max_bytes (additive key; unset: 2 GiB)
          text      an int tensor [BS] of class ids to condition on; None: the null token
          guidance  the w the maps are solved under; None: config.cfg_w, so that the sampler under the same class reproduces the
                    latents.  Any float works: the maps absorb whatever the prediction is (unlike `invert`, nothing is unstable here)
          rng       "reference": n + 1 `torch.randn_like(x)` draws in the order i = 0 .. n; "philox": `dc_philox_normal` row i * BS + b
                    keyed by `seed` (counterfactual's convention), no torch generator touched, the same bits from call to call; HIP
                    backbones only, C * H * W a multiple of 4
        Every refusal comes before the first draw.  HIP backbones run a pair session per chunk of images (classify's launch-size rule)
        and one `dc_ddpm_noise_map` per pass and chunk, nothing is copied to the host inside the loop; a foreign nn.Module takes the
        eager form (ddpm_invert.py).  Needs the ancestral sampler only when decoded: `counterfactual(..., start="ddpm_invert")`.
        With config.vae_path, x, start and noise are LATENTS (`encode_latents` / `decode_latents`).
        schedule='scaled_linear' (needs config.timestep_spacing): the same on `sample`'s integer grid with the unclipped mean
        mu_i = a z + b x — one unclamped `dc_solver_step` per pass and chunk, the map (x_{i+1} - mu_i) / sd_i in torch on that mean.
        config.variance = "learned" (see `sample`): sd_i is per element, the learned deviation at (x_i, text) — noise[i] =
        (x_{i+1} - mu_i) / sde_i, one `dc_ddpm_noise_map` in DC_STEP_LEARNED_RANGE per pass and chunk, by the device code the step
        multiplies with, so the decode under the same class lands on x_{i+1} again."""
        self._refuse_sdxl_generation("invert_ddpm")
        self._refuse_discrete("invert_ddpm", from_t)
        return DI.invert(self, x, text, from_t, guidance, rng, seed)

    # ---- inference driver and checkpoint ingest (reference :581-655, :769-805) ----
    @torch.no_grad()
    def inference(self, optimizer=None, train_dataloader=None, val_dataloader=None, lr_scheduler=None, metrics=None,
                  plot_function=None, classification=False, from_t=1, checkpoint_folder="checkpoints"):
        """Same arguments and return value as the reference.  No accelerate object: the process's current HIP
        device is used, batches are moved to it, metrics are summed over `torch.distributed` when initialised —
        unless `config.shard_grid` is True (every rank then scored the same images: the counters are already global).
        A caller that grid-shards through `classify(..., group=pg)` instead of the config key drives `classify` itself
        and owns its metric reduction; this driver only knows the config key."""
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        if self.config.experiment_path is not None:
            os.makedirs(os.path.join(self.config.experiment_path, "inference_images/"), exist_ok=True)
            ckpt = os.path.join(self.config.experiment_path, checkpoint_folder)
            if os.path.isdir(ckpt):
                self.load_checkpoint(ckpt)
        self.to(dev)
        if metrics is not None:
            for metric in metrics:
                metric.set_device(dev)
        self.model.eval()

        on_device = (lambda loader: self.prefetch_to_device(loader, dev)) if dev.type == "cuda" else \
            (lambda loader: ({k: v for k, v in b.items()} for b in loader))
        val_samples, batches, metrics = self.evaluate(on_device(val_dataloader), metrics=metrics,
                                                      stop_idx=self.config.evaluation_batches,
                                                      classification=classification, from_t=from_t)
        metric_output = []
        if metrics is not None:
            for metric in metrics:
                # grid sharding scores ONE replicated batch stream on all ranks: the counters are already global, summing
                # them over ranks would multiply them by the world size.  Without it the ranks saw different images
                # (the reference's dataloader sharding) and the counters are summed (utils/metrics.py:56-58).
                if self.config.shard_grid is not True:
                    metric.sync_across_processes(None)
                metric_output.append(metric.get_output())
        if plot_function is not None and not classification:
            plot_function(output_dir=os.path.join(self.config.experiment_path, "inference_images/"), batches=batches,
                          samples=val_samples, epoch=0, process_idx=D.world()[0])
        return (metric_output, val_samples, batches) if metrics is not None else (val_samples, batches)

    # accelerate.save_state layout written by the reference's training run (:382-386, :741): the prepared modules in
    # registration order -> model.safetensors (backbone), model_1.safetensors (EMA wrapper: `ema_model.*`,
    # `online_model.*`, `initted`, `step`), model_2.safetensors (nn.Embedding encoder: `weight`); plus
    # experiment_state.pth {epoch, best_metric, experiment_key} (:744-752).
    _CKPT_FILES = ("model", "model_1", "model_2")

    @staticmethod
    def _read_state(directory, stem):
        """`<stem>.safetensors`, or accelerate's safe_serialization=False spelling `pytorch_<stem>.bin`, under `directory`."""
        st = os.path.join(directory, stem + ".safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            return load_file(st)
        alt = os.path.join(directory, "pytorch_" + stem + ".bin")
        if os.path.exists(alt):
            return torch.load(alt, map_location="cpu", weights_only=True)
        return None

    def load_checkpoint(self, checkpoint_path, accelerator=None):
        """Ingest a reference checkpoint directory (reference :769-805).  Returns the reference's triple
        (epoch, best_metric, experiment_key); (None, None, None) when experiment_state.pth is absent."""
        sd = self._read_state(checkpoint_path, "model")
        if sd is None:
            raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {checkpoint_path}")
        self.model.load_state_dict(sd)
        ema_sd = self._read_state(checkpoint_path, "model_1")
        if ema_sd is None:
            # classification always runs on the EMA copy: scoring silently with the online weights would be a wrong answer
            raise FileNotFoundError(f"no model_1.safetensors / pytorch_model_1.bin (EMA weights) under {checkpoint_path}")
        inner = {k[len("ema_model."):]: v for k, v in ema_sd.items() if k.startswith("ema_model.")}
        self.ema.ema_model.load_state_dict(inner)
        for k in ("initted", "step"):
            if k in ema_sd:
                getattr(self.ema, k).copy_(ema_sd[k].reshape(()))
        enc_sd = self._read_state(checkpoint_path, "model_2")
        if self.encoder is not None:
            if enc_sd is None:
                raise FileNotFoundError(f"no model_2.safetensors (class-token encoder) under {checkpoint_path}")
            self.encoder.load_state_dict(enc_sd)
            if self.encoder_type in ('t5', 'clip'):
                self._prompts_set = True         # the checkpoint's table is the encoder's output for the prompts it was saved with
        st = os.path.join(checkpoint_path, "experiment_state.pth")
        if os.path.exists(st):
            state = torch.load(st, map_location="cpu", weights_only=False)
            print(f"Checkpoint loaded. Resuming from epoch {state.get('epoch')}. Best metric {state.get('best_metric')}")
            return state.get("epoch"), state.get("best_metric"), state.get("experiment_key")
        return None, None, None

    def save_checkpoint(self, checkpoint_dir, epoch=0, best_metric=None, experiment_key=None):
        """Write the same directory layout (used for round trips and for handing weights back to the reference)."""
        from safetensors.torch import save_file
        os.makedirs(checkpoint_dir, exist_ok=True)
        cpu = lambda sd: {k: v.detach().cpu().contiguous() for k, v in sd.items()}
        save_file(cpu(self.model.state_dict()), os.path.join(checkpoint_dir, "model.safetensors"))
        ema_sd = {"ema_model." + k: v for k, v in self.ema.ema_model.state_dict().items()}
        ema_sd.update({"online_model." + k: v for k, v in self.model.state_dict().items()})
        ema_sd.update(initted=self.ema.initted.reshape(1), step=self.ema.step.reshape(1))
        save_file(cpu(ema_sd), os.path.join(checkpoint_dir, "model_1.safetensors"))
        if self.encoder is not None:
            save_file(cpu(self.encoder.state_dict()), os.path.join(checkpoint_dir, "model_2.safetensors"))
        torch.save({"epoch": epoch + 1, "best_metric": best_metric, "experiment_key": experiment_key},
                   os.path.join(checkpoint_dir, "experiment_state.pth"))
