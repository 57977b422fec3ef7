"""Test-side oracle pieces for a published-style DiT (learned variance, the discrete 'ddpm_linear' schedule): an independent fp64
restatement of the schedule's log-SNR table, `oracle.OracleDiT` behind a wrapper that keeps the eps channels and takes the DDPM step as
its time input, `oracle.OracleDiffusionClassifier` over it, and the small models / directories the host and GPU tests share.  No GPU."""
import contextlib
import copy
import io
import json
import math

import torch
import torch.nn as nn

import diffusion_classifier_amd as dca
import oracle

# the two small geometries: eps is 16 of the 32 projection columns (the XL/2 case, below one N tile) and 64 of 128
DIT_A = dict(num_attention_heads=2, attention_head_dim=32, in_channels=4, out_channels=8, num_layers=2, sample_size=8, patch_size=2,
             num_embeds_ada_norm=10)
DIT_B = dict(DIT_A, patch_size=4, sample_size=16)
CFG = dict(pred_param="eps", schedule="ddpm_linear", cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1, encoder_type="DiT", classes=3,
           n_stages=1, evaluation_per_stage=[4], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32")


def ref_logsnr(N=1000, b0=1e-4, b1=0.02):
    """Independent fp64 restatement of the DDPM linear schedule: plain Python floats -> [N] log(abar_k / (1 - abar_k))."""
    lam, abar = [], 1.0
    for i in range(N):
        beta = b0 + (b1 - b0) * i / (N - 1) if N > 1 else b0
        abar *= 1.0 - beta
        lam.append(math.log(abar / (1.0 - abar)))
    return lam


def randomise_vectors(m):
    """Default inits leave biases tiny: randomise them so a dropped or misplaced bias row shows."""
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)


def make_dit(kw, seed):
    torch.manual_seed(seed)
    m = dca.DiT(**kw)
    randomise_vectors(m)
    return m


def eps_twin(m):
    """The out_channels = in_channels model whose proj_out_2 holds exactly the eps rows (py * p + px) * oc + c, c < C, of `m`; every
    other parameter is m's.  Written out here with a reshape, not through the package's row index."""
    cfg = m.config
    p, C, oc = cfg.patch_size, cfg.in_channels, cfg.out_channels
    kw = dict(num_attention_heads=cfg.num_attention_heads, attention_head_dim=cfg.attention_head_dim, in_channels=C, out_channels=C,
              num_layers=cfg.num_layers, sample_size=cfg.sample_size, patch_size=p, num_embeds_ada_norm=cfg.num_embeds_ada_norm)
    twin = dca.DiT(**kw)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    D = sd["proj_out_2.weight"].shape[1]
    sd["proj_out_2.weight"] = sd["proj_out_2.weight"].reshape(p * p, oc, D)[:, :C].reshape(p * p * C, D).contiguous()
    sd["proj_out_2.bias"] = sd["proj_out_2.bias"].reshape(p * p, oc)[:, :C].reshape(-1).contiguous()
    twin.load_state_dict(sd, strict=True)
    return twin


class EpsOfStepDiT(nn.Module):
    """`oracle.OracleDiT` as the backbone of the oracle classifier: records every time input it was fed (`seen_labels`), runs the full
    model and keeps the first in_channels channels — eps, the variance half dropped."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.config = inner.config
        self.seen_labels = []

    def forward(self, x, noise_labels, encoder_hidden_states=None):
        self.seen_labels.append(noise_labels.detach().clone())
        return self.inner(x, noise_labels, encoder_hidden_states)[:, :self.config.in_channels]


class OracleDiscreteClassifier(oracle.OracleDiffusionClassifier):
    """The oracle's scoring loop on the discrete grid: alpha and sigma from the fp64 table's log-SNR of step k = min(floor(t N), N - 1),
    the backbone fed float(k).  The oracle's loop forms alpha / sigma from what `schedule(t)` returns and hands its backbone the same
    tensor: `schedule` returns the table's log-SNR, and `_StepFed` in front of the backbone turns it back into its step by an exact
    lookup in the (strictly decreasing) table."""

    def __init__(self, backbone, config, table):
        super().__init__(backbone, oracle.AttrBag(**dict(config, schedule="cosine")))      # (the oracle knows the cosine names only)
        self.table = torch.tensor(table, dtype=torch.float64).to(torch.float32)
        assert bool((self.table[1:] < self.table[:-1]).all())                               # strictly decreasing: the lookup is exact
        self.ema_model = _StepFed(self.ema_model, self.table)

    def schedule(self, t):
        N = self.table.numel()
        k = torch.clamp(torch.floor(t.to(torch.float64) * N), 0, N - 1).to(torch.int64)
        return self.table[k]


class _StepFed(nn.Module):
    def __init__(self, inner, table):
        super().__init__()
        self.inner, self.table = inner, table

    def forward(self, x, noise_labels, encoder_hidden_states=None):
        hit = noise_labels.reshape(-1, 1) == self.table.reshape(1, -1)
        assert bool((hit.sum(1) == 1).all())
        return self.inner(x, hit.float().argmax(1).to(torch.float32), encoder_hidden_states)


def oracle_classifier(m, cfg, **table_kw):
    """The oracle classifier for the HIP model `m` (its weights loaded into an OracleDiT) under `cfg` -> (classifier, the wrapper whose
    `seen_labels` hold every time input the oracle backbone was fed)."""
    kw = {k: getattr(m.config, k) for k in ("num_attention_heads", "attention_head_dim", "in_channels", "out_channels", "num_layers",
                                            "sample_size", "patch_size", "num_embeds_ada_norm")}
    o = oracle.OracleDiT(**kw)
    o.load_state_dict(m.state_dict())
    oc = OracleDiscreteClassifier(EpsOfStepDiT(o), cfg, ref_logsnr(**table_kw))
    return oc, oc.ema_model.inner


def classifier(backbone, **over):
    """DiffusionClassifier over a copy of `backbone` (moving the classifier to a device leaves the caller's model where it is) under CFG
    with `over` -> (classifier, the config as a dict)."""
    backbone = copy.deepcopy(backbone)
    cfg = dict(CFG, noise_d=backbone.config.sample_size, image_size=backbone.config.sample_size)
    cfg.update(over)
    with contextlib.redirect_stdout(io.StringIO()):
        return dca.DiffusionClassifier(backbone, dca.Config(**cfg)), cfg


# ---- directories ---------------------------------------------------------------------------------
PUBLISHED_EXTRAS = dict(cross_attention_dim=None, num_vector_embeds=None, only_cross_attention=False, use_linear_projection=False,
                        double_self_attention=False, attention_type="default", caption_channels=None, interpolation_scale=None,
                        activation_fn="gelu-approximate", attention_bias=True, dropout=0.0, norm_elementwise_affine=False, norm_num_groups=32,
                        norm_type="ada_norm_zero", upcast_attention=False, norm_eps=1e-5)


def write_transformer(root, name, kw, sd=None, extra_cfg=None, drop=()):
    """A diffusers-style transformer directory under `root`: config.json with the published key set around `kw`, and the weights."""
    from safetensors.torch import save_file
    d = root / name
    d.mkdir(parents=True)
    cfg = dict(PUBLISHED_EXTRAS, **kw)
    cfg.update(_class_name="Transformer2DModel", _diffusers_version="0.12.0.dev0", _name_or_path="somewhere")
    cfg.update(extra_cfg or {})
    for k in drop:
        del cfg[k]
    (d / "config.json").write_text(json.dumps(cfg))
    if sd is not None:
        save_file({k: v.detach().cpu().contiguous() for k, v in sd.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    return str(d)


def write_scheduler(root, name="scheduler", **kw):
    d = root / name
    d.mkdir(parents=True)
    cfg = dict(_class_name="KarrasDiffusionSchedulers", beta_schedule="linear", beta_start=1e-4, beta_end=0.02, num_train_timesteps=1000,
               prediction_type="epsilon")
    cfg.update(kw)
    (d / "scheduler_config.json").write_text(json.dumps(cfg))
    return str(d)
