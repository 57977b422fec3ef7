"""Host: the two ancestral step kinds (ancestral.py) state the same step.  `Clipped` is the cosine schedules' `ddpm_sampler_step`,
`Linear` the discrete grid's mu = a z + b x; where the clip is inactive they are two fp32 spellings of one posterior, and nothing else
in the suite ties them together.  No GPU, no library.

Cases: pred_param in {eps, v} x guidance weight in {0, 2} x two neighbouring grid points (1 -> 2 of 4 steps from from_t = 0.2) of a
cosine grid and of a discrete grid (N = 1000, trailing: steps 149 -> 99), tensors [2, 3, 8, 8].  A small foreign module whose output is
bounded by 0.1 and inputs |x|, |e| < 0.3 keep the data prediction inside (-1, 1): asserted for every case, measured |x_pred| <= 0.42.

The reference is the posterior mean evaluated in fp64 from the same inputs (z, the prediction pair, the two fp32 log-SNRs, w).  Worst
fp32 deviation of either kind from it, measured on the CPU over all cases (this file prints them; values are about 0.3, one ulp 3e-8):
  mean     5.28e-8   (Clipped 5.28e-8, Linear 4.62e-8)      MEAN_BOUND   = 2.2e-7
  update   6.23e-8   (Clipped 6.23e-8, Linear 5.76e-8)      UPDATE_BOUND = 2.5e-7
  map      3.97e-7   (Clipped 3.97e-7, Linear 3.61e-7)      MAP_BOUND    = 1.6e-6   (the mean's error over sd; sd = 0.118 and 0.213)
Each bound is 4 x the measured value, the margin DESIGN §6p takes for its coefficient checks (other platforms' libm).  Every kind must
stay within the bound of fp64, and the two kinds within the bound of each other (measured: mean 5.96e-8, update 5.96e-8, map 5.07e-7).
"""
import contextlib
import io
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import ancestral as AN
from diffusion_classifier_amd import trajectory as TJ

MEAN_BOUND, UPDATE_BOUND, MAP_BOUND = 2.2e-7, 2.5e-7, 1.6e-6
T = 1                                                                          # the step 1 -> 2 of the 4-step grid


class SmallNet(nn.Module):
    """A foreign module with |output| <= 0.1 that depends on x, the context and the time input."""

    def __init__(self, ch=3, hid=4):
        super().__init__()
        self.config = SimpleNamespace(encoder_hid_dim=hid)
        self.mix = nn.Parameter(torch.randn(ch, ch))
        self.lin = nn.Linear(hid, ch)

    def forward(self, x, noise_labels, encoder_hidden_states=None):
        t = noise_labels.to(x.dtype).reshape(-1, 1).expand(x.shape[0], 1)
        gain = torch.tanh(self.lin(encoder_hidden_states[:, 0])) + torch.cos(0.37 * t)
        return 0.1 * torch.tanh(torch.einsum("oc,bchw->bohw", self.mix, x) * gain[:, :, None, None])


def _dc(schedule, pred_param, w):
    torch.manual_seed(5)
    cfg = dict(pred_param=pred_param, schedule=schedule, noise_d=8, image_size=8, cfg_w=w, ema_beta=0.999, ema_warmup=0, ema_update_freq=1,
               encoder_type="nn", classes=3, n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, sampling_steps=4)
    if schedule == "scaled_linear":
        cfg.update(train_timesteps=1000, timestep_spacing="trailing")
    with contextlib.redirect_stdout(io.StringIO()):
        return dca.DiffusionClassifier(SmallNet(), dca.Config(**cfg))


def _case(schedule, pred_param, w):
    """The three quantities of step T by both kinds and in fp64, from one set of inputs -> {name: (clipped, linear, fp64)}, |x_pred|.max."""
    dc = _dc(schedule, pred_param, w)
    g = TJ.grid(dc, 0.2, 0.0)
    gen = torch.Generator().manual_seed(11)
    x, e, e_next, noise = (torch.rand(2, 3, 8, 8, generator=gen) * 0.6 - 0.3 for _ in range(4))
    (al_t, sg_t), (al_s, sg_s) = TJ.point_scalars(g.lam[T]), TJ.point_scalars(g.lam[T + 1])
    z, x_next = al_t * x + sg_t * e, al_s * x + sg_s * e_next
    with torch.no_grad():
        cond, null, lens = TJ.contexts(dc, torch.tensor([2, 0]), x.device, dc.ema.ema_model)
        pred, u_pred = TJ.guided_pair(dc, z, g.label[T].unsqueeze(0), cond, null, lens)
        got = []
        for kind in (AN.Clipped(dc, g, w), AN.Linear(dc, g, w)):
            mu, spread = kind.mean(z, pred, u_pred, T)
            got.append((mu, kind.update(mu, noise, spread), kind.noise_map(x_next, mu, spread)))
    # fp64, the posterior of `ddpm_sampler_step` without the clip
    lt, ls = g.lam[T].double(), g.lam[T + 1].double()
    c = -torch.special.expm1(lt - ls)
    at, as_, st, ss = torch.sqrt(torch.sigmoid(lt)), torch.sqrt(torch.sigmoid(ls)), torch.sqrt(torch.sigmoid(-lt)), torch.sqrt(torch.sigmoid(-ls))
    pr = (1 + w) * pred.double() - w * u_pred.double()
    x_pred = at * z.double() - st * pr if pred_param == "v" else (z.double() - st * pr) / at
    mu = as_ * (z.double() * (1 - c) / at + c * x_pred)
    sd = torch.sqrt(ss ** 2 * c)
    want = (mu, mu + sd * noise.double(), (x_next.double() - mu) / sd)
    return {name: (got[0][j], got[1][j], want[j]) for j, name in enumerate(("mean", "update", "map"))}, float(x_pred.abs().max()), float(sd)


@pytest.mark.parametrize("w", [0.0, 2.0])
@pytest.mark.parametrize("pred_param", ["eps", "v"])
@pytest.mark.parametrize("schedule", ["cosine", "scaled_linear"])
def test_clipped_and_linear_kinds_agree_where_the_clip_is_inactive(schedule, pred_param, w):
    vals, x_max, sd = _case(schedule, pred_param, w)
    assert x_max < 1.0, x_max                                                  # the clip is inactive: the case says something
    for name, bound in (("mean", MEAN_BOUND), ("update", UPDATE_BOUND), ("map", MAP_BOUND)):
        clipped, linear, want = vals[name]
        assert clipped.dtype == linear.dtype == torch.float32
        dc_, dl, dd = (float((a.double() - b.double()).abs().max()) for a, b in ((clipped, want), (linear, want), (clipped, linear)))
        print(f"{schedule} {pred_param} w={w} {name}: |x_pred|.max {x_max:.3f}, sd {sd:.3f}, Clipped vs fp64 {dc_:.2e}, Linear vs fp64 {dl:.2e}, "
              f"Clipped vs Linear {dd:.2e} (bound {bound:g})")
        assert dc_ <= bound and dl <= bound and dd <= bound, (name, dc_, dl, dd, bound)
