"""The names the discrete grid's ancestral statements had before ancestral.py held every loop once: thin aliases, no loop of their own.
New code takes `ancestral.step_kind` and the loops there."""
from . import ancestral as AN
from . import trajectory as TJ

posterior_scalars = AN.Linear.scalars
mean_eager = AN.linear_mean


def latent_scalars(g):
    return [TJ.point_scalars(v) for v in g.lam]


def ancestral_eager(dc, z0, conds, null, g, lens=None, noise_maps=None):
    return AN.ancestral_eager(AN.step_kind(dc, g, dc.cfg_w), z0, conds, null, lens, noise_maps)


def noise_maps_eager(dc, x, lab, g, w):
    return AN.noise_maps_eager(AN.step_kind(dc, g, w), x, lab)
