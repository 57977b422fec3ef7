"""float64 oracle of the WEIGHTED scoring losses (diffusion_classifier_amd/loss.py "Weights", include/dcamd.h pixel_w / trial_w): the
sums of tests/score_loss_oracle.py with a pixel weight m[y, x] >= 0 on every term and a trial weight w >= 0 on every unit, and that
module's error model carried one step further.  m and w are the fp32 numbers the implementation sees, taken to float64 exactly.

    err = w * sum over C H W of m t(d)            v[y, x] = w * m[y, x] * sum over the channels of t(d)

Error model (score_loss_oracle's notation: u, gamma(k), R roundings of a term, `adds` additions on the path of a term, Ab the absolute
part that the rounded difference d^ leaves, SQRT_SQUARE for l2's sqrt-then-square):
  a weighted term   m t(d^) costs one more fp32 multiply than t(d^): R + 1 roundings (l2 as the kernels form it, (m d^) d^ with the
                    second product fused into the sum, rounds once in all: R + 1 covers it).  m is exact, so the absolute part scales:
                    Ab_w = sum m Lip h (l2: sum m (2 |d| h + h^2)).
  the sum           m >= 0 keeps every term non-negative, so score_loss_oracle's argument holds unchanged: the computed sum is within
                    gamma(R + 1 + adds) of the exact sum of the computed terms.
  the unit          r (after l2's SQRT_SQUARE roundings) times w: one more rounding per unit.  All of these are relative roundings of
                    one non-negative number, hence
                        |computed - w S| <= w [gamma(R + 1 + adds (+ SQRT_SQUARE) + 1) (S + Ab_w) + Ab_w],     S = sum m t(d).
  a map pixel       the channel sum as before (R roundings, C - 1 adds), then times m and times w: two more roundings, then the
                    quantisation:  |plane - w m v0| <= w m [gamma(R + C - 1 + 2) (v0 + Ab_pix) + Ab_pix] + QUANT.
  pixel sum         the pixel sum of a unit's dequantised plane against the scalar error of the same unit, as in score_loss_oracle: both
                    sides are within their own bound of w S, the planes' H W quantisations add up.
Nothing here was fitted to what an implementation returns."""
import numpy as np

import score_loss_oracle as O

M_ROUNDINGS = 1          # the multiply by m, per term
W_ROUNDINGS = 1          # the multiply by w, per unit


def weighted_sums(d, h, kind, delta, m, w):
    """(d, h) of score_loss_oracle.differences [n, C, H, W]; m [n, H, W] and w [n], the units' own weights (float64) -> dict like
    score_loss_oracle.sums: err / Ab [n] (S and Ab_w above, NOT yet times w), v / Ab_pix [n, H, W] (the unweighted channel sums), plus
    m and w."""
    with np.errstate(all="ignore"):
        t = O.term(d, kind, delta)
        if kind == "l2":
            ab = 2 * np.abs(d) * h + h * h
        else:
            ab = (1.0 if kind == "l1" else float(np.float32(delta))) * h
        mm = m[:, None]
        return dict(err=(mm * t).sum(axis=(1, 2, 3)), Ab=(mm * ab).sum(axis=(1, 2, 3)), v=t.sum(axis=1), Ab_pix=ab.sum(axis=1), m=m, w=w)


def scalar_value(o):
    return o["w"] * o["err"]


def scalar_bound(o, kind, adds):
    g = O.gamma(O.ROUNDINGS[kind] + M_ROUNDINGS + adds + (O.SQRT_SQUARE if kind == "l2" else 0) + W_ROUNDINGS)
    return o["w"] * (g * (o["err"] + o["Ab"]) + o["Ab"])


def pixel_value(o):
    return o["w"][:, None, None] * o["m"] * o["v"]


def pixel_bound(o, kind, C):
    g = O.gamma(O.ROUNDINGS[kind] + C - 1 + M_ROUNDINGS + W_ROUNDINGS)
    return o["w"][:, None, None] * o["m"] * (g * (o["v"] + o["Ab_pix"]) + o["Ab_pix"]) + O.QUANT


def pixel_sum_bound(o, kind, C, H, W, adds_scalar):
    """|pixel sum of a unit's dequantised plane - the unit's scalar error| per unit: the two bounds above, summed."""
    return pixel_bound(o, kind, C).sum(axis=(1, 2)) + scalar_bound(o, kind, adds_scalar)
