"""float64 oracle of the scoring losses (diffusion_classifier_amd/loss.py, include/dcamd.h DC_LOSS_*): the three sums over C * H * W and
the per-pixel channel sums v[y, x], computed from the fp32 tensors the implementation sees (taken to float64 exactly) and written from
the definitions, independently of the package's torch statements.  Plus the tolerances, with their derivation.

Definitions, d = eps_hat - eps (eps-param: eps_hat = pred; v-param: eps_hat = sigma z + alpha pred, z = alpha x + sigma eps):
    l2      t(d) = d^2
    l1      t(d) = |d|
    huber   t(d) = 0.5 d^2 if |d| <= delta else delta (|d| - 0.5 delta)
err = sum over C * H * W of t(d),  v[y, x] = sum over the channels of t(d).

Error model (u = 2^-24, the fp32 unit roundoff; gamma(k) = k u / (1 - k u), the usual bound on k accumulated relative roundings; the
bounds on d are first order in u, as tests/evidence_oracle.py's are: what is dropped is below 1e-6 of what is kept).

  the difference   fp32 computes d^ = d + eta with |eta| <= h:
                     eps-param   one subtraction: h = u |d|
                     v-param     A = |alpha x| + |sigma eps|, B = |sigma z|, P = |alpha pred|, E = |eps|.  z is off by u (A + |z|),
                                 sigma z by |sigma| u (A + |z|) + u B = u (|sigma| A + 2 B), alpha pred by u P, their sum by
                                 u |eps_hat| <= u (B + P), d by u |d| <= u (B + P + E):  h = u (|sigma| A + 4 B + 3 P + E).
                                 (A fused multiply-add only removes roundings.)
  the term         t is Lipschitz in d: |t(d^) - t(d)| <= Lip h with Lip = 1 (l1) and delta (huber: |t'| <= delta everywhere, and t is
                   continuous at |d| = delta, so which branch the rounded d^ takes does not matter).  For l2 |t(d^) - t(d)| <=
                   2 |d| h + h^2.  Evaluating t(d^) in fp32 costs R relative roundings of the (non-negative) result:
                     l1 0 (|.| is exact);  l2 1 (the product);  huber 2: 0.5 d^ is exact and its product with d^ rounds once, and on
                     the other branch |d^| - 0.5 delta rounds once (0.5 delta is exact) and its product with delta once more.
  a sum            all terms are non-negative, so a sum that puts at most `adds` additions on the path of any term is within
                   gamma(R + adds) of the exact sum of the computed terms, whatever the order:
                     dc_eps_mse          a lane's strided sum of ceil(N / 256) terms, 6 shuffle steps, 3 adds of wave partials:
                                         adds = ceil(N / 256) + 9 (N = C H W), as evidence_oracle.pixel_sum_bound counts them
                     a pixel of the map  the channels in order: adds = C - 1
                     torch on the host   an order this file does not know: adds = N - 1 covers every order
                   l2 alone goes through sqrt then square: u, then 2 u + u: SQRT_SQUARE = 4 more roundings.
  together         with T^ = sum t(d^) (exact sum of exact terms of the rounded differences) and Ab = sum Lip h (l2: sum 2 |d| h + h^2):
                     |T^ - T| <= Ab   and   |computed - T^| <= gamma(R + adds) T^ <= gamma(R + adds) (T + Ab)
                   so |computed - T| <= gamma(R + adds) (T + Ab) + Ab: a relative part and an absolute part.
  the map          each unit-pixel is quantised, rint((double) v 2^F) 2^-F: within QUANT = 2^-(F + 1) of the fp32 v.
  pixel sum        the pixel sum of a unit's dequantised plane against the scalar error of the same unit: both sides are within their
                   own bound of T, so |sum - scalar| <= [gamma(R + C - 1) + gamma(R + adds_scalar (+ 4 for l2))] (T + Ab) + 2 Ab
                   + H W QUANT; on the host both sides start from the same fp32 d^ (one subtraction, the same bits), which makes T^
                   the common truth and drops the 2 Ab: `pixel_sum_bound(..., same_d=True)`.
These are derived bounds: nothing here was fitted to what an implementation returns."""
import numpy as np

U = 2.0 ** -24
F = 30
QUANT = 2.0 ** -(F + 1)
KINDS = ("l2", "l1", "huber")
ROUNDINGS = {"l2": 1, "l1": 0, "huber": 2}
SQRT_SQUARE = 4


def gamma(k):
    return k * U / (1.0 - k * U)


def term(d, kind, delta=1.0):
    """t(d) in float64."""
    d = np.asarray(d, dtype=np.float64)
    if kind == "l2":
        return d * d
    a = np.abs(d)
    if kind == "l1":
        return a
    assert kind == "huber" and delta > 0
    dl = float(np.float32(delta))                    # delta as fp32
    return np.where(a <= dl, 0.5 * d * d, dl * (a - 0.5 * dl))


def differences(pred, eps, x, alpha, sigma, bj_of_unit, img_of_bj, v_param):
    """pred [n_units, C, H, W], eps [n_bj, C, H, W], x [n_img, C, H, W], alpha / sigma [n_bj] (fp32 arrays) -> (d, h): float64
    [n_units, C, H, W], the exact difference and the bound on what its fp32 evaluation is off by."""
    pred, eps = np.asarray(pred, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    e = eps[np.asarray(bj_of_unit)]
    with np.errstate(all="ignore"):
        if not v_param:
            d = pred - e
            return d, U * np.abs(d)
        al = np.asarray(alpha, dtype=np.float64)[bj_of_unit][:, None, None, None]
        sg = np.asarray(sigma, dtype=np.float64)[bj_of_unit][:, None, None, None]
        xi = np.asarray(x, dtype=np.float64)[np.asarray(img_of_bj)[bj_of_unit]]
        z = al * xi + sg * e
        d = sg * z + al * pred - e
        A, B, P, E = np.abs(al * xi) + np.abs(sg * e), np.abs(sg * z), np.abs(al * pred), np.abs(e)
        return d, U * (np.abs(sg) * A + 4 * B + 3 * P + E)


def sums(d, h, kind, delta=1.0):
    """(d, h) of `differences` -> dict: err [n] and v [n, H, W], the exact sums; Ab [n] and Ab_pix [n, H, W], the absolute parts."""
    with np.errstate(all="ignore"):
        t = term(d, kind, delta)
        if kind == "l2":
            ab = 2 * np.abs(d) * h + h * h
        else:
            ab = (1.0 if kind == "l1" else float(np.float32(delta))) * h
        return dict(err=t.sum(axis=(1, 2, 3)), v=t.sum(axis=1), Ab=ab.sum(axis=(1, 2, 3)), Ab_pix=ab.sum(axis=1))


def scalar_bound(o, kind, adds):
    """|computed error - o["err"]| per unit for a sum with `adds` additions on a path (dc_eps_mse: eps_mse_adds(N))."""
    g = gamma(ROUNDINGS[kind] + adds + (SQRT_SQUARE if kind == "l2" else 0))
    return g * (o["err"] + o["Ab"]) + o["Ab"]


def eps_mse_adds(N):
    return -(-N // 256) + 9


def pixel_bound(o, kind, C):
    """|dequantised plane - o["v"]| per unit-pixel."""
    return gamma(ROUNDINGS[kind] + C - 1) * (o["v"] + o["Ab_pix"]) + o["Ab_pix"] + QUANT


def pixel_sum_bound(o, kind, C, H, W, adds_scalar, same_d):
    """|pixel sum of a unit's dequantised plane - the unit's scalar error|, per unit (the model: this file's docstring, `pixel sum`)."""
    R = ROUNDINGS[kind]
    g = gamma(R + C - 1) + gamma(R + adds_scalar + (SQRT_SQUARE if kind == "l2" else 0))
    return g * (o["err"] + o["Ab"]) + (0.0 if same_d else 2.0 * o["Ab"]) + H * W * QUANT
