"""float64 oracle of the class evidence maps (diffusion_classifier_amd/evidence.py, include/dcamd.h `dc_err_map` / `dc_evidence_maps`),
written from the definitions and independently of the package's own torch statement, plus the tolerances with their derivation.

Inputs are the fp32 tensors the implementation sees, taken to float64 exactly.  `unit_maps` gives, per (unit, pixel), the exact
v = sum_ch (eps_hat - eps)^2 and a bound on what an fp32 evaluation of it can be off by; `maps` turns per-unit values into the
mean / delta maps of a call and carries the bounds along.

Tolerances (u = 2^-24, the fp32 unit roundoff; every bound first-order with the second-order terms written out where they are kept):

  per unit-pixel, eps-param   d = fl(pred - eps) is off by u |d|, d*d by another u, so each term d^2 carries at most 3 u d^2; the
                              sequential sum of C non-negative terms adds (C - 1) u v: |fl(v) - v| <= (C + 2) u v.  (A fused
                              multiply-add only removes roundings.)
  per unit-pixel, v-param     eps_hat = fl(sigma * fl(alpha x + sigma eps) + alpha pred) with 0 <= sigma <= 1 (a square root of a
                              sigmoid).  With A = |alpha x| + |sigma eps|, B = |sigma z|, P = |alpha pred|, E = |eps|:  z is off by
                              u (A + |z|), sigma z by sigma u (A + |z|) + u B <= u (A + 2 B), alpha pred by u P, their sum by
                              u |eps_hat| <= u (B + P), and d = eps_hat - eps by u |d| <= u (B + P + E):
                              |fl(d) - d| <= u (A + 4 B + 3 P + E) <= 4 u M,  M = A + B + P + E.  Then |fl(d)^2 - d^2| <= 2 |d| (4 u M) +
                              (4 u M)^2, the product rounds once more (u d^2), the channel sum adds (C - 1) u v:
                              |fl(v) - v| <= sum_ch (8 u M |d| + 16 u^2 M^2) + (C + 1) u v   (second order in u dropped in the last term).
  quantisation                rint((double) v 2^F) 2^-F is within 2^-(F+1) of v, per unit.
  a map value                 mean = (sum over the n units of a cell) / n: the unit bounds add and are divided by n; delta sums the
                              bounds of the class's and of the winner's units.  The int64 sum is exact; int64 -> double and the double
                              division are within 2 * 2^-53 relative; the one rounding to f32 is u |value|.  `FINAL` = u + 2^-51 covers
                              the three.
These are derived bounds: nothing here was fitted to what an implementation returns."""
import numpy as np

U = 2.0 ** -24
F = 30
VMAX = 2.0 ** 14
QUANT = 2.0 ** -(F + 1)
FINAL = U + 2.0 ** -51


def unpatchify(pred_rows, C, H, W, patch):
    """The prediction as the image [n, C, H, W] from the layout the kernels read: patch <= 1: NHWC rows [n, H, W, ld]; patch > 1: DiT's
    projection [n, H/p, W/p, ld] with k = (py * p + px) * C + c."""
    n = pred_rows.shape[0]
    if patch > 1:
        p = patch
        g = pred_rows[..., :p * p * C].reshape(n, H // p, W // p, p, p, C)
        return np.ascontiguousarray(g.transpose(0, 5, 1, 3, 2, 4).reshape(n, C, H, W))
    return np.ascontiguousarray(pred_rows[..., :C].transpose(0, 3, 1, 2))


def unit_maps(pred, eps, x, alpha, sigma, bj_of_unit, img_of_bj, v_param):
    """pred [n_units, C, H, W], eps [n_bj, C, H, W], x [n_img, C, H, W], alpha / sigma [n_bj] (fp32 arrays) -> (v, bound): float64
    [n_units, H, W], the exact channel sum and the fp32 evaluation bound plus the quantisation (non-finite where v is)."""
    pred, eps, x = (np.asarray(a, dtype=np.float64) for a in (pred, eps, x))
    C = pred.shape[1]
    e = eps[bj_of_unit]
    with np.errstate(all="ignore"):
        if v_param:
            al = np.asarray(alpha, dtype=np.float64)[bj_of_unit][:, None, None, None]
            sg = np.asarray(sigma, dtype=np.float64)[bj_of_unit][:, None, None, None]
            xi = x[np.asarray(img_of_bj)[bj_of_unit]]
            z = al * xi + sg * e
            eh = sg * z + al * pred
            d = eh - e
            M = np.abs(al * xi) + np.abs(sg * e) + np.abs(sg * z) + np.abs(al * pred) + np.abs(e)
            v = (d * d).sum(1)
            bound = (8 * U * M * np.abs(d) + 16 * U * U * M * M).sum(1) + (C + 1) * U * v
        else:
            d = pred - e
            v = (d * d).sum(1)
            bound = (C + 2) * U * v
    return v, bound + QUANT


def maps(v, bound, cell_of_unit, trial_of_unit, stage_ends, BS, C, n_eval, winner):
    """Per-unit maps -> the call's maps.  cell_of_unit [n_units] (b * C + c; < 0: a padded slot, ignored), trial_of_unit [n_units],
    stage_ends ascending, n_eval [BS, C] (0 or a stage end), winner [BS] (-1: none).  A unit counts for its cell iff its trial is below
    n_eval of the cell.  Returns dict(mean, delta, mean_bound, delta_bound [BS, C, H, W] float64 — NaN where the definition says NaN —,
    invalid [BS], bad [BS, C]: the values that are not finite or above VMAX among the counted units)."""
    H, W = v.shape[1:]
    nan = np.full((H, W), np.nan)
    S = np.zeros((BS, C, H, W)); SB = np.zeros((BS, C, H, W)); bad = np.zeros((BS, C), dtype=np.int64)
    # the winner's sum over the trials class c has: Sw[b, c]
    Sw = np.zeros((BS, C, H, W)); SwB = np.zeros((BS, C, H, W))
    ok_v = np.isfinite(v) & (v >= 0) & (v <= VMAX)
    vz, bz = np.where(ok_v, v, 0.0), np.where(ok_v, bound, 0.0)
    for u in range(v.shape[0]):
        cell = int(cell_of_unit[u])
        if cell < 0:
            continue
        b, c = divmod(cell, C)
        j = int(trial_of_unit[u])
        if j < int(n_eval[b, c]):
            S[b, c] += vz[u]; SB[b, c] += bz[u]; bad[b, c] += int((~ok_v[u]).sum())
        if int(winner[b]) == c:
            for cc in range(C):
                if j < int(n_eval[b, cc]):
                    Sw[b, cc] += vz[u]; SwB[b, cc] += bz[u]
    out = dict(mean=np.zeros((BS, C, H, W)), delta=np.zeros((BS, C, H, W)), mean_bound=np.zeros((BS, C, H, W)),
               delta_bound=np.zeros((BS, C, H, W)), bad=bad, invalid=np.zeros(BS, dtype=np.int64))
    ends = [int(e) for e in stage_ends]
    for b in range(BS):
        for c in range(C):
            n = int(n_eval[b, c])
            if n > 0 and n in ends:
                out["invalid"][b] += bad[b, c]
            if n == 0 or n not in ends or bad[b, c] > 0 or not 0 <= int(winner[b]) < C:
                for k in ("mean", "delta", "mean_bound", "delta_bound"):
                    out[k][b, c] = nan
                continue
            out["mean"][b, c] = S[b, c] / n
            out["delta"][b, c] = (S[b, c] - Sw[b, c]) / n
            out["mean_bound"][b, c] = SB[b, c] / n + FINAL * np.abs(out["mean"][b, c])
            out["delta_bound"][b, c] = (SB[b, c] + SwB[b, c]) / n + FINAL * np.abs(out["delta"][b, c])
            if int(winner[b]) == c:
                out["delta_bound"][b, c] = 0.0           # exactly 0: the int64 difference of a plane with itself
    return out


def check(ev, o, label=""):
    """A ClassEvidence (tensors) against `maps`' result: the NaN pattern must be the oracle's, every other pixel within its bound.
    Returns the measured maxima of error / bound."""
    got_m, got_d = ev.mean_map.detach().cpu().double().numpy(), ev.delta_map.detach().cpu().double().numpy()
    measured = {}
    for name, got, want, bound in (("mean", got_m, o["mean"], o["mean_bound"]), ("delta", got_d, o["delta"], o["delta_bound"])):
        assert got.shape == want.shape, (label, name, got.shape, want.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (label, name, "NaN pattern")
        fin = ~np.isnan(want)
        assert np.isfinite(got[fin]).all(), (label, name)
        err = np.abs(got - want)[fin]
        measured[name + "_over_bound"] = float((err / np.maximum(bound[fin], 1e-300)).max()) if fin.any() else 0.0
        measured[name + "_abs"] = float(err.max()) if fin.any() else 0.0
        assert (err <= bound[fin]).all(), (label, name, measured)
    assert np.array_equal(ev.invalid.detach().cpu().numpy().astype(np.int64), o["invalid"]), (label, ev.invalid, o["invalid"])
    return measured


def pixel_sum_bound(C, H, W, n):
    """(rel, abs): how far the pixel sum of mean_map[b, c] (taken in float64 from the f32 map) may be from the posterior's fp32
    means[b, c] when both are computed from the same fp32 predictions (eps-param), |sum - mean| <= rel * mean + abs.
      map side    every v within (C + 2) u v, every unit-pixel quantised within 2^-(F+1) (H W of them per unit, averaged over n units:
                  abs = H W 2^-(F+1)), one rounding of the map value to f32 (u)
      mean side   dc_eps_mse: d^2 within 3 u, a lane's strided sum of ceil(N / 256) terms, 6 shuffle steps and 3 adds of wave partials
                  (N = C H W; all terms non-negative, so the relative bound is the number of additions on a path: ceil(N / 256) + 9),
                  sqrt then square (u, then 2 u + u), the posterior's sequential sum of n errors and its division (n + 1) u
    The same (rel, abs) bound the pixel sum of delta_map against the posterior's delta when rel multiplies mean[c] + the winner's mean
    over the trials of c, and abs is doubled."""
    N = C * H * W
    rel = ((C + 2) + 1 + 3 + (-(-N // 256) + 9) + 4 + (n + 1)) * U
    return rel, H * W * QUANT
