"""float64 oracle of the class posterior (include/dcamd.h `dc_class_posterior`), written image by image from the definitions and
independently of the package's own statement (diffusion_classifier_amd/posterior.py), which the tests check against this one.

`oracle(errors, t_end, temperature)` -> dict of float64 / int64 tensors; `synthetic_rows()` / `random_case()` build the inputs the CPU
and the GPU tests share; `check_against_oracle()` holds the tolerances, each derived from the fp32 operations involved."""
import math

import torch

INF, NAN = float("inf"), float("nan")
U = 2.0 ** -24          # fp32 unit roundoff


def _order(means, ids):
    """ids sorted by (mean, id) with NaN after every number; -0 == +0."""
    return sorted(ids, key=lambda c: (1, 0.0, c) if math.isnan(means[c]) else (0, means[c] + 0.0, c))


def oracle(errors, t_end, temperature=1.0):
    E_all = errors.detach().cpu().double()[:, :, :t_end]
    BS, C, _ = E_all.shape
    out = dict(probs=torch.zeros(BS, C, dtype=torch.float64), entropy=torch.zeros(BS, dtype=torch.float64),
               margin=torch.zeros(BS, dtype=torch.float64), margin_z=torch.zeros(BS, dtype=torch.float64),
               winner=torch.zeros(BS, dtype=torch.int64), runner=torch.zeros(BS, dtype=torch.int64),
               invalid=torch.zeros(BS, dtype=torch.int64), n=torch.zeros(BS, C, dtype=torch.int64),
               means=torch.zeros(BS, C, dtype=torch.float64), delta=torch.zeros(BS, C, dtype=torch.float64),
               S=torch.zeros(BS, C, dtype=torch.float64), Sw=torch.zeros(BS, C, dtype=torch.float64),
               stderr=torch.full((BS,), NAN, dtype=torch.float64))
    for b in range(BS):
        E = E_all[b]
        ev = ~(E == INF)                                     # [C, t_end]; NaN is evaluated
        n = ev.sum(1)
        Ez = torch.where(ev, E, torch.zeros_like(E))
        S = Ez.sum(1)
        means = torch.where(n > 0, S / n.clamp(min=1), torch.full_like(S, INF))
        finalists = [c for c in range(C) if int(n[c]) == t_end]
        ml = means.tolist()
        ranked = _order(ml, finalists)
        winner = ranked[0] if ranked else -1
        runner = ranked[1] if len(ranked) > 1 else -1
        out["n"][b], out["S"][b], out["means"][b] = n, S, means
        out["winner"][b], out["runner"][b] = winner, runner
        out["invalid"][b] = int((torch.isnan(E) & ev).sum())
        if winner < 0:
            for k in ("probs", "delta", "Sw"):
                out[k][b] = NAN
            for k in ("entropy", "margin", "margin_z"):
                out[k][b] = NAN
            continue
        Ew = E[winner]
        Sw = torch.where(ev, Ew[None, :].expand_as(E), torch.zeros_like(E)).sum(1)
        delta = (S - Sw) / n                                 # n = 0: 0 / 0 = NaN
        out["Sw"][b], out["delta"][b] = Sw, delta
        out["probs"][b] = softmax_of_delta(delta, n, temperature)
        out["entropy"][b] = entropy_of(out["probs"][b])
        if runner < 0:
            out["margin"][b] = out["margin_z"][b] = INF
        else:
            d = E[runner] - Ew
            margin = d.sum() / t_end
            var = ((d - margin) ** 2).sum() / torch.tensor(float(t_end - 1), dtype=torch.float64)      # t_end = 1: 0 / 0
            out["margin"][b] = margin
            out["stderr"][b] = torch.sqrt(var / t_end)
            out["margin_z"][b] = margin / out["stderr"][b]
        if math.isnan(ml[winner]):
            out["probs"][b] = NAN
            for k in ("entropy", "margin", "margin_z"):
                out[k][b] = NAN
    return out


def softmax_of_delta(delta, n, temperature):
    """float64 softmax(-delta / temperature) over the classes with n > 0 and a finite delta; exactly 0 elsewhere.  One image."""
    delta = delta.double()
    ok = (n > 0) & torch.isfinite(delta)
    p = torch.zeros_like(delta)
    if ok.any():
        a = -delta[ok] / temperature
        e = torch.exp(a - a.max())
        p[ok] = e / e.sum()
    return p


def entropy_of(p):
    p = p.double()
    nz = p[p > 0]
    return -(nz * torch.log(nz)).sum()


# ------------------------------------------------------------------------------------------------ inputs
def random_case(BS, C, T, t_end, seed, prune=True):
    """Errors as a multi-stage classify leaves them: every class scored on a prefix of the trials, at least two on all t_end; cells
    behind t_end hold NaN and 1e30 alternately (they must change nothing)."""
    g = torch.Generator().manual_seed(seed)
    E = 100.0 + 20.0 * torch.rand(BS, C, T, generator=g) + 3.0 * torch.randn(BS, C, 1, generator=g)
    if prune and t_end > 1 and C > 2:
        cut = torch.randint(1, t_end + 1, (BS, C), generator=g)
        keep = torch.stack([torch.randperm(C, generator=g)[:2] for _ in range(BS)])
        cut.scatter_(1, keep, t_end)
        E = torch.where(torch.arange(T)[None, None, :] < cut[:, :, None], E, torch.full_like(E, INF))
    tail = torch.where(torch.arange(T) % 2 == 0, torch.tensor(NAN), torch.tensor(1e30)).expand(BS, C, T)
    E = torch.where(torch.arange(T)[None, None, :] >= t_end, tail, E)
    return E.float().contiguous()


def synthetic_rows():
    """[7, 4, 3] with t_end = 3: one image per edge case of the issue."""
    rows = [
        # two identical finalists: the lower id wins, equal probs, margin 0
        [[5., 6., 7.], [5., 6., 7.], [9., 9., 9.], [8., INF, INF]],
        # a single finalist: no runner
        [[5., 6., INF], [4., 6., 7.], [9., INF, INF], [INF, INF, INF]],
        # no finalist
        [[5., INF, INF], [4., 6., INF], [INF, INF, INF], [INF, INF, INF]],
        # a NaN cell in a losing finalist
        [[5., 6., 7.], [5.5, NAN, 7.], [6., 6., 7.5], [INF, INF, INF]],
        # delta = 1e4
        [[5., 6., 7.], [10005., 10006., 10007.], [5.25, 6.5, 7.], [5.5, INF, INF]],
        # a negative delta on a non-finalist (a foreign tensor: classify never writes this)
        [[5., 6., 7.], [6., 6., 7.], [3., INF, INF], [5., 5., INF]],
        # every finalist NaN
        [[NAN, 6., 7.], [5., NAN, 7.], [6., INF, INF], [INF, INF, INF]],
    ]
    return torch.tensor(rows, dtype=torch.float32)


SYNTH_T_END = 3


# ------------------------------------------------------------------------------------------------ comparison
def same_class(got, want):
    """Non-finite values agree by class (NaN / +inf / -inf); returns the mask of entries finite in `want`."""
    got, want = got.double().cpu(), want.double().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (got, want)
    assert torch.equal(got == INF, want == INF), (got, want)
    assert torch.equal(got == -INF, want == -INF), (got, want)
    return torch.isfinite(want)


def check_against_oracle(E, t_end, tau, post, winner, means, delta, label="", exact_fp32_sums=True):
    """`post` (ClassPosterior), winner, means, delta of an fp32 implementation against the float64 oracle.  Returns the measured maxima.
    Tolerances:
      delta     2 t_end u max(|S|, |Sw|) / n per entry: two sequential fp32 sums of <= t_end terms (each within t_end u sum|x|, and the
                errors are of one sign in every test, so sum|x| = |S|), one subtraction, one division
      probs     against the float64 softmax of the implementation's OWN fp32 delta: rtol 1e-4, atol 1e-7 (argument rounding near -88 is
                about 1e-5 relative, exp a few ulp, a sum of at most 1024 terms)
      entropy   against float64 on the implementation's own probs: atol 1e-5
      margin    rtol 8 t_end u  plus the sum bound 2 t_end u max(|S_runner|, |S_winner|) / t_end
      margin_z  the same relative bound on margin, carried through the division: bound(margin) / standard error, plus rtol 8 t_end u"""
    o = oracle(E, t_end, tau)
    BS, C, _ = E.shape
    w = torch.as_tensor(winner).cpu().long().view(-1)
    assert torch.equal(w, o["winner"]), (label, w, o["winner"])
    assert torch.equal(post.runner_up.cpu().long(), o["runner"]), (label, post.runner_up, o["runner"])
    assert post.runner_up.dtype == torch.int64
    assert torch.equal(post.n_trials.cpu().long(), o["n"]), label
    assert torch.equal(post.invalid.cpu().long(), o["invalid"]), (label, post.invalid, o["invalid"])
    measured = {}

    fin = same_class(means, o["means"])
    measured["means_rel"] = float(((means.double().cpu() - o["means"])[fin].abs() / o["means"][fin].abs().clamp(min=1e-300)).max()) if fin.any() else 0.0
    assert measured["means_rel"] <= 2 * t_end * U, (label, measured)

    fin = same_class(delta, o["delta"])
    bound = 2 * t_end * U * torch.maximum(o["S"].abs(), o["Sw"].abs()) / o["n"].clamp(min=1)
    err = (delta.double().cpu() - o["delta"]).abs()
    measured["delta_over_bound"] = float((err[fin] / bound[fin].clamp(min=1e-300)).max()) if fin.any() else 0.0
    assert (err[fin] <= bound[fin]).all(), (label, measured)

    probs = post.probs.double().cpu()
    good = ~torch.isnan(o["probs"][:, 0])
    assert torch.equal(torch.isnan(probs), torch.isnan(o["probs"])), label
    pe, ee, se = 0.0, 0.0, 0.0
    for b in range(BS):
        if not good[b]:
            assert math.isnan(float(post.entropy[b])), label
            continue
        want = softmax_of_delta(delta[b].cpu(), o["n"][b], tau)
        assert bool((probs[b][(o["n"][b] == 0) | ~torch.isfinite(o["delta"][b])] == 0).all()), (label, b)       # exactly 0
        tol = 1e-7 + 1e-4 * want.abs()
        d = (probs[b] - want).abs()
        pe = max(pe, float((d / tol).max()))
        assert bool((d <= tol).all()), (label, b, probs[b], want)
        se = max(se, abs(float(probs[b].sum()) - 1.0))
        ee = max(ee, abs(float(post.entropy[b]) - float(entropy_of(probs[b]))))
        assert int(probs[b].argmax()) == int(w[b]) or float(delta[b][torch.isfinite(delta[b])].min()) < 0, (label, b)
    measured.update(probs_over_tol=pe, entropy_abs=ee, sum_probs_abs=se)
    assert se <= 1e-5 and ee <= 1e-5, (label, measured)

    fin = same_class(post.margin, o["margin"]) & same_class(post.margin_z, o["margin_z"])
    rows = torch.arange(BS)
    Sr, Sw_ = o["S"][rows, o["runner"].clamp(min=0)], o["S"][rows, o["winner"].clamp(min=0)]
    mb = 8 * t_end * U * o["margin"].abs() + 2 * t_end * U * torch.maximum(Sr.abs(), Sw_.abs()) / t_end
    me = (post.margin.double().cpu() - o["margin"]).abs()
    measured["margin_over_bound"] = float((me[fin] / mb[fin].clamp(min=1e-300)).max()) if fin.any() else 0.0
    assert (me[fin] <= mb[fin]).all(), (label, measured, post.margin, o["margin"])
    # margin_z = margin / se: the margin's bound divided by the standard error, the same bound on the deviations inside se (relative
    # to se: d_j - margin carries the margin's error, so se moves by at most mb), plus the rounding of the handful of operations
    se_ = o["stderr"]
    zb = 8 * t_end * U * o["margin_z"].abs() + mb / se_ + o["margin_z"].abs() * mb / se_
    ze = (post.margin_z.double().cpu() - o["margin_z"]).abs()
    measured["margin_z_over_bound"] = float((ze[fin] / zb[fin].clamp(min=1e-300)).max()) if fin.any() else 0.0
    assert (ze[fin] <= zb[fin]).all(), (label, measured, post.margin_z, o["margin_z"])
    return measured
