"""CPU: the class posterior's C-ABI surface and refusals, the package's torch statement against the float64 oracle, the foreign-backbone
classify(return_posterior=True), evaluate's routing of the posterior, and the histogram metrics (AUROC, SelectiveAccuracy)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import posterior as P
from diffusion_classifier_amd.utils.metrics import AUROC, Accuracy, SelectiveAccuracy
from helpers import load_case, standin_from
import posterior_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = ["2stage_pruned", "fast", "1stage_eps"]


# ------------------------------------------------------------------------------------------------ C-ABI
def test_struct_fields_match_the_header_and_the_abi_version_stays():
    src = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    ptr, sz = ctypes.sizeof(ctypes.c_void_p), ctypes.sizeof(L.ClassPosteriorParams)
    assert sz == 11 * ptr + 6 * 4
    assert "dc_class_posterior" in L.EXPORTS
    lib = L.lib()
    assert lib.dc_class_posterior is not None
    assert lib.dc_abi_version() == 5 and L.ABI_VERSION == 5
    assert re.search(r"#define DC_ABI_VERSION 5\b", src)


def _params(**over):
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    kw = dict(errors=a, probs=a, entropy=a, margin=a, margin_z=a, winner=a, runner=a, invalid=a, means=None, delta=None, n_eval=None,
              BS=1, C=2, T=2, t_end=2, temperature=1.0, pad_=0)
    kw.update(over)
    return L.ClassPosteriorParams(**kw), buf


@pytest.mark.parametrize("over,code,word", [
    (dict(errors=None), -1, "null"), (dict(probs=None), -1, "null"), (dict(entropy=None), -1, "null"),
    (dict(margin_z=None), -1, "null"), (dict(winner=None), -1, "null"), (dict(invalid=None), -1, "null"),
    (dict(C=1025), -2, "C=1025"), (dict(T=2, t_end=3), -2, "t_end=3"), (dict(BS=0), -2, "BS=0"),
    (dict(temperature=0.0), -1, "temperature"), (dict(temperature=-1.0), -1, "temperature"),
    (dict(temperature=float("nan")), -1, "temperature"),
])
def test_refusals_before_any_launch(over, code, word):
    """Argument and shape checks run before the launch: they answer without a GPU and touch no memory."""
    lib = L.lib()
    p, _keep = _params(**over)
    assert lib.dc_class_posterior(ctypes.byref(p), None) == code
    assert word in lib.dc_last_error().decode()


def test_null_params_is_refused():
    lib = L.lib()
    assert lib.dc_class_posterior(None, None) == -1


# ------------------------------------------------------------------------------------------------ the torch statement
def _torch_vs_oracle(E, t_end, tau, label):
    post, winner, means, delta = P.class_posterior_torch(E, t_end, tau, return_parts=True)
    assert post.probs.dtype == torch.float32 and post.runner_up.dtype == torch.int64
    return O.check_against_oracle(E, t_end, tau, post, winner, means, delta, label=label), post, winner


@pytest.mark.parametrize("name", GOLDENS)
def test_torch_statement_on_the_reference_written_errors(name):
    g, cfg = load_case(name)
    E = torch.from_numpy(g["errors"])
    t_end = E.shape[2]
    _, post, winner = _torch_vs_oracle(E, t_end, 1.0, name)
    out = torch.from_numpy(g["out"]).long()
    assert torch.equal(winner, out)
    assert torch.equal(post.probs.argmax(dim=1), out)
    o = O.oracle(E, t_end, 1.0)
    assert float(o["delta"][torch.isfinite(o["delta"])].min()) == 0.0          # a pruned class lost on exactly its prefix


@pytest.mark.parametrize("shape", [(3, 2, 1, 1), (2, 65, 7, 5), (2, 130, 3, 3), (1, 1024, 2, 2)])
@pytest.mark.parametrize("tau", [1.0, 0.5, 20.0])
def test_torch_statement_on_random_pruned_errors(shape, tau):
    BS, C, T, t_end = shape
    E = O.random_case(BS, C, T, t_end, seed=11)
    _, post, _ = _torch_vs_oracle(E, t_end, tau, str(shape))
    if t_end == 1:
        assert torch.isnan(post.margin_z).all() and torch.isfinite(post.margin).all()
    # cells behind t_end change nothing
    E2 = E.clone()
    E2[:, :, t_end:] = 7.0
    post2 = P.class_posterior_torch(E2, t_end, tau)
    for a, b in zip(post, post2):
        assert torch.equal(a.view(-1).view(torch.int32) if a.dtype == torch.float32 else a, b.view(-1).view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("tau", [1.0, 0.5, 20.0])
def test_torch_statement_on_the_synthetic_rows(tau):
    E = O.synthetic_rows()
    _, post, winner = _torch_vs_oracle(E, O.SYNTH_T_END, tau, "synthetic")
    inf = float("inf")
    # two identical finalists
    assert winner[0] == 0 and post.runner_up[0] == 1 and post.probs[0, 0] == post.probs[0, 1] and post.margin[0] == 0
    assert math.isnan(float(post.margin_z[0]))                                   # 0 / 0
    # a single finalist
    assert winner[1] == 1 and post.runner_up[1] == -1 and post.margin[1] == inf and post.margin_z[1] == inf
    # no finalist
    assert winner[2] == -1 and post.runner_up[2] == -1
    assert torch.isnan(post.probs[2]).all() and all(math.isnan(float(v[2])) for v in (post.entropy, post.margin, post.margin_z))
    # a NaN cell in a losing finalist: p = 0 for it, counted, the others as if it had not been scored
    assert winner[3] == 0 and post.probs[3, 1] == 0 and post.invalid[3] == 1 and post.invalid[0] == 0
    E3 = E[3:4].clone()
    E3[0, 1] = inf
    ref = P.class_posterior_torch(E3, O.SYNTH_T_END, tau)
    assert torch.equal(ref.probs[0], post.probs[3]) and ref.margin[0] == post.margin[3] and ref.runner_up[0] == post.runner_up[3] == 2
    # delta = 1e4 underflows to exactly 0 at tau = 1 and leaves the entropy finite
    if tau == 1.0:
        assert post.probs[4, 1] == 0
    assert torch.isfinite(post.entropy[4]) and post.entropy[4] > 0
    # a negative delta on a non-finalist: the softmax still sums to one, the winner is still the best finalist
    assert winner[5] == 0 and post.probs[5].argmax() == 2 and abs(float(post.probs[5].sum()) - 1) < 1e-6
    # every finalist NaN: the lowest id is the winner, the scores are NaN and the cells are counted
    assert winner[6] == 0 and torch.isnan(post.probs[6]).all() and post.invalid[6] == 2


def test_temperature_comes_from_the_config():
    assert P.temperature_of(dca.Config()) == 1.0
    assert P.temperature_of(dca.Config(posterior_temperature=20)) == 20.0
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            P.temperature_of(dca.Config(posterior_temperature=bad))
    assert dca.ClassPosterior is P.ClassPosterior
    assert dca.ClassPosterior._fields == ("probs", "entropy", "runner_up", "margin", "margin_z", "n_trials", "invalid")


# ------------------------------------------------------------------------------------------------ classify / evaluate
def _foreign(name, **extra):
    g, cfg = load_case(name)
    dc = dca.DiffusionClassifier(standin_from(g, cfg), dca.Config(**dict(cfg, **extra)))
    if dc.encoder is not None:
        dc.encoder.weight.data.copy_(torch.from_numpy(g["encoder.weight"]))
    fast = bool(g["fast"])
    kw = dict(fast=fast, t=torch.from_numpy(g["t"]), eps=torch.from_numpy(g["eps"]),
              fast_select=torch.from_numpy(g["fast_select"]) if fast else None)
    return g, dc, torch.from_numpy(g["x"]), (torch.from_numpy(g["labels"]) if fast else None), kw


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("tau", [None, 20.0])
def test_foreign_classify_returns_the_posterior(name, tau):
    g, dc, x, lab, kw = _foreign(name, **({} if tau is None else {"posterior_temperature": tau}))
    out, err, post = dc.classify(x, lab, return_errors=True, return_posterior=True, **kw)
    out2, post2 = dc.classify(x, lab, return_posterior=True, **kw)
    assert isinstance(post, dca.ClassPosterior) and isinstance(post2, dca.ClassPosterior)
    np.testing.assert_array_equal(out.numpy(), g["out"])
    np.testing.assert_array_equal(out2.numpy(), g["out"])
    np.testing.assert_array_equal(err.numpy(), g["errors"])
    assert torch.equal(post.probs.argmax(dim=1), out)
    T = err.shape[2]
    _, winner, means, delta = P.class_posterior_torch(err, T, tau or 1.0, return_parts=True)
    O.check_against_oracle(err, T, tau or 1.0, post, out, means, delta, label=name)
    for a, b in zip(post, post2):
        assert torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0))
    assert torch.equal(dc.classify(x, lab, **kw), out)                          # the flag off: the plain return


def test_a_bad_temperature_is_refused_only_when_the_posterior_is_asked_for():
    g, dc, x, lab, kw = _foreign("1stage_eps", posterior_temperature=0.0)
    dc.classify(x, lab, **kw)
    with pytest.raises(ValueError):
        dc.classify(x, lab, return_posterior=True, **kw)


class _Spy(Accuracy):
    def __init__(self, name, wants):
        super().__init__(name)
        self.wants_posterior = wants
        self.seen = []

    def update(self, output):
        self.seen.append(output)
        super().update(output[:2])


def test_evaluate_hands_the_posterior_only_to_the_metrics_that_want_it():
    g, dc, x, lab, kw = _foreign("1stage_eps")
    loader = [{"images": x, "prompt": torch.from_numpy(g["out"]).long()}]
    plain, wants = _Spy("plain", False), _Spy("wants", True)
    torch.manual_seed(int(g["seed"]))
    dc.evaluate(loader, metrics=[plain, wants], classification=True)
    assert len(plain.seen) == len(wants.seen) == 1
    assert len(plain.seen[0]) == 2 and len(wants.seen[0]) == 3
    assert isinstance(wants.seen[0][2], dca.ClassPosterior)
    assert torch.equal(plain.seen[0][0], wants.seen[0][0])
    np.testing.assert_array_equal(plain.seen[0][0].numpy(), g["out"])
    # no metric wants it: today's call, today's tuple
    only = _Spy("plain", False)
    torch.manual_seed(int(g["seed"]))
    dc.evaluate(loader, metrics=[only], classification=True)
    assert len(only.seen[0]) == 2
    # the real metrics run through evaluate
    au, sel = AUROC("auroc"), SelectiveAccuracy("sel", 0.5)
    assert au.wants_posterior and sel.wants_posterior and not getattr(Accuracy("a"), "wants_posterior", False)
    torch.manual_seed(int(g["seed"]))
    dc.evaluate(loader, metrics=[au, sel], classification=True)
    assert int(au.hist.sum()) == int((loader[0]["prompt"] <= 1).sum()) and int(sel.total.sum()) == x.shape[0]


# ------------------------------------------------------------------------------------------------ metrics
def _post(probs1=None, conf=None, by="margin_z"):
    n = len(probs1 if probs1 is not None else conf)
    z = torch.zeros(n)
    probs = torch.stack([1 - probs1, probs1], dim=1) if probs1 is not None else torch.full((n, 2), 0.5)
    f = dict(probs=probs, entropy=z, runner_up=z.long(), margin=z, margin_z=z, n_trials=z.int(), invalid=z.int())
    if conf is not None:
        f[by] = conf
    return dca.ClassPosterior(**f)


def _rank_auroc(score, y):
    pos, neg = score[y == 1].double(), score[y == 0].double()
    gt = (pos[:, None] > neg[None, :]).sum().item()
    eq = (pos[:, None] == neg[None, :]).sum().item()
    return (gt + 0.5 * eq) / (len(pos) * len(neg))


def _fixed_scores(n=200, bins=1024):
    g = torch.Generator().manual_seed(3)
    y = (torch.rand(n, generator=g) < 0.4).long()
    raw = (torch.randn(n, generator=g) * 0.2 + 0.4 + 0.2 * y).clamp(0, 1)
    centre = (torch.floor(raw * bins).clamp(max=bins - 1) + 0.5) / bins
    return y, raw, centre


def test_auroc_equals_the_rank_statistic_on_bin_centres_and_counters_add():
    y, _, centre = _fixed_scores()
    assert len(torch.unique(centre)) < len(centre)                                 # there are ties: the half rule is exercised
    m = AUROC("auroc", bins=1024)
    m.update((y, {"prompt": y}, _post(probs1=centre)))
    assert m.hist.dtype == torch.int64 and tuple(m.hist.shape) == (2, 1024)
    assert m.compute()["auroc"] == _rank_auroc(centre, y)
    # two instances, half of the images each: the summed counters (the all-reduce) give the same number
    a, b = AUROC("auroc"), AUROC("auroc")
    a.update((y[:90], {"prompt": y[:90]}, _post(probs1=centre[:90])))
    b.update((y[90:], {"prompt": y[90:]}, _post(probs1=centre[90:])))
    assert not torch.equal(a.hist, m.hist)
    a.hist = a.hist + b.hist
    assert torch.equal(a.hist, m.hist) and a.compute() == m.compute()
    m.reset()
    assert int(m.hist.sum()) == 0 and math.isnan(m.compute()["auroc"])


def test_auroc_on_raw_scores_lies_within_what_one_bin_of_ties_allows():
    y, raw, _ = _fixed_scores()
    for bins in (1024, 16):
        m = AUROC("auroc", bins=bins)
        m.update((y, {"prompt": y}, _post(probs1=raw)))
        neg, pos = m.hist[0].double(), m.hist[1].double()
        # a (positive, negative) pair in one bin counts 1/2 where the exact statistic counts 0, 1/2 or 1; every other pair counts the same
        bound = float((pos * neg).sum() / (2 * pos.sum() * neg.sum()))
        assert abs(m.compute()["auroc"] - _rank_auroc(raw, y)) <= bound + 1e-15
    assert bound > 0


def test_auroc_edge_scores():
    y = torch.tensor([1, 0, 1, 0])
    m = AUROC("auroc", bins=8)
    m.update((y, {"prompt": y}, _post(probs1=torch.tensor([1.0, 0.0, float("nan"), 0.99]))))
    assert m.hist[1, 7] == 1 and m.hist[0, 0] == 1 and m.hist[1, 0] == 1 and m.hist[0, 7] == 1


def _sorted_selective(conf, correct, coverage):
    k = max(1, math.ceil(coverage * len(conf) - 1e-9))
    key = torch.nan_to_num(conf.double(), nan=-float("inf"), posinf=float("inf"))
    key = torch.where(torch.isnan(conf), torch.full_like(key, -float("inf")), key)
    order = torch.argsort(key, descending=True, stable=True)
    return correct[order[:k]].double().mean().item()


@pytest.mark.parametrize("by", ["margin_z", "margin", "entropy"])
@pytest.mark.parametrize("coverage", [0.1, 0.5, 0.8, 1.0])
def test_selective_accuracy_equals_a_sort_on_bin_centre_confidences(by, coverage):
    """One image per bin (distinct bin-centre confidences), so the sort has no ties to break; -inf, negative values, +inf and NaN
    included.  The NaN image sorts last; the two +inf images first (both correct: their order does not matter)."""
    sel = SelectiveAccuracy("sel", coverage, by=by)
    n = 200
    g = torch.Generator().manual_seed(5)
    bins = torch.randperm((1 << sel.bits) - 300, generator=g)[:n] + 150            # distinct bins, away from the non-finite keys
    shift = 32 - sel.bits
    key = (bins.long() << shift) + (1 << (shift - 1))                              # the centre of each bin, as an order key
    u = torch.where(key >= 0x80000000, key - 0x80000000, 0xFFFFFFFF - key)
    conf = (u - (u >= 0x80000000).long() * (1 << 32)).to(torch.int32).view(torch.float32).clone()
    assert torch.isfinite(conf).all() and (conf < 0).any() and (conf > 0).any()
    assert torch.equal(sel.bin_of(conf), bins + 1)
    conf[:2] = float("inf")
    conf[2] = float("nan")
    conf[3] = -float("inf")
    y = torch.randint(0, 2, (n,), generator=g)
    pred = torch.where(torch.rand(n, generator=g) < 0.6 + 0.3 * (conf > 0), y, 1 - y)
    pred[:2] = y[:2]
    fed = -conf if by == "entropy" else conf
    half = n // 2
    a, b = SelectiveAccuracy("sel", coverage, by=by), SelectiveAccuracy("sel", coverage, by=by)
    a.update((pred[:half], {"prompt": y[:half]}, _post(conf=fed[:half], by=by)))
    b.update((pred[half:], {"prompt": y[half:]}, _post(conf=fed[half:], by=by)))
    sel.update((pred, {"prompt": y}, _post(conf=fed, by=by)))
    assert sel.total.dtype == torch.int64 and int(sel.total.sum()) == n
    assert sel.total[-1] == 2 and sel.total[0] == 1                                # +inf above, NaN below everything
    a.total, a.correct = a.total + b.total, a.correct + b.correct                  # the all-reduce
    assert torch.equal(a.total, sel.total) and torch.equal(a.correct, sel.correct)
    want = _sorted_selective(conf, pred == y, coverage)
    assert abs(sel.compute()["sel"] - want) < 1e-12 and a.compute() == sel.compute()


def test_selective_accuracy_shares_a_bin_the_cut_falls_into():
    sel = SelectiveAccuracy("sel", 0.5, by="max_prob")
    y = torch.tensor([1, 1, 0, 0])
    pred = torch.tensor([1, 0, 0, 0])
    post = _post(probs1=torch.tensor([0.9, 0.9, 0.1, 0.1]))                        # max_prob 0.9 everywhere: one bin, 3 of 4 correct
    sel.update((pred, {"prompt": y}, post))
    assert abs(sel.compute()["sel"] - 0.75) < 1e-12
