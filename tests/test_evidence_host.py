"""CPU: classify(return_evidence=True) on the stand-in backbone (the `_ForeignRunner` path, evidence.py's torch statements) against
the float64 oracle (tests/evidence_oracle.py, which holds the tolerances and their derivation), the shape of the return value, what
the flag must leave alone, the refusals, and grid sharding over gloo."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import evidence as EV
from diffusion_classifier_amd import posterior as P
from helpers import load_case, standin_from
import early_stop_oracle as SO
import evidence_oracle as O
import evidence_workers as WK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(v):
    v = v.cpu().contiguous()
    return v.view(torch.int32) if v.dtype == torch.float32 else v


def _golden_dc(name, **extra):
    g, cfg = load_case(name)
    dc = dca.DiffusionClassifier(standin_from(g, cfg), dca.Config(**dict(cfg, **extra)))
    if dc.encoder is not None:
        dc.encoder.weight.data.copy_(torch.from_numpy(g["encoder.weight"]))
    fast = bool(g["fast"])
    kw = dict(fast=fast, t=torch.from_numpy(g["t"]), eps=torch.from_numpy(g["eps"]),
              fast_select=torch.from_numpy(g["fast_select"]) if fast else None)
    return dc, torch.from_numpy(g["x"]), (torch.from_numpy(g["labels"]) if fast else None), kw


def _record(dc):
    """Every backbone call of the next classify: (z, lambda, conditioning, prediction) as the scoring loop saw them."""
    calls = []
    h = dc.ema.ema_model.register_forward_hook(
        lambda mod, args, kwargs, out: calls.append((kwargs["x"].clone(), kwargs["noise_labels"].clone(),
                                                     kwargs["encoder_hidden_states"].clone(), out.clone())), with_kwargs=True)
    return calls, h


def _oracle_of_calls(dc, calls, x, t, eps, n_eval, winner):
    """The oracle's maps from the recorded predictions.  Every row of a call is one (image, class, trial) unit: the trial and the image
    from the row's lambda (the injected t are all different), the class from its conditioning."""
    cfg = dc.config
    T, BS = t.shape
    lam = torch.stack([dc.schedule(t[j].clone()) for j in range(T)])
    alpha = torch.stack([torch.sqrt(torch.sigmoid(lam[j].clone())) for j in range(T)])
    sigma = torch.stack([torch.sqrt(torch.sigmoid(-lam[j].clone())) for j in range(T)])
    assert len(set(lam.reshape(-1).tolist())) == T * BS
    where = {float(lam[j, b]): (j, b) for j in range(T) for b in range(BS)}
    pred, bj, cell, trial = [], [], [], []
    for z, lm, emb, out in calls:
        for r in range(z.shape[0]):
            j, b = where[float(lm[r])]
            if dc.encoder is None:
                c = int(emb[r])
            else:
                hit = (dc.encoder.weight == emb[r, 0]).all(dim=1).nonzero().view(-1)
                assert hit.numel() == 1
                c = int(hit)
            pred.append(out[r].numpy()); bj.append(j * BS + b); cell.append(b * cfg.classes + c); trial.append(j)
    v, bound = O.unit_maps(np.stack(pred), eps.reshape(T * BS, *eps.shape[2:]).numpy(), x.numpy(), alpha.reshape(-1).numpy(),
                           sigma.reshape(-1).numpy(), np.array(bj), np.tile(np.arange(BS), T), dc.pred_param == "v")
    assert np.isfinite(v).all() and v.max() < O.VMAX / 4
    return O.maps(v, bound, np.array(cell), np.array(trial), cfg.evaluation_per_stage, BS, cfg.classes, n_eval.numpy(), winner.numpy())


@pytest.mark.parametrize("name", ["1stage_eps", "2stage_pruned", "fast", "v_shifted", "dit_labels"])
def test_maps_on_the_standin_match_the_oracle_and_the_flag_changes_nothing_else(name):
    dc, x, lab, kw = _golden_dc(name)
    out0, err0, post0 = dc.classify(x, lab, return_errors=True, return_posterior=True, **kw)
    calls, hook = _record(dc)
    out, err, post, ev = dc.classify(x, lab, return_errors=True, return_posterior=True, return_evidence=True, **kw)
    hook.remove()
    assert isinstance(ev, dca.ClassEvidence) and isinstance(post, dca.ClassPosterior)
    assert torch.equal(out, out0) and torch.equal(_bits(err), _bits(err0))
    for a, b in zip(post, post0):
        assert torch.equal(_bits(a), _bits(b))
    BS, C = x.shape[0], dc.config.classes
    assert tuple(ev.mean_map.shape) == tuple(ev.delta_map.shape) == (BS, C, 8, 8) and ev.mean_map.dtype == torch.float32
    assert torch.equal(ev.n_trials, post.n_trials) and ev.n_trials.dtype == torch.int32
    assert ev.invalid.dtype == torch.int32 and ev.invalid.tolist() == [0] * BS
    _, winner, _, _ = P.class_posterior_torch(err, err.shape[2], return_parts=True)
    assert torch.equal(winner, out)
    o = _oracle_of_calls(dc, calls, x, kw["t"], kw["eps"], post.n_trials, winner)
    m = O.check(ev, o, label=name)
    print(f"evidence host {name}: " + " ".join(f"{k}={v:.3g}" for k, v in m.items()))
    rows = torch.arange(BS)
    assert (ev.delta_map[rows, out] == 0).all()                                       # exactly 0, every pixel
    never = post.n_trials == 0
    assert torch.isnan(ev.mean_map[never]).all() and torch.isnan(ev.delta_map[never]).all()
    assert torch.isfinite(ev.mean_map[~never]).all() and torch.isfinite(ev.delta_map[~never]).all()
    if name == "fast":
        assert int(never.sum()) == BS * (C - dc.config.n_fast_classes)                # the classes fast mode never scored
    if name == "2stage_pruned":
        assert sorted(set(post.n_trials.reshape(-1).tolist())) == [4, 10]
    # two calls: the same bits
    ev2 = dc.classify(x, lab, return_evidence=True, **kw)[1]
    for a, b in zip(ev, ev2):
        assert torch.equal(_bits(a), _bits(b))


def test_return_value_order_for_every_flag_combination():
    dc, x, lab, kw = _golden_dc("1stage_eps")
    kinds = dict(return_errors=torch.Tensor, return_posterior=dca.ClassPosterior, return_evidence=dca.ClassEvidence, return_trials=torch.Tensor)
    names = list(kinds)
    for mask in range(16):
        flags = {n: bool(mask >> i & 1) for i, n in enumerate(names)}
        res = dc.classify(x, lab, **flags, **kw)
        if mask == 0:
            assert torch.is_tensor(res) and res.dtype == torch.int64
            continue
        assert isinstance(res, tuple) and len(res) == 1 + sum(flags.values())
        assert res[0].dtype == torch.int64
        want = [kinds[n] for n in names if flags[n]]
        for v, k in zip(res[1:], want):
            assert isinstance(v, k), (flags, type(v), k)
        if flags["return_errors"]:
            assert res[1].dim() == 3
        if flags["return_trials"]:
            assert res[-1].dtype == torch.int32 and res[-1].dim() == 1


def test_pruned_and_stopped_classes_are_paired_over_their_own_prefix():
    """Two stages [3, 7] keeping [2, 1] with per-image stopping: an image that stops at 3 has every class at n = 3, one that runs on
    has its pruned class at n = 3 and the finalists at 7 — the pruned class's delta map is its stage-0 plane minus the WINNER's stage-0
    plane only, whatever the winner collected afterwards."""
    over = dict(n_stages=2, evaluation_per_stage=[3, 7], n_keep_per_stage=[2, 1])
    dc, x, t, eps = SO.standin_classifier(dca, **over)
    _, err0 = dc.classify(x, t=t, eps=eps, return_errors=True)
    z = P.class_posterior_torch(err0, 3).margin_z
    thr = float(z.median())
    dc.config.stop_margin_z = thr
    lab0, err0, post0, td0 = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, return_trials=True)
    calls, hook = _record(dc)
    lab, err, post, ev, t_done = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, return_evidence=True, return_trials=True)
    hook.remove()
    assert (t_done == 3).any() and (t_done == 7).any(), t_done
    assert torch.equal(lab, lab0) and torch.equal(_bits(err), _bits(err0)) and torch.equal(t_done, td0)
    for a, b in zip(post, post0):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(ev.n_trials, post.n_trials)
    _, winner, _, _ = P.class_posterior_torch(err, t_done, return_parts=True, t_values=[3, 7])
    assert torch.equal(winner, lab)
    o = _oracle_of_calls(dc, calls, x, t, eps, post.n_trials, winner)
    m = O.check(ev, o, label="stop")
    print("evidence host stop: " + " ".join(f"{k}={v:.3g}" for k, v in m.items()))
    assert (ev.delta_map[torch.arange(5), lab] == 0).all()
    # by hand, for one image that ran to T: the pruned class against per-trial maps of the recorded predictions
    b = int((t_done == 7).nonzero()[0])
    n = post.n_trials[b]
    pruned = int((n == 3).nonzero()[0])
    w = int(lab[b])
    lam = torch.stack([dc.schedule(t[j].clone()) for j in range(7)])
    per_trial = {}
    for zt, lm, emb, out in calls:
        for r in range(zt.shape[0]):
            hit = (lam == lm[r]).nonzero()[0]
            j, bb = int(hit[0]), int(hit[1])
            c = int((dc.encoder.weight == emb[r, 0]).all(dim=1).nonzero()[0])
            if bb == b:
                per_trial[(c, j)] = ((out[r].double() - eps[j, b].double()) ** 2).sum(0)
    assert sorted(j for (c, j) in per_trial if c == pruned) == [0, 1, 2]
    want = sum(per_trial[(pruned, j)] - per_trial[(w, j)] for j in range(3)) / 3
    full = sum(per_trial[(pruned, j)] for j in range(3)) / 3 - sum(per_trial[(w, j)] for j in range(7)) / 7
    got = ev.delta_map[b, pruned].double()
    tol = o["delta_bound"][b, pruned]
    assert (np.abs((got - want).numpy()) <= tol).all()
    assert float((want - full).abs().max()) > 100 * float(tol.max())          # the two readings differ by far more than the tolerance


def test_refusals():
    dc, x, lab, kw = _golden_dc("1stage_eps", simulate_rank=(0, 2))
    dc.ema.ema_model.register_forward_hook(lambda *a: pytest.fail("the backbone ran"))
    with pytest.raises(ValueError, match="simulate_rank"):
        dc.classify(x, lab, return_evidence=True, **kw)
    T = (1 << 18) + 1
    dc2, x, lab, kw = _golden_dc("1stage_eps", evaluation_per_stage=[T])
    dc2.ema.ema_model.register_forward_hook(lambda *a: pytest.fail("the backbone ran"))
    with pytest.raises(ValueError, match="2\\^18"):
        dc2.classify(x[:1], return_evidence=True)
    EV.check_trials(1 << 18)
    assert EV.F == 30 and EV.VMAX == 2.0 ** 14


def test_header_and_python_agree_on_the_fixed_point_format():
    import re
    hdr = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    assert int(re.search(r"#define DC_EVIDENCE_FRAC_BITS (\d+)", hdr).group(1)) == EV.F == O.F
    assert float(re.search(r"#define DC_EVIDENCE_VMAX ([0-9.]+)f", hdr).group(1)) == EV.VMAX == O.VMAX
    assert dca._lib.OP_ERR_MAP == int(re.search(r"DC_OP_ERR_MAP = (\d+)", hdr).group(1)) == 19


def test_new_ctypes_structs_match_the_header_field_for_field():
    for cls, pointers in ((dca._lib.ErrMapParams, ["pred", "eps", "x", "alpha", "sigma", "bj_of_unit", "img_of_bj", "out_index", "acc", "bad"]),
                          (dca._lib.EvidenceMapsParams, ["acc", "bad", "stage_ends", "n_eval", "winner", "mean_map", "delta_map", "invalid"])):
        assert [n for n, t in cls._fields_ if t is dca._lib.vp] == pointers, cls
    assert "dc_err_map" in dca._lib.EXPORTS and "dc_evidence_maps" in dca._lib.EXPORTS


def test_bad_values_are_left_out_counted_and_poison_their_cell_only():
    """The torch statements on hand-made accumulators: a NaN and a value above VMAX in two cells."""
    BS, C, H, W = 2, 3, 2, 2
    acc, bad = EV.new_slabs(2, BS * C, H * W, "cpu")
    e = torch.zeros(BS * C, 1, H, W)
    pred = torch.ones(BS * C, 1, H, W)
    pred[1, 0, 0, 1] = float("nan")
    pred[5, 0, 1, 0] = 200.0                                    # 4e4 > VMAX
    EV.err_map_torch(pred, e, torch.arange(BS * C), acc[0], bad[0])
    EV.err_map_torch(torch.full((1, 1, H, W), 2.0), e[:1], torch.tensor([BS * C]), acc[1], bad[1])        # a padded slot: the dump plane
    n_eval = torch.full((BS, C), 2, dtype=torch.int32)
    ev = EV.evidence_maps_torch(acc, bad, [2, 4], n_eval, torch.tensor([0, 0]), H, W)
    nan_cells = torch.isnan(ev.mean_map).all(dim=(2, 3))
    assert nan_cells.tolist() == [[False, True, False], [False, False, True]]
    assert torch.equal(torch.isnan(ev.mean_map), torch.isnan(ev.delta_map))
    assert ev.invalid.tolist() == [1, 1] and int(acc[1, :BS * C].abs().sum()) == 0 and int(acc[1, BS * C, 0]) == 4 << 30
    assert (ev.mean_map[0, 0] == 0.5).all() and (ev.delta_map[0, 2] == 0).all()
    # an n that is no stage end, a class never scored, an image without a winner
    n_eval[0, 2], n_eval[1, 0] = 3, 0
    ev = EV.evidence_maps_torch(acc, bad, [2, 4], n_eval, torch.tensor([0, -1]), H, W)
    assert torch.isnan(ev.mean_map[0, 2]).all() and torch.isnan(ev.mean_map[1]).all() and torch.isfinite(ev.mean_map[0, 0]).all()


# ------------------------------------------------------------------------------------------------ grid sharding (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_maps_are_bit_identical_to_the_single_process(world):
    one = WK.standin_run(shard=False)
    assert np.isfinite(one["mean_map"]).any() and (one["n_trials"] > 0).all()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=WK.gloo_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == list(range(world))
    for rank, got in res:
        assert sorted(got) == sorted(one)
        for k in one:
            assert got[k].dtype == one[k].dtype, k
            a, b = (v.view(np.int32) if v.dtype == np.float32 else v for v in (got[k], one[k]))
            np.testing.assert_array_equal(a, b, err_msg=f"rank {rank} {k}")
