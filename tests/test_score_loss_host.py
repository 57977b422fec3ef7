"""CPU: config.score_loss ("l2" | "l1" | "huber", config.huber_delta) — the validation of the two keys, classify on a foreign backbone
(the `_ForeignRunner` path, loss.py's torch statements) against the float64 oracle (tests/score_loss_oracle.py, which holds the
tolerances and their derivation), what None / "l2" must leave alone, the per-pixel form against the scalar, the derived binding of the
two structs that gained the fields, and the refusals of the two entry points before any launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import evidence as EV
from diffusion_classifier_amd import loss as LS
import early_stop_oracle as SO
import score_loss_oracle as O
from test_abi_host import _c_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_STAGE = dict(n_stages=1, evaluation_per_stage=[7], n_keep_per_stage=[1])
LOSSES = [("l1", None), ("huber", 1.0), ("huber", 0.25)]


def _bits(v):
    v = v.cpu().contiguous()
    return v.view(torch.int32) if v.dtype == torch.float32 else v


def _keys(kind, delta):
    return dict(score_loss=kind, **({} if delta is None else {"huber_delta": delta}))


# ------------------------------------------------------------------------------------------------ the two config keys
def test_the_keys_resolve_to_a_kind_and_a_delta():
    assert (L.LOSS_L2, L.LOSS_L1, L.LOSS_HUBER) == (0, 1, 2)
    for cfg, want in ((dict(), (0, 1.0)), (dict(score_loss=None), (0, 1.0)), (dict(score_loss="l2"), (0, 1.0)), (dict(score_loss="l1"), (1, 1.0)),
                      (dict(score_loss="huber"), (2, 1.0)), (dict(score_loss="huber", huber_delta=0.25), (2, 0.25)),
                      (dict(score_loss="huber", huber_delta=3), (2, 3.0)), (dict(score_loss="huber", huber_delta=None), (2, 1.0))):
        assert LS.score_loss_of(dca.Config(**cfg)) == want, cfg
        dc, _, _, _ = SO.standin_classifier(dca, **cfg)
        assert dc.score_loss == want                     # resolved once, at construction


@pytest.mark.parametrize("bad", ["L1", "mse", "", "l2 ", 1, 0, True, ("l1",)])
def test_an_unknown_loss_is_refused_by_name(bad):
    with pytest.raises(ValueError, match="score_loss.*'l2'.*'l1'.*'huber'"):
        LS.score_loss_of(dca.Config(score_loss=bad))
    with pytest.raises(ValueError, match="score_loss"):
        SO.standin_classifier(dca, score_loss=bad)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "1.0", True, [1.0]])
def test_a_bad_huber_delta_is_refused(bad):
    with pytest.raises(ValueError, match="huber_delta"):
        LS.score_loss_of(dca.Config(score_loss="huber", huber_delta=bad))
    with pytest.raises(ValueError, match="huber_delta"):
        SO.standin_classifier(dca, score_loss="huber", huber_delta=bad)


@pytest.mark.parametrize("other", [None, "l2", "l1"])
def test_huber_delta_without_huber_is_refused(other):
    cfg = dict(huber_delta=0.5, **({} if other is None else {"score_loss": other}))
    with pytest.raises(ValueError, match="huber_delta.*score_loss"):
        LS.score_loss_of(dca.Config(**cfg))
    with pytest.raises(ValueError, match="huber_delta"):
        SO.standin_classifier(dca, **cfg)


# ------------------------------------------------------------------------------------------------ a foreign backbone against the oracle
def _record(dc):
    calls = []
    h = dc.ema.ema_model.register_forward_hook(
        lambda mod, args, kwargs, out: calls.append((kwargs["noise_labels"].clone(), kwargs["encoder_hidden_states"].clone(), out.clone())),
        with_kwargs=True)
    return calls, h


def _oracle_cells(dc, calls, x, t, eps, kind, delta):
    """Per (image, class, trial) cell the oracle's sums of the recorded prediction: the trial and the image from the row's lambda (the
    injected t are all different), the class from its conditioning -> (o, cell index arrays b, c, j)."""
    T, BS = t.shape
    lam = torch.stack([dc.schedule(t[j].clone()) for j in range(T)])
    alpha = torch.stack([torch.sqrt(torch.sigmoid(lam[j].clone())) for j in range(T)])
    sigma = torch.stack([torch.sqrt(torch.sigmoid(-lam[j].clone())) for j in range(T)])
    assert len(set(lam.reshape(-1).tolist())) == T * BS
    where = {float(lam[j, b]): (j, b) for j in range(T) for b in range(BS)}
    pred, bj, bb, cc, jj = [], [], [], [], []
    for lm, emb, out in calls:
        for r in range(out.shape[0]):
            j, b = where[float(lm[r])]
            hit = (dc.encoder.weight == emb[r, 0]).all(dim=1).nonzero().view(-1)
            assert hit.numel() == 1
            pred.append(out[r].numpy()); bj.append(j * BS + b); bb.append(b); cc.append(int(hit)); jj.append(j)
    d, h = O.differences(np.stack(pred), eps.reshape(T * BS, *eps.shape[2:]).numpy(), x.numpy(), alpha.reshape(-1).numpy(),
                         sigma.reshape(-1).numpy(), np.array(bj), np.tile(np.arange(BS), T), dc.pred_param == "v")
    return O.sums(d, h, kind, 1.0 if delta is None else delta), d, (np.array(bb), np.array(cc), np.array(jj))


@pytest.mark.parametrize("pred_param", ["eps", "v"])
@pytest.mark.parametrize("kind,delta", LOSSES)
def test_classify_on_a_foreign_backbone_matches_the_oracle_per_cell(kind, delta, pred_param):
    dc, x, t, eps = SO.standin_classifier(dca, pred_param=pred_param, **ONE_STAGE, **_keys(kind, delta))
    calls, hook = _record(dc)
    lab, err, post = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True)
    hook.remove()
    BS, C, T = err.shape
    assert len(calls) == T * C and torch.isfinite(err).all()
    o, d, (b, c, j) = _oracle_cells(dc, calls, x, t, eps, kind, delta)
    if kind == "huber":                                  # elements on both sides of delta: both branches are exercised
        inside = float((np.abs(d) <= delta).mean())
        assert 0.02 < inside < 0.98, inside
    N = x.shape[1] * x.shape[2] * x.shape[3]
    bound = O.scalar_bound(o, kind, adds=N - 1)          # torch's summation order is its own: any order has at most N - 1 adds on a path
    got = err.double().numpy()[b, c, j]
    ratio = float((np.abs(got - o["err"]) / bound).max())
    print(f"score loss host {kind} delta={delta} {pred_param}: worst |err - oracle| / bound = {ratio:.3g} over {got.size} cells")
    assert got.size == BS * C * T and ratio <= 1.0, ratio
    # the l2 errors of the same predictions are another tensor altogether: the key was honoured
    l2 = O.sums(d, 0 * d, "l2")["err"]
    assert float((np.abs(got - l2) / l2).min()) > 1e-3
    assert torch.equal(lab, err.mean(dim=2).argmin(dim=1))
    assert torch.equal(post.probs.argmax(dim=1), lab)


def test_none_and_l2_are_the_key_absent_bit_for_bit():
    res = []
    for keys in (dict(), dict(score_loss=None), dict(score_loss="l2")):
        dc, x, t, eps = SO.standin_classifier(dca, **keys)
        res.append(dc.classify(x, t=t, eps=eps, return_errors=True, return_evidence=True))
    lab0, err0, ev0 = res[0]
    assert torch.isfinite(ev0.mean_map).any()
    for lab, err, ev in res[1:]:
        assert torch.equal(lab, lab0) and torch.equal(_bits(err), _bits(err0))
        for a, b in zip(ev, ev0):
            assert torch.equal(_bits(a), _bits(b))
    # and a loss that is not l2 moves all three
    dc, x, t, eps = SO.standin_classifier(dca, score_loss="l1")
    _, err1, ev1 = dc.classify(x, t=t, eps=eps, return_errors=True, return_evidence=True)
    assert not torch.equal(_bits(err1), _bits(err0)) and not torch.equal(_bits(ev1.mean_map), _bits(ev0.mean_map))


# ------------------------------------------------------------------------------------------------ the per-pixel form
@pytest.mark.parametrize("kind,delta", [("l2", None)] + LOSSES)
def test_the_pixel_sum_of_a_units_map_is_its_scalar_error(kind, delta):
    """`err_map_torch` against `error_torch` on the same fp32 predictions, and both against the oracle.  The bound of the pixel sum is
    score_loss_oracle.pixel_sum_bound (same_d: both sides start from the same fp32 difference), derived as
    evidence_oracle.pixel_sum_bound derives its own."""
    g = torch.Generator().manual_seed(11)
    n, C, H, W = 6, 3, 5, 7
    pred, e = torch.randn(n, C, H, W, generator=g), torch.randn(n, C, H, W, generator=g)
    k, dl = LS.KINDS[kind], 1.0 if delta is None else delta
    acc, bad = EV.new_slabs(1, n, H * W, "cpu")
    EV.err_map_torch(pred, e, torch.arange(n), acc[0], bad[0], k, dl)
    assert int(bad.sum()) == 0 and int(acc[0, n].abs().sum()) == 0
    planes = acc[0, :n].double().numpy().reshape(n, H, W) * 2.0 ** -O.F
    scalar = LS.error_torch(pred, e, k, dl).double().numpy()
    d, h = O.differences(pred.numpy(), e.numpy(), None, None, None, np.arange(n), None, False)
    o = O.sums(d, h, kind, dl)
    N = C * H * W
    r_pix = float((np.abs(planes - o["v"]) / O.pixel_bound(o, kind, C)).max())
    r_sc = float((np.abs(scalar - o["err"]) / O.scalar_bound(o, kind, adds=N - 1)).max())
    r_sum = float((np.abs(planes.sum(axis=(1, 2)) - scalar) / O.pixel_sum_bound(o, kind, C, H, W, adds_scalar=N - 1, same_d=True)).max())
    print(f"score loss host {kind} delta={delta}: error / bound — planes {r_pix:.3g}, scalar {r_sc:.3g}, pixel sum against scalar {r_sum:.3g}")
    assert r_pix <= 1.0 and r_sc <= 1.0 and r_sum <= 1.0, (r_pix, r_sc, r_sum)


def test_err_map_torch_defaults_to_l2():
    g = torch.Generator().manual_seed(12)
    pred, e = torch.randn(2, 3, 4, 4, generator=g), torch.randn(2, 3, 4, 4, generator=g)
    a0, b0 = EV.new_slabs(1, 2, 16, "cpu")
    a1, b1 = EV.new_slabs(1, 2, 16, "cpu")
    EV.err_map_torch(pred, e, torch.arange(2), a0[0], b0[0])
    EV.err_map_torch(pred, e, torch.arange(2), a1[0], b1[0], L.LOSS_L2, 7.0)
    want = torch.round(((pred - e) ** 2).sum(1).double() * 2.0 ** 30).to(torch.int64).reshape(2, 16)
    assert torch.equal(a0, a1) and torch.equal(a0[0, :2], want)
    nan = pred.clone()
    nan[1, 0, 0, 0] = float("nan")
    for k in (L.LOSS_L2, L.LOSS_L1, L.LOSS_HUBER):       # NaN is left out and counted, for every kind
        a, b = EV.new_slabs(1, 2, 16, "cpu")
        EV.err_map_torch(nan, e, torch.arange(2), a[0], b[0], k, 1.0)
        assert b[0].tolist() == [0, 1, 0] and int(a[0, 1, 0]) == 0
        assert torch.isnan(LS.error_torch(nan, e, k, 1.0)).tolist() == [False, True]


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_the_two_structs_gained_the_fields_and_nothing_else_moved(tmp_path):
    for cls in (L.EpsMseParams, L.ErrMapParams):
        assert cls._fields_[-2:] == [("loss", L.i32), ("huber_delta", L.f32)], cls
        p = cls(loss=L.LOSS_HUBER, huber_delta=0.25)
        assert (p.loss, p.huber_delta) == (2, 0.25)
        assert (cls().loss, cls().huber_delta) == (0, 0.0)            # zero-initialised: l2
    assert [n for n, _ in L.EpsMseParams._fields_][:-2] == ["pred", "eps", "x", "alpha", "sigma", "bj_of_unit", "img_of_bj", "out_index", "out",
                                                           "n_units", "C", "H", "W", "ld", "v_param", "patch"]
    assert [n for n, _ in L.ErrMapParams._fields_][:-2] == ["pred", "eps", "x", "alpha", "sigma", "bj_of_unit", "img_of_bj", "out_index", "acc", "bad",
                                                           "n_units", "C", "H", "W", "ld", "v_param", "patch", "T", "cells", "pad_"]
    # sizeof / offsetof as the host C compiler reads the header (tests/test_abi_host.py's method)
    structs = ("dc_eps_mse_params", "dc_err_map_params")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "dcamd.h"', "int main(void) {",
             '  printf("kinds %d %d %d\\n", DC_LOSS_L2, DC_LOSS_L1, DC_LOSS_HUBER);']
    for s in structs:
        lines.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        for name, _, _ in L.ABI.structs[s]:
            lines.append(f'  printf("{s}.{name} %zu %zu\\n", offsetof({s}, {name}), sizeof((({s}*)0)->{name}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_c_compiler(), "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    theirs = {key: tuple(map(int, nums)) for key, *nums in (ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert theirs.pop("kinds") == (0, 1, 2)
    ours = {}
    for s in structs:
        cls = L.STRUCTS[s]
        ours[s] = (ctypes.sizeof(cls),)
        for name, _ in cls._fields_:
            ours[f"{s}.{name}"] = (getattr(cls, name).offset, getattr(cls, name).size)
    assert ours == theirs
    h = L.ABI
    assert (len(h.structs), len(h.functions), len(h.enums["dc_op_kind"])) == (32, 77, 23)
    assert L.ABI_VERSION == 5 and L.lib().dc_abi_version() == 5


def _params(cls, **over):
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    kw = dict(pred=a, eps=a, n_units=1, C=1, H=2, W=2, ld=1)
    kw.update(dict(out=a) if cls is L.EpsMseParams else dict(acc=a, bad=a, T=1, cells=1))
    kw.update(over)
    return cls(**kw), buf


@pytest.mark.parametrize("entry,cls", [("dc_eps_mse", L.EpsMseParams), ("dc_err_map", L.ErrMapParams)])
@pytest.mark.parametrize("over,word", [
    (dict(loss=3), "loss=3"), (dict(loss=-1), "loss=-1"), (dict(loss=1 << 20, huber_delta=1.0), "loss="),
    (dict(loss=2), "huber_delta"), (dict(loss=2, huber_delta=0.0), "huber_delta"), (dict(loss=2, huber_delta=-0.5), "huber_delta"),
    (dict(loss=2, huber_delta=float("nan")), "huber_delta"), (dict(loss=2, huber_delta=float("inf")), "huber_delta"),
])
def test_a_bad_kind_or_delta_is_refused_before_any_launch(entry, cls, over, word):
    """DC_ERR_ARG, answered without a GPU (a call that passed the checks would launch: none does here)."""
    lib = L.lib()
    p, _keep = _params(cls, **over)
    assert getattr(lib, entry)(ctypes.byref(p), None) == -1
    msg = lib.dc_last_error().decode()
    assert entry in msg and word in msg, msg
    # the older checks still come first: a shape error is a shape error whatever the kind says
    p, _keep = _params(cls, H=0, **over)
    assert getattr(lib, entry)(ctypes.byref(p), None) == -2
