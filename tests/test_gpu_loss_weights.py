"""GPU: the weighted instances of dc_eps_mse and dc_err_map through the C-ABI against the float64 oracle (tests/loss_weights_oracle.py,
which carries tests/score_loss_oracle.py's error model one rounding per term for m and one per unit for w further), on every read path
of the two kernels and for all three losses; classify with config.trial_weighting and pixel_weight on the HIP backbones against the same
classifier driving the oracle backbone as a foreign module; the evidence maps under weights; DiffusionClassifier.loss.

Measured on an MI355X (first run of this file), worst error / bound over all cases: weighted dc_eps_mse against the oracle
0.145, weighted dc_err_map planes 0.516; classify f32 per-cell errors 3.1e-7 (UNet) and 2.2e-7 (DiT) relative (bar 1e-4); bf16 errors
rel-L2 9.7e-5 against r_o = 1.62e-4, bound 2 r_o; evidence maps within 3.2e-6 / 9.7e-7 of the host path (gate 1e-4), pixel sums at 0.009
/ 0.017 of their bound; loss 1.5e-7 (UNet) and 6.3e-8 (DiT) relative (bar 1e-4)."""
import ctypes

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import evidence as EV
from diffusion_classifier_amd import loss as LS
import evidence_oracle as EO
import loss_weights_oracle as WO
import oracle
import score_loss_oracle as O
import test_gpu_evidence as TE
import test_gpu_score_loss as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KIND = TS.KIND
LOSSES = ["l2", "l1", "huber"]
LAYOUTS = TS.LAYOUTS                 # one and two trips of the pixel-owner loop, the element loop, the patch read
U_, N_IMG = TS.U_, 2
T_, CELLS = 2, 6                     # 12 slots of errors[cell, trial] and the dump slot behind them
DUMP = CELLS * T_
DUMP_UNIT = 3


def _bits(v):
    v = v.cpu().contiguous()
    return v.view(torch.int32) if v.dtype == torch.float32 else v


_WCASES = {}


def _wcase(C, H, W, ld, patch, v_param):
    """test_gpu_score_loss's inputs of the layout (12 units over 3 pairs, permuted bj_of_unit, img_of_bj = [1, 0, 1]; left unchanged) with
    an out_index of this file's: a permutation of the 12 slots with one unit sent to the dump slot; m uniform in [0, 2] with a block of
    exact zeros, w in [0.25, 4].  -> the case, the units' own (m, w) rows as float64 for the oracle, everything the kernels read on DEV."""
    key = (C, H, W, ld, patch, v_param)
    if key in _WCASES:
        return _WCASES[key]
    base = TS._case(C, H, W, ld, patch, v_param, 1.0)
    g = torch.Generator().manual_seed(500 + 10 * C + H + v_param)
    oi = torch.randperm(U_, generator=g).to(torch.int32)
    oi[DUMP_UNIT] = DUMP
    m = torch.rand(N_IMG, H, W, generator=g) * 2
    m[:, H // 4:H // 2 + 1, 1:W // 2 + 1] = 0.0
    w = 0.25 + 3.75 * torch.rand(N_IMG, T_, generator=g)
    img_u = torch.tensor([1, 0, 1])[base["bj"].long()]
    w_u = w[img_u, oi.long() % T_].clone()
    w_u[DUMP_UNIT] = 1.0                                 # the dump slot of padded units takes weight 1
    assert int((m == 0).sum()) > 0 and 0.25 <= float(w.min()) and float(w.max()) <= 4.0
    _WCASES[key] = dict(base=base, oi=oi, img_u=img_u, m=m, w=w, m_u=m[img_u].double().numpy(), w_u=w_u.double().numpy(),
                        dev=[t.to(DEV).contiguous() for t in (oi, m, w)])
    return _WCASES[key]


def _fields(wc, C, H, W, ld, patch, v_param, kind, m=None, w=None):
    pd, eps, x, al, sg, bj, img, _ = wc["base"]["dev"]
    f = dict(pred=pd.data_ptr(), eps=eps.data_ptr(), x=x.data_ptr(), alpha=al.data_ptr(), sigma=sg.data_ptr(), bj_of_unit=bj.data_ptr(),
             img_of_bj=img.data_ptr(), out_index=wc["dev"][0].data_ptr(), n_units=U_, C=C, H=H, W=W, ld=ld, v_param=v_param, patch=patch,
             loss=KIND[kind], huber_delta=1.0)
    if m is not None or w is not None:       # the flag and the block behind the struct (dcamd.h DC_LOSS_WEIGHTED)
        f.update(loss=KIND[kind] | L.LOSS_WEIGHTED, pixel_w=m.data_ptr() if m is not None else None,
                 trial_w=w.data_ptr() if w is not None else None, w_T=T_, w_cells=CELLS)
    return f


def _call(entry, cls, fields):
    """The entry on the struct, or on the struct with the weights block behind it when the fields carry one."""
    p = (LS.weighted_params(cls) if "pixel_w" in fields else cls)(**fields)
    return getattr(L.lib(), entry)(ctypes.cast(ctypes.pointer(p), ctypes.POINTER(cls)), L.stream_ptr())


def _eps_mse(wc, *a, **weights):
    out = torch.full((DUMP + 1,), float("nan"), device=DEV)
    L.check(_call("dc_eps_mse", L.EpsMseParams, dict(_fields(wc, *a, **weights), out=out.data_ptr())), "dc_eps_mse")
    torch.cuda.synchronize()
    return out


def _err_map(wc, *a, **weights):
    acc, bad = EV.new_slabs(1, CELLS, a[1] * a[2], DEV)
    L.check(_call("dc_err_map", L.ErrMapParams, dict(_fields(wc, *a, **weights), acc=acc.data_ptr(), bad=bad.data_ptr(), T=T_, cells=CELLS)),
            "dc_err_map")
    torch.cuda.synchronize()
    return acc[0], bad[0]


# ------------------------------------------------------------------------------------------------ the two ops
@pytest.mark.parametrize("v_param", [0, 1])
@pytest.mark.parametrize("kind", LOSSES)
@pytest.mark.parametrize("C,H,W,ld,patch", LAYOUTS)
def test_weighted_ops_against_the_oracle(C, H, W, ld, patch, kind, v_param):
    """dc_eps_mse: |got - w S| <= w [gamma(R + 1 + adds + 1 (+ 4 for l2)) (S + Ab_w) + Ab_w] per unit, adds = ceil(N / 256) + 9;
    dc_err_map: every cell's plane against the sum of its units' w m v within the sum of their pixel bounds
    (loss_weights_oracle).  Ones give the bits of the unweighted call, int64 planes included; a second launch gives the same bits; a
    NaN in m makes exactly its image's units NaN."""
    wc = _wcase(C, H, W, ld, patch, v_param)
    a = (C, H, W, ld, patch, v_param, kind)
    oi, m, w = wc["dev"]
    o = WO.weighted_sums(wc["base"]["d"], wc["base"]["h"], kind, 1.0, wc["m_u"], wc["w_u"])
    assert float(WO.pixel_value(o).max()) < EV.VMAX / 8                   # far below DC_EVIDENCE_VMAX, on the CPU oracle first
    out = _eps_mse(wc, *a, m=m, w=w)
    got = out.cpu().double().numpy()[wc["oi"].long().numpy()]
    r_sc = float((np.abs(got - WO.scalar_value(o)) / WO.scalar_bound(o, kind, O.eps_mse_adds(C * H * W))).max())
    # the planes: two units per cell, the dump unit alone in the extra plane
    acc, bad = _err_map(wc, *a, m=m, w=w)
    cell = (wc["oi"].long() // T_).numpy()
    want, bound = np.zeros((CELLS + 1, H, W)), np.zeros((CELLS + 1, H, W))
    np.add.at(want, cell, WO.pixel_value(o))
    np.add.at(bound, cell, WO.pixel_bound(o, kind, C))
    planes = acc.cpu().double().numpy().reshape(CELLS + 1, H, W) * 2.0 ** -O.F
    r_pix = float((np.abs(planes - want) / bound).max())
    print(f"weighted ops {kind} C{C} {H}x{W} ld{ld} p{patch} v{v_param}: error / bound — dc_eps_mse {r_sc:.3g}, dc_err_map planes {r_pix:.3g}")
    assert np.isfinite(got).all() and int(bad.sum()) == 0 and r_sc <= 1.0 and r_pix <= 1.0, (r_sc, r_pix)
    assert cell[DUMP_UNIT] == CELLS and int(acc[CELLS].abs().sum()) > 0
    unweighted = O.sums(wc["base"]["d"], wc["base"]["h"], kind, 1.0)["err"]
    assert float(np.median(np.abs(got / unweighted - 1))) > 1e-2           # not the unweighted sums (a single unit may come close)
    # a second launch: the same bits
    assert torch.equal(_bits(_eps_mse(wc, *a, m=m, w=w)), _bits(out))
    acc2, bad2 = _err_map(wc, *a, m=m, w=w)
    assert torch.equal(acc2, acc) and torch.equal(bad2, bad)
    # ones: the bits of the call without weights, through each pointer alone and through both
    plain, (acc0, bad0) = _eps_mse(wc, *a), _err_map(wc, *a)
    one_m, one_w = torch.ones_like(m), torch.ones_like(w)
    for weights in (dict(m=one_m, w=one_w), dict(m=one_m), dict(w=one_w)):
        assert torch.equal(_bits(_eps_mse(wc, *a, **weights)), _bits(plain)), list(weights)
        acc1, bad1 = _err_map(wc, *a, **weights)
        assert torch.equal(acc1, acc0) and torch.equal(bad1, bad0), list(weights)
    assert torch.isfinite(plain.cpu()[wc["oi"].long()]).all()
    # trial weights alone: the unweighted result times w, one fp32 product
    only_w = _eps_mse(wc, *a, w=w).cpu()[wc["oi"].long()]
    assert torch.equal(_bits(only_w), _bits(plain.cpu()[wc["oi"].long()] * torch.from_numpy(wc["w_u"]).float()))
    # a NaN in m of image 1: exactly that image's units are NaN, the others keep their bits
    m_nan = m.clone()
    m_nan[1, H - 1, W - 1] = float("nan")
    poisoned = _eps_mse(wc, *a, m=m_nan, w=w).cpu()[wc["oi"].long()]
    hit = (wc["img_u"] == 1)
    assert torch.isnan(poisoned).tolist() == hit.tolist() and 0 < int(hit.sum()) < U_
    assert torch.equal(_bits(poisoned[~hit]), _bits(out.cpu()[wc["oi"].long()][~hit]))
    acc3, bad3 = _err_map(wc, *a, m=m_nan, w=w)
    want_bad = np.zeros(CELLS + 1, dtype=np.int64)
    np.add.at(want_bad, cell[hit.numpy()], 1)
    assert bad3.cpu().tolist() == want_bad.tolist()
    assert set((acc3 != acc).nonzero()[:, 1].tolist()) <= {H * W - 1}


def test_trial_weights_without_their_maps_launch_nothing():
    C, H, W, ld, patch = LAYOUTS[0]
    wc = _wcase(C, H, W, ld, patch, 0)
    oi, m, w = wc["dev"]
    out = torch.full((DUMP + 1,), 7.0, device=DEV)
    acc, bad = EV.new_slabs(1, CELLS, H * W, DEV)
    for over in (dict(out_index=None), dict(img_of_bj=None), dict(w_T=0), dict(w_cells=0)):
        f = dict(_fields(wc, C, H, W, ld, patch, 0, "l2", m=m, w=w), **over)
        assert _call("dc_eps_mse", L.EpsMseParams, dict(f, out=out.data_ptr())) == -1, over
    for over in (dict(out_index=None), dict(img_of_bj=None), dict(T=0), dict(cells=0)):
        f = dict(_fields(wc, C, H, W, ld, patch, 0, "l2", m=m, w=w), acc=acc.data_ptr(), bad=bad.data_ptr(), T=T_, cells=CELLS)
        assert _call("dc_err_map", L.ErrMapParams, dict(f, **over)) in (-1, -2), over
    torch.cuda.synchronize()
    assert (out == 7.0).all() and int(acc.abs().sum()) == 0 and int(bad.sum()) == 0


# ------------------------------------------------------------------------------------------------ classify
def _mask(x):
    """A 0/1 mask on x's grid: a centred box, and one more row block for image 1 so that the images' masks differ."""
    BS, _, H, W = x.shape
    m = torch.zeros(BS, H, W)
    m[:, H // 4:3 * H // 4, W // 8:7 * W // 8] = 1.0
    m[1, :2] = 1.0
    return m


def _weighted_structs(dc):
    """(plan key, dc_eps_mse struct) of every score plan of the classifier."""
    return [(key, s) for key, sp in dc._score_plans.items()
            for (k, _, _), s in zip(sp["plan"].pb.ops, sp["plan"].pb.structs) if k == L.OP_EPS_MSE]


@pytest.mark.parametrize("kind", ["unet", "dit"])
def test_classify_f32_with_train_weights_and_a_mask(kind):
    """The smallest HIP UNet / DiT of tests/test_gpu_evidence.py (f32, BS = 2, 3 classes, T = 4, two stages) with trial_weighting =
    "train" and a 0/1 mask, against the same classifier over the CPU oracle backbone (`_ForeignRunner`, loss.py's torch statements):
    per-cell errors within the project's f32 bar of 1e-4 relative, equal labels; the same bits when every launch holds a single pair;
    and no call is served a plan or a buffer of another call's weights."""
    dc, host = TE._pair(kind, "f32", trial_weighting="train")
    x, t, eps = TE._draws(kind)
    xd, kw = TE._on_dev(x, t, eps)
    m = _mask(x)
    md = m.to(DEV)
    lab, err = dc.classify(xd, return_errors=True, pixel_weight=md, **kw)
    ref_lab, ref_err = host.classify(x, t=t, eps=eps, return_errors=True, pixel_weight=m)
    fin = torch.isfinite(ref_err)
    assert torch.equal(torch.isfinite(err), fin) and int(fin.sum()) == 2 * (3 * 2 + 2 * 2)
    rel = float(((err - ref_err).abs() / ref_err)[fin].max())
    print(f"classify f32 {kind} train + mask: per-cell error max rel {rel:.3g} (bar 1e-4); labels {lab.tolist()} / {ref_lab.tolist()}")
    assert rel <= 1e-4 and torch.equal(lab.cpu(), ref_lab)
    for key, s in _weighted_structs(dc):
        assert ("weights", True, True) in key and s.pixel_w and s.trial_w and (s.w_T, s.w_cells) == (4, 2 * 3)
        assert s.loss == L.LOSS_L2 | L.LOSS_WEIGHTED
        assert s.patch == (4 if kind == "dit" else 0)
    # one pair per launch: the same bits
    dc3, _ = TE._pair(kind, "f32", trial_weighting="train", units_per_launch=3)
    lab3, err3 = dc3.classify(xd, return_errors=True, pixel_weight=md, **kw)
    assert {sp["n_bj"] for sp in dc3._score_plans.values()} == {1}
    assert torch.equal(lab3, lab) and torch.equal(_bits(err3), _bits(err))
    # switching the mask and the weighting between calls
    _, err_nomask = dc.classify(xd, return_errors=True, **kw)
    _, err_other = dc.classify(xd, return_errors=True, pixel_weight=1.0 - md, **kw)
    _, err_again = dc.classify(xd, return_errors=True, pixel_weight=md, **kw)
    assert torch.equal(_bits(err_again), _bits(err))
    assert not torch.equal(_bits(err_nomask), _bits(err)) and not torch.equal(_bits(err_other), _bits(err))
    _, ref_nomask = host.classify(x, t=t, eps=eps, return_errors=True)
    f2 = torch.isfinite(ref_nomask)
    assert torch.equal(torch.isfinite(err_nomask), f2) and float(((err_nomask - ref_nomask).abs() / ref_nomask)[f2].max()) <= 1e-4
    dc.trial_weighting = None                            # the same object without trial weights, with and without the mask
    plain, _ = TE._pair(kind, "f32")
    _, err_m_only = dc.classify(xd, return_errors=True, pixel_weight=md, **kw)
    _, want_m_only = plain.classify(xd, return_errors=True, pixel_weight=md, **kw)
    assert torch.equal(_bits(err_m_only), _bits(want_m_only))
    _, err_plain = dc.classify(xd, return_errors=True, **kw)
    _, want_plain = plain.classify(xd, return_errors=True, **kw)
    assert torch.equal(_bits(err_plain), _bits(want_plain))
    assert sum(1 for key in dc._score_plans if not any(isinstance(k, tuple) and k and k[0] == "weights" for k in key)) == 2
    for key, s in _weighted_structs(plain):              # the plain path: no marker in the key, no weighted instance behind the op
        marker = [k for k in key if isinstance(k, tuple) and k and k[0] == "weights"]
        assert bool(marker) == hasattr(s, "pixel_w") == bool(s.loss & L.LOSS_WEIGHTED) and not getattr(s, "trial_w", None)
    dc.check_device_errors()


def test_classify_bf16_within_twice_the_oracles_own_bf16_distance():
    """One stage (no pruning).  r_o: the errors of the classifier over the oracle backbone with bf16 storage rounding (lowp=True)
    against those over the fp32 oracle, relative L2 over the errors tensor, both on the CPU and both weighted; the HIP bf16 errors must
    lie within 2 r_o of the fp32 oracle's (the rule of tests/test_gpu_score_loss.py)."""
    keys = dict(trial_weighting="train", n_stages=1, evaluation_per_stage=[4], n_keep_per_stage=[1])
    dc, host = TE._pair("unet", "bf16", **keys)
    o16 = oracle.OracleUNetCondition2D(**dca.small_unet_kwargs(), lowp=True)
    o16.load_state_dict(host.model.state_dict())
    host16 = dca.DiffusionClassifier(o16, dca.Config(**TE._cfg("unet", "bf16", **keys)))
    host16.encoder.load_state_dict(host.encoder.state_dict())
    x, t, eps = TE._draws("unet")
    xd, kw = TE._on_dev(x, t, eps)
    m = _mask(x)
    lab, err = dc.classify(xd, return_errors=True, pixel_weight=m.to(DEV), **kw)
    ref_lab, ref_err = host.classify(x, t=t, eps=eps, return_errors=True, pixel_weight=m)
    _, err16 = host16.classify(x, t=t, eps=eps, return_errors=True, pixel_weight=m)
    assert torch.isfinite(err).all() and torch.isfinite(ref_err).all()
    r, r_o = TS._rel_l2(err, ref_err), TS._rel_l2(err16, ref_err)
    print(f"classify bf16 train + mask: errors rel-L2 {r:.3e} (r_o {r_o:.3e}, bound {2 * r_o:.3e}); labels {lab.tolist()} / {ref_lab.tolist()}")
    assert r <= 2 * r_o, (r, r_o)
    dc.check_device_errors()


# ------------------------------------------------------------------------------------------------ evidence
@pytest.mark.parametrize("kind", ["unet", "dit"])
def test_evidence_with_weights(kind):
    """l1, a bounded trial weighting (w = 0.5 + sigmoid(logsnr): every v stays far below DC_EVIDENCE_VMAX) and the mask: the winner's
    delta_map is exactly 0, the maps pass the parity gate of tests/test_gpu_evidence.py against the host path, and the pixel sum of
    mean_map[b, c] is the mean of errors[b, c, :n] within tests/evidence_oracle.pixel_sum_bound with the weights' roundings added: two
    on the map side (m, w on every pixel) and two on the mean side (m on every term, w on every unit)."""
    keys = dict(score_loss="l1", trial_weighting=lambda lam: 0.5 + torch.sigmoid(lam))
    dc, host = TE._pair(kind, "f32", **keys)
    x, t, eps = TE._draws(kind)
    xd, kw = TE._on_dev(x, t, eps)
    m = _mask(x)
    lab, err, post, ev = dc.classify(xd, return_errors=True, return_posterior=True, return_evidence=True, pixel_weight=m.to(DEV), **kw)
    ref_lab, ref = host.classify(x, t=t, eps=eps, return_evidence=True, pixel_weight=m)
    BS, ncls = err.shape[:2]
    C, H, W = x.shape[1:]
    assert ev.invalid.tolist() == [0] * BS and torch.equal(lab.cpu(), ref_lab)
    assert (ev.delta_map[torch.arange(BS), lab] == 0).all()
    TE._parity(ev, ref, f"weights {kind}")
    hidden = (m == 0)[:, None].expand(BS, ncls, H, W)
    assert bool((ev.mean_map.cpu()[hidden] == 0).all())
    sm, worst = ev.mean_map.cpu().double().sum(dim=(2, 3)), 0.0
    for b in range(BS):
        for c in range(ncls):
            n = int(ev.n_trials[b, c])
            rel, ab = EO.pixel_sum_bound(C, H, W, n)
            mean = float(err[b, c, :n].double().mean())
            bound = (rel + 4 * EO.U) * mean + ab
            worst = max(worst, abs(float(sm[b, c]) - mean) / bound)
    print(f"evidence with weights {kind}: pixel sums against the mean errors, worst error / bound = {worst:.3g}")
    assert worst <= 1.0, worst
    for key, sp in dc._score_plans.items():
        s = [s for (k, _, _), s in zip(sp["plan"].pb.ops, sp["plan"].pb.structs) if k == L.OP_ERR_MAP]
        assert len(s) == 1 and s[0].pixel_w and s[0].trial_w and s[0].loss == L.LOSS_L1 | L.LOSS_WEIGHTED and key[-1] == "evidence"
    dc.check_device_errors()


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("kind", ["unet", "dit"])
def test_loss_on_a_hip_backbone_against_the_foreign_run(kind):
    """One draw per image through the scoring plans (one trial, the label column, the weighted dc_eps_mse) against the reference's
    statements in eager torch over the oracle backbone, at the same injected (t, eps): the project's 1e-4 bar."""
    dc, host = TE._pair(kind, "f32")
    x, t, eps = TE._draws(kind)
    text = torch.tensor([2, 0])
    got = dc.loss(x.to(DEV), text, t=t[0], eps=eps[0].to(DEV))
    want = host.loss(x, text, t=t[0], eps=eps[0])
    rel = abs(float(got) - float(want)) / float(want)
    print(f"loss {kind}: HIP {float(got):.8g} foreign {float(want):.8g} rel {rel:.3g} (bar 1e-4)")
    assert got.is_cuda and got.dtype == torch.float32 and got.dim() == 0 and want.dim() == 0 and rel <= 1e-4
    for key, s in _weighted_structs(dc):
        assert ("weights", False, True) in key and s.trial_w and not s.pixel_w and (s.w_T, s.w_cells, s.loss) == (1, 2 * 3, L.LOSS_L2 | L.LOSS_WEIGHTED)
    # the EMA copy holds the same weights here; another label column is another number
    assert abs(float(dc.loss(x.to(DEV), text, t=t[0], eps=eps[0].to(DEV), ema=True)) - float(want)) / float(want) <= 1e-4
    assert float(dc.loss(x.to(DEV), torch.tensor([1, 1]), t=t[0], eps=eps[0].to(DEV))) != float(got)
    with pytest.raises(ValueError, match="text"):
        dc.loss(x.to(DEV), t=t[0], eps=eps[0].to(DEV))
    with pytest.raises(ValueError, match="text"):
        dc.loss(x.to(DEV), torch.tensor([0, 3]), t=t[0], eps=eps[0].to(DEV))
    dc.check_device_errors()
