"""GPU: the l1 and Huber instances of dc_eps_mse and dc_err_map through the C-ABI against the float64 oracle (tests/score_loss_oracle.py,
which holds the error model and the bounds), on every read path of the two kernels, and classify under config.score_loss on the HIP
backbones against the same classifier driving the oracle backbone as a foreign module.

Measured on an MI355X (first run of this file), worst error / bound over all cases: dc_eps_mse against the oracle 0.129,
dc_err_map planes 0.74, pixel sums against dc_eps_mse 0.091; classify f32 per-cell errors 9.5e-8 (l1), 1.7e-7 (Huber), DiT 1.5e-7
relative (bar 1e-4); bf16 errors rel-L2 5.8e-5 against r_o = 6.8e-5 (l1) and 8.6e-5 against 9.1e-5 (Huber), bound 2 r_o."""
import ctypes

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import evidence as EV
import evidence_oracle as EO
import oracle
import score_loss_oracle as O
import test_gpu_evidence as TE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KIND = {"l2": L.LOSS_L2, "l1": L.LOSS_L1, "huber": L.LOSS_HUBER}
LOSSES = [("l1", 1.0), ("huber", 1.0), ("huber", 0.25)]
# (C, H, W, ld, patch): the pixel-owner path at one trip and at two of the 256-lane stride loop (320 pixels), the generic element loop
# (C > 16), the patch > 1 read with rows longer than C p^2
LAYOUTS = [(3, 8, 8, 3, 0), (3, 20, 16, 4, 0), (20, 4, 4, 32, 0), (4, 8, 8, 24, 2)]
N_BJ, K_CLS = 3, 4
U_ = N_BJ * K_CLS


def _bits(v):
    v = v.cpu().contiguous()
    return v.view(torch.int32) if v.dtype == torch.float32 else v


_CASES = {}


def _case(C, H, W, ld, patch, v_param, delta):
    """Inputs of one layout (unit-normal pred / eps, so Huber has elements on both sides of delta), computed once and left unchanged:
    12 units over 3 (trial, image) pairs, with permuted bj_of_unit / out_index and a non-trivial img_of_bj.  One element has
    |d| == delta exactly: eps-param pred = 0.5 + delta against eps = 0.5; v-param alpha = 0.5, x = eps = 0, pred = 2 delta."""
    key = (C, H, W, ld, patch, v_param, delta)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000 * C + 10 * H + patch + v_param)
    pp = max(patch, 1)
    x, eps = torch.rand(2, C, H, W, generator=g) * 2 - 1, torch.randn(N_BJ, C, H, W, generator=g)
    alpha = 0.3 + 0.65 * torch.rand(N_BJ, generator=g)
    alpha[0] = 0.5
    sigma = torch.sqrt(1 - alpha * alpha)
    img = torch.tensor([1, 0, 1], dtype=torch.int32)
    bj = (torch.randperm(U_, generator=g) // K_CLS).to(torch.int32)
    oi = torch.randperm(U_, generator=g).to(torch.int32)
    pred = torch.randn(U_, C, H, W, generator=g)
    u0 = int((bj == 0).nonzero()[0])
    c0, y0, x0 = C - 1, H // 2, 1
    if v_param:
        x[1, c0, y0, x0] = 0.0                          # img_of_bj[0] = 1
        eps[0, c0, y0, x0] = 0.0
        pred[u0, c0, y0, x0] = 2 * delta
    else:
        eps[0, c0, y0, x0] = 0.5
        pred[u0, c0, y0, x0] = 0.5 + delta
    if patch > 1:
        rows = pred.view(U_, C, H // pp, pp, W // pp, pp).permute(0, 2, 4, 3, 5, 1).reshape(U_, H // pp, W // pp, pp * pp * C)
    else:
        rows = pred.permute(0, 2, 3, 1)
    pd = torch.full((U_, H // pp, W // pp, ld), float("nan"))          # behind a row's real features: never read
    pd[..., :rows.shape[-1]] = rows
    assert np.array_equal(EO.unpatchify(pd.numpy(), C, H, W, patch), pred.numpy())
    d, h = O.differences(pred.numpy(), eps.numpy(), x.numpy(), alpha.numpy(), sigma.numpy(), bj.numpy().astype(np.int64),
                         img.numpy().astype(np.int64), bool(v_param))
    assert abs(d[u0, c0, y0, x0]) == delta
    dev = [t.to(DEV).contiguous() for t in (pd, eps, x, alpha, sigma, bj, img, oi)]
    _CASES[key] = dict(d=d, h=h, dev=dev, oi=oi.long(), bj=bj, pred=pred, u0=u0)
    return _CASES[key]


def _mse_params(case, C, H, W, ld, patch, v_param, out, **loss):
    pd, eps, x, al, sg, bj, img, oi = case["dev"]
    return L.EpsMseParams(pred=pd.data_ptr(), eps=eps.data_ptr(), x=x.data_ptr(), alpha=al.data_ptr(), sigma=sg.data_ptr(),
                          bj_of_unit=bj.data_ptr(), img_of_bj=img.data_ptr(), out_index=oi.data_ptr(), out=out.data_ptr(),
                          n_units=U_, C=C, H=H, W=W, ld=ld, v_param=v_param, patch=patch, **loss)


def _eps_mse(case, C, H, W, ld, patch, v_param, pred=None, **loss):
    out = torch.full((U_,), float("nan"), device=DEV)
    p = _mse_params(case, C, H, W, ld, patch, v_param, out, **loss)
    if pred is not None:
        p.pred = pred.data_ptr()
    L.check(L.lib().dc_eps_mse(ctypes.byref(p), L.stream_ptr()), "dc_eps_mse")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ dc_eps_mse
@pytest.mark.parametrize("v_param", [0, 1])
@pytest.mark.parametrize("kind,delta", LOSSES)
@pytest.mark.parametrize("C,H,W,ld,patch", LAYOUTS)
def test_eps_mse_against_the_oracle(C, H, W, ld, patch, kind, delta, v_param):
    """|got - oracle| <= gamma(R + ceil(N / 256) + 9) (err + Ab) + Ab per unit (score_loss_oracle.scalar_bound); a second launch gives the
    same bits; a NaN in one prediction makes that unit NaN and no other."""
    case = _case(C, H, W, ld, patch, v_param, delta)
    o = O.sums(case["d"], case["h"], kind, delta)
    if kind == "huber":
        inside = float((np.abs(case["d"]) <= delta).mean())
        assert 0.05 < inside < 0.95, inside
    loss = dict(loss=KIND[kind], huber_delta=delta)
    out = _eps_mse(case, C, H, W, ld, patch, v_param, **loss)
    got = out.cpu().double().numpy()[case["oi"].numpy()]
    bound = O.scalar_bound(o, kind, O.eps_mse_adds(C * H * W))
    ratio = float((np.abs(got - o["err"]) / bound).max())
    print(f"dc_eps_mse {kind} delta={delta} C{C} {H}x{W} ld{ld} p{patch} v{v_param}: worst |err - oracle| / bound = {ratio:.3g} "
          f"(max rel err {float((np.abs(got - o['err']) / o['err']).max()):.3g})")
    assert np.isfinite(got).all() and ratio <= 1.0, ratio
    l2 = O.sums(case["d"], case["h"], "l2")["err"]
    assert float((np.abs(got - l2) / l2).min()) > 1e-3                   # not the squared error
    assert torch.equal(_bits(_eps_mse(case, C, H, W, ld, patch, v_param, **loss)), _bits(out))
    # NaN in, NaN out, for that unit only
    pd = case["dev"][0].clone()
    u = (case["u0"] + 5) % U_
    pd[u, 0, 0, 0] = float("nan")
    bad = _eps_mse(case, C, H, W, ld, patch, v_param, pred=pd, **loss).cpu()[case["oi"]]
    assert torch.isnan(bad).tolist() == [i == u for i in range(U_)]
    others = [i for i in range(U_) if i != u]
    assert torch.equal(_bits(bad[others]), _bits(out.cpu()[case["oi"]][others]))


@pytest.mark.parametrize("C,H,W,ld,patch", LAYOUTS)
def test_eps_mse_kind_zero_is_the_struct_without_the_field(C, H, W, ld, patch):
    """loss = DC_LOSS_L2 spelled out, with a huber_delta that must be ignored, against a struct that never names the two fields; and the
    l2 value itself against the oracle with its sqrt-then-square roundings."""
    case = _case(C, H, W, ld, patch, 1, 1.0)
    plain = _eps_mse(case, C, H, W, ld, patch, 1)
    named = _eps_mse(case, C, H, W, ld, patch, 1, loss=L.LOSS_L2, huber_delta=float("nan"))
    assert torch.equal(_bits(plain), _bits(named)) and torch.isfinite(plain).all()
    o = O.sums(case["d"], case["h"], "l2")
    got = plain.cpu().double().numpy()[case["oi"].numpy()]
    assert (np.abs(got - o["err"]) <= O.scalar_bound(o, "l2", O.eps_mse_adds(C * H * W))).all()
    # l1 ignores the delta as well
    a = _eps_mse(case, C, H, W, ld, patch, 1, loss=L.LOSS_L1, huber_delta=float("nan"))
    b = _eps_mse(case, C, H, W, ld, patch, 1, loss=L.LOSS_L1, huber_delta=0.5)
    assert torch.equal(_bits(a), _bits(b)) and torch.isfinite(a).all()


def test_refusal_codes():
    C, H, W, ld, patch = LAYOUTS[0]
    case = _case(C, H, W, ld, patch, 0, 1.0)
    out = torch.full((U_,), 7.0, device=DEV)
    lib = L.lib()
    acc, bad = EV.new_slabs(1, U_, H * W, DEV)
    for over in (dict(loss=3), dict(loss=-1), dict(loss=2, huber_delta=0.0), dict(loss=2, huber_delta=-1.0), dict(loss=2),
                 dict(loss=2, huber_delta=float("nan")), dict(loss=2, huber_delta=float("inf"))):
        p = _mse_params(case, C, H, W, ld, patch, 0, out, **over)
        assert lib.dc_eps_mse(ctypes.byref(p), L.stream_ptr()) == -1, over
        q = _map_params(case, C, H, W, ld, patch, 0, acc[0], bad[0], **over)
        assert lib.dc_err_map(ctypes.byref(q), L.stream_ptr()) == -1, over
    torch.cuda.synchronize()
    assert (out == 7.0).all() and int(acc.abs().sum()) == 0 and int(bad.sum()) == 0          # nothing was launched


# ------------------------------------------------------------------------------------------------ dc_err_map
def _map_params(case, C, H, W, ld, patch, v_param, acc, bad, first=0, count=U_, **loss):
    """Every unit its own cell (T = 1: cell = out_index[u]); units [first, first + count) of the case."""
    pd, eps, x, al, sg, bj, img, oi = case["dev"]
    return L.ErrMapParams(pred=pd[first:].data_ptr(), eps=eps.data_ptr(), x=x.data_ptr(), alpha=al.data_ptr(), sigma=sg.data_ptr(),
                          bj_of_unit=bj[first:].data_ptr(), img_of_bj=img.data_ptr(), out_index=oi[first:].data_ptr(),
                          acc=acc.data_ptr(), bad=bad.data_ptr(), n_units=count, C=C, H=H, W=W, ld=ld, v_param=v_param, patch=patch,
                          T=1, cells=U_, **loss)


def _err_map(case, C, H, W, ld, patch, v_param, splits, **loss):
    acc, bad = EV.new_slabs(1, U_, H * W, DEV)
    for first, count in splits:
        p = _map_params(case, C, H, W, ld, patch, v_param, acc[0], bad[0], first, count, **loss)
        L.check(L.lib().dc_err_map(ctypes.byref(p), L.stream_ptr()), "dc_err_map")
    torch.cuda.synchronize()
    return acc[0], bad[0]


@pytest.mark.parametrize("v_param", [0, 1])
@pytest.mark.parametrize("kind,delta", LOSSES)
@pytest.mark.parametrize("C,H,W,ld,patch", LAYOUTS)
def test_err_map_against_the_oracle_and_the_scalar(C, H, W, ld, patch, kind, delta, v_param):
    case = _case(C, H, W, ld, patch, v_param, delta)
    o = O.sums(case["d"], case["h"], kind, delta)
    loss = dict(loss=KIND[kind], huber_delta=delta)
    acc, bad = _err_map(case, C, H, W, ld, patch, v_param, [(0, U_)], **loss)
    assert int(bad.sum()) == 0 and int(acc[U_].abs().sum()) == 0
    planes = acc[:U_].cpu().double().numpy()[case["oi"].numpy()].reshape(U_, H, W) * 2.0 ** -O.F
    r_pix = float((np.abs(planes - o["v"]) / O.pixel_bound(o, kind, C)).max())
    # split launches (5 + 7 units, and one unit at a time) add up to the single launch's int64 bits
    for splits in ([(0, 5), (5, 7)], [(u, 1) for u in range(U_)]):
        acc2, bad2 = _err_map(case, C, H, W, ld, patch, v_param, splits, **loss)
        assert torch.equal(acc2, acc) and torch.equal(bad2, bad)
    # the pixel sums are dc_eps_mse's scalars
    scalar = _eps_mse(case, C, H, W, ld, patch, v_param, **loss).cpu().double().numpy()[case["oi"].numpy()]
    b_sum = O.pixel_sum_bound(o, kind, C, H, W, adds_scalar=O.eps_mse_adds(C * H * W), same_d=False)
    r_sum = float((np.abs(planes.sum(axis=(1, 2)) - scalar) / b_sum).max())
    print(f"dc_err_map {kind} delta={delta} C{C} {H}x{W} ld{ld} p{patch} v{v_param}: error / bound — planes {r_pix:.3g}, "
          f"pixel sum against dc_eps_mse {r_sum:.3g}")
    assert r_pix <= 1.0 and r_sum <= 1.0, (r_pix, r_sum)
    # a NaN prediction: its pixel is left out and counted, in that unit's cell only
    pd = case["dev"][0]
    keep = pd[2, 0, 0, 0].clone()
    pd[2, 0, 0, 0] = float("nan")
    try:
        acc3, bad3 = _err_map(case, C, H, W, ld, patch, v_param, [(0, U_)], **loss)
    finally:
        pd[2, 0, 0, 0] = keep
    cell = int(case["oi"][2])
    assert bad3.tolist() == [int(i == cell) for i in range(U_ + 1)]
    diff = (acc3 != acc).nonzero()
    assert diff.shape[0] == 1 and int(diff[0, 0]) == cell and int(acc3[cell, diff[0, 1]]) == 0


@pytest.mark.parametrize("C,H,W,ld,patch", LAYOUTS[1:2] + LAYOUTS[3:])
def test_err_map_kind_zero_is_the_struct_without_the_field(C, H, W, ld, patch):
    case = _case(C, H, W, ld, patch, 1, 1.0)
    a, _ = _err_map(case, C, H, W, ld, patch, 1, [(0, U_)])
    b, _ = _err_map(case, C, H, W, ld, patch, 1, [(0, U_)], loss=L.LOSS_L2, huber_delta=float("nan"))
    assert torch.equal(a, b) and int(a.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ end to end
def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("kind,delta", [("l1", None), ("huber", 1.0)])
def test_classify_f32_against_the_oracle_backbone_as_a_foreign_module(kind, delta):
    """The small UNetCondition2D of tests/test_gpu_evidence.py: the HIP classifier and the same classifier over the CPU oracle backbone
    (`_ForeignRunner`, loss.py's torch statements).  Per-cell errors within the project's f32 bar of 1e-4 relative, identical labels,
    the maps within test_gpu_evidence's parity gate; the plans carry the kind, and another loss never gets them."""
    keys = dict(score_loss=kind, **({} if delta is None else {"huber_delta": delta}))
    dc, host = TE._pair("unet", "f32", **keys)
    x, t, eps = TE._draws("unet")
    xd, kw = TE._on_dev(x, t, eps)
    lab, err, ev = dc.classify(xd, return_errors=True, return_evidence=True, **kw)
    ref_lab, ref_err, ref = host.classify(x, t=t, eps=eps, return_errors=True, return_evidence=True)
    fin = torch.isfinite(ref_err)
    assert torch.equal(torch.isfinite(err), fin) and int(fin.sum()) == 2 * (3 * 2 + 2 * 2)
    rel = float(((err - ref_err).abs() / ref_err)[fin].max())
    print(f"classify f32 {kind} delta={delta}: per-cell error max rel {rel:.3g} (bar 1e-4); labels {lab.tolist()} / {ref_lab.tolist()}")
    assert rel <= 1e-4, rel
    assert torch.equal(lab.cpu(), ref_lab)
    TE._parity(ev, ref, f"score_loss {kind}")
    for key, sp in dc._score_plans.items():
        assert ("loss", KIND[kind], 1.0 if delta is None else delta) in key and key[-1] == "evidence"
        structs = [s for (k, _, _), s in zip(sp["plan"].pb.ops, sp["plan"].pb.structs) if k in (L.OP_EPS_MSE, L.OP_ERR_MAP)]
        assert len(structs) == 2 and all((s.loss, s.huber_delta) == (KIND[kind], 1.0 if delta is None else delta) for s in structs)
    # the same object asked for l2 builds plans of its own and returns the squared error
    n_plans = len(dc._score_plans)
    dc.score_loss = (L.LOSS_L2, 1.0)
    _, err2 = dc.classify(xd, return_errors=True, **kw)
    dc2, _ = TE._pair("unet", "f32")
    _, want2 = dc2.classify(xd, return_errors=True, **kw)
    assert len(dc._score_plans) > n_plans and torch.equal(_bits(err2), _bits(want2))
    dc.check_device_errors()


@pytest.mark.parametrize("kind,delta", [("l1", None), ("huber", 1.0)])
def test_classify_bf16_within_twice_the_oracles_own_bf16_distance(kind, delta):
    """One stage (no pruning: every cell is scored on every side).  r_o: the errors of the classifier over the oracle backbone with
    bf16 storage rounding (lowp=True) against those over the fp32 oracle, relative L2 over the errors tensor, both on the CPU; the HIP
    bf16 errors must lie within 2 r_o of the fp32 oracle's, as DESIGN §6o holds the bf16 forward.  The same for the mean maps."""
    keys = dict(score_loss=kind, n_stages=1, evaluation_per_stage=[4], n_keep_per_stage=[1], **({} if delta is None else {"huber_delta": delta}))
    dc, host = TE._pair("unet", "bf16", **keys)
    o16 = oracle.OracleUNetCondition2D(**dca.small_unet_kwargs(), lowp=True)
    o16.load_state_dict(host.model.state_dict())
    host16 = dca.DiffusionClassifier(o16, dca.Config(**TE._cfg("unet", "bf16", **keys)))
    host16.encoder.load_state_dict(host.encoder.state_dict())
    x, t, eps = TE._draws("unet")
    xd, kw = TE._on_dev(x, t, eps)
    lab, err, ev = dc.classify(xd, return_errors=True, return_evidence=True, **kw)
    ref_lab, ref_err, ref = host.classify(x, t=t, eps=eps, return_errors=True, return_evidence=True)
    _, err16, ev16 = host16.classify(x, t=t, eps=eps, return_errors=True, return_evidence=True)
    assert torch.isfinite(err).all() and torch.isfinite(ref_err).all() and torch.isfinite(ev.mean_map).all()
    r, r_o = _rel_l2(err, ref_err), _rel_l2(err16, ref_err)
    rm, rm_o = _rel_l2(ev.mean_map.cpu(), ref.mean_map), _rel_l2(ev16.mean_map, ref.mean_map)
    print(f"classify bf16 {kind} delta={delta}: errors rel-L2 {r:.3e} (r_o {r_o:.3e}, bound {2 * r_o:.3e}); mean maps {rm:.3e} "
          f"(r_o {rm_o:.3e}); labels {lab.tolist()} / {ref_lab.tolist()}")
    assert r <= 2 * r_o and rm <= 2 * rm_o, (r, r_o, rm, rm_o)
    dc.check_device_errors()


def test_classify_dit_runs_the_patch_read_inside_a_plan():
    """DiT at the DiT tests' smallest grid (16 x 16, patch 4), f32, Huber with delta = 0.25."""
    dc, host = TE._pair("dit", "f32", score_loss="huber", huber_delta=0.25)
    x, t, eps = TE._draws("dit")
    xd, kw = TE._on_dev(x, t, eps)
    lab, err, ev = dc.classify(xd, return_errors=True, return_evidence=True, **kw)
    ref_lab, ref_err, ref = host.classify(x, t=t, eps=eps, return_errors=True, return_evidence=True)
    fin = torch.isfinite(ref_err)
    assert torch.equal(torch.isfinite(err), fin)
    rel = float(((err - ref_err).abs() / ref_err)[fin].max())
    print(f"classify f32 DiT huber delta=0.25: per-cell error max rel {rel:.3g} (bar 1e-4); labels {lab.tolist()} / {ref_lab.tolist()}")
    assert rel <= 1e-4 and torch.equal(lab.cpu(), ref_lab)
    TE._parity(ev, ref, "score_loss DiT huber")
    for sp in dc._score_plans.values():
        s = [s for (k, _, _), s in zip(sp["plan"].pb.ops, sp["plan"].pb.structs) if k == L.OP_EPS_MSE]
        assert len(s) == 1 and s[0].patch == 4 and (s[0].loss, round(s[0].huber_delta, 6)) == (L.LOSS_HUBER, 0.25)
    dc.check_device_errors()
