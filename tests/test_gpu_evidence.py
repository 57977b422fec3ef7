"""GPU: dc_err_map + dc_evidence_maps through the C-ABI against the float64 oracle (tests/evidence_oracle.py, which also holds the
tolerances and their derivation), and classify(return_evidence=True) on the HIP backbones: what the flag must leave alone, the maps'
reproducibility, their pixel sums against the posterior, parity with the host path, and grid sharding."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import evidence as EV
from diffusion_classifier_amd import posterior as P
import evidence_oracle as O
import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(v):
    v = v.cpu().contiguous()
    return v.view(torch.int32) if v.dtype == torch.float32 else v


# ------------------------------------------------------------------------------------------------ the two kernels
T_OP, ENDS, CELLS, WINNER = 17, [6, 17], 3, 2
N_EVAL = [6, 17, 17]             # cell 0 pruned after stage 0: 6 + 17 + 17 = 40 units on 3 cells


def _op_case(C, H, W, ld, patch, v_param, plant, seed=0):
    """40 units over two launches (one per stage) plus one padded slot each; bj = trial (one image, stored as image 1 of 2)."""
    g = torch.Generator().manual_seed(seed)
    pp = max(patch, 1)
    rows = (H // pp, W // pp)
    stage_units = [[(c, j) for j in range(0, 6) for c in range(3)], [(c, j) for j in range(6, 17) for c in (1, 2)]]
    eps = torch.randn(T_OP, C, H, W, generator=g)
    x = torch.rand(2, C, H, W, generator=g) * 2 - 1
    alpha = 0.3 + 0.65 * torch.rand(T_OP, generator=g)
    sigma = torch.sqrt(1 - alpha * alpha)
    launches = []
    for s, units in enumerate(stage_units):
        n = len(units) + 1                                               # the last slot is padding: the dump cell
        pred = torch.randn(n, *rows, ld, generator=g)
        pred[..., C * pp * pp:] = float("nan")                           # behind the row's real features: never read
        cell = [c for c, _ in units] + [-1]
        trial = [j for _, j in units] + [units[0][1]]
        if plant and s == 0:
            u_nan, u_big = units.index((0, 3)), units.index((1, 5))
            pred[u_nan, rows[0] // 2, 1, 0] = float("nan")
            pred[u_big, 0, rows[1] - 1, C - 1] = 1e4
        launches.append(dict(pred=pred, cell=cell, trial=trial))
    return dict(eps=eps, x=x, alpha=alpha, sigma=sigma, launches=launches)


def _run_op(case, C, H, W, ld, patch, v_param, perm=None):
    """Both launches into acc[s] / bad[s], then dc_evidence_maps.  perm: a permutation applied to the units of every launch."""
    dev = DEV
    acc, bad = EV.new_slabs(2, CELLS, H * W, dev)
    eps, x, al, sg = (case[k].to(dev).contiguous() for k in ("eps", "x", "alpha", "sigma"))
    img_of_bj = torch.ones(T_OP, dtype=torch.int32, device=dev)
    keep = []
    for s, la in enumerate(case["launches"]):
        n = la["pred"].shape[0]
        order = list(range(n)) if perm is None else [int(i) for i in torch.randperm(n, generator=torch.Generator().manual_seed(perm + s))]
        pred = la["pred"][order].to(dev).contiguous()
        bj = torch.tensor([la["trial"][i] for i in order], dtype=torch.int32, device=dev)
        oi = torch.tensor([la["cell"][i] * T_OP + la["trial"][i] if la["cell"][i] >= 0 else CELLS * T_OP for i in order],
                          dtype=torch.int32, device=dev)
        p = L.ErrMapParams(pred=pred.data_ptr(), eps=eps.data_ptr(), x=x.data_ptr(), alpha=al.data_ptr(), sigma=sg.data_ptr(),
                           bj_of_unit=bj.data_ptr(), img_of_bj=img_of_bj.data_ptr(), out_index=oi.data_ptr(),
                           acc=acc[s].data_ptr(), bad=bad[s].data_ptr(), n_units=n, C=C, H=H, W=W, ld=ld, v_param=v_param, patch=patch,
                           T=T_OP, cells=CELLS)
        L.check(L.lib().dc_err_map(ctypes.byref(p), L.stream_ptr()), "dc_err_map")
        keep += [pred, bj, oi]
    n_eval = torch.tensor([N_EVAL], dtype=torch.int32, device=dev)
    ev = EV.evidence_maps_hip(acc, bad, ENDS, n_eval, torch.tensor([WINNER], dtype=torch.int32, device=dev), H, W)
    torch.cuda.synchronize()
    return acc, bad, ev


def _op_oracle(case, C, H, W, patch, v_param):
    pred = np.concatenate([O.unpatchify(la["pred"].numpy(), C, H, W, patch) for la in case["launches"]])
    cell = np.array(sum((la["cell"] for la in case["launches"]), []))
    trial = np.array(sum((la["trial"] for la in case["launches"]), []))
    v, bound = O.unit_maps(pred, case["eps"].numpy(), case["x"].numpy(), case["alpha"].numpy(), case["sigma"].numpy(), trial,
                           np.ones(T_OP, dtype=np.int64), bool(v_param))
    return v, bound, cell, trial


OP_SHAPES = [(3, 6, 10, 4, 0, 0), (12, 17, 19, 12, 0, 1), (20, 8, 8, 32, 0, 0), (4, 8, 8, 16, 2, 0), (4, 8, 8, 16, 2, 1)]


@pytest.mark.parametrize("C,H,W,ld,patch,v_param", OP_SHAPES)
def test_kernels_against_the_oracle(C, H, W, ld, patch, v_param):
    label = f"C{C} {H}x{W} ld{ld} p{patch} v{v_param}"
    # clean inputs: every cell finite, the deltas of both losing cells non-trivial
    case = _op_case(C, H, W, ld, patch, v_param, plant=False)
    v, bound, cell, trial = _op_oracle(case, C, H, W, patch, v_param)
    assert np.isfinite(v).all() and v.max() < O.VMAX / 4, v.max()
    o = O.maps(v, bound, cell, trial, ENDS, 1, 3, np.array([N_EVAL]), np.array([WINNER]))
    acc, bad, ev = _run_op(case, C, H, W, ld, patch, v_param)
    m = O.check(ev, o, label=label)
    print(f"evidence op {label}: " + " ".join(f"{k}={x:.3g}" for k, x in m.items()))
    assert ev.invalid.tolist() == [0] and int(bad.sum()) == 0
    assert (ev.delta_map[0, WINNER] == 0).all() and float(ev.delta_map[0, :2].abs().max()) > 0 and torch.isfinite(ev.mean_map).all()
    # the padded slots went to the dump plane of their stage and nowhere else: the planes hold exactly the quantised oracle values
    q = np.rint(v * 2.0 ** O.F)
    for s in range(2):
        lo, hi = (0, 19) if s == 0 else (19, 42)
        pad = hi - 1
        dump = acc[s, CELLS].cpu().double().numpy().reshape(H, W)
        assert np.abs(dump - q[pad]).max() <= np.ceil((bound[pad] * 2.0 ** O.F).max()) + 1
    # planted: a NaN in cell 0, a value above VMAX in cell 1 — exactly those two cells are NaN, both are counted, nothing else moves
    case_p = _op_case(C, H, W, ld, patch, v_param, plant=True)
    vp, bp, cell, trial = _op_oracle(case_p, C, H, W, patch, v_param)
    notfin = ~np.isfinite(vp)
    big = np.isfinite(vp) & (vp > O.VMAX)
    assert int(notfin.sum()) == 1 and int(big.sum()) == 1 and np.nanmax(np.where(big, 0, vp)) < O.VMAX / 4
    op = O.maps(vp, bp, cell, trial, ENDS, 1, 3, np.array([N_EVAL]), np.array([WINNER]))
    assert op["bad"].tolist() == [[1, 1, 0]]
    acc_p, bad_p, ev_p = _run_op(case_p, C, H, W, ld, patch, v_param)
    nan_cells = torch.isnan(ev_p.mean_map[0]).flatten(1)
    assert nan_cells.all(dim=1).tolist() == [True, True, False] and nan_cells.any(dim=1).tolist() == [True, True, False]
    assert torch.equal(torch.isnan(ev_p.mean_map), torch.isnan(ev_p.delta_map))
    O.check(ev_p, op, label=label + " planted")
    assert ev_p.invalid.tolist() == [2] and bad_p.cpu().tolist() == [[1, 1, 0, 0], [0, 0, 0, 0]]
    # a second pair of launches: the same bits; the units of each launch in another order: the same accumulators
    acc2, bad2, ev2 = _run_op(case, C, H, W, ld, patch, v_param)
    acc3, bad3, ev3 = _run_op(case, C, H, W, ld, patch, v_param, perm=5)
    for other in ((acc2, bad2, ev2), (acc3, bad3, ev3)):
        assert torch.equal(other[0], acc) and torch.equal(other[1], bad)
        for a, b in zip(other[2], ev):
            assert torch.equal(_bits(a), _bits(b))


def test_kernels_refuse_bad_arguments():
    z = torch.zeros(64, device=DEV)
    ok = dict(pred=z.data_ptr(), eps=z.data_ptr(), acc=z.data_ptr(), bad=z.data_ptr(), n_units=1, C=1, H=2, W=2, ld=1, T=1, cells=1)
    lib = L.lib()
    assert lib.dc_err_map(ctypes.byref(L.ErrMapParams(**dict(ok, acc=None))), L.stream_ptr()) == -1
    assert lib.dc_err_map(ctypes.byref(L.ErrMapParams(**dict(ok, v_param=1))), L.stream_ptr()) == -1          # v-param without x / alpha / sigma
    assert lib.dc_err_map(ctypes.byref(L.ErrMapParams(**dict(ok, ld=3, patch=2))), L.stream_ptr()) == -2
    assert lib.dc_err_map(ctypes.byref(L.ErrMapParams(**dict(ok, H=3, W=2, ld=4, patch=2))), L.stream_ptr()) == -2
    assert lib.dc_err_map(ctypes.byref(L.ErrMapParams(**dict(ok, T=0))), L.stream_ptr()) == -2
    m = dict(acc=z.data_ptr(), bad=z.data_ptr(), stage_ends=z.data_ptr(), n_eval=z.data_ptr(), winner=z.data_ptr(),
             mean_map=z.data_ptr(), delta_map=z.data_ptr(), invalid=z.data_ptr(), n_stages=1, BS=1, C=1, HW=4)
    assert lib.dc_evidence_maps(ctypes.byref(L.EvidenceMapsParams(**dict(m, winner=None))), L.stream_ptr()) == -1
    assert lib.dc_evidence_maps(ctypes.byref(L.EvidenceMapsParams(**dict(m, n_stages=0))), L.stream_ptr()) == -2
    assert lib.dc_evidence_maps(ctypes.byref(L.EvidenceMapsParams(**dict(m, n_stages=65))), L.stream_ptr()) == -2
    assert lib.dc_evidence_maps(ctypes.byref(L.EvidenceMapsParams(**dict(m, HW=0))), L.stream_ptr()) == -2
    torch.cuda.synchronize()


def test_maps_kernel_equals_its_torch_statement_bit_for_bit():
    """dc_evidence_maps against evidence_maps_torch on hand-made accumulators: pruned prefixes, an n that is no stage end, a class never
    scored, an image without a winner, bad counts, more classes than a workgroup has lanes."""
    g = torch.Generator().manual_seed(3)
    BS, C, HW, ends = 3, 300, 70, [2, 5, 9]
    acc = torch.randint(0, 1 << 40, (3, BS * C + 1, HW), generator=g, dtype=torch.int64)
    bad = (torch.rand(3, BS * C + 1, generator=g) < 0.05).to(torch.int32) * 3
    n_eval = torch.tensor([0, 2, 5, 9, 4])[torch.randint(0, 5, (BS, C), generator=g)].to(torch.int32)
    winner = torch.tensor([7, -1, 299], dtype=torch.int32)
    n_eval[0, 7] = n_eval[2, 299] = 9
    want = EV.evidence_maps_torch(acc, bad, ends, n_eval, winner, 7, 10)
    got = EV.evidence_maps_hip(acc.to(DEV), bad.to(DEV), ends, n_eval.to(DEV), winner.to(DEV), 7, 10)
    for a, b in zip(got, want):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.isnan(got.mean_map[1]).all() and int(got.invalid.sum()) > 0 and torch.isfinite(got.mean_map[0]).any()


# ------------------------------------------------------------------------------------------------ end to end
UNET_CFG = dict(pred_param="eps", schedule="cosine", noise_d=32, image_size=32, cfg_w=0.0, ema_beta=0.999, ema_warmup=0,
                ema_update_freq=1, encoder_type="nn", classes=3, n_stages=2, evaluation_per_stage=[2, 4],
                n_keep_per_stage=[2, 1], n_fast_classes=2)
DIT_KW = dict(num_attention_heads=2, attention_head_dim=32, in_channels=4, num_layers=2, sample_size=16, patch_size=4, num_embeds_ada_norm=10)


def _backbones(kind, seed=0):
    """The HIP backbone and the CPU oracle backbone with the same weights (1-d parameters randomised as in test_gpu_model.py)."""
    torch.manual_seed(seed)
    m = dca.UNetCondition2D(**dca.small_unet_kwargs()) if kind == "unet" else dca.DiT(**DIT_KW)
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    o = oracle.OracleUNetCondition2D(**dca.small_unet_kwargs()) if kind == "unet" else oracle.OracleDiT(**DIT_KW)
    o.load_state_dict(m.state_dict())
    return m, o


def _cfg(kind, dtype, **over):
    cfg = dict(UNET_CFG, compute_dtype=dtype)
    if kind == "dit":
        cfg.update(encoder_type="DiT", image_size=16, noise_d=16)
    cfg.update(over)
    return cfg


def _pair(kind, dtype, **over):
    """(HIP classifier on the device, the same classifier on the CPU oracle backbone: the `_ForeignRunner` host path)."""
    m, o = _backbones(kind)
    cfg = _cfg(kind, dtype, **over)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg))
    host = dca.DiffusionClassifier(o, dca.Config(**cfg))
    if dc.encoder is not None:
        host.encoder.load_state_dict(dc.encoder.state_dict())
    return dc.to(DEV), host


def _draws(kind, BS=2, T=4):
    torch.manual_seed(1)
    C, S = (3, 32) if kind == "unet" else (4, 16)
    return torch.rand(BS, C, S, S) * 2 - 1, torch.rand(T, BS), torch.randn(T, BS, C, S, S)


def _on_dev(x, t, eps):
    return x.to(DEV), dict(t=t, eps=eps.to(DEV))


def _parity(ev, ref, label):
    """The project's f32 parity gate (1e-4) per pixel, relative to each cell's mean pixel value of the host path's map."""
    got_m, got_d, want_m, want_d = (v.cpu().double() for v in (ev.mean_map, ev.delta_map, ref.mean_map, ref.delta_map))
    assert torch.equal(torch.isnan(got_m), torch.isnan(want_m)) and torch.equal(torch.isnan(got_d), torch.isnan(want_d)), label
    assert torch.equal(ev.n_trials.cpu(), ref.n_trials) and torch.equal(ev.invalid.cpu(), ref.invalid), label
    scale = torch.nan_to_num(want_m).mean(dim=(2, 3), keepdim=True)
    fin = ~torch.isnan(want_m)
    em = float((((got_m - want_m).abs() / scale)[fin]).max())
    ed = float((((got_d - want_d).abs() / scale)[fin]).max())
    print(f"evidence parity {label}: mean_map {em:.3g} delta_map {ed:.3g} (gate 1e-4)")
    assert em <= 1e-4 and ed <= 1e-4, (label, em, ed)


@pytest.mark.parametrize("kind,dtype", [("unet", "f32"), ("unet", "bf16"), ("dit", "f32")])
def test_classify_with_the_flag(kind, dtype):
    dc, host = _pair(kind, dtype)
    x, t, eps = _draws(kind)
    xd, kw = _on_dev(x, t, eps)
    lab0, err0, post0 = dc.classify(xd, return_errors=True, return_posterior=True, **kw)
    plans_off = {k: sp["plan"].pb.nops for k, sp in dc._score_plans.items()}
    lab, err, post, ev = dc.classify(xd, return_errors=True, return_posterior=True, return_evidence=True, **kw)
    assert isinstance(ev, dca.ClassEvidence) and all(v.is_cuda for v in ev)
    # the flag leaves labels, errors and posterior alone, bit for bit, and costs exactly one op per plan
    assert torch.equal(lab, lab0) and torch.equal(_bits(err), _bits(err0))
    for a, b in zip(post, post0):
        assert torch.equal(_bits(a), _bits(b))
    plans_on = {k[:-1]: sp["plan"].pb.nops for k, sp in dc._score_plans.items() if k[-1] == "evidence"}
    assert sorted(plans_on) == sorted(plans_off) and len(plans_on) == 2
    assert all(plans_on[k] == plans_off[k] + 1 for k in plans_off)
    for sp in dc._score_plans.values():
        kinds = [k for k, _, _ in sp["plan"].pb.ops]
        assert kinds.count(L.OP_ERR_MAP) == (1 if "emap_acc" in sp["score"] else 0)
        if "emap_acc" in sp["score"]:
            assert kinds[-2:] == [L.OP_EPS_MSE, L.OP_ERR_MAP]
    BS, C = 2, 3
    H = W = x.shape[-1]
    assert tuple(ev.mean_map.shape) == tuple(ev.delta_map.shape) == (BS, C, H, W) and ev.mean_map.dtype == torch.float32
    assert torch.equal(ev.n_trials, post.n_trials) and ev.invalid.tolist() == [0, 0]
    assert all(sorted(r) == [2, 4, 4] for r in ev.n_trials.tolist())
    assert torch.isfinite(ev.mean_map).all() and torch.isfinite(ev.delta_map).all()
    assert (ev.delta_map[torch.arange(BS), lab] == 0).all()
    # two calls: the same bits; f32: also when every launch holds a single pair
    ev2 = dc.classify(xd, return_evidence=True, **kw)[1]
    for a, b in zip(ev, ev2):
        assert torch.equal(_bits(a), _bits(b))
    if dtype == "f32":
        dc3, _ = _pair(kind, dtype, units_per_launch=3)
        lab3, err3, ev3 = dc3.classify(xd, return_errors=True, return_evidence=True, **kw)
        assert {sp["n_bj"] for sp in dc3._score_plans.values()} == {1}
        assert torch.equal(lab3, lab) and torch.equal(_bits(err3), _bits(err))
        for a, b in zip(ev3, ev):
            assert torch.equal(_bits(a), _bits(b))
    # summed over the pixels the maps are the posterior's means and deltas (bound: evidence_oracle.pixel_sum_bound)
    _, winner, means, delta = P.class_posterior_hip(err.to(DEV), 4, 1.0, return_parts=True)
    means, delta, E = means.cpu().double(), delta.cpu().double(), err.double()
    sm, sd = ev.mean_map.cpu().double().sum(dim=(2, 3)), ev.delta_map.cpu().double().sum(dim=(2, 3))
    worst = 0.0
    for b in range(BS):
        for c in range(C):
            n = int(ev.n_trials[b, c])
            rel, ab = O.pixel_sum_bound(x.shape[1], H, W, n)
            mw = float(E[b, int(lab[b]), :n].sum()) / n
            bm, bd = rel * float(means[b, c]) + ab, rel * (float(means[b, c]) + mw) + 2 * ab
            worst = max(worst, abs(float(sm[b, c] - means[b, c])) / bm, abs(float(sd[b, c] - delta[b, c])) / bd)
            assert abs(float(sm[b, c] - means[b, c])) <= bm and abs(float(sd[b, c] - delta[b, c])) <= bd, (b, c, sm[b, c], means[b, c], sd[b, c], delta[b, c])
    print(f"evidence {kind} {dtype}: pixel sums against the posterior, worst error / bound = {worst:.3g}")
    if dtype == "f32":
        ref_lab, ref = host.classify(x, t=t, eps=eps, return_evidence=True)
        assert torch.equal(ref_lab, lab.cpu())
        _parity(ev, ref, f"{kind} f32")
    dc.check_device_errors()


def test_fast_mode_against_the_host_path():
    dc, host = _pair("unet", "f32", classes=4, n_stages=1, evaluation_per_stage=[3], n_keep_per_stage=[1])
    x, t, eps = _draws("unet", T=3)
    xd, kw = _on_dev(x, t, eps)
    text, sel = torch.tensor([2, 0]), torch.tensor([[1], [0]])
    lab, ev = dc.classify(xd, text.to(DEV), fast=True, fast_select=sel, return_evidence=True, **kw)
    ref_lab, ref = host.classify(x, text, fast=True, fast_select=sel, t=t, eps=eps, return_evidence=True)
    assert torch.equal(lab.cpu(), ref_lab)
    never = ev.n_trials.cpu() == 0
    assert int(never.sum()) == 4 and torch.isnan(ev.mean_map.cpu()[never]).all() and torch.isnan(ev.delta_map.cpu()[never]).all()
    assert torch.isfinite(ev.mean_map.cpu()[~never]).all()
    _parity(ev, ref, "fast")
    dc.check_device_errors()


def test_early_stopping_against_the_host_path():
    """Stages [2, 4, 6] keeping [3, 2, 1], BS 4, a threshold halfway between the second and the third largest z-score of the first
    checkpoint (so the last bits that differ between the two paths cannot move an image across it): two images stop at 2 trials."""
    over = dict(n_stages=3, evaluation_per_stage=[2, 4, 6], n_keep_per_stage=[3, 2, 1])
    dc, host = _pair("unet", "f32", **over)
    x, t, eps = _draws("unet", BS=4, T=6)
    xd, kw = _on_dev(x, t, eps)
    _, err = dc.classify(xd, return_errors=True, **kw)
    z = sorted(P.class_posterior_torch(err, 2).margin_z.tolist(), reverse=True)
    assert all(np.isfinite(z)) and z[1] > z[2]
    thr = 0.5 * (z[1] + z[2])
    dc.config.stop_margin_z = host.config.stop_margin_z = thr
    lab, post, ev, t_done = dc.classify(xd, return_posterior=True, return_evidence=True, return_trials=True, **kw)
    ref_lab, ref, ref_t = host.classify(x, t=t, eps=eps, return_evidence=True, return_trials=True)
    assert sorted(t_done.tolist())[:2] == [2, 2] and torch.equal(t_done.cpu(), ref_t) and torch.equal(lab.cpu(), ref_lab)
    assert torch.equal(ev.n_trials, post.n_trials) and (ev.delta_map[torch.arange(4), lab] == 0).all()
    assert (ev.n_trials.max(dim=1).values == t_done).all()
    _parity(ev, ref, "stop_margin_z")
    dc.check_device_errors()


# ------------------------------------------------------------------------------------------------ grid sharding
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(world, tmp_path):
    port = _free_port()
    outs = [str(tmp_path / f"evidence_w{world}_r{r}.npz") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    worker = os.path.join(HERE, "hip_evidence_shard_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), outs[r]], env=env) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    return [dict(np.load(o)) for o in outs]


def test_evidence_world_size_2_is_bit_identical_to_world_size_1(tmp_path):
    one = _launch(1, tmp_path)[0]
    two = _launch(2, tmp_path)
    assert one["mean_map"].shape == (2, 3, 32, 32) and np.isfinite(one["mean_map"]).all() and sorted(one["n_trials"][0].tolist()) == [2, 4, 4]
    for r in two:
        assert sorted(r) == sorted(one)
        for k in one:
            assert r[k].dtype == one[k].dtype
            np.testing.assert_array_equal(r[k].view(np.int32) if r[k].dtype == np.float32 else r[k],
                                          one[k].view(np.int32) if one[k].dtype == np.float32 else one[k])
