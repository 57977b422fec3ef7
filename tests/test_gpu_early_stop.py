"""GPU: per-image early stopping (config key `stop_margin_z`) — dc_stage_stop against posterior.stop_rule_torch bit for bit,
dc_stage_maps_rows against host-built control blocks, classify with stopping on the small UNet / DiT against the unstopped run with
the same draws, the index-cache key, and a two-rank run on one GPU."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import dist as D
from diffusion_classifier_amd import posterior as P
from diffusion_classifier_amd.diffusion import diffusion_classifier as DCM
import early_stop_oracle as O
from helpers import expected_unit_maps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
INF = float("inf")


def _bits(v):
    v = v.detach().cpu().contiguous()
    return v.view(torch.int32) if v.dtype == torch.float32 else v


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ dc_stage_stop
def _kernel_stop(E, t_end, z_stop, t_done, labels):
    """dc_stage_stop with a marked margin_z buffer: rows the kernel must not touch keep the mark."""
    BS, C, T = E.shape
    Ed, td, lb = E.to(DEV).contiguous(), t_done.to(DEV), labels.to(DEV)
    out = torch.full((BS + 1,), -9, dtype=torch.int32, device=DEV)
    z = torch.full((BS,), -5.0, device=DEV)
    L.check(L.lib().dc_stage_stop(Ed.data_ptr(), BS, C, T, t_end, z_stop, td.data_ptr(), lb.data_ptr(), out.data_ptr(), out[BS:].data_ptr(),
                                  z.data_ptr(), L.stream_ptr()), "dc_stage_stop")
    torch.cuda.synchronize()
    return td.cpu(), lb.cpu(), out[:BS].cpu(), int(out[BS]), z.cpu(), Ed


@pytest.mark.parametrize("t_end", [1, 2, 7])
@pytest.mark.parametrize("C", [1, 2, 10, 65])
@pytest.mark.parametrize("BS", [1, 3, 64, 65, 300])
def test_stage_stop_equals_the_torch_statement_bit_for_bit(BS, C, t_end):
    for shift in range(O.ROW_KINDS if BS == 1 else 1):
        E = O.crafted_errors(BS, C, T=8, seed=5, shift=shift)
        post_z = None
        for mode in ("all", "some", "none"):
            for z_stop in (0.5, 3.0, INF):
                t0, l0 = O.crafted_state(BS, t_end, mode)
                t_ref, l_ref = t0.clone(), l0.clone()
                ids_ref, n_ref, z_ref = P.stop_rule_torch(E, t_end, z_stop, t_ref, l_ref)
                td, lb, ids, n, z, Ed = _kernel_stop(E, t_end, z_stop, t0, l0)
                assert torch.equal(td, t_ref) and torch.equal(lb, l_ref)
                assert torch.equal(ids, ids_ref) and n == int(n_ref)
                if post_z is None:
                    post_z = P.class_posterior_hip(Ed, t_end).margin_z.cpu()
                act = t0 == 0
                assert _same(z[act], post_z[act])                              # the z-score dc_class_posterior reports, the same bits
                assert _same(z[act], z_ref[act])                               # and the torch statement's
                assert (z[~act] == -5.0).all() and (lb[~act] == 7).all() and torch.equal(td[~act], t0[~act])     # decided rows: untouched
                if mode == "none":
                    assert n == 0 and (ids == -1).all()


def test_stage_stop_is_the_same_from_launch_to_launch_and_refuses_bad_arguments():
    E = O.crafted_errors(300, 10, T=8, seed=6)
    t0, l0 = O.crafted_state(300, 7, "some")
    a = _kernel_stop(E, 7, 1.5, t0, l0)
    b = _kernel_stop(E, 7, 1.5, t0, l0)
    for u, v in zip(a[:5], b[:5]):
        assert u == v if isinstance(u, int) else _same(u, v)
    assert a[2][:a[3]].tolist() == sorted(a[2][:a[3]].tolist()) and (a[2][a[3]:] == -1).all()
    Ed = a[5]
    td, lb = t0.to(DEV), l0.to(DEV)
    out = torch.zeros(301, dtype=torch.int32, device=DEV)
    lib = L.lib()
    args = lambda **o: [o.get("E", Ed.data_ptr()), 300, o.get("C", 10), 8, o.get("t_end", 7), o.get("z", 2.0), td.data_ptr(), lb.data_ptr(),
                        out.data_ptr(), out[300:].data_ptr(), None, L.stream_ptr()]
    assert lib.dc_stage_stop(*args(z=0.0)) == -1 and lib.dc_stage_stop(*args(E=None)) == -1
    assert lib.dc_stage_stop(*args(t_end=9)) == -2 and lib.dc_stage_stop(*args(C=1025)) == -2
    L.check(lib.dc_stage_stop(*args()), "dc_stage_stop")                        # margin_z is optional
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ dc_stage_maps_rows
@pytest.mark.parametrize("world,rank", [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
def test_stage_maps_rows_match_the_host_built_control_blocks(world, rank):
    """The index arithmetic classify does on the host for stage 0 (scoring.py `index_blocks`, from _HipRunner.run_stage), over the images
    rows = [1, 3, 4] of 5; every n_mb * n_bj leaves a padded tail."""
    BS, Cn, T, k, t0, t1, n_bj = 5, 9, 12, 2, 4, 12, 7
    rows = [1, 3, 4]
    torch.manual_seed(43)
    keep = torch.stack([torch.randperm(Cn)[:k] for _ in range(BS)]).to(torch.int32)
    pairs = D.local_pairs_rows(t0, t1, rows, rank, world)
    n_mb = -(-len(pairs) // n_bj)
    assert n_mb * n_bj > len(pairs)
    U, dump = n_bj * k, BS * Cn * T
    maps = torch.full((n_mb, 2 * U), -7, dtype=torch.int32, device=DEV)
    kd, rd = keep.to(DEV), torch.tensor(rows, dtype=torch.int32, device=DEV)
    L.check(L.lib().dc_stage_maps_rows(kd.data_ptr(), rd.data_ptr(), len(rows), BS, Cn, T, k, t0, len(pairs), rank, world, n_bj, n_mb, dump,
                                       maps.data_ptr(), L.stream_ptr()), "dc_stage_maps_rows")
    got = maps.cpu()
    cl, oi = expected_unit_maps(pairs, keep, n_bj, Cn, T, dump)
    for m in range(n_mb):
        assert torch.equal(got[m, :U].long(), cl[m]) and torch.equal(got[m, U:].long(), oi[m])
    if world == 1:
        # all images as rows: dc_stage_maps; an id outside [0, BS) is clamped, not followed
        allr = torch.arange(BS, dtype=torch.int32, device=DEV)
        pa = D.local_pairs(t0, t1, BS, 0, 1)
        nm = -(-len(pa) // n_bj)
        a = torch.empty((nm, 2 * U), dtype=torch.int32, device=DEV)
        b = torch.empty_like(a)
        L.check(L.lib().dc_stage_maps_rows(kd.data_ptr(), allr.data_ptr(), BS, BS, Cn, T, k, t0, len(pa), 0, 1, n_bj, nm, dump, a.data_ptr(),
                                           L.stream_ptr()), "dc_stage_maps_rows")
        L.check(L.lib().dc_stage_maps(kd.data_ptr(), BS, Cn, T, k, t0, len(pa), 0, 1, n_bj, nm, dump, b.data_ptr(), L.stream_ptr()), "dc_stage_maps")
        assert torch.equal(a, b)
        bad = torch.tensor([-4, 99], dtype=torch.int32, device=DEV)
        c = torch.empty((1, 2 * 2 * k), dtype=torch.int32, device=DEV)
        L.check(L.lib().dc_stage_maps_rows(kd.data_ptr(), bad.data_ptr(), 2, BS, Cn, T, k, t0, 2, 0, 1, 2, 1, dump, c.data_ptr(), L.stream_ptr()),
                "dc_stage_maps_rows")
        oi = c.cpu()[0, 2 * k:]
        assert (oi >= 0).all() and (oi < dump).all()


# ------------------------------------------------------------------------------------------------ end to end
STAGES = dict(classes=3, n_stages=3, evaluation_per_stage=[2, 4, 7], n_keep_per_stage=[3, 2, 1])
BASE = dict(pred_param="eps", schedule="cosine", noise_d=32, image_size=32, cfg_w=0.0, ema_beta=0.999, ema_warmup=0,
            ema_update_freq=1, encoder_type="nn", n_fast_classes=2, units_per_launch=4, **STAGES)
ENDS = [2, 4, 7]
# seeds at which the draws satisfy the tests' precondition (asserted below): distinct finite z-scores at the first checkpoint, an
# image that stops early and one that runs to T at the median threshold
SEED = {"unet": 0, "dit": 0}


def _unet(dtype, **over):
    torch.manual_seed(SEED["unet"])
    dc = dca.DiffusionClassifier(dca.UNetCondition2D(**dca.small_unet_kwargs()), dca.Config(**dict(BASE, compute_dtype=dtype, **over))).to(DEV)
    torch.manual_seed(SEED["unet"] + 1)
    BS, T = 5, 7
    return dc, (torch.rand(BS, 3, 32, 32) * 2 - 1).to(DEV), torch.rand(T, BS), torch.randn(T, BS, 3, 32, 32).to(DEV)


def _dit(**over):
    kw = dict(num_attention_heads=2, attention_head_dim=32, in_channels=4, num_layers=2, sample_size=16, patch_size=4, num_embeds_ada_norm=10)
    torch.manual_seed(SEED["dit"])
    m = dca.DiT(**kw)
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    cfg = dict(BASE, encoder_type="DiT", image_size=16, noise_d=16, compute_dtype="f32", **over)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg)).to(DEV)
    torch.manual_seed(SEED["dit"] + 1)
    BS, T = 5, 7
    return dc, (torch.rand(BS, 4, 16, 16) * 2 - 1).to(DEV), torch.rand(T, BS), torch.randn(T, BS, 4, 16, 16).to(DEV)


def _count_pairs(monkeypatch):
    seen = []
    orig = DCM._HipRunner.run_stage

    def wrapped(self, pairs, *a, **kw):
        seen.append(len(pairs))
        return orig(self, pairs, *a, **kw)
    monkeypatch.setattr(DCM._HipRunner, "run_stage", wrapped)
    return seen


def _check_stopping_run(dc, x, kw, monkeypatch, label):
    """One unstopped and one stopped classify with the same draws; the checks of the stopped one against the other."""
    T = ENDS[-1]
    lab0, err0 = dc.classify(x, return_errors=True, **kw)
    z = P.class_posterior_hip(err0.to(DEV), ENDS[0]).margin_z.cpu()
    thr = float(z.median())
    dc.config.stop_margin_z = thr
    seen = _count_pairs(monkeypatch)
    lab, err, post, t_done = dc.classify(x, return_errors=True, return_posterior=True, return_trials=True, **kw)
    td = t_done.cpu()
    print(f"early stop {label}: z = {z.tolist()} threshold = {thr} t_done = {td.tolist()} launches of pairs = {seen}")
    assert torch.isfinite(z).all() and len(set(z.tolist())) == 5, z                       # the precondition of the test
    assert (td < T).any() and (td == T).any(), td
    assert t_done.is_cuda and t_done.dtype == torch.int32 and lab.dtype == torch.int64
    for b in range(5):
        n = int(td[b])
        assert _same(err[b, :, :n], err0[b, :, :n])                                       # the same bits as without stopping
        assert (err[b, :, n:] == INF).all()
    # the rule replayed stage by stage on the unstopped run's errors
    t_ref, l_ref = torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)
    for e in ENDS[:-1]:
        P.stop_rule_torch(err0, e, thr, t_ref, l_ref)
    l_ref = torch.where(t_ref == 0, lab0.cpu(), l_ref)
    t_ref = torch.where(t_ref == 0, torch.full_like(t_ref, T), t_ref)
    assert torch.equal(td, t_ref) and torch.equal(lab.cpu(), l_ref)
    # the posterior of every image at its own number of trials
    for v in sorted(set(td.tolist())):
        ref = P.class_posterior_hip(err.to(DEV), v, P.temperature_of(dc.config))
        for a, r in zip(post, ref):
            assert _same(a[td == v], r[td == v])
    assert torch.equal(post.probs.argmax(dim=1), lab)
    assert sum(seen) == int(td.sum())                                                     # only the undecided images were scored
    dc.check_device_errors()
    return td


@pytest.mark.parametrize("rng", ["reference", "philox"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_small_unet_stops_images_and_keeps_every_scored_cell(dtype, rng, monkeypatch):
    dc, x, t, eps = _unet(dtype)
    kw = dict(t=t, eps=eps) if rng == "reference" else dict(t=t, rng="philox", seed=31)
    _check_stopping_run(dc, x, kw, monkeypatch, f"unet {dtype} {rng}")


def test_small_dit_stops_images_and_keeps_every_scored_cell(monkeypatch):
    dc, x, t, eps = _dit()
    _check_stopping_run(dc, x, dict(t=t, eps=eps), monkeypatch, "dit f32")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_never_stopping_is_bit_identical_to_the_key_unset(dtype):
    dc, x, t, eps = _unet(dtype, posterior_temperature=20.0)
    lab0, err0, post0 = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True)
    dc.config.stop_margin_z = INF
    lab, err, post, t_done = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, return_trials=True)
    assert torch.equal(lab, lab0) and _same(err, err0) and t_done.tolist() == [7] * 5
    for a, b in zip(post, post0):
        assert _same(a, b)


def test_two_image_subsets_with_the_same_ends_do_not_share_cached_indices():
    """Pair lists over the images {0, 2, 4} and {0, 3, 4}: the same trials, length, first and last pair, on one plan."""
    dc, x, t, eps = _unet("f32", units_per_launch=64, n_stages=1, evaluation_per_stage=[7], n_keep_per_stage=[1])     # every cell is scored
    BS, T, ncls = 5, 7, 3
    lab0, err0 = dc.classify(x, t=t, eps=eps, return_errors=True)
    lam = torch.stack([dc.schedule(t[j].clone()) for j in range(T)])
    draws = dict(logsnr=lam, alpha=torch.stack([torch.sqrt(torch.sigmoid(lam[j].clone())) for j in range(T)]),     # row by row, as classify
                 sigma=torch.stack([torch.sqrt(torch.sigmoid(-lam[j].clone())) for j in range(T)]),
                 eps_of={j: eps[j] for j in range(T)}, philox=False, seed=0)
    classes = torch.arange(ncls).repeat(BS, 1)
    plans = []
    for rows, other in (([0, 2, 4], [1, 3]), ([0, 3, 4], [1, 2])):
        runner = DCM._HipRunner(dc, dc.ema.ema_model, x, T, draws)
        pairs = D.local_pairs_rows(0, T, rows, 0, 1)
        assert len(pairs) == 21 and pairs[0] == (0, 0) and pairs[-1] == (6, 4)
        runner.run_stage(pairs, classes, stage=(0, 0, 1), rows=rows)
        got = runner.errors().cpu()
        assert _same(got[rows], err0[rows]), rows
        assert (got[other] == INF).all()
        plans.append(id(runner.err_dev))
    assert plans[0] == plans[1]                                                           # one plan served both calls


# ------------------------------------------------------------------------------------------------ grid sharding
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(world, thr, tmp_path):
    port = _free_port()
    outs = [str(tmp_path / f"early_stop_w{world}_r{r}.npz") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    worker = os.path.join(HERE, "hip_early_stop_shard_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), outs[r], repr(thr)], env=env) for r in range(world)]
    try:
        for p in procs:
            assert p.wait(timeout=240) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [dict(np.load(o)) for o in outs]


def test_stopping_at_world_size_2_is_bit_identical_to_world_size_1(tmp_path):
    one = _launch(1, 0.0, tmp_path)[0]
    thr = float(one["thr"][0])
    assert (one["t_done"] < 7).any() and (one["t_done"] == 7).any(), one["t_done"]
    two = _launch(2, thr, tmp_path)
    for r in two:
        assert sorted(r) == sorted(one)
        for k in one:
            assert r[k].dtype == one[k].dtype
            np.testing.assert_array_equal(r[k].view(np.int32) if r[k].dtype == np.float32 else r[k],
                                          one[k].view(np.int32) if one[k].dtype == np.float32 else one[k])
