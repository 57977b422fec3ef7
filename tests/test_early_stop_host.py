"""CPU: per-image early stopping (config key `stop_margin_z`) — the torch statement of the stop rule against the sequential float32
loop, classify on the stand-in backbone against a reference-style loop over the active images, the goldens at "never stop", the
config refusals, the pair dealing over a subset of the images, a gloo run, and the C-ABI surface of the two new entry points."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import dist as D
from diffusion_classifier_amd import posterior as P
from helpers import load_case, standin_from
import early_stop_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _same_f32(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int32), b[~np.isnan(b)].view(np.int32))


# ------------------------------------------------------------------------------------------------ the stop rule
@pytest.mark.parametrize("t_end", [1, 2, 7])
@pytest.mark.parametrize("C", [1, 2, 3, 65])
@pytest.mark.parametrize("BS", [1, 5])
def test_stop_rule_torch_equals_the_sequential_loop(BS, C, t_end):
    stops = {False: 0, True: 0}
    for shift in range(O.ROW_KINDS if BS == 1 else 1):           # BS = 1: every kind of row gets its turn
        E = O.crafted_errors(BS, C, T=8, seed=3, shift=shift)
        for mode in ("all", "some", "none"):
            for z_stop in (0.5, 3.0, INF):
                t_done, labels = O.crafted_state(BS, t_end, mode)
                want = O.stop_rule_loop(E.numpy(), t_end, z_stop, t_done.numpy(), labels.numpy())
                ids, n, z = P.stop_rule_torch(E, t_end, z_stop, t_done, labels)
                assert ids.dtype == torch.int32 and n.dtype == torch.int32 and tuple(n.shape) == (1,) and z.dtype == torch.float32
                np.testing.assert_array_equal(t_done.numpy(), want[0])
                np.testing.assert_array_equal(labels.numpy(), want[1])
                np.testing.assert_array_equal(ids.numpy(), want[2])
                assert int(n) == want[3]
                assert _same_f32(z.numpy(), want[4]), (z, want[4])
                was = O.crafted_state(BS, t_end, mode)[0].numpy()
                assert np.array_equal(labels.numpy()[was != 0], np.full(int((was != 0).sum()), 7))     # decided rows are left alone
                for b in np.nonzero(was == 0)[0]:
                    stops[bool(t_done[b] != 0)] += 1
    if not (t_end == 1 and C > 1):
        assert stops[True] > 0
    assert stops[False] > 0


def test_stop_rule_torch_equals_the_loop_where_torch_takes_its_vector_paths():
    """64 images: torch's CPU kernels run whole vectors here (their fp32 sqrt is not the correctly rounded one in that path)."""
    E = O.crafted_errors(64, 3, T=8, seed=5)
    t_done, labels = O.crafted_state(64, 7, "some")
    want = O.stop_rule_loop(E.numpy(), 7, 3.0, t_done.numpy(), labels.numpy())
    ids, n, z = P.stop_rule_torch(E, 7, 3.0, t_done, labels)
    np.testing.assert_array_equal(t_done.numpy(), want[0])
    np.testing.assert_array_equal(labels.numpy(), want[1])
    np.testing.assert_array_equal(ids.numpy(), want[2])
    assert int(n) == want[3] and 0 < int(n) < 64 and _same_f32(z.numpy(), want[4])


def test_stop_rule_on_the_rows_by_name():
    E = O.crafted_errors(5, 3, T=8, seed=3)
    t_done, labels = O.crafted_state(5, 7, "all")
    ids, n, z = P.stop_rule_torch(E, 7, 1e-3, t_done, labels)
    post = P.class_posterior_torch(E, 7)
    assert _same_f32(z.numpy(), post.margin_z.numpy())               # the z-score the posterior reports
    assert torch.isfinite(z[0]) and t_done[0] == 7 and labels[0] == int(E[0, :, :7].sum(dim=1).argmin())
    assert torch.isfinite(z[1]) and t_done[1] == 7                   # a NaN cell in a loser, a pruned class: still decided on the two finalists
    assert torch.isnan(z[2]) and t_done[2] == 0 and labels[2] == -3  # an exact tie: 0 / 0
    assert z[3] == INF and t_done[3] == 7 and labels[3] == 3 % 3     # no runner-up stops
    assert torch.isnan(z[4]) and t_done[4] == 0                      # a NaN winner mean never stops
    assert ids.tolist() == [2, 4, -1, -1, -1] and int(n) == 2
    # t_end = 1: the variance is 0 / 0 — nobody with a runner-up stops, whatever the threshold
    t_done, labels = O.crafted_state(5, 1, "all")
    ids, n, z = P.stop_rule_torch(E, 1, 1e-30, t_done, labels)
    assert t_done.tolist() == [0, 0, 0, 1, 0] and int(n) == 4
    # +inf: only "no runner-up" reaches it
    t_done, labels = O.crafted_state(5, 7, "all")
    P.stop_rule_torch(E, 7, INF, t_done, labels)
    assert t_done.tolist() == [0, 0, 0, 7, 0]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            P.stop_rule_torch(E, 7, bad, t_done, labels)


def test_per_image_posterior_takes_each_row_at_its_own_t_end():
    E = O.crafted_errors(5, 3, T=8, seed=4, shift=0)
    t_done = torch.tensor([2, 7, 4, 7, 2], dtype=torch.int32)
    post, winner, means, delta = P.class_posterior_torch(E, t_done, 2.0, return_parts=True)
    for v in (2, 4, 7):
        ref, w, m, d = P.class_posterior_torch(E, v, 2.0, return_parts=True)
        pick = t_done == v
        for a, b in zip(tuple(post) + (winner, means, delta), tuple(ref) + (w, m, d)):
            assert _same_f32(a[pick].double().numpy(), b[pick].double().numpy())
    same = P.class_posterior_torch(E, t_done, 2.0, t_values=[2, 4, 7])
    for a, b in zip(post, same):
        assert _same_f32(a.double().numpy(), b.double().numpy())
    with pytest.raises(ValueError):
        P.class_posterior_torch(E, t_done[:3], 2.0)


# ------------------------------------------------------------------------------------------------ classify on the stand-in
def _median_first_checkpoint_z(dc, x, t, eps):
    lab, err = dc.classify(x, t=t, eps=eps, return_errors=True)
    z = P.class_posterior_torch(err, dc.config.evaluation_per_stage[0]).margin_z
    return lab, err, z, float(z.median())


def test_classify_on_the_standin_equals_the_reference_style_loop():
    dc, x, t, eps = O.standin_classifier(dca)
    T = 7
    lab0, err0, z, thr = _median_first_checkpoint_z(dc, x, t, eps)
    assert torch.isfinite(z).all() and len(set(z.tolist())) == 5, z
    dc.config.stop_margin_z = thr
    lab, err, post, t_done = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, return_trials=True)
    with torch.no_grad():
        want_lab, want_t, want_err, scored = O.reference_loop(dc, x, t, eps, thr)
    print("z at the first checkpoint", z.tolist(), "threshold", thr, "t_done", t_done.tolist())
    assert (t_done < T).any() and (t_done == T).any(), t_done                  # the precondition: somebody stops, somebody runs to T
    assert (t_done == 2).sum() >= 3                                            # the median and everything above it stop at the first look
    assert t_done.dtype == torch.int32 and lab.dtype == torch.int64 and tuple(t_done.shape) == (5,)
    np.testing.assert_array_equal(lab.numpy(), want_lab)
    np.testing.assert_array_equal(t_done.numpy(), want_t)
    assert np.array_equal(err.numpy().view(np.int32), want_err.numpy().view(np.int32))
    for b in range(5):
        assert torch.isinf(err[b, :, int(t_done[b]):]).all() and (err[b, :, int(t_done[b]):] > 0).all()
        assert torch.isfinite(err[b, :, :2]).all()
        assert torch.equal(err[b, :, :2], err0[b, :, :2])                      # the first stage ran on the full batches
        fin = post.n_trials[b] == t_done[b]
        assert fin.any() and post.n_trials[b].max() == t_done[b]               # the finalists have exactly the trials the image used
        ref = P.class_posterior_torch(err, int(t_done[b]))
        for a, r in zip(post, ref):
            assert _same_f32(a[b].double().numpy(), r[b].double().numpy())
    assert torch.equal(post.probs.argmax(dim=1), lab)
    assert scored == int(t_done.sum())
    # every shape and order of the return value
    kw = dict(t=t, eps=eps)
    assert torch.equal(dc.classify(x, **kw), lab)
    l2, td2 = dc.classify(x, return_trials=True, **kw)
    l3, p3, td3 = dc.classify(x, return_posterior=True, return_trials=True, **kw)
    l4, e4, td4 = dc.classify(x, return_errors=True, return_trials=True, **kw)
    l5, e5 = dc.classify(x, return_errors=True, **kw)
    for l_ in (l2, l3, l4, l5):
        assert torch.equal(l_, lab)
    for td in (td2, td3, td4):
        assert torch.equal(td, t_done)
    assert isinstance(p3, dca.ClassPosterior) and torch.equal(e4, err) and torch.equal(e5, err)
    # the key unset: return_trials reports T for everybody
    dc.config.stop_margin_z = None
    l6, td6 = dc.classify(x, return_trials=True, **kw)
    assert torch.equal(l6, lab0) and td6.tolist() == [T] * 5 and td6.dtype == torch.int32


def test_everybody_stops_at_the_first_checkpoint_and_the_later_stages_are_skipped():
    dc, x, t, eps = O.standin_classifier(dca, stop_margin_z=1e-6)
    calls = []
    bb = dc.ema.ema_model
    bb.register_forward_hook(lambda *a: calls.append(1))
    lab, err, t_done = dc.classify(x, t=t, eps=eps, return_errors=True, return_trials=True)
    assert t_done.tolist() == [2] * 5 and len(calls) == 2 * 3
    assert torch.isinf(err[:, :, 2:]).all() and torch.isfinite(err[:, :, :2]).all()
    assert torch.equal(lab, P.class_posterior_torch(err, 2, return_parts=True)[1])


@pytest.mark.parametrize("name", ["1stage_eps", "2stage_pruned", "fast"])
def test_never_stopping_reproduces_the_goldens(name):
    def run(**extra):
        g, cfg = load_case(name)
        dc = dca.DiffusionClassifier(standin_from(g, cfg), dca.Config(**dict(cfg, **extra)))
        if dc.encoder is not None:
            dc.encoder.weight.data.copy_(torch.from_numpy(g["encoder.weight"]))
        fast = bool(g["fast"])
        kw = dict(fast=fast, t=torch.from_numpy(g["t"]), eps=torch.from_numpy(g["eps"]),
                  fast_select=torch.from_numpy(g["fast_select"]) if fast else None)
        lab = torch.from_numpy(g["labels"]) if fast else None
        return g, dc.classify(torch.from_numpy(g["x"]), lab, return_errors=True, return_posterior=True, return_trials=True, **kw)
    g, (out, err, post, t_done) = run(stop_margin_z=INF)
    _, (out0, err0, post0, t_done0) = run()
    np.testing.assert_array_equal(out.numpy(), g["out"])
    np.testing.assert_array_equal(err.numpy(), g["errors"])
    assert torch.equal(t_done, t_done0) and (t_done == err.shape[2]).all()
    for a, b in zip(post, post0):
        assert _same_f32(a.double().numpy(), b.double().numpy())


# ------------------------------------------------------------------------------------------------ config
@pytest.mark.parametrize("bad", [0, -1, float("nan"), "x"])
def test_a_bad_threshold_is_refused_at_the_top_of_classify(bad):
    dc, x, t, eps = O.standin_classifier(dca, stop_margin_z=bad)
    dc.ema.ema_model.register_forward_hook(lambda *a: pytest.fail("the backbone ran"))
    with pytest.raises(ValueError):
        dc.classify(x, t=t, eps=eps)


def test_stopping_with_simulate_rank_is_refused():
    dc, x, t, eps = O.standin_classifier(dca, stop_margin_z=2.0, simulate_rank=(0, 2))
    with pytest.raises(ValueError):
        dc.classify(x, t=t, eps=eps)
    assert P.stop_margin_of(dca.Config()) is None and P.stop_margin_of(dca.Config(stop_margin_z=INF)) == INF
    assert P.stop_margin_of(dca.Config(stop_margin_z=2)) == 2.0


# ------------------------------------------------------------------------------------------------ dist
@pytest.mark.parametrize("rows", [[0], [1, 3, 4], [0, 1, 2, 3, 4]])
def test_pairs_over_a_subset_are_a_balanced_partition(rows):
    BS, s0, s1 = 5, 2, 7
    want = [p for p in D.stage_pairs(s0, s1, BS) if p[1] in rows]
    for world in range(1, 6):
        got = [D.local_pairs_rows(s0, s1, rows, r, world) for r in range(world)]
        assert sorted(sum(got, [])) == sorted(want)
        assert [p for i in range(len(want)) for p in got[i % world][i // world:i // world + 1]] == want      # dealt round-robin in trial-major order
        sizes = [len(x) for x in got]
        assert max(sizes) - min(sizes) <= 1 and max(sizes) == D.slab_len(s0, s1, len(rows), world)
        if len(rows) == BS:
            assert got == [D.local_pairs(s0, s1, BS, r, world) for r in range(world)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _between(z, k):
    """A threshold strictly between the k-th and the (k+1)-th largest z-score: a last-bit difference between batch compositions
    (CPU kernels; the ranks score other sub-batches than one process does) cannot move an image across it."""
    s = sorted(z.tolist(), reverse=True)
    return 0.5 * (s[k - 1] + s[k])


def _worker(rank, world, port, thr, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import diffusion_classifier_amd as dca_
    import early_stop_oracle as O_
    dc, x, t, eps = O_.standin_classifier(dca_, stop_margin_z=thr, shard_grid=True)
    lab, err, post, t_done = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, return_trials=True)
    q.put((rank, lab.numpy(), err.numpy(), t_done.numpy(), post.n_trials.numpy()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_classify_with_stopping_equals_the_single_process(world):
    dc, x, t, eps = O.standin_classifier(dca)
    _, _, z, _ = _median_first_checkpoint_z(dc, x, t, eps)
    thr = _between(z, 3)
    dc.config.stop_margin_z = thr
    lab, err, post, t_done = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, return_trials=True)
    assert (t_done < 7).any() and (t_done == 7).any()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, thr, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == list(range(world))
    for rank, lab_r, err_r, t_r, n_r in res:
        np.testing.assert_array_equal(lab_r, lab.numpy())
        np.testing.assert_array_equal(t_r, t_done.numpy())                      # the ranks agree on t_done (each equals the single process)
        np.testing.assert_array_equal(n_r, post.n_trials.numpy())
        np.testing.assert_array_equal(err_r, res[0][2])                         # every rank holds the same errors, bit for bit
        fin = np.isfinite(err.numpy())
        assert np.array_equal(np.isfinite(err_r), fin)
        np.testing.assert_allclose(err_r[fin], err.numpy()[fin], rtol=3e-7)     # sub-batches differ from the single process's batches


# ------------------------------------------------------------------------------------------------ C-ABI
def test_both_symbols_are_exported_and_declared_and_the_abi_version_stays():
    src = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    lib = L.lib()
    for name in ("dc_stage_stop", "dc_stage_maps_rows"):
        assert name in L.EXPORTS and getattr(lib, name) is not None
        assert re.search(r"\bint %s\(" % name, src)
    assert lib.dc_abi_version() == 5 and L.ABI_VERSION == 5
    assert re.search(r"#define DC_ABI_VERSION 5\b", src)


def _stop_args(**over):
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    kw = dict(errors=a, BS=1, C=2, T=2, t_end=2, z_stop=2.0, t_done=a, labels=a, active_ids=a, n_active=a, margin_z=None)
    kw.update(over)
    return [kw[k] for k in ("errors", "BS", "C", "T", "t_end", "z_stop", "t_done", "labels", "active_ids", "n_active", "margin_z")] + [None], buf


@pytest.mark.parametrize("over,code,word", [
    (dict(errors=None), -1, "null"), (dict(t_done=None), -1, "null"), (dict(labels=None), -1, "null"),
    (dict(active_ids=None), -1, "null"), (dict(n_active=None), -1, "null"),
    (dict(z_stop=0.0), -1, "z_stop"), (dict(z_stop=-1.0), -1, "z_stop"), (dict(z_stop=float("nan")), -1, "z_stop"),
    (dict(BS=0), -2, "BS=0"), (dict(C=1025), -2, "C=1025"), (dict(T=2, t_end=3), -2, "t_end=3"), (dict(t_end=0), -2, "t_end=0"),
])
def test_stage_stop_refuses_before_any_launch(over, code, word):
    lib = L.lib()
    args, _keep = _stop_args(**over)
    assert lib.dc_stage_stop(*args) == code
    assert word in lib.dc_last_error().decode()


def _maps_args(**over):
    buf = (ctypes.c_int32 * 64)()
    a = ctypes.addressof(buf)
    kw = dict(keep=a, rows=a, n_rows=3, BS=5, C=4, T=6, k=2, t0=2, n_pairs=6, rank=0, world=1, n_bj=4, n_mb=2, dump=120, maps=a)
    kw.update(over)
    order = ("keep", "rows", "n_rows", "BS", "C", "T", "k", "t0", "n_pairs", "rank", "world", "n_bj", "n_mb", "dump", "maps")
    return [kw[k] for k in order] + [None], buf


@pytest.mark.parametrize("over,code,word", [
    (dict(keep=None), -1, "null"), (dict(rows=None), -1, "null"), (dict(maps=None), -1, "null"),
    (dict(n_rows=0), -2, "rows=0"), (dict(n_rows=6), -2, "rows=6"), (dict(k=5), -2, "k=5"), (dict(rank=1), -2, "rank=1/1"),
    (dict(n_mb=1), -2, "n_mb=1"), (dict(n_mb=3), -2, "n_mb=3"), (dict(t0=6), -2, "t0=6"),
    (dict(n_pairs=13, n_mb=4), -2, "beyond trial"), (dict(BS=1 << 20, C=1 << 10, T=1 << 10, t0=0), -2, "too large"),
])
def test_stage_maps_rows_refuses_before_any_launch(over, code, word):
    lib = L.lib()
    args, _keep = _maps_args(**over)
    assert lib.dc_stage_maps_rows(*args) == code
    assert word in lib.dc_last_error().decode()
