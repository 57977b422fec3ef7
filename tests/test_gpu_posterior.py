"""GPU: dc_class_posterior against the float64 oracle (tests/posterior_oracle.py, which also holds the tolerances and their
derivation), its agreement with dc_reduce_argmin, and classify(return_posterior=True) on the HIP backbone, unsharded and sharded."""
import ctypes
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import posterior as P
from helpers import load_case
import posterior_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


def _golden(name):
    E = torch.from_numpy(load_case(name)[0]["errors"])
    return E, E.shape[2]


CASES = {
    "golden_2stage_pruned": lambda: _golden("2stage_pruned"),           # (5, 10, 10, 10)
    "golden_fast": lambda: _golden("fast"),                             # (5, 6, 5, 5)
    "golden_1stage_eps": lambda: _golden("1stage_eps"),                 # (5, 4, 6, 6)
    "t_end_1": lambda: (O.random_case(3, 2, 1, 1, seed=11), 1),
    "wrap_tail": lambda: (O.random_case(2, 65, 7, 5, seed=11), 5),      # classes wrap the lane stride; NaN / 1e30 behind t_end
    "three_rounds": lambda: (O.random_case(2, 130, 3, 3, seed=11), 3),
    "max_classes": lambda: (O.random_case(1, 1024, 2, 2, seed=11), 2),
    "synthetic": lambda: (O.synthetic_rows(), O.SYNTH_T_END),
}


def _argmin(E, t_end):
    BS, C, T = E.shape
    lab = torch.empty(BS, dtype=torch.int64, device=DEV)
    means = torch.empty((BS, C), dtype=torch.float32, device=DEV)
    L.check(L.lib().dc_reduce_argmin(E.data_ptr(), BS, C, T, t_end, lab.data_ptr(), means.data_ptr(), L.stream_ptr()), "dc_reduce_argmin")
    return lab.cpu(), means.cpu()


def _bits(v):
    v = v.cpu().contiguous()
    return v.view(torch.int32) if v.dtype == torch.float32 else v


@pytest.mark.parametrize("tau", [1.0, 0.5, 20.0])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_oracle(name, tau):
    E, t_end = CASES[name]()
    assert E.shape[2] >= t_end
    Ed = E.to(DEV).contiguous()
    post, winner, means, delta = P.class_posterior_hip(Ed, t_end, tau, return_parts=True)
    post2, winner2, means2, delta2 = P.class_posterior_hip(Ed, t_end, tau, return_parts=True)
    torch.cuda.synchronize()
    measured = O.check_against_oracle(E, t_end, tau, post, winner, means, delta, label=name)
    print(f"posterior {name} tau={tau}: " + " ".join(f"{k}={v:.3g}" for k, v in measured.items()))
    # two launches: the same bits
    for a, b in zip(tuple(post) + (winner, means, delta), tuple(post2) + (winner2, means2, delta2)):
        assert torch.equal(_bits(a), _bits(b))
    # the label's own kernel: the same winner, and bitwise the same means for the finalists (same operations, same order)
    lab, amean = _argmin(Ed, t_end)
    fin = post.n_trials.cpu() == t_end
    sure = fin.any(dim=1) & ~torch.isnan(post.probs[:, 0].cpu())      # (all finalists NaN: the label's key prefers a pruned class's +inf)
    assert torch.equal(winner.cpu().long()[sure], lab[sure])
    assert torch.equal(_bits(means)[fin], _bits(amean)[fin])
    if name.startswith("golden"):
        out = torch.from_numpy(load_case(name[7:])[0]["out"]).long()
        assert torch.equal(winner.cpu().long(), out) and torch.equal(post.probs.argmax(dim=1).cpu(), out)
        assert float(delta[torch.isfinite(delta)].min()) == 0.0      # (a class never scored has no delta: NaN)


def test_kernel_ignores_cells_behind_t_end():
    E, t_end = CASES["wrap_tail"]()
    assert not torch.isfinite(E[:, :, t_end:]).all()
    E2 = E.clone()
    E2[:, :, t_end:] = 3.0
    a = P.class_posterior_hip(E.to(DEV), t_end, 1.0, return_parts=True)
    b = P.class_posterior_hip(E2.to(DEV), t_end, 1.0, return_parts=True)
    for u, v in zip(tuple(a[0]) + a[1:], tuple(b[0]) + b[1:]):
        assert torch.equal(_bits(u), _bits(v))


def test_kernel_synthetic_rows_by_name():
    E = O.synthetic_rows().to(DEV)
    post, winner, means, delta = P.class_posterior_hip(E, O.SYNTH_T_END, 1.0, return_parts=True)
    post = dca.ClassPosterior(*(v.cpu() for v in post))
    winner, inf = winner.cpu(), float("inf")
    assert winner.tolist() == [0, 1, -1, 0, 0, 0, 0] and post.runner_up.tolist() == [1, -1, -1, 2, 2, 1, 1]
    assert post.probs[0, 0] == post.probs[0, 1] and post.margin[0] == 0
    assert post.margin[1] == inf and post.margin_z[1] == inf
    assert torch.isnan(post.probs[2]).all() and all(math.isnan(float(v[2])) for v in (post.entropy, post.margin, post.margin_z))
    assert post.probs[3, 1] == 0 and post.invalid.tolist() == [0, 0, 0, 1, 0, 0, 2]
    E3 = E[3:4].clone()
    E3[0, 1] = inf
    ref = P.class_posterior_hip(E3, O.SYNTH_T_END, 1.0)
    assert torch.equal(_bits(ref.probs[0]), _bits(post.probs[3])) and float(ref.margin[0]) == float(post.margin[3])
    assert post.probs[4, 1] == 0 and torch.isfinite(post.entropy[4]) and post.entropy[4] > 0
    assert delta.cpu()[5, 2] == -2.0 and post.probs[5].argmax() == 2
    assert torch.isnan(post.probs[6]).all()


def test_kernel_refuses_bad_arguments_with_a_device_present():
    E = torch.zeros(1, 2, 2, device=DEV)
    with pytest.raises(ValueError):
        P.class_posterior_hip(E, 3, 1.0)
    with pytest.raises(ValueError):
        P.class_posterior_hip(E, 2, 0.0)
    p = L.ClassPosteriorParams(errors=E.data_ptr(), probs=E.data_ptr(), entropy=E.data_ptr(), margin=E.data_ptr(), margin_z=E.data_ptr(),
                               winner=E.data_ptr(), runner=E.data_ptr(), invalid=E.data_ptr(), BS=1, C=1025, T=2, t_end=2, temperature=1.0)
    assert L.lib().dc_class_posterior(ctypes.byref(p), L.stream_ptr()) == -2


# ------------------------------------------------------------------------------------------------ end to end
def _dc(dtype, **over):
    cfg = dict(pred_param="eps", schedule="cosine", noise_d=32, image_size=32, cfg_w=0.0, ema_beta=0.999, ema_warmup=0,
               ema_update_freq=1, encoder_type="nn", classes=3, n_stages=2, evaluation_per_stage=[2, 4],
               n_keep_per_stage=[2, 1], n_fast_classes=2, compute_dtype=dtype)
    cfg.update(over)
    torch.manual_seed(0)
    return dca.DiffusionClassifier(dca.UNetCondition2D(**dca.small_unet_kwargs()), dca.Config(**cfg)).to(DEV)


def _draws(BS=2, T=4):
    torch.manual_seed(1)
    return (torch.rand(BS, 3, 32, 32) * 2 - 1).to(DEV), torch.rand(T, BS), torch.randn(T, BS, 3, 32, 32).to(DEV)


@pytest.mark.parametrize("dtype,fast,tau", [("f32", False, None), ("bf16", False, 20.0), ("f32", True, None)])
def test_classify_returns_the_posterior_of_its_own_errors(dtype, fast, tau):
    dc = _dc(dtype, **({} if tau is None else {"posterior_temperature": tau}))
    x, t, eps = _draws()
    kw = dict(t=t, eps=eps)
    text = None
    if fast:
        text, kw = torch.tensor([2, 0]), dict(kw, fast=True, fast_select=torch.tensor([[1], [0]]))
    plain = dc.classify(x, text, **kw)
    lab, err, post = dc.classify(x, text, return_errors=True, return_posterior=True, **kw)
    lab2, post2 = dc.classify(x, text, return_posterior=True, **kw)
    assert isinstance(post, dca.ClassPosterior) and all(v.is_cuda for v in post)
    assert torch.equal(lab, plain) and torch.equal(lab2, plain)
    for a, b in zip(post, post2):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(post.probs.argmax(dim=1), lab)
    n = post.n_trials.cpu()
    if fast:
        assert sorted(n[0].tolist()) == [0, 4, 4] and n[0, 2] == 4 and n[1, 0] == 4       # the true class and one drawn wrong class, both kept by stage 0
    else:
        assert all(sorted(row) == [2, 4, 4] for row in n.tolist())                        # the pruned class at 2, the finalists at 4
    _, winner, means, delta = P.class_posterior_hip(err.to(DEV), 4, tau or 1.0, return_parts=True)
    O.check_against_oracle(err, 4, tau or 1.0, post, lab, means, delta, label=f"{dtype} fast={fast}")
    dc.check_device_errors()


def test_evaluate_feeds_auroc_and_selective_accuracy_from_the_device():
    from diffusion_classifier_amd.utils.metrics import AUROC, Accuracy, SelectiveAccuracy
    dc = _dc("f32", classes=2, n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1])
    x, _, _ = _draws()
    loader = [{"images": x, "prompt": torch.tensor([1, 0], device=DEV)}]
    ms = [Accuracy("acc"), AUROC("auroc"), SelectiveAccuracy("sel", 0.5)]
    torch.manual_seed(3)
    dc.evaluate(loader, metrics=ms, classification=True)
    assert int(ms[0].total) == 2 and int(ms[1].hist.sum()) == 2 and int(ms[2].total.sum()) == 2
    assert 0.0 <= ms[1].compute()["auroc"] <= 1.0 and 0.0 <= ms[2].compute()["sel"] <= 1.0


# ------------------------------------------------------------------------------------------------ grid sharding
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(world, tmp_path):
    port = _free_port()
    outs = [str(tmp_path / f"posterior_w{world}_r{r}.npz") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    worker = os.path.join(HERE, "hip_posterior_shard_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), outs[r]], env=env) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    return [dict(np.load(o)) for o in outs]


def test_posterior_world_size_2_is_bit_identical_to_world_size_1(tmp_path):
    one = _launch(1, tmp_path)[0]
    two = _launch(2, tmp_path)
    assert one["probs"].shape == (2, 3) and np.isfinite(one["probs"]).all()
    for r in two:
        assert sorted(r) == sorted(one)
        for k in one:
            assert r[k].dtype == one[k].dtype
            np.testing.assert_array_equal(r[k].view(np.int32) if r[k].dtype == np.float32 else r[k],
                                          one[k].view(np.int32) if one[k].dtype == np.float32 else one[k])
