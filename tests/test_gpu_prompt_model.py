"""GPU: UNet cross-attention over prompts of several tokens, end to end — forward and classify (encoder_type='prompt') against the
test-side oracle (tests/prompt_oracle.py), the plan's structure, properties that need no oracle, 16-bit forwards, `sample` and
grid sharding."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
import oracle
from diffusion_classifier_amd import _lib as L
from helpers import hip_preds, pred_rel_l2
from prompt_oracle import PromptOracleClassifier, PromptOracleUNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
BASE = dict(pred_param="eps", schedule="cosine", noise_d=32, image_size=32, cfg_w=0.0, ema_beta=0.999, ema_warmup=0, ema_update_freq=1,
            encoder_type="prompt", n_stages=1, evaluation_per_stage=[2], n_keep_per_stage=[1], n_fast_classes=2, compute_dtype="f32")
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}


def relerr(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _randomise_vectors(m):
    """Default inits leave norm affines at (1, 0) and biases tiny: randomise them so a dropped bias or a swapped pair shows."""
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)


def make_pair(kw, seed, lowp=None):
    """(HIP model, test oracle) with the same randomised weights; lowp: None (fp32 oracle) or 'bf16' / 'f16' (storage-rounded)."""
    torch.manual_seed(seed)
    m = dca.UNetCondition2D(**kw)
    _randomise_vectors(m)
    o = PromptOracleUNet(**kw, lowp=lowp is not None, lowp_dtype=TDT.get(lowp, torch.bfloat16))
    o.load_state_dict(m.state_dict())
    return m, o


def _classifiers(kw, cfg, seed):
    m, o = make_pair(kw, seed)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg))
    with torch.no_grad():
        dc.encoder.weight.mul_(3.0)            # prompts far enough apart that classes differ visibly
    oc = PromptOracleClassifier(o, oracle.AttrBag(**cfg))
    oc.encoder.load_state_dict(dc.encoder.state_dict())
    return dc, oc


def _cross_ops(pb):
    return [(f, mt) for (kind, _, f), mt in zip(pb.ops, pb.meta) if kind == L.OP_CROSS_ATTENTION]


# ------------------------------------------------------------------------------------------------ fp32 against the oracle
@pytest.mark.parametrize("S", [2, 5, 77])
def test_small_unet_f32_forward_and_prompt_classify(S):
    kw = dca.small_unet_kwargs()
    m, o = make_pair(kw, seed=41 + S)
    torch.manual_seed(42)
    x, lam, emb = torch.randn(2, 3, 32, 32) * 0.5, torch.tensor([0.5, -3.0]), torch.randn(2, S, kw["encoder_hid_dim"])
    with torch.no_grad():
        ref = o(x, lam, encoder_hidden_states=emb)
    got = m.to(DEV)(x.to(DEV), lam.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    r = relerr(got, ref)
    print(f"small UNet f32 forward, S = {S}: rel-L2 {r:.2e} (bound 1e-4)")
    assert r < 1e-4, r
    ops = _cross_ops(next(iter(m._plans.values())).pb)
    assert len(ops) == 4 and all(f["S"] == S and mt["variant"] == "fp32" for f, mt in ops)      # down 1, mid 1, up 2 transformers
    cfg = dict(BASE, prompt_tokens=S, classes=3)
    dc, oc = _classifiers(kw, cfg, seed=43 + S)
    torch.manual_seed(44)
    BS, T = 2, 2
    xs = torch.rand(BS, 3, 32, 32) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 3, 32, 32)
    ref_l, ref_e, ref_p = oc.classify(xs, t=t, eps=eps, return_errors=True, return_preds=True)
    dc = dc.to(DEV)
    got_l, got_e = dc.classify(xs.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    rel = ((got_e - ref_e).abs() / ref_e).max().item()
    pr = pred_rel_l2(hip_preds(dc, T, BS), ref_p)
    print(f"small UNet f32 prompt classify, S = {S}: per-cell eps-MSE max rel err {rel:.2e} (bound 1e-4), predictions rel-L2 (worst sample) {pr:.2e} (bound 1e-4)")
    assert rel < 1e-4, rel
    assert got_l.cpu().tolist() == ref_l.tolist()
    assert pr < 1e-4, pr                      # the forward bar above, every (trial, image, class) sample on its own


def test_cfg2_architecture_prompt_classify_f32_with_and_without_sharing(monkeypatch):
    """The benched architecture (10 classes, class-shared trunk and skip halves) on prompts of 4 tokens against the oracle, then the
    same scores with each sharing switched off."""
    kw = dca.cifar10_unet_kwargs()
    cfg = dict(BASE, prompt_tokens=4, classes=10)
    dc, oc = _classifiers(kw, cfg, seed=51)
    torch.manual_seed(52)
    BS, T = 2, 2
    x = torch.rand(BS, 3, 32, 32) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 3, 32, 32)
    ref_l, ref_e, ref_p = oc.classify(x, t=t, eps=eps, return_errors=True, return_preds=True)
    dc = dc.to(DEV)
    got_l, got_e = dc.classify(x.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    rel = ((got_e - ref_e).abs() / ref_e).max().item()
    pr = pred_rel_l2(hip_preds(dc, T, BS), ref_p)
    print(f"cfg2 architecture f32 prompt classify (S = 4): per-cell eps-MSE max rel err {rel:.2e} (bound 1e-4), predictions rel-L2 {pr:.2e}")
    assert rel < 1e-4, rel
    assert got_l.cpu().tolist() == ref_l.tolist()
    assert pr < 1e-4, pr
    plan = next(iter(dc._score_plans.values()))["plan"]
    names = [mt["name"] for mt in plan.pb.meta]
    assert plan.n_cls == 10 and plan.S == 4 and sum(n.endswith(".conv1s") for n in names) == 5   # the class-shared skip halves are in play
    ops = _cross_ops(plan.pb)
    assert len(ops) == len(dc.ema.ema_model.packed_weights(plan.dt, torch.device(DEV)).attns) and all(f["S"] == 4 for f, _ in ops)
    dc.ema.ema_model.share_trunk = False
    e_noshare = dc.classify(x.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)[1]
    dc.ema.ema_model.share_trunk = True
    monkeypatch.setenv("DCAMD_NO_SKIP_SPLIT", "1")
    dc._score_plans.clear()
    e_nosplit = dc.classify(x.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)[1]
    for other in (e_noshare, e_nosplit):
        assert ((other - got_e).abs() / got_e).max().item() < 2e-5
        assert ((other - ref_e).abs() / ref_e).max().item() < 1e-4


# ------------------------------------------------------------------------------------------------ plan structure
def test_plan_structure_one_token_and_prompt():
    kw = dca.cifar10_unet_kwargs()
    torch.manual_seed(61)
    m = dca.UNetCondition2D(**kw).to(DEV).set_compute_dtype("bf16")
    from diffusion_classifier_amd import engine as E
    sites = len(m.packed_weights(E.DT["bf16"], torch.device(DEV)).attns)
    one, default = m.make_plan(4, 10, 10, torch.device(DEV), S=1), m.make_plan(4, 10, 10, torch.device(DEV))
    sig = lambda plan: [(kind, mt["name"], mt.get("family")) for (kind, _, _), mt in zip(plan.pb.ops, plan.pb.meta)]
    assert sig(one) == sig(default) and tuple(one.ctx.shape) == (10, kw["encoder_hid_dim"])
    assert not any(kind == L.OP_CROSS_ATTENTION for kind, _, _ in one.pb.ops)
    assert [mt["name"] for mt in one.ctx_pb.meta][:2] == ["ctx.hid_proj", "ctx.to_v"]
    # one token: the class vector is a row vector of every block's attn1.to_out epilogue (or of the one-launch front)
    rv = [f for kind, _, f in one.pb.ops if (kind == L.OP_TBLOCK_FRONT or (kind == L.OP_IGEMM and f["out"] is not None and f["out"].name.endswith(".attn_out")))]
    assert len(rv) == sites and all(f["rowvec"] is not None for f in rv)
    for share in (True, False):
        p = m.make_plan(4, 10, 10, torch.device(DEV), S=7, share_trunk=share)
        assert tuple(p.ctx.shape) == (10, 7, kw["encoder_hid_dim"])
        assert [mt["name"] for mt in p.ctx_pb.meta] == ["ctx.hid_proj", "ctx.to_kv"]          # ONE stacked K | V GEMM for all sites
        ops = _cross_ops(p.pb)
        assert len(ops) == sites
        assert not any(kind == L.OP_TBLOCK_FRONT for kind, _, _ in p.pb.ops)
        for i, (f, mt) in enumerate(ops):
            n, Lq, dp = 40, f["q"].H * f["q"].W, f["q"].C // 8
            assert f["kv_map"] is not None and f["S"] == 7 and f["k"].dom == "ctx" and f["out"].dom == "unit" and f["n"] == n
            assert mt["family"] == "cross_attention" and mt["variant"] == "mfma"
            assert mt["flops"] == 4.0 * n * 8 * Lq * 7 * dp and mt["bytes"] == 2.0 * n * Lq * f["q"].C * 2
            # class-shared trunk: the first site's queries are per (image, trial) pair, read through bj_of_unit
            if share and i == 0:
                assert f["q"].dom == "bj" and f["q_map"] is not None
            else:
                assert f["q"].dom == "unit" and f["q_map"] is None


# ------------------------------------------------------------------------------------------------ properties that need no oracle
def test_copies_of_the_class_token_reproduce_the_one_token_plan():
    kw = dca.small_unet_kwargs()
    torch.manual_seed(71)
    m = dca.UNetCondition2D(**kw)
    _randomise_vectors(m)
    m = m.to(DEV)
    x, lam, emb = (torch.randn(2, 3, 32, 32) * 0.5).to(DEV), torch.tensor([0.5, -2.0]).to(DEV), torch.randn(2, 1, kw["encoder_hid_dim"]).to(DEV)
    one = m(x, lam, encoder_hidden_states=emb).cpu()
    eight = m(x, lam, encoder_hidden_states=emb.expand(2, 8, -1).contiguous()).cpu()
    r = relerr(eight, one)
    print(f"8 copies of the class token vs the one-token plan, f32: rel-L2 {r:.2e} (bound 3e-5)")
    assert r < 3e-5, r


def test_the_last_token_of_a_ragged_prompt_is_attended():
    """Adding 1.0 to the last of 5 tokens moves the f32 prediction by more than 1e-2 relative (the CPU oracle measured 3.9e-2): a
    dropped ragged key cannot pass."""
    kw = dca.small_unet_kwargs()
    torch.manual_seed(72)
    m = dca.UNetCondition2D(**kw)
    _randomise_vectors(m)
    m = m.to(DEV)
    x, lam, emb = (torch.randn(2, 3, 32, 32) * 0.5).to(DEV), torch.tensor([0.5, -2.0]).to(DEV), torch.randn(2, 5, kw["encoder_hid_dim"]).to(DEV)
    a = m(x, lam, encoder_hidden_states=emb).cpu()
    emb2 = emb.clone()
    emb2[:, -1] += 1.0
    b = m(x, lam, encoder_hidden_states=emb2).cpu()
    r = relerr(b, a)
    print(f"+1.0 on the last of 5 tokens moves the f32 prediction by {r:.2e} relative (must exceed 1e-2)")
    assert r > 1e-2, r


# ------------------------------------------------------------------------------------------------ 16-bit forwards
ARCHS = {
    "small": lambda: (dca.small_unet_kwargs(), (3, 32)),
    "padded_heads": lambda: (dict(dca.small_unet_kwargs(), block_out_channels=(128, 384), sample_size=32), (3, 32)),
    "chexpert_experiment": lambda: (dict(dca.chexpert_experiment_unet_kwargs(image_channels=1), sample_size=64), (4, 64)),
}


@pytest.mark.parametrize("S", [5, 77])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("arch", list(ARCHS))
def test_lowp_forward_against_the_storage_rounded_oracle(arch, dt, S):
    kw, (cin, size) = ARCHS[arch]()
    m, o = make_pair(kw, seed=81, lowp=dt)
    torch.manual_seed(82)
    x, lam, emb = torch.randn(1, cin, size, size) * 0.5, torch.tensor([1.0]), torch.randn(1, S, kw["encoder_hid_dim"])
    with torch.no_grad():
        ref = o(x, lam, encoder_hidden_states=emb)
    m = m.to(DEV).set_compute_dtype(dt)
    got = m(x.to(DEV), lam.to(DEV), encoder_hidden_states=emb.to(DEV)).cpu()
    assert torch.isfinite(got).all()
    r = relerr(got, ref)
    print(f"{arch} {dt} forward, S = {S}: rel-L2 vs the storage-rounded oracle {r:.2e} (bound 2e-2)")
    assert r < 2e-2, r
    ops = _cross_ops(next(iter(m._plans.values())).pb)
    # heads of 16 (the small UNet's) run the exact fp32 kernel in every dtype; every wider head runs on the matrix cores
    assert ops and all(mt["variant"] == ("fp32" if f["d"] == 16 else "mfma") and f["S"] == S for f, mt in ops)
    assert arch == "small" or any(mt["variant"] == "mfma" for _, mt in ops)


# ------------------------------------------------------------------------------------------------ sample
def test_sample_on_prompts_fused_pair_matches_the_two_call_path():
    """`sample` with 3-token prompts: one batch-2 plan launch (prompt || null prompt) + dc_ddpm_step per step against the reference's
    form (two backbone calls + the torch expressions) on the SAME backbone — the bound of the one-token case
    (test_sample_batch2_plan_with_fused_step_matches_the_two_call_path: fp32 plans of different launch shapes)."""
    cfg = dict(BASE, cfg_w=2.0, sampling_steps=3, classes=4, pred_param="v", prompt_tokens=3)
    torch.manual_seed(33)
    m = dca.UNetCondition2D(**dca.small_unet_kwargs())
    _randomise_vectors(m)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg)).to(DEV)
    x, lab = torch.rand(3, 3, 32, 32) * 2 - 1, torch.tensor([1, 3, 0])
    bb = dc.ema.ema_model
    outs = []
    for fused in (True, False):
        torch.manual_seed(7)
        if not fused:
            real = type(bb).forward_pair
            del type(bb).forward_pair                   # no pair entry point: `sample` takes the two-call path
        try:
            outs.append(dc.sample(x.to(DEV), lab.to(DEV), from_t=0.8).cpu())
        finally:
            if not fused:
                type(bb).forward_pair = real
    assert outs[0].shape == x.shape and torch.isfinite(outs[0]).all()
    assert any(k[0] == "pair" and k[-1] == 3 for k in bb._plans) and any(k[0] == "fwd" and k[-1] == 3 for k in bb._plans)
    d = (outs[0] - outs[1]).abs().max().item()
    print(f"sample on 3-token prompts, fused pair vs two calls: max abs difference {d:.2e} (bound 3e-4)")
    assert d < 3e-4, d


# ------------------------------------------------------------------------------------------------ grid sharding
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(world, tmp_path):
    port = _free_port()
    outs = [str(tmp_path / f"prompt_w{world}_r{r}.npz") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    worker = os.path.join(HERE, "hip_prompt_shard_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), outs[r]], env=env) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    return [dict(np.load(o)) for o in outs]


def test_prompt_classify_world_size_2_is_bit_identical_to_world_size_1(tmp_path):
    one = _launch(1, tmp_path)[0]
    two = _launch(2, tmp_path)
    assert (one["ncross"] == 4).all()                               # every score plan ran attn2 as attention, once per transformer
    pruned = np.isinf(one["err"])
    assert pruned.any() and not pruned.all()                        # two-stage pruning really left cells unevaluated
    for r in two:
        for k in ("lab", "err", "lab_p", "err_p"):
            np.testing.assert_array_equal(r[k], one[k])             # bit-identical errors and labels on every rank
