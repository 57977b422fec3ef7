"""GPU: UNet cross-attention over prompts of different lengths, end to end — forward (`encoder_lengths`), classify on a ragged
PromptTable, the plan's structure, 16-bit forwards, `sample` and grid sharding.

The oracle is the one of tests/test_gpu_prompt_model.py (tests/prompt_oracle.py) fed the prompt TRUNCATED to its length, one sample at
a time: masking keys >= len out of the softmax is attending the truncated prompt (tests/test_prompt_len_host.py).  Every bound is the
one the uniform-length test of the same comparison uses."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E
from test_gpu_prompt_model import BASE, DEV, HERE, _classifiers, _free_port, _randomise_vectors, make_pair, relerr

pytestmark = pytest.mark.gpu


def _truncated(o, x, lam, emb, lens):
    """The oracle one sample at a time on the first lens[i] tokens of its prompt."""
    with torch.no_grad():
        return torch.cat([o(x[i:i + 1], lam[i:i + 1], encoder_hidden_states=emb[i:i + 1, :n]) for i, n in enumerate(lens)])


def _kinds(pb):
    return [kind for kind, _, _ in pb.ops]


def _inputs(kw, S, N=3, seed=42):
    torch.manual_seed(seed)
    return torch.randn(N, 3, 32, 32) * 0.5, torch.tensor([0.5, -3.0, 1.5][:N]), torch.randn(N, S, kw["encoder_hid_dim"])


# ------------------------------------------------------------------------------------------------ fp32 forward
def test_small_unet_f32_forward_with_lengths():
    """N = 3, S = 5, lengths [5, 2, 1] against the oracle on the truncated prompts (bound 1e-4, the forward bar); the content of the pad
    rows is irrelevant to the last bit; lengths that are all S give the bits of the call without lengths."""
    kw = dca.small_unet_kwargs()
    S, lens = 5, [5, 2, 1]
    m, o = make_pair(kw, seed=141)
    x, lam, emb = _inputs(kw, S)
    ref = _truncated(o, x, lam, emb, lens)
    m = m.to(DEV)
    run = lambda e, ln=None: m(x.to(DEV), lam.to(DEV), encoder_hidden_states=e.to(DEV),
                               **({} if ln is None else {"encoder_lengths": torch.tensor(ln)})).cpu()
    got = run(emb, lens)
    r = relerr(got, ref)
    print(f"small UNet f32 forward, S = {S}, lengths {lens}: rel-L2 vs the oracle on truncated prompts {r:.2e} (bound 1e-4)")
    assert torch.isfinite(got).all() and r < 1e-4, r
    plan = m._plans[("fwd", 3, DEV, "f32", m.share_trunk, S, "varlen")]
    assert plan.varlen and plan.ctx_len.dtype == torch.int32 and plan.ctx_len.tolist() == lens
    kinds = _kinds(plan.pb)
    assert kinds.count(L.OP_CROSS_ATTENTION_LEN) == 4 and L.OP_CROSS_ATTENTION not in kinds
    # pad rows at 0 and at 1e4 * randn: identical bits
    mask = (torch.arange(S)[None, :] >= torch.tensor(lens)[:, None])[..., None]
    zeros, wild = emb.masked_fill(mask, 0.0), torch.where(mask, 1e4 * torch.randn_like(emb), emb)
    a, b = run(zeros, lens), run(wild, lens)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), got.view(torch.int32))
    # lengths all S: the bits of today's plan, which is still built (and keyed) as before
    full, plain = run(emb, [S] * 3), run(emb)
    assert torch.equal(full.view(torch.int32), plain.view(torch.int32))
    today = m._plans[("fwd", 3, DEV, "f32", m.share_trunk, S)]
    assert not today.varlen and today.ctx_len is None and L.OP_CROSS_ATTENTION_LEN not in _kinds(today.pb)
    assert relerr(got, plain) > 1e-4                                 # ... further apart than what counts as equal here: the lengths reach the kernel
    for bad in ([5, 0, 1], [5, 6, 1], [5, 2], [5.0, 2.0, 1.0]):
        with pytest.raises(L.DcamdError):
            run(emb, bad)
    with pytest.raises(L.DcamdError):                                 # one token is always attended: no varlen plan at S = 1
        m(x.to(DEV), lam.to(DEV), encoder_hidden_states=emb[:, :1].to(DEV), encoder_lengths=torch.tensor([1, 1, 1]))


# ------------------------------------------------------------------------------------------------ fp32 classify
def test_small_unet_f32_classify_on_a_ragged_table():
    """3 classes + null, S = 4, class lengths [4, 1, 2]; BS = 2, T = 2, fixed t / eps; class-shared trunk on and off.  Reference: the
    oracle's loop (oracle/classifier.py) with the truncated prompt, one (image, class) cell at a time."""
    kw = dca.small_unet_kwargs()
    S, lens = 4, [4, 1, 2, 4]
    cfg = dict(BASE, prompt_tokens=S, classes=3)
    dc, oc = _classifiers(kw, cfg, seed=143)
    dc.encoder.set_lengths(lens)                                      # the pad rows keep their random content: it must not matter
    torch.manual_seed(144)
    BS, T = 2, 2
    xs = torch.rand(BS, 3, 32, 32) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 3, 32, 32)
    ref_e = torch.zeros(BS, 3, T)
    with torch.no_grad():
        for j in range(T):
            logsnr = oc.schedule(t[j])
            alpha, sigma = torch.sqrt(torch.sigmoid(logsnr)).view(-1, 1, 1, 1), torch.sqrt(torch.sigmoid(-logsnr)).view(-1, 1, 1, 1)
            z = alpha * xs + sigma * eps[j]
            for c in range(3):
                for b in range(BS):
                    emb = oc.encoder.weight[c:c + 1, :lens[c]]
                    pred = oc.ema_model(x=z[b:b + 1], noise_labels=logsnr[b:b + 1], encoder_hidden_states=emb)
                    ref_e[b, c, j] = torch.norm((pred - eps[j, b:b + 1]).view(1, -1), dim=1, p=2) ** 2
    ref_l = ref_e.mean(dim=2).argmin(dim=1)
    dc = dc.to(DEV)
    for share in (True, False):
        dc.ema.ema_model.share_trunk = share
        got_l, got_e = dc.classify(xs.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
        rel = ((got_e - ref_e).abs() / ref_e).max().item()
        print(f"small UNet f32 classify, ragged table {lens[:3]} of S = {S}, share_trunk = {share}: per-cell eps-MSE max rel err {rel:.2e} (bound 1e-4)")
        assert rel < 1e-4, rel
        assert got_l.cpu().tolist() == ref_l.tolist()
        plan = list(dc._score_plans.values())[-1]["plan"]
        kinds = _kinds(plan.pb)
        assert plan.varlen and plan.ctx_len.tolist() == lens[:3]
        assert kinds.count(L.OP_CROSS_ATTENTION_LEN) == 4 and L.OP_CROSS_ATTENTION not in kinds
    # the same table with uniform lengths builds (and keys) today's plan
    dc.encoder.set_lengths([S] * 4)
    dc._score_plans.clear()
    uni_e = dc.classify(xs.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)[1]
    plan = next(iter(dc._score_plans.values()))["plan"]
    assert not plan.varlen and _kinds(plan.pb).count(L.OP_CROSS_ATTENTION) == 4 and L.OP_CROSS_ATTENTION_LEN not in _kinds(plan.pb)
    assert all(k[-1] == S for k in dc._score_plans)
    assert ((uni_e - ref_e).abs() / ref_e).max().item() > 1e-4        # outside the bound without the lengths: they had reached the kernel


# ------------------------------------------------------------------------------------------------ plan structure
def test_varlen_plan_structure():
    """varlen: every cross-attention op is dc_cross_attention_len reading the plan's ctx_len, everything else is the uniform plan op for
    op; varlen=False is today's plan; S = 1 has no varlen plan."""
    kw = dca.cifar10_unet_kwargs()
    torch.manual_seed(61)
    m = dca.UNetCondition2D(**kw).to(DEV).set_compute_dtype("bf16")
    dev = torch.device(DEV)
    sites = len(m.packed_weights(E.DT["bf16"], dev).attns)
    sig = lambda plan: [(kind, mt["name"], mt.get("family")) for (kind, _, _), mt in zip(plan.pb.ops, plan.pb.meta)]
    for share in (True, False):
        uni = m.make_plan(4, 10, 10, dev, S=7, share_trunk=share)
        off = m.make_plan(4, 10, 10, dev, S=7, share_trunk=share, varlen=False)
        var = m.make_plan(4, 10, 10, dev, S=7, share_trunk=share, varlen=True)
        assert sig(off) == sig(uni) and off.ctx_len is None and not off.varlen
        assert tuple(var.ctx_len.shape) == (10,) and var.ctx_len.dtype == torch.int32 and var.ctx_len.tolist() == [7] * 10
        swap = lambda s: [(L.OP_CROSS_ATTENTION_LEN if kind == L.OP_CROSS_ATTENTION else kind, name, fam) for kind, name, fam in s]
        assert sig(var) == swap(sig(uni))
        assert [mt["name"] for mt in var.ctx_pb.meta] == [mt["name"] for mt in uni.ctx_pb.meta] == ["ctx.hid_proj", "ctx.to_kv"]
        ops = [(f, mt) for (kind, _, f), mt in zip(var.pb.ops, var.pb.meta) if kind == L.OP_CROSS_ATTENTION_LEN]
        ref = [(f, mt) for (kind, _, f), mt in zip(uni.pb.ops, uni.pb.meta) if kind == L.OP_CROSS_ATTENTION]
        assert len(ops) == len(ref) == sites
        for (f, mt), (fr, mr) in zip(ops, ref):
            assert f["kv_len"] == var.ctx_len.data_ptr() and f["kv_map"] is not None and f["S"] == 7
            assert mt["family"] == "cross_attention" and mt["variant"] == "mfma" == mr["variant"]
            assert mt["flops"] == mr["flops"] and mt["bytes"] == mr["bytes"]           # computed with S: the upper bound
    with pytest.raises(L.DcamdError):
        m.make_plan(4, 10, 10, dev, S=1, varlen=True)


# ------------------------------------------------------------------------------------------------ 16-bit forwards
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_lowp_forward_with_lengths_against_the_storage_rounded_oracle(dt):
    kw = dca.small_unet_kwargs()
    S, lens = 5, [5, 2, 1]
    m, o = make_pair(kw, seed=181, lowp=dt)
    x, lam, emb = _inputs(kw, S, seed=182)
    ref = _truncated(o, x, lam, emb, lens)
    m = m.to(DEV).set_compute_dtype(dt)
    got = m(x.to(DEV), lam.to(DEV), encoder_hidden_states=emb.to(DEV), encoder_lengths=torch.tensor(lens)).cpu()
    assert torch.isfinite(got).all()
    r = relerr(got, ref)
    print(f"small UNet {dt} forward, S = {S}, lengths {lens}: rel-L2 vs the storage-rounded oracle on truncated prompts {r:.2e} (bound 2e-2)")
    assert r < 2e-2, r
    kinds = _kinds(next(iter(m._plans.values())).pb)
    assert kinds.count(L.OP_CROSS_ATTENTION_LEN) == 4 and L.OP_CROSS_ATTENTION not in kinds


# ------------------------------------------------------------------------------------------------ sample
def test_sample_on_a_ragged_table_fused_pair_matches_the_two_call_path():
    """3-token table, class prompts of 3 and 2 tokens, a null prompt of 1; 2 sampling steps.  The fused pair against the two-call path
    on the same backbone within 3e-4 (the bound of the uniform case), and both further than that from the run that ignores the
    lengths: two runs within 3e-4 count as the same run here, so a difference beyond it shows that the lengths reached the kernels."""
    cfg = dict(BASE, cfg_w=2.0, sampling_steps=2, classes=2, pred_param="v", prompt_tokens=3)
    torch.manual_seed(133)
    m = dca.UNetCondition2D(**dca.small_unet_kwargs())
    _randomise_vectors(m)
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg))
    with torch.no_grad():
        dc.encoder.weight.mul_(3.0)
    dc.encoder.set_lengths([3, 2, 1])
    dc = dc.to(DEV)
    x, lab = torch.rand(3, 3, 32, 32) * 2 - 1, torch.tensor([1, 0, 1])
    bb = dc.ema.ema_model

    def run(fused):
        torch.manual_seed(7)
        if not fused:
            real = type(bb).forward_pair
            del type(bb).forward_pair                   # no pair entry point: `sample` takes the two-call path
        try:
            return dc.sample(x.to(DEV), lab.to(DEV), from_t=0.8).cpu()
        finally:
            if not fused:
                type(bb).forward_pair = real
    pair, two = run(True), run(False)
    assert pair.shape == x.shape and torch.isfinite(pair).all() and torch.isfinite(two).all()
    assert any(k[0] == "pair" and k[-1] == "varlen" for k in bb._plans) and any(k[0] == "fwd" and k[-1] == "varlen" for k in bb._plans)
    assert bb._plans[[k for k in bb._plans if k[0] == "pair"][0]].ctx_len.tolist() == [2, 1, 3, 1, 2, 1]      # 2b = cond[b], 2b + 1 = null[b]
    d = (pair - two).abs().max().item()
    print(f"sample on a ragged 3-token table, fused pair vs two calls: max abs difference {d:.2e} (bound 3e-4)")
    assert d < 3e-4, d
    dc.encoder.set_lengths([3, 3, 3])
    blind = run(True)
    assert any(k[0] == "pair" and k[-1] == 3 for k in bb._plans)
    dp, dt_ = (pair - blind).abs().max().item(), (two - blind).abs().max().item()
    print(f"against the run that ignores the lengths: fused pair {dp:.2e}, two calls {dt_:.2e} (must exceed 3e-4)")
    assert dp > 3e-4 and dt_ > 3e-4, (dp, dt_)


# ------------------------------------------------------------------------------------------------ grid sharding
def _launch(world, tmp_path):
    port = _free_port()
    outs = [str(tmp_path / f"prompt_len_w{world}_r{r}.npz") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    worker = os.path.join(HERE, "hip_prompt_len_shard_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), outs[r]], env=env) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    return [dict(np.load(o)) for o in outs]


def test_ragged_classify_world_size_2_is_bit_identical_to_world_size_1(tmp_path):
    one = _launch(1, tmp_path)[0]
    two = _launch(2, tmp_path)
    assert (one["nlen"] == 4).all() and (one["ncross"] == 0).all()   # every score plan ran attn2 with lengths, once per transformer
    pruned = np.isinf(one["err"])
    assert pruned.any() and not pruned.all()
    for r in two:
        for k in ("lab", "err", "lab_p", "err_p"):
            np.testing.assert_array_equal(r[k], one[k])
