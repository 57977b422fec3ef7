"""GPU: the CLIP text encoder end to end — CLIPTextEncoder.forward against the pinned transformers outputs (tests/golden/clip_tiny.npz)
and the storage-rounded restatement (tests/clip_oracle.py), properties that need no oracle, and encoder_type='clip' through classify /
sample on the small UNet of tests/test_gpu_prompt_model.py with an encoder_hid_dim of 128.

Bars are the project's (tests/test_gpu_t5_model.py): 1e-4 relative L2 for fp32 forwards, 2e-2 for 16-bit forwards against the
storage-rounded oracle, 1e-4 per-cell relative error of the eps-MSE in fp32."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import diffusion_classifier_amd as dca
import oracle
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd.nets.clip import CLIPTextEncoder
from clip_oracle import clip_encode
from prompt_oracle import PromptOracleClassifier
from test_gpu_prompt_model import BASE, DEV, make_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
ACTS = ("quick_gelu", "gelu")
_CACHE = {}


def golden():
    if not _CACHE:
        g = np.load(os.path.join(ROOT, "tests", "golden", "clip_tiny.npz"))
        _CACHE.update(cfg=json.loads(str(g["config"])), sd={k[3:]: torch.from_numpy(g[k]).float() for k in g.files if k.startswith("sd.")},
                      ids=torch.from_numpy(g["input_ids"]), mask=torch.from_numpy(g["attention_mask"]), ids77=torch.from_numpy(g["input_ids77"]),
                      out={a: torch.from_numpy(g["last_hidden_state." + a]) for a in ACTS},
                      out77={a: torch.from_numpy(g["last_hidden_state77." + a]) for a in ACTS})
        _CACHE["lens"] = _CACHE["mask"].sum(1).tolist()
    return _CACHE


def encoder(dt="f32", act="quick_gelu"):
    G = golden()
    m = CLIPTextEncoder(**dict(G["cfg"], hidden_act=act))
    m.load_state_dict(G["sd"], strict=True)
    return m.to(DEV).set_compute_dtype(dt)


def per_prompt_rel(got, ref, lens):
    """Largest relative L2 over the prompts, on the rows below each length."""
    return max(((got[i, :n].double() - ref[i, :n].double()).norm() / ref[i, :n].double().norm()).item() for i, n in enumerate(lens))


def pad_rows_are_zero(out, lens):
    return all(bool((out[i, n:] == 0).all()) for i, n in enumerate(lens))


def write_hf_directory(path):
    from safetensors.torch import save_file
    G = golden()
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(dict(G["cfg"], model_type="clip_text_model"), fh)
    save_file({k: v.clone().contiguous() for k, v in G["sd"].items()}, os.path.join(path, "model.safetensors"))
    return str(path)


@pytest.mark.parametrize("act", ACTS)
def test_f32_forward_matches_transformers(act):
    G = golden()
    m = encoder("f32", act)
    out = m(G["ids"].to(DEV), G["mask"].to(DEV))
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == tuple(G["out"][act].shape)
    got = out.cpu()
    assert torch.isfinite(got).all() and pad_rows_are_zero(got, G["lens"])
    r = per_prompt_rel(got, G["out"][act], G["lens"])
    plan = next(iter(m._plans.values()))
    kinds = [k for k, _, _ in plan.pb.ops]
    nl = G["cfg"]["num_hidden_layers"]
    assert kinds.count(L.OP_ATTENTION_CAUSAL) == nl and kinds.count(L.OP_ACT_PASS) == nl and kinds.count(L.OP_LAYERNORM_ROWS) == 2 * nl + 1
    assert kinds.count(L.OP_EMBED_ROWS_POS) == 1 and kinds.count(L.OP_IGEMM) == 4 * nl and len(kinds) == 8 * nl + 2
    assert kinds[0] == L.OP_EMBED_ROWS_POS and kinds[-1] == L.OP_LAYERNORM_ROWS
    assert kinds[1:9] == [L.OP_LAYERNORM_ROWS, L.OP_IGEMM, L.OP_ATTENTION_CAUSAL, L.OP_IGEMM, L.OP_LAYERNORM_ROWS, L.OP_IGEMM, L.OP_ACT_PASS,
                          L.OP_IGEMM]
    full = m(G["ids77"].to(DEV)).cpu()                                          # no mask: every row a real state, the full context
    assert torch.isfinite(full).all()
    r77 = per_prompt_rel(full, G["out77"][act], [77, 77])
    print(f"CLIP text encoder f32 ({act}) vs transformers: largest per-prompt rel-L2 {r:.2e} (lengths {G['lens']}), {r77:.2e} (2 x 77, no "
          f"mask) (bound 1e-4)")
    assert r < 1e-4 and r77 < 1e-4, (r, r77)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_lowp_forward_against_the_storage_rounded_restatement(dt, act):
    G = golden()
    m = encoder(dt, act)
    got = m(G["ids"].to(DEV), G["mask"].to(DEV)).cpu()
    ref = clip_encode(G["sd"], G["cfg"], G["ids"], G["mask"], store=TDT[dt], dtype=torch.float64, hidden_act=act)
    assert torch.isfinite(got).all() and pad_rows_are_zero(got, G["lens"])
    r, r32 = per_prompt_rel(got, ref, G["lens"]), per_prompt_rel(got, G["out"][act], G["lens"])
    plan = next(iter(m._plans.values()))
    variants = {mt["variant"] for (k, _, _), mt in zip(plan.pb.ops, plan.pb.meta) if k == L.OP_ATTENTION_CAUSAL}
    got77 = m(G["ids77"].to(DEV)).cpu()
    ref77 = clip_encode(G["sd"], G["cfg"], G["ids77"], None, store=TDT[dt], dtype=torch.float64, hidden_act=act)
    r77 = per_prompt_rel(got77, ref77, [77, 77])
    print(f"CLIP text encoder {dt} ({act}) vs the storage-rounded restatement: largest per-prompt rel-L2 {r:.2e}, {r77:.2e} at 2 x 77 "
          f"(bound 2e-2); vs fp32 transformers {r32:.2e}; attention on {variants}")
    assert variants == {"mfma"}
    assert r < 2e-2 and r77 < 2e-2, (r, r77)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_mask_pad_ids_and_prompt_order_change_no_bit(dt):
    """The valid rows are bit-identical with and without the mask; changing the ids at pad positions changes no bit of the masked
    output; permuting the prompts permutes the output bit for bit."""
    G = golden()
    m = encoder(dt)
    ids, mask = G["ids"].to(DEV), G["mask"].to(DEV)
    a = m(ids, mask)
    free = m(ids)
    for i, n in enumerate(G["lens"]):
        assert torch.equal(a[i, :n].view(torch.int32), free[i, :n].view(torch.int32)), i
    assert bool((free[1, G["lens"][1]:] != 0).any())                            # without a mask the later rows are real states
    wild = torch.where(mask.bool(), ids, torch.randint(0, G["cfg"]["vocab_size"], ids.shape, device=DEV))
    assert not torch.equal(wild, ids)
    b = m(wild, mask)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    perm = torch.tensor([2, 3, 0, 1], device=DEV)
    c = m(ids[perm], mask[perm])
    assert torch.equal(c.view(torch.int32), a[perm].view(torch.int32))


def test_classify_and_sample_with_encoder_type_clip(tmp_path):
    """encoder_type='clip' (local directory, set_class_prompts with ragged prompts) gives the bits of encoder_type='prompt' with the
    table filled by hand from CLIPTextEncoder.forward + set_lengths; in f32 both agree with the oracle's loop fed the restatement's
    embeddings (truncated to each prompt's length) to 1e-4 per cell, with equal labels; one sample() call runs through forward_pair."""
    G = golden()
    kw = dict(dca.small_unet_kwargs(), encoder_hid_dim=128)
    S, classes, Lq = 48, 3, G["ids"].shape[1]
    lens = G["lens"]
    cfg = dict(BASE, prompt_tokens=S, classes=classes, sampling_steps=2)
    path = write_hf_directory(tmp_path / "clip")
    m, o = make_pair(kw, seed=401)
    dcc = dca.DiffusionClassifier(copy.deepcopy(m), dca.Config(**dict(cfg, encoder_type="clip", clip_path=path))).to(DEV)
    dcp = dca.DiffusionClassifier(copy.deepcopy(m), dca.Config(**dict(cfg, encoder_type="prompt"))).to(DEV)
    with pytest.raises(RuntimeError, match="set_class_prompts"):
        dcc.classify(torch.zeros(2, 3, 32, 32, device=DEV))
    dcc.set_class_prompts(G["ids"], G["mask"])
    assert dcc.encoder.lengths.tolist() == lens and dcc.encoder.varlen
    emb = encoder("f32")(G["ids"].to(DEV), G["mask"].to(DEV))                   # by hand: the output into the table, the counts into set_lengths
    with torch.no_grad():
        dcp.encoder.weight.zero_()
        dcp.encoder.weight[:, :Lq] = emb
    dcp.encoder.set_lengths(lens)
    assert torch.equal(dcc.encoder.weight.view(torch.int32), dcp.encoder.weight.view(torch.int32))
    assert bool((dcc.encoder.weight[:, Lq:] == 0).all())
    torch.manual_seed(402)
    BS, T = 2, 2
    xs = torch.rand(BS, 3, 32, 32) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 3, 32, 32)
    lc, ec = dcc.classify(xs.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    lp, ep = dcp.classify(xs.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
    assert torch.equal(ec.view(torch.int32), ep.view(torch.int32)) and torch.equal(lc.cpu(), lp.cpu())
    # the oracle's loop on the restatement's embeddings, one (image, class) cell at a time on the truncated prompt
    ref_emb = clip_encode(G["sd"], G["cfg"], G["ids"], G["mask"])
    oc = PromptOracleClassifier(o, oracle.AttrBag(**dict(cfg, encoder_type="prompt")))
    ref_e = torch.zeros(BS, classes, T)
    with torch.no_grad():
        for j in range(T):
            logsnr = oc.schedule(t[j])
            alpha, sigma = torch.sqrt(torch.sigmoid(logsnr)).view(-1, 1, 1, 1), torch.sqrt(torch.sigmoid(-logsnr)).view(-1, 1, 1, 1)
            z = alpha * xs + sigma * eps[j]
            for c in range(classes):
                for b in range(BS):
                    pred = oc.ema_model(x=z[b:b + 1], noise_labels=logsnr[b:b + 1], encoder_hidden_states=ref_emb[c:c + 1, :lens[c]])
                    ref_e[b, c, j] = torch.norm((pred - eps[j, b:b + 1]).view(1, -1), dim=1, p=2) ** 2
    rel = ((ec.cpu() - ref_e).abs() / ref_e).max().item()
    print(f"classify with encoder_type='clip' (prompt lengths {lens[:classes]}) vs the oracle on the restatement's embeddings: per-cell "
          f"eps-MSE max rel err {rel:.2e} (bound 1e-4)")
    assert rel < 1e-4, rel
    assert lc.cpu().tolist() == ref_e.mean(dim=2).argmin(dim=1).tolist()
    # sample(): the fused pair path on the same object
    bb = dcc.ema.ema_model
    calls = []
    fp = bb.forward_pair
    bb.forward_pair = lambda *a, **k: (calls.append(sorted(k)), fp(*a, **k))[1]
    torch.manual_seed(403)
    img = dcc.sample(torch.zeros(2, 3, 32, 32, device=DEV), torch.tensor([0, 2], device=DEV), from_t=0.8)
    assert len(calls) == 3 and all("cond_lengths" in k for k in calls)
    assert tuple(img.shape) == (2, 3, 32, 32) and torch.isfinite(img).all()
    dcc.check_device_errors()
