"""Host: DiT.from_directory and its envelope, the published XL/2 geometry, the 'ddpm_linear' DDPM schedule of DiffusionClassifier, the
eps rows of a learned-variance projection, and the refusal of every other output width.  No GPU."""
import math
import os
import re

import pytest
import torch

import dit_dir_oracle as DO
import draws_fixture
from diffusion_classifier_amd import packing
from diffusion_classifier_amd.nets.dit import DiT

TINY = dict(DO.DIT_A, num_layers=1)


# ------------------------------------------------------------------------------------------------ loading
def test_from_directory_round_trip_strays_missing_keys_and_config_fields(tmp_path):
    src = DO.make_dit(TINY, seed=3)
    sd = src.state_dict()
    m = DiT.from_directory(DO.write_transformer(tmp_path, "ok", TINY, sd))          # the published key set at its defaults, `_` keys ignored
    assert list(m.state_dict()) == list(sd) and all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert all(not p.requires_grad for p in m.parameters())
    assert m.config.out_channels == 8 and m.config.in_channels == 4 and m.config.sample_size == 8 and m.config.num_embeds_ada_norm == 10
    # overrides win over the file, for a constructor key and for a fixed one
    assert DiT.from_directory(DO.write_transformer(tmp_path, "ok2", TINY, sd), sample_size=16).config.sample_size == 16
    DiT.from_directory(DO.write_transformer(tmp_path, "ok3", TINY, sd, extra_cfg=dict(cross_attention_dim=64)), cross_attention_dim=None)
    with pytest.raises(NotImplementedError, match="attention_type"):
        DiT.from_directory(DO.write_transformer(tmp_path, "ok4", TINY, sd), attention_type="gated")
    # a config without the nullable keys loads as well
    DiT.from_directory(DO.write_transformer(tmp_path, "bare", TINY, sd, drop=list(DiT.FIXED_KEYS)))
    with pytest.raises(RuntimeError, match="stray.weight"):
        DiT.from_directory(DO.write_transformer(tmp_path, "stray", TINY, dict(sd, **{"stray.weight": torch.zeros(2)})))
    lost = "transformer_blocks.0.norm1.emb.class_embedder.embedding_table.weight"
    with pytest.raises(RuntimeError, match=lost.replace(".", r"\.")):
        DiT.from_directory(DO.write_transformer(tmp_path, "lost", TINY, {k: v for k, v in sd.items() if k != lost}))
    with pytest.raises(RuntimeError, match="proj_out_2"):                            # the eps-only twin's file does not fit a 2C model
        DiT.from_directory(DO.write_transformer(tmp_path, "twin", TINY, DO.eps_twin(src).state_dict()))
    with pytest.raises(ValueError, match="patch_size"):
        DiT.from_directory(DO.write_transformer(tmp_path, "nofield", TINY, sd, drop=["patch_size"]))
    for name in ("config.json", "diffusion_pytorch_model.safetensors"):
        d = DO.write_transformer(tmp_path, "no_" + name.split(".")[0], TINY, sd)
        os.remove(os.path.join(d, name))
        with pytest.raises(FileNotFoundError, match=re.escape(name)):
            DiT.from_directory(d)
    with pytest.raises(FileNotFoundError):
        DiT.from_directory(str(tmp_path / "nowhere"))


@pytest.mark.parametrize("bad, word", [
    (dict(norm_type="layer_norm"), "norm_type"), (dict(cross_attention_dim=64), "cross_attention_dim"),
    (dict(num_vector_embeds=100), "num_vector_embeds"), (dict(only_cross_attention=True), "only_cross_attention"),
    (dict(use_linear_projection=True), "use_linear_projection"), (dict(double_self_attention=True), "double_self_attention"),
    (dict(attention_type="gated"), "attention_type"), (dict(caption_channels=4096), "caption_channels"),
    (dict(interpolation_scale=2.0), "interpolation_scale"), (dict(activation_fn="geglu"), "activation_fn"),
    (dict(some_future_key=1), "some_future_key"),
])
def test_from_directory_refuses_by_name(tmp_path, bad, word):
    sd = DO.make_dit(TINY, seed=4).state_dict()
    with pytest.raises(NotImplementedError, match=word):
        DiT.from_directory(DO.write_transformer(tmp_path, "bad", TINY, sd, extra_cfg=bad))


# ------------------------------------------------------------------------------------------------ published geometry
def test_published_xl2_geometry_on_the_meta_device():
    with torch.device("meta"):
        m = DiT(out_channels=8)
    cfg = m.config
    assert (cfg.num_attention_heads, cfg.attention_head_dim, cfg.num_layers, cfg.patch_size, cfg.sample_size, cfg.in_channels,
            cfg.num_embeds_ada_norm) == (16, 72, 28, 2, 32, 4, 1000)
    per_block = ["norm1.emb.timestep_embedder.linear_1", "norm1.emb.timestep_embedder.linear_2", "norm1.emb.class_embedder.embedding_table",
                 "norm1.linear", "attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "ff.net.0.proj", "ff.net.2"]
    want = {"pos_embed.proj", "proj_out_1", "proj_out_2"} | {f"transformer_blocks.{i}.{g}" for i in range(28) for g in per_block}
    names = dict(m.named_parameters())
    assert {k.rsplit(".", 1)[0] for k in names} == want
    assert list(m.state_dict()) == list(names)                                       # the position table is no persistent buffer
    D = 1152
    assert tuple(names["pos_embed.proj.weight"].shape) == (D, 4, 2, 2) and tuple(names["proj_out_2.weight"].shape) == (32, D)
    assert tuple(names["transformer_blocks.27.norm1.emb.class_embedder.embedding_table.weight"].shape) == (1001, D)
    assert tuple(names["transformer_blocks.0.norm1.linear.weight"].shape) == (6 * D, D) and tuple(names["proj_out_1.weight"].shape) == (2 * D, D)
    assert sum(p.numel() for p in m.parameters()) == 749_826_464


# ------------------------------------------------------------------------------------------------ schedule
def _classifier(**over):
    return draws_fixture.classifier(over.pop("schedule", "ddpm_linear"), **over)


@pytest.mark.parametrize("N, b0, b1", [(1000, 1e-4, 0.02), (50, 1e-3, 0.02)])
def test_ddpm_linear_schedule_against_an_fp64_restatement(N, b0, b1):
    over = {} if N == 1000 else dict(train_timesteps=N, beta_start=b0, beta_end=b1)
    dc = _classifier(**over)
    ref = DO.ref_logsnr(N, b0, b1)
    t = torch.tensor([0.0, 1.0 / N, 0.5, 1.0 - 1e-7, 1.0], dtype=torch.float32)
    k_ref = [min(int(math.floor(float(v) * N)), N - 1) for v in t.tolist()]       # the fp32 value of t, the product in fp64
    assert k_ref == [0, 1 if N == 1000 else 0, N // 2, N - 1, N - 1]
    lam, lab = dc.schedule(t), dc.noise_labels(t)
    assert dc.discrete and dc.train_timesteps == N and dc.steps_offset == 0
    assert lam.dtype == torch.float32 and lab.dtype == torch.float32 and lab.tolist() == [float(k) for k in k_ref]      # the integer step
    assert torch.equal(dc.ddpm_step(t), torch.tensor(k_ref))
    assert torch.equal(lam, torch.tensor([ref[k] for k in k_ref], dtype=torch.float64).to(torch.float32))
    table = dc.ddpm_logsnr
    assert tuple(table.shape) == (N,) and torch.equal(table, torch.tensor(ref, dtype=torch.float64).to(torch.float32))
    assert bool((table[1:] < table[:-1]).all())                                    # strictly decreasing in k
    al, sg = torch.sqrt(torch.sigmoid(table)), torch.sqrt(torch.sigmoid(-table))
    assert float((al * al + sg * sg - 1).abs().max()) <= 4 * torch.finfo(torch.float32).eps
    assert float(dc.schedule(torch.tensor(0.5))) == float(lam[2]) and torch.equal(dc.schedule(t.reshape(5, 1)), lam.reshape(5, 1))
    # not the other discrete schedule under the same numbers
    other = _classifier(schedule="scaled_linear", train_timesteps=N, beta_start=b0, beta_end=b1)
    assert not torch.equal(other.ddpm_logsnr, table)


def test_trial_draws_carry_the_step_as_label():
    dc = _classifier()
    T, BS = draws_fixture.T, draws_fixture.BS
    t = torch.linspace(0, 1, T * BS).reshape(T, BS)
    d = dc._trial_draws(torch.zeros(BS, 3, 4, 4), T, t, torch.zeros(T, BS, 3, 4, 4), "reference", 0)
    assert torch.equal(d["label"], torch.clamp(torch.floor(t.double() * 1000), max=999).float())
    assert torch.equal(d["logsnr"], dc.ddpm_logsnr[d["label"].long()])
    assert torch.equal(d["alpha"], torch.sqrt(torch.sigmoid(d["logsnr"]))) and torch.equal(d["sigma"], torch.sqrt(torch.sigmoid(-d["logsnr"])))


def test_scheduler_path_parsing_and_the_two_cross_refusals(tmp_path):
    write = lambda name, **kw: DO.write_scheduler(tmp_path, name, **dict(dict(beta_start=0.001, num_train_timesteps=50), **kw))
    dc = _classifier(scheduler_path=write("a"))
    assert dc.train_timesteps == 50 and torch.equal(dc.ddpm_logsnr, torch.tensor(DO.ref_logsnr(50, 0.001, 0.02), dtype=torch.float64).float())
    assert _classifier(scheduler_path=os.path.join(write("b"), "scheduler_config.json")).train_timesteps == 50      # the file itself
    assert _classifier(scheduler_path=write("c"), train_timesteps=20).train_timesteps == 20                          # the config's own key wins
    assert _classifier(scheduler_path=write("o", steps_offset=1)).steps_offset == 1
    assert _classifier(scheduler_path=write("v", prediction_type="v_prediction"), pred_param="v").train_timesteps == 50
    with pytest.raises(ValueError, match="prediction_type"):
        _classifier(scheduler_path=write("d", prediction_type="v_prediction"))
    with pytest.raises(ValueError, match="prediction_type"):
        _classifier(scheduler_path=write("e"), pred_param="v")
    # the two cross refusals: each discrete schedule refuses the other's file, naming the key
    with pytest.raises(ValueError, match="beta_schedule.*scaled_linear"):
        _classifier(scheduler_path=write("f", beta_schedule="scaled_linear"))
    with pytest.raises(ValueError, match="beta_schedule.*'linear'"):
        _classifier(schedule="scaled_linear", scheduler_path=write("g", beta_schedule="linear"))
    with pytest.raises(ValueError, match="beta_schedule"):
        _classifier(scheduler_path=write("h", beta_schedule="squaredcos_cap_v2"))
    # a file without the key takes the schedule's own
    assert _classifier(scheduler_path=DO.write_scheduler(tmp_path, "i", beta_schedule="linear")).train_timesteps == 1000


def test_generation_entry_points_refuse_without_timestep_spacing_and_take_the_grid_with_it():
    dc = _classifier(sampling_steps=4)
    x = torch.zeros(2, 3, 32, 32)
    for call in (lambda: dc.sample(x, torch.tensor([0, 1])), lambda: dc.counterfactual(x), lambda: dc.invert(x), lambda: dc.invert_ddpm(x)):
        with pytest.raises(NotImplementedError, match=r"ddpm_linear.*timestep_spacing"):
            call()
    with pytest.raises(ValueError, match="timestep_spacing"):
        _classifier(schedule="cosine", timestep_spacing="trailing")
    from diffusion_classifier_amd import trajectory as TJ
    dc = _classifier(sampling_steps=4, timestep_spacing="trailing")
    assert TJ.discrete_steps(dc, 1.0) == [999, 749, 499, 249, 0]
    g = TJ.grid(dc, 1.0, 0.0)
    assert [float(v) for v in g.label] == [999.0, 749.0, 499.0, 249.0, 0.0] and all(torch.equal(g.lam[i], dc.ddpm_logsnr[k]) for i, k in enumerate(g.steps))
    dc = _classifier(sampling_steps=4, timestep_spacing="leading", steps_offset=1)
    assert TJ.discrete_steps(dc, 1.0) == [751, 501, 251, 1, 0]


# ------------------------------------------------------------------------------------------------ eps rows
def _unpatchify(h, p, oc):
    N, g = h.shape[0], h.shape[1]
    return h.reshape(N, g, g, p, p, oc).permute(0, 5, 1, 3, 2, 4).reshape(N, oc, g * p, g * p)


@pytest.mark.parametrize("p, C", [(2, 4), (4, 4), (2, 3)])
def test_eps_rows_are_the_first_channels_of_the_full_projection(p, C):
    """Project with the full proj_out_2 and un-patchify with 2C channels; project with the selected rows and un-patchify with C: the
    first C channels of the former are the latter, element for element.  (The projection is written as a product and a sum over K per
    output feature, so that a feature's value does not depend on how many features are computed beside it.)"""
    torch.manual_seed(40 + p + C)
    oc, D, N, g = 2 * C, 24, 2, 3
    W, b, hn = torch.randn(p * p * oc, D), torch.randn(p * p * oc), torch.randn(N, g, g, D)
    project = lambda W, b: (hn.unsqueeze(-2) * W).sum(-1) + b
    rows = packing.eps_rows(p, C, oc)
    assert rows.dtype == torch.int64 and rows.tolist() == [(py * p + px) * oc + c for py in range(p) for px in range(p) for c in range(C)]
    full = _unpatchify(project(W, b), p, oc)
    sel = _unpatchify(project(W[rows], b[rows]), p, C)
    assert torch.equal(full[:, :C], sel)
    assert not torch.equal(full[:, C:], sel)                                       # and not the variance half
    assert packing.eps_rows(p, C, C) is None
    # the twin the GPU tests compare against holds the same rows
    if (p, C) == (2, 4):
        m = DO.make_dit(TINY, seed=5)
        tw = DO.eps_twin(m)
        assert torch.equal(tw.proj_out_2.weight, m.proj_out_2.weight[rows]) and torch.equal(tw.proj_out_2.bias, m.proj_out_2.bias[rows])


@pytest.mark.parametrize("oc", [6, 12, 2])
def test_other_output_widths_are_refused_for_scoring_and_pair_plans(oc):
    """out_channels outside {C, 2C}: refused when a scoring plan or a pair plan is built, before anything touches the device, and the
    message names both numbers.  The plain forward's plan is not concerned."""
    m = DiT(**dict(TINY, out_channels=oc))
    dev = torch.device("cpu")
    for call in (lambda: m.make_plan(2, 3, None, dev, score=dict(x=None)), lambda: m.make_plan(2, 2, None, dev, eps_only=True),
                 lambda: m._label_plan(("pair",), 2, dev, (torch.zeros(2), torch.zeros(2))),
                 lambda: m._label_plan(("pair_session", 0), 2, dev, (torch.zeros(2), torch.zeros(2)))):
        with pytest.raises(NotImplementedError, match=rf"out_channels = {oc}\b.*in_channels = 4\b"):
            call()
    with pytest.raises(NotImplementedError, match=r"out_channels = 6\b.*in_channels = 4\b"):
        packing.eps_rows(2, 4, 6)


def test_step_fields_take_twice_the_channels_from_a_dit_only():
    from types import SimpleNamespace
    from diffusion_classifier_amd import _lib as L, trajectory as TJ
    dc = SimpleNamespace(pred_param="eps")
    f = TJ.step_fields(dc, DiT(**TINY), (2, 4, 8, 8), 0.0)
    assert (f["C"], f["patch"]) == (4, 2)
    with pytest.raises(L.DcamdError, match="out_channels"):
        TJ.step_fields(dc, DiT(**dict(TINY, out_channels=6)), (2, 4, 8, 8), 0.0)
    unet_like = SimpleNamespace(config=SimpleNamespace(out_channels=8))            # no backbone but DiT cuts its projection to eps
    with pytest.raises(L.DcamdError, match="out_channels"):
        TJ.step_fields(dc, unet_like, (2, 4, 8, 8), 0.0)
