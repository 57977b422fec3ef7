"""Development-machine tool: writes tests/golden/clip_proj_tiny.npz, the pinned oracle of CLIPTextEncoderWithProjection.

A tiny `transformers.CLIPTextModelWithProjection` is built from a config and a fixed seed (never `from_pretrained`: nothing is fetched),
run in fp32 on the CPU, and its weights, inputs and outputs are stored.  Three layers, so that the penultimate state is neither the first
layer's output nor the last one's.  The same weights run under both `hidden_act` values and under both of transformers' EOS rules:
  case "argmax"   config.eos_token_id = 2, the legacy config Stable Diffusion XL's text_encoder_2 carries: the pooled position is
                  argmax(input_ids[b]); the ids' largest value (vocab_size - 1) is the EOS and stands at the prompt's last position
  case "first"    config.eos_token_id = 7: the pooled position is the FIRST position that holds 7; every prompt holds it twice, once in
                  the middle (or at position 0) and once at its last position, and holds larger ids too (argmax would pick another row)
Stored:
  sd.<key>                           every entry of the state dict under the PUBLISHED key names (`text_model.` prefix, and
                                     `text_projection.weight` without one), stored ONCE as float16 (every parameter is rounded to a
                                     float16-representable value before the model runs, so this is lossless)
  input_ids.<case>, attention_mask   [3, 16] int64, right-padded, lengths (16, 7, 2); pad positions hold id 0
  hidden_states_m2.<case>.<act>[.nomask]  hidden_states[-2]: [3, 16, 64] fp32, the residual stream after 2 of the 3 layers, no final LayerNorm
  last_hidden_state.<case>.<act>     [3, 16, 64] fp32, with the mask
  text_embeds.<case>.<act>[.nomask]  [3, 64] fp32
  config                             the config fields the encoder reads, as a JSON string (hidden_act = "quick_gelu", eos_token_id = 2)
  eos_first                          the eos_token_id of case "first"

    python tools/capture_clip_proj_golden.py
"""
import json
import os

import numpy as np
import torch
from transformers import CLIPTextConfig, CLIPTextModelWithProjection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (16, 7, 2)
EOS_FIRST = 7
FIELDS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings",
          "hidden_act", "layer_norm_eps", "projection_dim", "eos_token_id")


def main():
    torch.manual_seed(1234)
    kw = dict(vocab_size=100, hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=3,
              max_position_embeddings=16, projection_dim=64, bos_token_id=0, pad_token_id=1)
    cfg = CLIPTextConfig(hidden_act="quick_gelu", eos_token_id=2, **kw)
    model = CLIPTextModelWithProjection(cfg).eval().float()
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "layer_norm" in k and k.endswith(".weight"):
                p.copy_(1.0 + 0.25 * torch.randn_like(p))
            elif "layer_norm" in k and k.endswith(".bias"):
                p.copy_(0.1 * torch.randn_like(p))
            elif k.endswith("text_projection.weight"):
                p.copy_(0.2 * torch.randn_like(p))
        for p in model.parameters():
            p.copy_(p.half().float())
    sd = {k: v for k, v in model.state_dict().items() if not k.endswith("position_ids")}
    sd = {(k if k.startswith(("text_model.", "text_projection.")) else "text_model." + k): v for k, v in sd.items()}
    assert "text_projection.weight" in sd and not any(k.startswith("text_projection.") and k != "text_projection.weight" for k in sd)
    L, V = 16, cfg.vocab_size
    g = torch.Generator().manual_seed(9)
    lens = torch.tensor(LENGTHS)
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    ids_a = torch.randint(3, V - 1, (len(LENGTHS), L), generator=g)          # no 2, no V - 1 inside
    ids_f = torch.randint(EOS_FIRST + 1, V, (len(LENGTHS), L), generator=g)  # no 7 inside, larger ids everywhere
    for b, n in enumerate(LENGTHS):
        ids_a[b, n - 1] = V - 1
        ids_f[b, n - 1] = EOS_FIRST
        ids_f[b, (n - 1) // 2] = EOS_FIRST                                    # the first occurrence: the pooled row
    ids_a, ids_f = ids_a * mask, ids_f * mask
    arrays = {"sd." + k: v.detach().half().numpy() for k, v in sd.items()}
    assert all(torch.equal(torch.from_numpy(arrays["sd." + k]).float(), v.float()) for k, v in sd.items())
    for case, ids, eos in (("argmax", ids_a, 2), ("first", ids_f, EOS_FIRST)):
        arrays["input_ids." + case] = ids.numpy()
        for act in ("quick_gelu", "gelu"):
            m = CLIPTextModelWithProjection(CLIPTextConfig(hidden_act=act, eos_token_id=eos, **kw)).eval().float()
            m.load_state_dict(model.state_dict(), strict=True)
            with torch.no_grad():
                for tag, am in (("", mask), (".nomask", None)):
                    out = m(input_ids=ids, attention_mask=am, output_hidden_states=True)
                    assert len(out.hidden_states) == cfg.num_hidden_layers + 1
                    arrays[f"hidden_states_m2.{case}.{act}{tag}"] = out.hidden_states[-2].numpy()
                    arrays[f"text_embeds.{case}.{act}{tag}"] = out.text_embeds.numpy()
                    if am is not None:
                        arrays[f"last_hidden_state.{case}.{act}"] = out.last_hidden_state.numpy()
    arrays.update(attention_mask=mask.numpy(), eos_first=np.array(EOS_FIRST),
                  config=np.array(json.dumps({k: getattr(cfg, k) for k in FIELDS})))
    path = os.path.join(ROOT, "tests", "golden", "clip_proj_tiny.npz")
    np.savez(path, **arrays)
    print(path, os.path.getsize(path), "bytes;", len(arrays), "arrays")


if __name__ == "__main__":
    main()
