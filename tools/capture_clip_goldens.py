"""Development-machine tool: writes tests/golden/clip_tiny.npz, the pinned oracle of the CLIP text encoder path.

A tiny `transformers.CLIPTextModel` is built from a config and a fixed seed (never `from_pretrained`: nothing is fetched), run in fp32
on the CPU with both `hidden_act` values (the same weights, only the config differs), and its weights, inputs and outputs are stored:
  sd.<key>                     every entry of the model's state dict, under the PUBLISHED key names (with the `text_model.` prefix, which
                               transformers 5.x's own CLIPTextModel.state_dict() drops), stored ONCE as float16
  input_ids, attention_mask    [4, 40] int64, right-padded, lengths (40, 7, 1, 33); pad positions hold id 0
  input_ids77                  [2, 77] int64, no mask (the full context, as Stable Diffusion feeds it)
  last_hidden_state.<act>      [4, 40, 128] fp32 with the mask, for act in (quick_gelu, gelu); all rows as transformers returns them
  last_hidden_state77.<act>    [2, 77, 128] fp32 without a mask
  config                       the CLIPTextConfig fields the encoder reads, as a JSON string (hidden_act = "quick_gelu")
Every LayerNorm weight is moved to 1 + 0.25 randn and every LayerNorm bias to 0.1 randn: the defaults (1 and 0) would let a dropped
parameter pass.  Before the model runs, every parameter is rounded to a float16-representable value, so that storing the state dict as
float16 is lossless: 283 k parameters in fp32 alone would exceed the 1 MiB a committed file may have.  The fp32 model that produced the
outputs has exactly the stored weights.

    python tools/capture_clip_goldens.py
"""
import json
import os

import numpy as np
import torch
from transformers import CLIPTextConfig, CLIPTextModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (40, 7, 1, 33)
FIELDS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings",
          "hidden_act", "layer_norm_eps")


def main():
    torch.manual_seed(4321)
    kw = dict(vocab_size=64, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=77)
    cfg = CLIPTextConfig(hidden_act="quick_gelu", **kw)
    model = CLIPTextModel(cfg).eval().float()
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "layer_norm" in k and k.endswith(".weight"):
                p.copy_(1.0 + 0.25 * torch.randn_like(p))
            elif "layer_norm" in k and k.endswith(".bias"):
                p.copy_(0.1 * torch.randn_like(p))
        for p in model.parameters():
            p.copy_(p.half().float())
    sd = {k: v for k, v in model.state_dict().items() if not k.endswith("position_ids")}
    sd = {(k if k.startswith("text_model.") else "text_model." + k): v for k, v in sd.items()}
    L = 40
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(1, cfg.vocab_size, (len(LENGTHS), L), generator=g)
    mask = (torch.arange(L)[None, :] < torch.tensor(LENGTHS)[:, None]).long()
    ids = ids * mask
    ids77 = torch.randint(1, cfg.vocab_size, (2, 77), generator=g)
    arrays = {"sd." + k: v.detach().half().numpy() for k, v in sd.items()}
    assert all(torch.equal(torch.from_numpy(arrays["sd." + k]).float(), v.float()) for k, v in sd.items())
    for act in ("quick_gelu", "gelu"):
        m = CLIPTextModel(CLIPTextConfig(hidden_act=act, **kw)).eval().float()
        m.load_state_dict(model.state_dict(), strict=True)
        with torch.no_grad():
            arrays["last_hidden_state." + act] = m(input_ids=ids, attention_mask=mask).last_hidden_state.numpy()
            arrays["last_hidden_state77." + act] = m(input_ids=ids77).last_hidden_state.numpy()
    arrays.update(input_ids=ids.numpy(), attention_mask=mask.numpy(), input_ids77=ids77.numpy(),
                  config=np.array(json.dumps({k: getattr(cfg, k) for k in FIELDS})))
    path = os.path.join(ROOT, "tests", "golden", "clip_tiny.npz")
    np.savez(path, **arrays)
    print(path, os.path.getsize(path), "bytes;", sorted(arrays))


if __name__ == "__main__":
    main()
