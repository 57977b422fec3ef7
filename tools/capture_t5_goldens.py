"""Development-machine tool: writes tests/golden/t5_tiny.npz, the pinned oracle of the T5 encoder path.

A tiny `transformers.T5EncoderModel` is built from a config and a fixed seed (never `from_pretrained`: nothing is fetched), run once in
fp32 on the CPU, and its weights, inputs and outputs are stored:
  sd.<key>            every entry of the model's state dict (fp32)
  input_ids           [4, 20] int64, pad positions hold the pad id 0
  attention_mask      [4, 20] int64, right-padded, lengths (20, 7, 1, 13)
  last_hidden_state   [4, 20, 64] fp32 (all rows, as transformers returns them: pad queries still attend the valid keys)
  position_bias       [1, 2, 20, 20] fp32, block 0's relative-position bias without the mask
  bucket              [1023] int64, the bidirectional bucket of every relative distance -511 .. 511
  config              the T5Config fields the encoder reads, as a JSON string
d_model = 64 with 2 heads of 64 gives inner = 128 != d_model on purpose (as in t5-3b).

    python tools/capture_t5_goldens.py
"""
import json
import os

import numpy as np
import torch
from transformers import T5Config, T5EncoderModel
from transformers.models.t5.modeling_t5 import T5Attention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (20, 7, 1, 13)


def main():
    torch.manual_seed(1234)
    cfg = T5Config(vocab_size=48, d_model=64, d_kv=64, num_heads=2, d_ff=128, num_layers=2, feed_forward_proj="relu", dropout_rate=0)
    model = T5EncoderModel(cfg).eval().float()
    with torch.no_grad():                 # the default initialisation leaves every norm weight at 1: move them, or a dropped weight passes
        for k, p in model.named_parameters():
            if k.endswith("layer_norm.weight"):
                p.copy_(1.0 + 0.25 * torch.randn_like(p))
    L = 20
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, cfg.vocab_size, (len(LENGTHS), L), generator=g)
    mask = (torch.arange(L)[None, :] < torch.tensor(LENGTHS)[:, None]).long()
    ids = ids * mask
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask).last_hidden_state
        att = model.encoder.block[0].layer[0].SelfAttention
        pb = att.compute_bias(L, L)
        rel = torch.arange(-511, 512)
        bucket = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=cfg.relative_attention_num_buckets,
                                                       max_distance=cfg.relative_attention_max_distance)
    arrays = {"sd." + k: v.detach().float().numpy() for k, v in model.state_dict().items()}
    fields = ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads", "relative_attention_num_buckets",
              "relative_attention_max_distance", "layer_norm_epsilon", "feed_forward_proj")
    arrays.update(input_ids=ids.numpy(), attention_mask=mask.numpy(), last_hidden_state=out.numpy(), position_bias=pb.numpy(),
                  bucket=bucket.numpy(), config=np.array(json.dumps({k: getattr(cfg, k) for k in fields})))
    path = os.path.join(ROOT, "tests", "golden", "t5_tiny.npz")
    np.savez(path, **arrays)
    print(path, os.path.getsize(path), "bytes;", sorted(arrays))


if __name__ == "__main__":
    main()
