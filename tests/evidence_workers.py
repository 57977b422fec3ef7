"""Workers of tests/test_evidence_host.py: one classify(return_evidence=True) on the stand-in backbone, alone or as one rank of a gloo
group with grid sharding on (modelled on tests/test_dist_gloo.py's worker).

The ranks of a sharded call feed the backbone other sub-batches than one process does, and torch's CPU kernels may differ in the last
bit between batch compositions.  What is under test is the accumulation — integer sums and one all-reduce, exact whatever the split — so
the backbone here scores one row at a time: a row's prediction then has the same bits in every batch, and every field of the result
must be bit-identical across world sizes."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rowwise_standin():
    from standin import TinyBackbone

    class RowwiseBackbone(TinyBackbone):
        def forward(self, x, noise_labels, encoder_hidden_states=None):
            one = super().forward
            return torch.cat([one(x[r:r + 1], noise_labels[r:r + 1], encoder_hidden_states[r:r + 1]) for r in range(x.shape[0])])

    return RowwiseBackbone


def standin_run(shard, group=None):
    """BS = 5, 3 classes, stages [2, 4, 7] keeping [3, 2, 1] (early_stop_oracle.STANDIN_CFG), injected draws -> dict of numpy arrays."""
    import diffusion_classifier_amd as dca
    import early_stop_oracle as SO
    torch.manual_seed(0)
    bb = _rowwise_standin()(ch=3, hid=8, n_classes=3, mode="nn")
    dc = dca.DiffusionClassifier(bb, dca.Config(**dict(SO.STANDIN_CFG, shard_grid=bool(shard))))
    BS, T = 5, 7
    x = torch.rand(BS, 3, 8, 8) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 3, 8, 8)
    lab, err, post, ev = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, return_evidence=True, group=group)
    out = dict(lab=lab.numpy(), err=err.numpy(), probs=post.probs.numpy())
    out.update({k: v.numpy() for k, v in ev._asdict().items()})
    return out


def gloo_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    q.put((rank, standin_run(shard=True)))
    dist.barrier()
    dist.destroy_process_group()
