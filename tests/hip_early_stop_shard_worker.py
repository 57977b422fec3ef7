"""One rank of the sharded classify-with-early-stopping rehearsal on a single GPU (tests/test_gpu_early_stop.py).

`python hip_early_stop_shard_worker.py RANK WORLD PORT OUT.npz THR`: the small UNet from fixed seeds, a gloo group of WORLD ranks that all
use cuda:0, one classify with grid sharding on and `stop_margin_z = THR` (BS = 5, 3 classes, stages [2, 4, 7]); writes the labels, the
errors, t_done and every field of the posterior.  WORLD == 1 (no process group) is the single-process result to compare with; THR = 0
there means: take the median first-checkpoint z-score of an unstopped run (written out as `thr` for the other ranks)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(rank, world, port, out, thr):
    import numpy as np
    import torch
    import torch.distributed as dist
    import diffusion_classifier_amd as dca
    from diffusion_classifier_amd import posterior as P
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = "cuda:0"
    cfg = dict(pred_param="eps", schedule="cosine", noise_d=32, image_size=32, cfg_w=0.0, ema_beta=0.999, ema_warmup=0,
               ema_update_freq=1, encoder_type="nn", classes=3, n_stages=3, evaluation_per_stage=[2, 4, 7],
               n_keep_per_stage=[3, 2, 1], n_fast_classes=2, compute_dtype="f32", shard_grid=world > 1, units_per_launch=4)
    torch.manual_seed(5)
    m = dca.UNetCondition2D(**dca.small_unet_kwargs())
    dc = dca.DiffusionClassifier(m, dca.Config(**cfg)).to(dev)
    torch.manual_seed(6)
    BS, T = 5, 7
    x = (torch.rand(BS, 3, 32, 32) * 2 - 1).to(dev)
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 3, 32, 32).to(dev)
    if thr == 0.0:
        assert world == 1
        _, err = dc.classify(x, t=t, eps=eps, return_errors=True)
        thr = float(P.class_posterior_hip(err.to(dev), 2).margin_z.median())
    dc.config.stop_margin_z = thr
    lab, err, post, t_done = dc.classify(x, t=t, eps=eps, return_errors=True, return_posterior=True, return_trials=True)
    np.savez(out, thr=np.array([thr], dtype=np.float64), lab=lab.cpu().numpy(), err=err.numpy(), t_done=t_done.cpu().numpy(),
             **{k: v.cpu().numpy() for k, v in post._asdict().items()})
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], float(sys.argv[5]))
