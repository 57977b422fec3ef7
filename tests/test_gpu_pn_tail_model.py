"""GPU: the tail fold at model level — the CIFAR-10 UNet in bf16 with conv_norm_out + SiLU + conv_out folded into the last ResNet conv
(the default) against the same plan with `DCAMD_NO_TAIL_FOLD` (producer-normalising conv + conv3_thin).  The two plans feed conv_out the
same bits and differ in the order of its fp32 sums only.

REL_BOUND: relative L2 difference of the two predictions, measured 1.9e-7 on the forward below and 1.4e-7 as the largest relative
difference of the eps-MSE errors of the classify below (MI355X); the bound is a decade above the larger figure."""
import pytest
import torch

import diffusion_classifier_amd as dca
from test_gpu_model import BASE, make_pair, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_BOUND = 2e-6
TAIL, THIN = "conv3_halo<bf16,4w,pn,tail>", "conv3_thin<bf16>"


def _switch(monkeypatch, on):
    if on:
        monkeypatch.delenv("DCAMD_NO_TAIL_FOLD", raising=False)
    else:
        monkeypatch.setenv("DCAMD_NO_TAIL_FOLD", "1")


def test_cifar_unet_bf16_forward_with_and_without_the_tail_fold(monkeypatch):
    kw = dca.cifar10_unet_kwargs()
    torch.manual_seed(23)
    x, lam, emb = torch.randn(5, 3, 32, 32), torch.tensor([4.0, 0.5, -6.0, 1.0, 9.0]), torch.randn(5, 1, 128)
    outs, fams = [], []
    for on in (True, False):
        _switch(monkeypatch, on)
        m, _ = make_pair(kw, seed=7)
        m = m.to(DEV).set_compute_dtype("bf16")
        outs.append(m(x.to(DEV), lam.to(DEV), encoder_hidden_states=emb.to(DEV)).float().cpu())
        plan = next(iter(m._plans.values()))
        fams.append([mt.get("family", "") for mt in plan.pb.meta])
    assert fams[0].count(TAIL) == 1 and THIN not in fams[0], fams[0]
    assert TAIL not in fams[1] and fams[1].count(THIN) == 1, fams[1]
    assert len(fams[0]) == len(fams[1]) - 1                      # one op fewer: the thin conv is gone, nothing took its place
    assert torch.isfinite(outs[0]).all()
    r = relerr(outs[0], outs[1])
    print(f"\ntail fold, cifar10 unet bf16 forward: relative L2 difference on / off {r:.3e}")
    assert r < REL_BOUND, r
    assert dca._lib.lib().dc_pn_timeouts() == 0


def test_classify_bf16_with_and_without_the_tail_fold(monkeypatch):
    cfg = dict(BASE, compute_dtype="bf16", evaluation_per_stage=[2])
    torch.manual_seed(24)
    BS, T = 2, 2
    x = torch.rand(BS, 3, 32, 32) * 2 - 1
    t, eps = torch.rand(T, BS), torch.randn(T, BS, 3, 32, 32)
    labels, errors = [], []
    for on in (True, False):
        _switch(monkeypatch, on)
        m, _ = make_pair(dca.cifar10_unet_kwargs(), seed=11)
        dc = dca.DiffusionClassifier(m, dca.Config(**cfg)).to(DEV)
        lab, err = dc.classify(x.to(DEV), t=t, eps=eps.to(DEV), return_errors=True)
        dc.check_device_errors()
        labels.append(lab.cpu())
        errors.append(err.double().cpu())
    assert torch.equal(labels[0], labels[1])
    r = ((errors[0] - errors[1]).abs() / errors[1].abs()).max().item()
    print(f"\ntail fold, classify 2 images x 2 trials: largest relative difference of the errors on / off {r:.3e}")
    assert r < REL_BOUND, r
