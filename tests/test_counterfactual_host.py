"""CPU: `DiffusionClassifier.counterfactual` on a foreign backbone against K calls of `sample` with the seed reset in front of each (the
written statement of the function), the difference maps against their torch statement, the refusals, and the C-ABI surface of
dc_ddpm_step_shared / dc_abs_diff_map."""
import ctypes
import os
import re

import pytest
import torch

import diffusion_classifier_amd as dca
from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import counterfactual as CF
from helpers import load_case, standin_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 17


def _dc(pred_param="eps", **extra):
    g, cfg = load_case("1stage_eps")
    cfg.update(pred_param=pred_param, cfg_w=1.5, sampling_steps=4, **extra)
    dc = dca.DiffusionClassifier(standin_from(g, cfg), dca.Config(**cfg))
    dc.encoder.weight.data.copy_(torch.from_numpy(g["encoder.weight"]))
    return dc, torch.from_numpy(g["x"]), cfg


def _reseeded(dc, x, cl, from_t):
    """K calls of `sample`, the seed reset in front of each: [BS, K, C, H, W]."""
    outs = []
    for k in range(cl.shape[1]):
        torch.manual_seed(SEED)
        outs.append(dc.sample(x, cl[:, k], from_t=from_t))
    return torch.stack(outs, dim=1)


def _maps(samples, base):
    """The torch statement: sum over channels, ascending, of |samples[b, k, c] - base[b, (k,) c]|."""
    base = base if base.dim() == samples.dim() else base.unsqueeze(1)
    out = torch.zeros(samples.shape[:2] + samples.shape[3:])
    for c in range(samples.shape[2]):
        out = out + (samples[:, :, c] - base[:, :, c]).abs()
    return out


# ------------------------------------------------------------------------------------------------ equality with reseeded sample()
@pytest.mark.parametrize("pred_param", ["eps", "v"])
@pytest.mark.parametrize("from_t", [0.5, 1])
@pytest.mark.parametrize("per_image", [False, True])
def test_samples_equal_k_reseeded_sample_calls(pred_param, from_t, per_image):
    dc, x, cfg = _dc(pred_param)
    BS, ncls = x.shape[0], cfg["classes"]
    if per_image:
        classes = torch.stack([(torch.arange(3) + b) % ncls for b in range(BS)])          # [BS, K]: another list per image
        cl = classes
    else:
        classes = torch.tensor([ncls - 1, 0, 1])                                          # [K]: the same for every image
        cl = classes.unsqueeze(0).expand(BS, -1)
    want = _reseeded(dc, x, cl, from_t)
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, classes, from_t)
    assert isinstance(cf, dca.Counterfactuals) and cf._fields == ("samples", "classes", "maps")
    assert cf.samples.dtype == torch.float32 and tuple(cf.samples.shape) == (BS, 3) + tuple(x.shape[1:])
    assert cf.classes.dtype == torch.int64 and torch.equal(cf.classes, cl)
    for k in range(3):
        assert torch.equal(cf.samples[:, k], want[:, k]), (k, (cf.samples[:, k] - want[:, k]).abs().max())
    assert not torch.equal(want[:, 0], want[:, 1])                                        # the labels do matter
    # the generator stands where one sample() call leaves it
    after = torch.rand(1)
    torch.manual_seed(SEED)
    dc.sample(x, cl[:, 0], from_t=from_t)
    assert torch.equal(after, torch.rand(1))


def test_default_classes_are_all_of_them_and_duplicates_share_a_trajectory():
    dc, x, cfg = _dc()
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x)
    assert cf.samples.shape[1] == cfg["classes"] and torch.equal(cf.classes[0], torch.arange(cfg["classes"]))
    torch.manual_seed(SEED)
    dup = dc.counterfactual(x, torch.tensor([2, 2, 0]))
    assert torch.equal(dup.samples[:, 0], dup.samples[:, 1]) and torch.equal(dup.samples[:, 0], cf.samples[:, 2])
    assert torch.equal(dup.samples[:, 2], cf.samples[:, 0])


# ------------------------------------------------------------------------------------------------ maps
def test_maps_equal_the_torch_statement_for_the_input_and_for_a_class():
    dc, x, cfg = _dc("v")
    BS = x.shape[0]
    classes = torch.tensor([1, 0, 2])
    torch.manual_seed(SEED)
    cf = dc.counterfactual(x, classes, 0.5)
    assert cf.maps.dtype == torch.float32 and tuple(cf.maps.shape) == (BS, 3) + tuple(x.shape[2:])
    assert torch.equal(cf.maps, _maps(cf.samples, x))
    against = torch.tensor([0, 2] * BS)[:BS]                                              # columns 1 and 2, alternating
    torch.manual_seed(SEED)
    cfa = dc.counterfactual(x, classes, 0.5, against=against)
    assert torch.equal(cfa.samples, cf.samples)
    col = torch.tensor([1, 2] * BS)[:BS]
    base = cf.samples[torch.arange(BS), col]
    assert torch.equal(cfa.maps, _maps(cf.samples, base))
    assert float(cfa.maps[torch.arange(BS), col].abs().max()) == 0.0                      # a trajectory against itself
    assert float(cfa.maps.max()) > 0.0
    with pytest.raises(ValueError, match="against"):
        dc.counterfactual(x, classes, 0.5, against=torch.full((BS,), 3))                  # a class that is not listed
    with pytest.raises(ValueError, match="against"):
        dc.counterfactual(x, classes, 0.5, against="output")
    with pytest.raises(ValueError, match="against"):
        dc.counterfactual(x, classes, 0.5, against=torch.zeros(BS + 1, dtype=torch.int64))


def test_base_rows_take_the_first_column_that_holds_the_class():
    cl = torch.tensor([[3, 1, 3], [0, 2, 2]])
    assert CF.base_rows(torch.tensor([3, 2]), cl).tolist() == [0, 0, 0, 4, 4, 4]
    assert CF.base_rows(torch.tensor([1, 0]), cl).tolist() == [1, 1, 1, 3, 3, 3]
    assert CF.image_chunks(5, 3, 12) == [(0, 2), (2, 4), (4, 5)]
    assert CF.image_chunks(5, 3, 1) == [(b, b + 1) for b in range(5)]                     # one image at least
    assert CF.image_chunks(4, 2, 1000) == [(0, 4)]
    assert CF.image_chunks(5, 1, 8) == [(0, 3), (3, 5)]                                   # equal chunks, not 4 + 1


# ------------------------------------------------------------------------------------------------ refusals
def test_argument_validation():
    dc, x, cfg = _dc()
    ncls, BS = cfg["classes"], x.shape[0]
    for bad in (0, 0.0, -0.5, 1.0001, 2, float("nan")):
        with pytest.raises(ValueError, match="from_t"):
            dc.counterfactual(x, None, bad)
    for bad in (torch.tensor([0, ncls]), torch.tensor([-1, 0]), torch.tensor([[0, ncls + 3]] * BS)):
        with pytest.raises(ValueError, match="class ids"):
            dc.counterfactual(x, bad)
    for bad in (torch.zeros(0, dtype=torch.int64), torch.zeros(BS + 1, 2, dtype=torch.int64), torch.zeros(1, 1, 2, dtype=torch.int64),
                torch.tensor([0.0, 1.0])):
        with pytest.raises(ValueError, match="classes"):
            dc.counterfactual(x, bad)
    with pytest.raises(L.DcamdError, match="philox"):
        dc.counterfactual(x, rng="philox")                                                # a foreign backbone has no device RNG
    with pytest.raises(ValueError, match="rng"):
        dc.counterfactual(x, rng="torch")
    # a refusal consumed no random numbers
    torch.manual_seed(SEED)
    a = torch.rand(1)
    torch.manual_seed(SEED)
    with pytest.raises(ValueError):
        dc.counterfactual(x, torch.tensor([0, ncls]))
    assert torch.equal(a, torch.rand(1))


# ------------------------------------------------------------------------------------------------ C-ABI
def test_struct_fields_match_the_header_and_the_abi_version_stays():
    src = open(os.path.join(ROOT, "include", "dcamd.h")).read()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(L.DdpmStepSharedParams) == 4 * ptr + 16 * 4
    assert ctypes.sizeof(L.AbsDiffMapParams) == 4 * ptr + 6 * 4
    # dc_ddpm_step keeps its struct
    assert ctypes.sizeof(L.DdpmStepParams) == 4 * ptr + 14 * 4
    lib = L.lib()
    for name in ("dc_ddpm_step_shared", "dc_abs_diff_map"):
        assert name in L.EXPORTS and getattr(lib, name) is not None
        assert re.search(r"\bint " + name + r"\(", src)
    assert lib.dc_abi_version() == 5 and L.ABI_VERSION == 5
    assert re.search(r"#define DC_ABI_VERSION 5\b", src)


def _step_params(**over):
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    kw = dict(z=a, pred=a, noise=a, out=a, n=6, C=1, H=2, W=2, ld=4, patch=0, v_param=0, noise_div=3, w=1.0, alpha_t=1.0, sigma_t=1.0,
              alpha_s=1.0, c=0.5, sd=0.5, one_plus_w=2.0, pad_=0)
    kw.update(over)
    return L.DdpmStepSharedParams(**kw), buf


@pytest.mark.parametrize("over,code,word", [
    (dict(noise_div=0), -1, "noise_div=0"), (dict(noise_div=-2), -1, "noise_div=-2"), (dict(noise_div=4), -1, "noise_div=4"),
    (dict(n=7), -1, "noise_div=3"), (dict(z=None), -1, "null"), (dict(out=None), -1, "null"),
    (dict(n=0), -2, "extents"), (dict(ld=0), -2, "extents"), (dict(patch=3, ld=16), -2, "patch=3"),
])
def test_ddpm_step_shared_refuses_before_any_launch(over, code, word):
    """A bad noise_div (and every other argument check) answers without a GPU and touches no memory."""
    lib = L.lib()
    p, _keep = _step_params(**over)
    assert lib.dc_ddpm_step_shared(ctypes.byref(p), None) == code
    assert word in lib.dc_last_error().decode()
    assert lib.dc_ddpm_step_shared(None, None) == -1


@pytest.mark.parametrize("over,code", [(dict(a=None), -1), (dict(r_of_a=None), -1), (dict(n=0), -2), (dict(m=0), -2), (dict(C=0), -2)])
def test_abs_diff_map_refuses_before_any_launch(over, code):
    lib = L.lib()
    buf = (ctypes.c_float * 16)()
    a = ctypes.addressof(buf)
    kw = dict(a=a, r=a, r_of_a=a, out=a, n=1, m=1, C=1, H=2, W=2, pad_=0)
    kw.update(over)
    assert lib.dc_abs_diff_map(ctypes.byref(L.AbsDiffMapParams(**kw)), None) == code
    assert lib.dc_abs_diff_map(None, None) == -1
