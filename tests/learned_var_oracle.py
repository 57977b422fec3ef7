"""Test-side fp64 statements of the learned-range ancestral step (config.variance = "learned"; diffusers' variance_type =
"learned_range"): the abar table and the step scalars in plain Python floats, the step and its noise map per element, the sampling and
inversion loops over any fp64 network that returns 2C channels, `oracle.OracleDiT` in fp64 as that network, and the packing of NCHW
features into the layout the step kernels read.  Nothing here imports the package's ancestral code.  No GPU."""
import math

import torch

import oracle


def abar64(N=1000, b0=1e-4, b1=0.02, scaled=False):
    """abar_k of linspace betas ('ddpm_linear'; scaled: linspace of the roots, squared — 'scaled_linear') in Python floats."""
    out, abar = [], 1.0
    for i in range(N):
        f = i / (N - 1) if N > 1 else 0.0
        beta = (math.sqrt(b0) + (math.sqrt(b1) - math.sqrt(b0)) * f) ** 2 if scaled else b0 + (b1 - b0) * f
        abar *= 1.0 - beta
        out.append(abar)
    return out


def scalars64(abar, kt, ks):
    """The step k_t -> k_s in abar form: alpha_t, sigma_t, the mean's a and b, log beta, log of the posterior variance (clamped below at
    1e-20 as diffusers clamps it) and sd, the fixed posterior deviation."""
    at, as_ = abar[kt], abar[ks]
    beta = 1.0 - at / as_
    post = max((1.0 - as_) / (1.0 - at) * beta, 1e-20)
    return dict(alpha_t=math.sqrt(at), sigma_t=math.sqrt(1.0 - at), a=math.sqrt(at / as_) * (1.0 - as_) / (1.0 - at),
                b=math.sqrt(as_) * beta / (1.0 - at), log_hi=math.log(beta), log_lo=math.log(post), sd=math.sqrt(post))


def mean64(z, pc, pu, sc, w, v_param):
    """(mu, x): mu = a z + b x on the guided eps, x the unclipped data prediction; every tensor fp64."""
    pr = (1.0 + w) * pc - w * pu
    x = sc["alpha_t"] * z - sc["sigma_t"] * pr if v_param else (z - sc["sigma_t"] * pr) / sc["alpha_t"]
    return sc["a"] * z + sc["b"] * x, x


def sde64(vc, sc):
    """The learned deviation from the conditional variance channels vc (not clamped)."""
    fr = 0.5 * vc + 0.5
    return torch.exp(0.5 * (fr * sc["log_hi"] + (1.0 - fr) * sc["log_lo"]))


def step64(net, z, k, lab, null, sc, w, v_param, learned):
    """(mu, deviation, x) of one pass at step k: two calls of `net(z, k, labels) -> [BS, 2C, H, W]`, eps guided, v from the
    conditional call.  learned=False: the fixed posterior deviation (a float)."""
    Cc = z.shape[1]
    oc, ou = net(z, k, lab), net(z, k, null)
    mu, x = mean64(z, oc[:, :Cc], ou[:, :Cc], sc, w, v_param)
    return mu, sde64(oc[:, Cc:], sc) if learned else sc["sd"], x


def sample64(net, z0, lab, null, ks, abar, w, v_param, noise, learned=True):
    """The ancestral loop from z0 over the steps ks (k_0 > ... > k_n = 0) under the labels lab [BS]: n passes add noise[i] times the
    deviation, the last pass repeats step n - 1 and keeps the mean, unclipped -> (result, every latent the passes were fed, the
    largest magnitude among latents and data predictions)."""
    n = len(ks) - 1
    z, fed = z0.double(), []
    scale = float(z.abs().max())
    for i in range(n + 1):
        t = min(i, n - 1)
        fed.append(z)
        mu, dev, x = step64(net, z, ks[t], lab, null, scalars64(abar, ks[t], ks[t + 1]), w, v_param, learned)
        z = mu if i == n else mu + noise[i].double() * dev
        scale = max(scale, float(x.abs().max()), float(z.abs().max()))
    return z, fed, scale


def noise_maps64(net, x, lab, null, ks, abar, w, v_param, draws, learned=True):
    """Edit-friendly inversion: x_i = sqrt(abar_i) x + sqrt(1 - abar_i) draws[i], map i = (x_{i+1} - mu_i) / deviation_i
    -> (latents [n + 1], maps [n], deviations [n])."""
    n = len(ks) - 1
    lat = [math.sqrt(abar[k]) * x.double() + math.sqrt(1.0 - abar[k]) * e.double() for k, e in zip(ks, draws)]
    maps, devs = [], []
    for i in range(n):
        mu, dev, _ = step64(net, lat[i], ks[i], lab, null, scalars64(abar, ks[i], ks[i + 1]), w, v_param, learned)
        maps.append((lat[i + 1] - mu) / dev)
        devs.append(dev)
    return lat, maps, devs


def dit64(m):
    """`oracle.OracleDiT` in fp64 with the weights of the HIP model `m` -> net(z, k, labels) for the loops above."""
    kw = {k: getattr(m.config, k) for k in ("num_attention_heads", "attention_head_dim", "in_channels", "out_channels", "num_layers",
                                            "sample_size", "patch_size", "num_embeds_ada_norm")}
    o = oracle.OracleDiT(**kw)
    o.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    o = o.double().requires_grad_(False)
    for b in o.transformer_blocks:
        # the oracle's sinusoid of the step is formed in fp32 whatever it is given: everything behind it runs in fp64
        b.norm1.emb.timestep_embedder.linear_1.register_forward_pre_hook(lambda mod, args: (args[0].double(),))

    @torch.no_grad()
    def net(z, k, labels):
        return o(z, torch.full((z.shape[0],), float(k), dtype=torch.float64), labels)
    return net


def pack_pred(pc, pu, vc, patch, ld, fstride, fill=float("nan")):
    """NCHW f32 features -> the prediction the step kernels read, [2n, H/p, W/p, ld] f32: row 2b the conditional features of image b
    (eps pc[b] at (py p + px) fstride + c, variance vc[b] C behind; patch <= 1: at c and C + c of pixel row p), row 2b + 1 the null
    row's eps pu[b].  Every slot the kernels must not read — padding, the null row's variance features — holds `fill`.
    vc None: eps alone (fstride = C is then the layout of the fixed step and of dc_solver_step)."""
    n, Cc, H, W = pc.shape
    p = max(int(patch), 1)
    fs = fstride if patch > 1 else 0
    pred = torch.full((2 * n, H // p, W // p, ld), fill, dtype=torch.float32)
    for py in range(p):
        for px in range(p):
            at = (py * p + px) * fs
            pred[0::2, :, :, at:at + Cc] = pc[:, :, py::p, px::p].permute(0, 2, 3, 1)
            if vc is not None:
                pred[0::2, :, :, at + Cc:at + 2 * Cc] = vc[:, :, py::p, px::p].permute(0, 2, 3, 1)
            pred[1::2, :, :, at:at + Cc] = pu[:, :, py::p, px::p].permute(0, 2, 3, 1)
    return pred.contiguous()
