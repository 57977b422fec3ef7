"""Oracles of per-image early stopping (config key `stop_margin_z`; include/dcamd.h `dc_stage_stop`).

`stop_rule_loop`: the stop rule image by image as a plain sequential float32 loop (numpy scalars) — what `posterior.stop_rule_torch` and
the kernel must reproduce bit for bit.  `crafted_errors`: errors tensors with the rows that matter.  `standin_classifier` /
`reference_loop`: a classify with stopping written in the reference's style (one backbone call per trial and class column, over the
images still active), on the stand-in backbone of tests/standin.py."""
import numpy as np
import torch

from standin import TinyBackbone

F = np.float32
ROW_KINDS = 5


def _argmin_nan_last(mean, cand):
    best = -1
    for c in cand:                                            # ascending ids: a tie keeps the lower one
        if best < 0:
            best = c
            continue
        a, b = mean[c], mean[best]
        if (not np.isnan(a) and np.isnan(b)) or (not np.isnan(a) and not np.isnan(b) and a < b):
            best = c
    return best


def decide_loop(Eb, t_end):
    """(winner, runner, mean_w, margin_z) of one image from Eb [C, T]: posterior.py's definitions, every sum fp32, sequential, j ascending."""
    C = Eb.shape[0]
    with np.errstate(all="ignore"):
        mean, fin = [], []
        for c in range(C):
            s, cnt = F(0), 0
            for j in range(t_end):
                v = F(Eb[c, j])
                if v != F(np.inf):
                    s = F(s + v)
                    cnt += 1
            mean.append(F(F(s / F(cnt)) + F(0)) if cnt else F(np.inf))
            if cnt == t_end:
                fin.append(c)
        win = _argmin_nan_last(mean, fin)
        if win < 0:
            return -1, -1, F(np.nan), F(np.nan)
        run = _argmin_nan_last(mean, [c for c in fin if c != win])
        if np.isnan(mean[win]):
            return win, run, mean[win], F(np.nan)
        if run < 0:
            return win, run, mean[win], F(np.inf)
        sd = F(0)
        for j in range(t_end):
            sd = F(sd + F(F(Eb[run, j]) - F(Eb[win, j])))
        margin = F(sd / F(t_end))
        ss = F(0)
        for j in range(t_end):
            d = F(F(F(Eb[run, j]) - F(Eb[win, j])) - margin)
            ss = F(ss + F(d * d))
        var = F(ss / F(t_end - 1))
        z = F(margin / F(np.sqrt(F(var / F(t_end)))))
        return win, run, mean[win], z


def stop_rule_loop(E, t_end, z_stop, t_done, labels):
    """E [BS, C, T] float32, t_done int32 (0 = active), labels int64 -> (t_done, labels, active_ids [BS] with -1 behind the active ones,
    n_active, margin_z [BS] with NaN in the rows that were not active), all new arrays."""
    E = np.asarray(E, dtype=F)
    t_done, labels = np.array(t_done, dtype=np.int32), np.array(labels, dtype=np.int64)
    BS = E.shape[0]
    z = np.full(BS, np.nan, dtype=F)
    for b in range(BS):
        if t_done[b] != 0:
            continue
        win, _, mean_w, zb = decide_loop(E[b], t_end)
        z[b] = zb
        if win >= 0 and not np.isnan(mean_w) and zb >= F(z_stop):          # NaN >= x is false
            labels[b], t_done[b] = win, t_end
    ids = [b for b in range(BS) if t_done[b] == 0]
    active = np.full(BS, -1, dtype=np.int32)
    active[:len(ids)] = ids
    return t_done, labels, active, len(ids), z


def crafted_errors(BS, C, T=8, seed=0, shift=0):
    """Row b is of kind (b + shift) % 5:
      0  plain: separated class means, noise on top
      1  a NaN cell in a losing class, a class pruned after its first cell (+inf from j = 1 on; C > 3), garbage that is not read elsewhere
      2  an exact tie: class 1 repeats class 0 cell by cell (margin 0, variance 0: a NaN z-score), the others far above
      3  no runner-up: every class but one was never scored
      4  a NaN in every class: the winner's mean is NaN (must not stop)
    Kinds that need more classes than C has fall back to what C allows."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * BS + C)
    E = (1.0 + 0.3 * torch.arange(C, dtype=torch.float32)[None, :, None] * torch.rand(BS, 1, 1, generator=g)
         + 0.25 * torch.rand(BS, C, T, generator=g)).contiguous()
    perm = torch.stack([torch.randperm(C, generator=g) for _ in range(BS)])
    E = torch.gather(E, 1, perm[:, :, None].expand(BS, C, T)).contiguous()      # the winner is not always class 0
    inf, nan = float("inf"), float("nan")
    for b in range(BS):
        kind = (b + shift) % ROW_KINDS
        if kind == 1 and C > 1:
            lose = int(E[b].sum(dim=1).argmax())
            E[b, lose, 0] = nan
            if C > 3:
                other = [c for c in range(C) if c != lose][-1]
                E[b, other, 1:] = inf
        elif kind == 2 and C > 1:
            E[b, 2:] += 5.0
            E[b, 1] = E[b, 0]
        elif kind == 3:
            keep = b % C
            for c in range(C):
                if c != keep:
                    E[b, c] = inf
        elif kind == 4:
            E[b, :, 0] = nan
    return E


def crafted_state(BS, t_end, mode):
    """t_done / labels before the rule runs.  'all': every image active; 'none': every image decided earlier; 'some': every third."""
    t_done = torch.zeros(BS, dtype=torch.int32)
    labels = torch.full((BS,), -3, dtype=torch.int64)
    if mode == "none":
        t_done[:] = max(1, t_end - 1)
    elif mode == "some":
        t_done[1::3] = max(1, t_end - 1)
    labels[t_done != 0] = 7
    return t_done, labels


# ------------------------------------------------------------------------------------------------ classify on the stand-in
STANDIN_CFG = dict(pred_param="eps", schedule="cosine", noise_d=8, image_size=8, cfg_w=0.0, ema_beta=0.999, ema_warmup=0,
                   ema_update_freq=1, encoder_type="nn", classes=3, n_stages=3, evaluation_per_stage=[2, 4, 7],
                   n_keep_per_stage=[3, 2, 1], n_fast_classes=2)


def standin_classifier(dca, seed=0, **over):
    """The classifier on the stand-in backbone, its images and injected draws: BS = 5, 3 classes, T = 7."""
    torch.manual_seed(seed)
    bb = TinyBackbone(ch=3, hid=8, n_classes=3, mode="nn")
    dc = dca.DiffusionClassifier(bb, dca.Config(**dict(STANDIN_CFG, **over)))
    BS, T = 5, 7
    x = torch.rand(BS, 3, 8, 8) * 2 - 1
    t = torch.rand(T, BS)
    eps = torch.randn(T, BS, 3, 8, 8)
    return dc, x, t, eps


def reference_loop(dc, x, t, eps, z_stop):
    """classify with per-image stopping in the reference's style: stage by stage, trial by trial, one backbone call per class column at
    the batch of the images still active (the same sub-batches the product feeds: CPU kernels may differ in the last bit between batch
    compositions), the stage end by the reference's mean / topk, the stop rule by `stop_rule_loop`."""
    cfg = dc.config
    bb = dc.ema.ema_model
    BS, ncls = x.shape[0], cfg.classes
    ends = [0] + list(cfg.evaluation_per_stage)
    T = ends[-1]
    errors = torch.full((BS, ncls, T), float("inf"))
    classes = torch.arange(ncls).repeat(BS, 1)
    t_done, labels = np.zeros(BS, dtype=np.int32), np.zeros(BS, dtype=np.int64)
    active = list(range(BS))
    scored = 0
    for i in range(cfg.n_stages):
        bs = torch.tensor(active)
        for j in range(ends[i], ends[i + 1]):
            lam_row = dc.schedule(t[j].clone())
            al_row, sg_row = torch.sqrt(torch.sigmoid(lam_row.clone())), torch.sqrt(torch.sigmoid(-lam_row.clone()))
            full = len(active) == BS
            lam = lam_row if full else lam_row[bs]
            al = (al_row if full else al_row[bs]).view(-1, 1, 1, 1)
            sg = (sg_row if full else sg_row[bs]).view(-1, 1, 1, 1)
            e = eps[j] if full else eps[j][bs]
            z = al * (x if full else x[bs]) + sg * e
            for c in range(classes.shape[1]):
                lab = classes[bs, c]
                pred = bb(x=z, noise_labels=lam, encoder_hidden_states=dc.encode_text_prompt(lab))
                errors[bs, lab, j] = torch.norm((pred - e).view(len(active), -1), dim=1, p=2) ** 2
            scored += len(active)
        _, classes = torch.topk(errors[:, :, :ends[i + 1]].mean(dim=2), cfg.n_keep_per_stage[i], dim=1, largest=False)
        if i == cfg.n_stages - 1:
            for b in active:
                labels[b], t_done[b] = int(classes[b, 0]), T
            break
        t_done, labels, ids, n, _ = stop_rule_loop(errors.numpy(), ends[i + 1], z_stop, t_done, labels)
        active = ids[:n].tolist()
        if not active:
            break
    return labels, t_done, errors, scored
