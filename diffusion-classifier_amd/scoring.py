"""How `classify` runs: the two runners behind it, the control block of a launch and the host index arithmetic that fills it (`ControlBlock`,
`launch_size`, `index_blocks`, `eps_runs`: no device work, importable and callable without a GPU).

The reference walks a Python double loop — T trials x C classes sequential eager backbone calls at batch BS (:686-714).  Here the
(image, trial, class) grid is flattened into micro-batches of work units; each micro-batch is ONE native call (`dc_run_plan`) that
enqueues q_sample -> backbone -> eps-MSE on the HIP stream, with z_t / eps materialised once per (image, trial), class-independent
layers computed once per (image, trial), and errors scattered straight into `errors[b, class, j]`.  The stage end (mean over trials,
top-k smallest, :718-721) runs ON THE DEVICE for the HIP backbones (`dc_stage_topk`, `dc_reduce_argmin`: fixed summation order, ties
to the lower class id, NaN last — identical on every rank), and so do the next stage's work-unit maps (`dc_stage_maps`): nothing is
copied to the host between stages as long as `stop_margin_z` is unset.  A foreign `nn.Module` backbone takes the reference's own torch
ops (`_ForeignRunner.stage_end`).

Per-image early stopping (`config.stop_margin_z`; the rule: posterior.py).  HIP backbones decide on the device (`stage_stop`) and build
the next stage's maps over the undecided images there (`dc_stage_maps_rows`); such a stage is sized by `launch_size`'s ladder.  Under
grid sharding every rank holds the same errors after each gather, takes the same decisions and builds the same image list: no extra
collective.
"""
import torch

from . import _lib as L
from . import evidence as EV
from . import loss as LS
from . import posterior as P
from . import trajectory as TJ


class ControlBlock:
    """The int32 control block of one launch of n_bj (trial, image) pairs x k classes, stated once:
        | pair_id (int64 x n_bj) | lam | alpha | sigma | img_of_bj | ctx_of_unit x U | out_index x U |        U = n_bj * k
    `fields[name]` = (word slice, dtype); the first `host_words` words are the host's in every stage (pair ids, lambda / alpha /
    sigma, image map), the two unit maps behind them come from `dc_stage_maps` once the classes live on the device.  pair_id stands
    first so that its int64 view is 8-byte aligned."""

    def __init__(self, n_bj, k):
        self.n_bj, self.k, self.U = n_bj, k, n_bj * k
        f32, i32 = torch.float32, torch.int32
        self.fields, o = {}, 0
        for name, n, dt in (("pair_id", 2 * n_bj, torch.int64), ("lam", n_bj, f32), ("alpha", n_bj, f32), ("sigma", n_bj, f32),
                            ("img_of_bj", n_bj, i32), ("ctx_of_unit", self.U, i32), ("out_index", self.U, i32)):
            self.fields[name] = (slice(o, o + n), dt)
            o += n
        self.words, self.host_words = o, self.fields["img_of_bj"][0].stop

    def view(self, block, name):
        """Field `name` of a block (a [words] int32 tensor, host or device) in the field's own dtype."""
        sl, dt = self.fields[name]
        return block[sl] if dt == torch.int32 else block[sl].view(dt)


def launch_size(n_pairs, cap, subset):
    """(trial, image) pairs per launch for a stage of n_pairs at a cap of `cap` pairs."""
    if not subset:
        n_bj = min(n_pairs, cap)
        # equal micro-batches: 800 pairs at a cap of 256 run as 4 x 200, not 3 x 256 + 32 padded to 256 (slots past the last pair
        # repeat a pair into the dump cell: 28 % wasted work on the CheXpert workload at 8 images per step)
        return -(-n_pairs // -(-n_pairs // n_bj))
    # a stage over the undecided images: their number changes from batch to batch, and every n_bj is a plan with an arena of
    # its own — take the smallest rung of cap, cap/2, ... cap/32 that holds the pairs (cap when there are more) and pad the
    # last micro-batch with dump-cell slots: at most 6 plan sizes per k, the default score_plan_cache
    n_bj = cap
    for _ in range(5):
        if n_bj == 1 or -(-n_bj // 2) < n_pairs:
            break
        n_bj = -(-n_bj // 2)
    return n_bj


def index_blocks(layout, pairs, classes, ncls, T, dump):
    """The index part of the control blocks of a stage, which depends on (pairs, classes) only -> (int32 template [n_mb, words], the
    (js, bs) trial / image tensors of every micro-batch).  Slots past the last pair repeat the chunk's first pair and write to the
    `dump` cell (BS * ncls * T); the lambda / alpha / sigma words stay zero; classes None (they live on the device): so do the maps."""
    n_bj = layout.n_bj
    n_mb = -(-len(pairs) // n_bj)
    tmpl = torch.zeros((n_mb, layout.words), dtype=torch.int32)
    jsb = []
    for m in range(n_mb):
        chunk = pairs[m * n_bj:(m + 1) * n_bj]
        row = tmpl[m]
        pad = n_bj - len(chunk)
        js = torch.tensor([p[0] for p in chunk] + [chunk[0][0]] * pad)
        bs = torch.tensor([p[1] for p in chunk] + [chunk[0][1]] * pad)
        layout.view(row, "pair_id").copy_(bs * T + js)
        layout.view(row, "img_of_bj").copy_(bs.to(torch.int32))
        if classes is not None:
            cl = classes[bs]                                       # [n_bj, k] class id of every unit
            oi = (bs[:, None] * ncls + cl) * T + js[:, None]       # errors[b, class, j], flat
            if pad:
                oi[len(chunk):] = dump
            layout.view(row, "ctx_of_unit").copy_(cl.reshape(-1).to(torch.int32))
            layout.view(row, "out_index").copy_(oi.reshape(-1).to(torch.int32))
        jsb.append((js, bs))
    return tmpl, jsb


def eps_runs(chunk):
    """The runs of consecutive images of one trial in a chunk of (trial, image) pairs, as (slot, trial, first image, count)."""
    runs, r = [], 0
    while r < len(chunk):
        j, b0 = chunk[r]
        r1 = r
        while r1 < len(chunk) and chunk[r1][0] == j and chunk[r1][1] == b0 + (r1 - r):
            r1 += 1
        runs.append((r, j, b0, r1 - r))
        r = r1
    return runs


class _Runner:
    """What the two runners share; `posterior` / `_evidence` are the torch or the HIP functions, `dev` the device their results live on."""

    ev = None            # (acc, bad) per-stage evidence accumulators of a return_evidence call (evidence.py), `ev_stage` the running stage

    def __init__(self, dc, backbone, x, T, draws, dev, pixel_w=None):
        self.dc, self.bb, self.x, self.T, self.d, self.dev = dc, backbone, x, T, draws, dev
        self.score_loss = dc.score_loss      # (kind, huber delta) of this call (DiffusionClassifier.loss sets l2 whatever the config says)
        # the loss weights of this call (loss.py), both None on the plain path: pixel_w fp32 [BS, H, W] on the runner's device,
        # trial_w fp32 [T, BS] on the host, where the draws live
        self.pixel_w = None if pixel_w is None else pixel_w.to(dev)
        self.trial_w = draws.get("weight")
        # what the backbone is fed as its time input: the log-SNR itself, unless the draws carry a `label` of their own (the
        # 'scaled_linear' schedule: the DDPM step; DiffusionClassifier.noise_labels)
        self.label = draws.get("label", draws["logsnr"])

    def evidence_begin(self, n_stages):
        BS, _, H, W = self.x.shape
        self.ev, self.ev_stage = EV.new_slabs(n_stages, BS * self.dc.config.classes, H * W, self.dev), 0

    def evidence(self, stage_ends, n_eval, winner):
        return self._evidence(self.ev[0], self.ev[1], stage_ends, n_eval, winner, self.x.shape[2], self.x.shape[3])

    def stop_state(self):
        BS = self.x.shape[0]
        return torch.zeros(BS, dtype=torch.int32, device=self.dev), torch.zeros(BS, dtype=torch.int64, device=self.dev)


class _ForeignRunner(_Runner):
    """Backbones that are plain nn.Modules (not this package's HIP backbones): the reference's
    semantics in eager torch on x.device, one backbone call per (trial, class column) at batch BS
    (reference :686-714).  This is NOT a fallback for UNetCondition2D / DiT — those always take
    _HipRunner and raise when libdcamd or the GPU is missing."""

    posterior, _evidence = staticmethod(P.class_posterior_torch), staticmethod(EV.evidence_maps_torch)

    def __init__(self, dc, backbone, x, T, draws, pixel_w=None):
        if draws["philox"]:
            raise L.DcamdError("rng='philox' needs a HIP backbone (UNetCondition2D / DiT)")
        dc._refuse_ragged_on_foreign()
        super().__init__(dc, backbone, x, T, draws, x.device, pixel_w)
        self.err = torch.full((x.shape[0], dc.config.classes, T), float("inf"), device=x.device)

    def errors(self):
        return self.err

    def stage_end(self, errors, t_end, num_keep, last=False):
        # identical torch ops to the reference (:718-721)
        end_of_stage_errors = errors.cpu()[:, :, :t_end].mean(dim=2)
        _, keep_indices = torch.topk(end_of_stage_errors, num_keep, dim=1, largest=False)
        return keep_indices

    def stage_stop(self, errors, t_end, z_stop, t_done, labels):
        """The stop rule at a stage boundary as torch statements (posterior.stop_rule_torch), in place; the undecided image ids as a list."""
        ids, n, _ = P.stop_rule_torch(errors, t_end, z_stop, t_done, labels)
        return ids[:int(n)].tolist()

    def rows_on_device(self, rows):
        return rows

    def run_stage(self, pairs, classes, stage=None, rows=None):
        dc, x, d = self.dc, self.x, self.d
        by_trial = {}
        for j, b in pairs:
            by_trial.setdefault(j, []).append(b)
        for j, bl in by_trial.items():
            bs = torch.tensor(bl)
            full = bl == list(range(x.shape[0]))       # the reference's own batch: use the tensors as they are
            al = (d["alpha"][j] if full else d["alpha"][j, bs]).view(-1, 1, 1, 1).to(x.device)
            sg = (d["sigma"][j] if full else d["sigma"][j, bs]).view(-1, 1, 1, 1).to(x.device)
            lam = (self.label[j] if full else self.label[j, bs]).to(x.device)
            e = d["eps_of"][j]
            e = (e if full else e[bs.to(e.device)]).to(x.device)
            z = al * (x if full else x[bs.to(x.device)]) + sg * e
            wt = dict(pixel_w=None if self.pixel_w is None else self.pixel_w[bs.to(x.device)],
                      trial_w=None if self.trial_w is None else self.trial_w[j, bs].to(x.device))
            for c in range(classes.shape[1]):
                lab = classes[bs, c].to(x.device)
                emb = dc.encode_text_prompt(lab)
                # (encoder_type='clip_dual': also added_cond_kwargs = {text_embeds, time_ids}, diffusers' names; {} otherwise)
                pred = self.bb(x=z, noise_labels=lam, encoder_hidden_states=emb, **dc.added_cond(lab))
                eps_pred = sg * z + al * pred if dc.pred_param == 'v' else pred
                err = LS.error_torch(eps_pred, e, *self.score_loss, **wt)      # l2: torch.norm(...) ** 2, the reference's statement
                self.err[bs.to(x.device), lab, j] = err
                if self.ev is not None:
                    EV.err_map_torch(eps_pred, e, bs.to(x.device) * dc.config.classes + lab, self.ev[0][self.ev_stage], self.ev[1][self.ev_stage],
                                     *self.score_loss, **wt)


class _HipRunner(_Runner):
    """Micro-batched execution of the (image, trial, class) grid through libdcamd plans."""

    posterior, _evidence = staticmethod(P.class_posterior_hip), staticmethod(EV.evidence_maps_hip)

    def __init__(self, dc, backbone, x, T, draws, pixel_w=None):
        self.lib = L.require_gpu()
        super().__init__(dc, backbone, x, T, draws, x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device()), pixel_w)
        self.x_dev = x.detach().to(self.dev, torch.float32).contiguous()
        # the call's trial weights in the kernels' layout [BS, T]: ONE host-to-device copy per call (like x), the stages copy on the device
        self.trial_w_dev = None if self.trial_w is None else self.trial_w.t().contiguous().to(self.dev)
        self.err_dev = None
        dt = dc.config.compute_dtype or "bf16"
        if getattr(backbone, "compute_dtype", None) != dt:
            backbone.set_compute_dtype(dt)
        self.dt = dt
        if draws["philox"]:
            assert (x.shape[1] * x.shape[2] * x.shape[3]) % 4 == 0

    def _plan(self, n_bj, k):
        """The entry of (n_bj, k) in `dc._score_plans` (LRU), built on a miss: one dict that has all its fields from the start."""
        dc, dev = self.dc, self.dev
        cfg = dc.config
        BS, Cc, H, W = self.x.shape
        wver = getattr(self.bb, "_wver", 0)
        S = int(dc.encoder.weight.shape[1]) if dc._table_mode() else 1                 # tokens per context
        varlen = dc._ragged_table()                                                    # prompts of different lengths: a plan with ctx_len
        key = (BS, n_bj, k, self.dt, str(dev), (Cc, H, W), bool(getattr(self.bb, "share_trunk", True)), id(self.bb),
               self.T, cfg.classes, wver, S) + (("varlen",) if varlen else ())
        if self.score_loss[0] != L.LOSS_L2:                # the loss is baked into the plan's two scoring ops: never serve another loss's plan
            key += (("loss",) + self.score_loss,)
        weighted = (self.pixel_w is not None, self.trial_w is not None)
        if any(weighted):                                # such plans own the weight buffers and launch the weighted kernel instances
            key += (("weights",) + weighted,)
        if self.ev is not None:
            key += ("evidence",)
        sp = dc._score_plans.get(key)
        if sp is not None:
            dc._score_plans[key] = dc._score_plans.pop(key)      # most recently used last
            return sp
        # plans hold raw pointers into the packed weights they were built from: entries of an older weights version of this
        # backbone (load_state_dict / .to() / EMA.update since) are stale — drop them so their arenas are freed
        for old in [k_ for k_, e in dc._score_plans.items() if e["bb"] == id(self.bb) and e["wver"] != wver]:
            del dc._score_plans[old]
        layout, T = ControlBlock(n_bj, k), self.T
        ctl = torch.zeros(layout.words, dtype=torch.int32, device=dev)
        score = dict(
            x=torch.zeros((BS, Cc, H, W), dtype=torch.float32, device=dev),
            eps=torch.zeros((n_bj, Cc, H, W), dtype=torch.float32, device=dev),
            errors=torch.full((BS * cfg.classes * T + 1,), float("inf"), dtype=torch.float32, device=dev),
            **{f: layout.view(ctl, f) for f in ("lam", "alpha", "sigma", "img_of_bj", "ctx_of_unit", "out_index")},
            v_param=dc.pred_param == 'v', loss=self.score_loss[0], huber_delta=self.score_loss[1])
        if any(weighted):                # per-call buffers, filled in _feed: switching the weights' values never needs another plan
            score["pixel_w"] = torch.ones((BS, H, W), dtype=torch.float32, device=dev) if weighted[0] else None
            score["trial_w"] = torch.ones((BS, T), dtype=torch.float32, device=dev) if weighted[1] else None
            score["T"], score["cells"] = T, BS * cfg.classes
        if self.ev is not None:          # such plans own the accumulators their map op adds into (one stage at a time: run_stage)
            score["emap_acc"], score["emap_bad"] = (v[0] for v in EV.new_slabs(1, BS * cfg.classes, H * W, dev))
            score["emap_T"] = T
        plan = self.bb.make_plan(n_bj, k, cfg.classes, dev, score=score, **({"S": S} if S > 1 else {}), **({"varlen": True} if varlen else {}))
        sp = dict(plan=plan, score=score, layout=layout, ctl=ctl, pair_id=layout.view(ctl, "pair_id"), n_bj=n_bj, k=k, U=layout.U,
                  bb=id(self.bb), wver=wver, host=None, host_ev=torch.cuda.Event(), idx_cache={})
        dc._score_plans[key] = sp
        # each entry owns an arena, a workspace and an errors buffer in HBM, and n_bj follows the pair count (per rank, per stage, per
        # last batch of a dataloader): keep the most recently used few (a multi-stage classify alternates between one plan per stage).
        # (Scores that do not depend on n_bj — i.e. on the world size or the micro-batch split — rest on every kernel giving a sample the
        # same bits wherever it sits in a launch and whichever tile shape the launch size selects; tests/test_gpu_dist.py and
        # test_cfg2_full_grid_properties_at_bench_size hold that, and caught the one epilogue branch that did not in round 4.)
        cap = int(getattr(cfg, "score_plan_cache", None) or 6)
        while len(dc._score_plans) > max(cap, 1):
            del dc._score_plans[next(iter(dc._score_plans))]
        return sp

    def errors(self):
        BS, ncls = self.x.shape[0], self.dc.config.classes
        if self.err_dev is None:   # this rank owned no trial so far
            self.err_dev = torch.full((BS * ncls * self.T + 1,), float("inf"), dtype=torch.float32, device=self.dev)
        return self.err_dev[:-1].view(BS, ncls, self.T)

    def stage_end(self, errors, t_end, num_keep, last=False):
        """Mean over trials [0, t_end) and the num_keep smallest classes per image, on the device.  Returns [BS, num_keep]:
        int64 labels for the last stage (dc_reduce_argmin), else the int32 class lists the next stage's maps are built from."""
        BS, ncls, T = errors.shape
        assert errors.is_contiguous() and errors.dtype == torch.float32
        if last and num_keep == 1:
            keep = torch.empty((BS, 1), dtype=torch.int64, device=errors.device)
            L.check(self.lib.dc_reduce_argmin(errors.data_ptr(), BS, ncls, T, t_end, keep.data_ptr(), None, L.stream_ptr()), "dc_reduce_argmin")
        else:
            keep = torch.empty((BS, num_keep), dtype=torch.int32, device=errors.device)
            L.check(self.lib.dc_stage_topk(errors.data_ptr(), BS, ncls, T, t_end, num_keep, keep.data_ptr(), None, L.stream_ptr()), "dc_stage_topk")
        return keep

    def stage_stop(self, errors, t_end, z_stop, t_done, labels):
        """The stop rule at a stage boundary on the device (dc_stage_stop: the posterior's own device code, so the z-score an image
        stopped on is the one the posterior reports), in place on t_done / labels.  Returns the undecided image ids (ascending) as a list: ONE pinned device-to-host copy of BS + 1 int32 (the ids and their count) and a wait for it — the
        host needs the count to size the next stage's launches.  The ids stay on the device for dc_stage_maps_rows."""
        BS = errors.shape[0]
        block = torch.empty(BS + 1, dtype=torch.int32, device=self.dev)          # | active ids [BS] | their count |
        ids, _, _ = P.stop_rule_hip(errors, t_end, z_stop, t_done, labels, out=block)
        host = getattr(self.dc, "_stop_host", None)          # pinned staging kept across calls (pin_memory() is slow); free again after the wait
        if host is None or host.numel() != BS + 1:
            host = self.dc._stop_host = torch.zeros(BS + 1, dtype=torch.int32).pin_memory()
        host.copy_(block, non_blocking=True)
        torch.cuda.current_stream(self.dev).synchronize()
        n = int(host[BS])
        active = host[:n].tolist()
        self._rows = (active, ids[:n])
        return active

    def rows_on_device(self, rows):
        """The int32 device tensor of an image list: the one dc_stage_stop wrote when it is the list it returned."""
        have = getattr(self, "_rows", None)
        if have is not None and have[0] == list(rows):
            return have[1]
        return torch.tensor(list(rows), dtype=torch.int32).to(self.dev)

    def _feed(self, plan, score, ncls):
        """The call's errors so far, x and the class contexts into the buffers of this stage's plan; its evidence sums start at 0."""
        if self.err_dev is None:
            score["errors"].fill_(float("inf"))
        elif score["errors"] is not self.err_dev:
            score["errors"].copy_(self.err_dev)
        self.err_dev = score["errors"]
        if self.ev is not None:
            score["emap_acc"].zero_()
            score["emap_bad"].zero_()
        score["x"].copy_(self.x_dev)
        if self.pixel_w is not None:
            score["pixel_w"].copy_(self.pixel_w)
        if self.trial_w is not None:
            score["trial_w"].copy_(self.trial_w_dev)
        if self.dc.encoder is not None:
            plan.ctx.copy_(self.dc.encoder.weight[:ncls].detach().to(self.dev, torch.float32).reshape(plan.ctx.shape))
            if plan.varlen:                              # the same on every rank: grid sharding needs nothing else
                plan.ctx_len.copy_(self.dc.encoder.lengths[:ncls].to(self.dev, torch.int32))
        if getattr(plan, "pooled", None) is not None:    # a StableDiffusionXLUNet: the pooled row of every class and the shared size ids
            if self.dc.encoder_type != 'clip_dual':
                raise L.DcamdError(f"{type(self.bb).__name__} needs encoder_type='clip_dual' (the pooled text rows and the size ids of its "
                                   f"text_time embedding), this classifier has {self.dc.encoder_type!r}")
            plan.pooled.copy_(self.dc.pooled_table[:ncls].detach().to(self.dev, torch.float32))
            plan.time_ids.copy_(self.dc.add_time_ids.to(self.dev, torch.float32).expand(ncls, 6))
        plan.run_ctx()                                   # per-class vectors: once per stage, not per micro-batch

    def _stage_blocks(self, sp, pairs, classes, stage, rows, dump):
        """The stage's control blocks in the entry's pinned staging buffer -> host [>= n_mb, words].  The index part of every block
        (pair ids, image / class / output maps) depends on (pairs, classes) only: built once and kept (stage 0 of every call sees the
        same pairs and the full class list); per call only the three float rows (lambda, alpha, sigma of this call's t draws) are
        gathered.  Host time here is GPU idle time."""
        layout, d, T, ncls = sp["layout"], self.d, self.T, self.dc.config.classes
        n_bj = layout.n_bj
        n_mb = -(-len(pairs) // n_bj)
        sp["host_ev"].synchronize()                      # the previous call's asynchronous control-block copies have left `host`
        host = sp["host"]                                # pinned staging, reused across calls (pin_memory() is slow)
        if host is None or host.shape[0] < n_mb:
            host = sp["host"] = torch.zeros((n_mb, layout.words), dtype=torch.int32).pin_memory()
        # (pairs over a subset of the images: two subsets can agree in length, first and last pair — the ids are part of the key; a
        # caller that hands over pairs without naming their stage is keyed by the pairs themselves)
        ck = (n_bj, len(pairs), pairs[0], pairs[-1], T, ncls, b"dev" if classes.is_cuda else classes.numpy().tobytes(),
              tuple(rows) if rows is not None else (None if stage is not None else tuple(pairs)))
        cache = sp["idx_cache"]
        ent = cache.get(ck)
        if ent is None:
            if len(cache) > 8:
                cache.clear()
            ent = cache[ck] = index_blocks(layout, pairs, None if classes.is_cuda else classes, ncls, T, dump)
        tmpl, jsb = ent
        host[:n_mb].copy_(tmpl)
        # (the block's `lam` slot feeds dc_sinusoid alone: it holds the backbone's time input, `self.label`)
        rows3 = [(layout.fields["lam"][0], self.label)] + [(layout.fields[f][0], d[f]) for f in ("alpha", "sigma")]
        for m in range(n_mb):
            js, bs = jsb[m]
            for sl, src in rows3:
                host[m, sl].view(torch.float32).copy_(src[js, bs])
        return host

    def _device_maps(self, layout, pairs, classes, stage, rows, dump):
        """The class-dependent maps of every micro-batch of the stage, built on the device from the surviving classes -> [n_mb, 2 U]."""
        BS, ncls, T = self.x.shape[0], self.dc.config.classes, self.T
        n_bj, k, n_mb = layout.n_bj, layout.k, -(-len(pairs) // layout.n_bj)
        t0, rank, ws = stage
        maps = torch.empty((n_mb, layout.words - layout.host_words), dtype=torch.int32, device=self.dev)
        if rows is None:
            L.check(self.lib.dc_stage_maps(classes.data_ptr(), BS, ncls, T, k, t0, len(pairs), rank, ws, n_bj, n_mb, dump,
                                           maps.data_ptr(), L.stream_ptr()), "dc_stage_maps")
        else:
            rd = self.rows_on_device(rows)
            L.check(self.lib.dc_stage_maps_rows(classes.data_ptr(), rd.data_ptr(), len(rows), BS, ncls, T, k, t0, len(pairs), rank, ws,
                                                n_bj, n_mb, dump, maps.data_ptr(), L.stream_ptr()), "dc_stage_maps_rows")
        return maps

    def run_stage(self, pairs, classes, stage=None, rows=None):
        """pairs: this rank's (trial, image) pairs of the stage = D.local_pairs(t0, t1, BS, rank, world); stage = (t0, rank, world).
        rows (per-image early stopping): the stage runs over these images only — pairs = D.local_pairs_rows(t0, t1, rows, rank, world)."""
        if not pairs:
            return
        dc, d = self.dc, self.d
        BS, Cc, H, W = self.x.shape
        ncls, k = dc.config.classes, classes.shape[1]
        on_dev = classes.is_cuda                         # stages >= 1: the surviving classes never left the device
        n_bj = launch_size(len(pairs), max(1, TJ.units_per_launch(dc.config, H, W, k) // k), rows is not None)
        sp = self._plan(n_bj, k)
        plan, score, ctl = sp["plan"], sp["score"], sp["ctl"]
        self._feed(plan, score, ncls)
        n_mb = -(-len(pairs) // n_bj)
        dump = BS * ncls * self.T
        host = self._stage_blocks(sp, pairs, classes, stage, rows, dump)
        if on_dev:
            hw = sp["layout"].host_words
            maps = self._device_maps(sp["layout"], pairs, classes, stage, rows, dump)
        for m in range(n_mb):
            if on_dev:
                ctl[:hw].copy_(host[m, :hw], non_blocking=True)
                ctl[hw:].copy_(maps[m], non_blocking=True)
            else:
                ctl.copy_(host[m], non_blocking=True)
            if d["philox"]:
                L.check(self.lib.dc_philox_normal(score["eps"].data_ptr(), n_bj, Cc * H * W, sp["pair_id"].data_ptr(),
                                                  d["seed"], L.stream_ptr()), "dc_philox_normal")
            else:
                n = min(n_bj, len(pairs) - m * n_bj)
                for r, j, b0, c in eps_runs(pairs[m * n_bj:m * n_bj + n]):
                    score["eps"][r:r + c].copy_(d["eps_of"][j][b0:b0 + c].to(torch.float32), non_blocking=True)
                if n < n_bj:
                    score["eps"][n:].copy_(score["eps"][0:1].expand(n_bj - n, -1, -1, -1))
            if dc._timed_sink is not None:
                dc._timed_sink.append((plan, plan.pb.run_timed()))
            else:
                plan.run()
        # `host` (pinned) must outlive the asynchronous copies: instead of draining the stream here (the GPU then idles while the
        # host prepares the next call) an event marks the last copy, and the next user of the buffer waits for it — by then it has
        # long fired, and the host side of call i+1 runs under the kernels of call i
        sp["host_ev"].record()
        if self.ev is not None:          # the stage's sums into the call's slab (int64 adds on the stream: exact)
            self.ev[0][self.ev_stage] += score["emap_acc"]
            self.ev[1][self.ev_stage] += score["emap_bad"]
