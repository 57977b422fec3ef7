"""UNet scoring-step engine: the packed weights (`UNetWeights`) and the launch plan (`UNetPlan`) of a UNetCondition2D or a
StableDiffusionUNet (nets/sd_unet.py: heads per attention site, no `encoder_hid_proj`, heads of 160 channels) or a StableDiffusionXLUNet
(several transformer blocks per site; the text_time side path, which makes the ResNet time vector per unit).

The plan model — ops, domains, the arena, `PlanBuilder`, the route switches — is plan.py; the weight packers are packing.py.  Their
names that tests, tools and nets/ have always reached through this module are imported below.
"""
import torch

from . import _lib as L
from .packing import (HEAD_DIMS, LazyPacks, f32c, fold_layernorm_bias, geglu_perm, pack_conv3x3, pack_geglu, pack_matrix,  # noqa: F401
                      pack_tail, pack_up4, pad_head_cols, pad_head_rows, pad_vec, padded_head_dim)
from .plan import DT, DT_SIZE, FAKE_PTR, TORCH_DT, Plan, PlanBuilder, TRef, bke, round_up, switches  # noqa: F401


# The one head width above HEAD_DIMS a UNet plan runs, unpadded: Stable Diffusion 1.x's 1280 channels in 8 heads.  dc_attention and
# dc_tblock_front do not serve it; attn1 and attn2 of such a site both go through dc_cross_attention (PlanBuilder.attention_strip).
# UNetCondition2D refuses the width at construction (packing.padded_head_dim), so only a StableDiffusionUNet gets here with it.
WIDE_HEAD = 160


def site_head_dim(d):
    """Channels per head q / k / v are packed with for heads of true width d: d itself at WIDE_HEAD, else padded_head_dim(d)."""
    return d if d == WIDE_HEAD else padded_head_dim(d)


def site_heads(cfg, key):
    """Heads of the attention site `key` (`down_blocks.i.attentions.j`, `mid_block.attentions.0`, `up_blocks.i.attentions.j`).
    cfg.attention_head_dim is diffusers' misnomer for that count: one int, or one entry per down block — the up blocks read it
    reversed, the mid block takes the last."""
    ahd = cfg.attention_head_dim
    if isinstance(ahd, int):
        return ahd
    part, i = key.split(".")[:2]
    return ahd[-1] if part == "mid_block" else ahd[int(i)] if part == "down_blocks" else ahd[::-1][int(i)]


class UNetWeights(LazyPacks):
    """Device-resident packed weights of a UNetCondition2D for one compute dtype."""

    def __init__(self, model, dt, device):
        self.dt, self.dev = dt, device
        cfg = model.config
        self.kin = round_up(9 * cfg.in_channels, bke(dt))
        P = {}
        sd = {k: v for k, v in model.state_dict().items()}

        def conv3(key, tile_n=128, kpad=None):
            P[key + ".w"] = pack_conv3x3(sd[key + ".weight"], dt, device, tile_n, kpad)
            P[key + ".b"] = f32c(sd[key + ".bias"], device)

        def conv1(key):
            w = sd[key + ".weight"]
            P[key + ".w"] = pack_matrix(w, dt, device)
            P[key + ".b"] = f32c(sd[key + ".bias"], device)

        def lin(key, dtype=None, bias=True):
            P[key + ".w"] = pack_matrix(sd[key + ".weight"], dt if dtype is None else dtype, device)
            if bias and key + ".bias" in sd:
                P[key + ".b"] = f32c(sd[key + ".bias"], device)

        def norm(key):
            P[key + ".g"] = f32c(sd[key + ".weight"], device)
            P[key + ".b"] = f32c(sd[key + ".bias"], device)

        conv3("conv_in", kpad=self.kin)
        lin("time_embedding.linear_1", L.DC_F32)
        lin("time_embedding.linear_2", L.DC_F32)
        if "encoder_hid_proj.weight" in sd:      # (a StableDiffusionUNet has none: the context is attn2's input as it is)
            lin("encoder_hid_proj", L.DC_F32)
        if "add_embedding.linear_1.weight" in sd:      # StableDiffusionXLUNet: the text_time side path, fp32 like the time embedding
            lin("add_embedding.linear_1", L.DC_F32)
            lin("add_embedding.linear_2", L.DC_F32)
        norm("conv_norm_out")
        conv3("conv_out", tile_n=32 if cfg.out_channels <= 32 else 128)
        self.resnets, self.attns, self.heads = [], [], {}      # heads: per attention site
        for k in sd:
            if k.endswith("samplers.0.conv.weight"):
                conv3(k[: -len(".weight")])
        for key in sorted({k.rsplit(".", 2)[0] for k in sd if k.endswith(".time_emb_proj.weight")}):
            self.resnets.append(key)
            norm(key + ".norm1"); conv3(key + ".conv1"); norm(key + ".norm2"); conv3(key + ".conv2")
            if key + ".conv_shortcut.weight" in sd:
                conv1(key + ".conv_shortcut")
        # all time_emb_proj stacked into one [sum Cout, 4*C0] fp32 GEMM
        tw = torch.cat([sd[k + ".time_emb_proj.weight"] for k in self.resnets], 0)
        tb = torch.cat([sd[k + ".time_emb_proj.bias"] for k in self.resnets], 0)
        self.tproj_off, o = {}, 0
        for k in self.resnets:
            self.tproj_off[k] = o
            o += sd[k + ".time_emb_proj.weight"].shape[0]
        self.tproj_total = o
        P["tproj.w"] = pack_matrix(tw, L.DC_F32, device)
        P["tproj.b"] = f32c(tb, device)
        # a site is one Transformer2DModel (`...attentions.j`); its blocks `<site>.transformer_blocks.{k}` run in sequence between one
        # proj_in and one proj_out.  depth[site]: their number (1 everywhere but in a StableDiffusionXLUNet); tblocks: every (site, block key)
        self.depth, self.tblocks = {}, []
        # the one-token plan (S = 1, the class-vector path) is refused for a text_time model (UNetPlan): its fp32 matrices are not packed
        one_token = getattr(cfg, "addition_embed_type", None) != "text_time"
        for key in sorted({k[: -len(".proj_in.weight")] for k in sd if k.endswith(".proj_in.weight")}):
            self.attns.append(key)
            norm(key + ".norm"); conv1(key + ".proj_in"); conv1(key + ".proj_out")
            heads = self.heads[key] = site_heads(cfg, key)
            d = sd[key + ".proj_in.weight"].shape[0] // heads
            dp = site_head_dim(d)
            pre = key + ".transformer_blocks."
            self.depth[key] = 1 + max(int(k[len(pre):].split(".")[0]) for k in sd if k.startswith(pre))
            for kb in range(self.depth[key]):
                tb_ = pre + str(kb)
                self.tblocks.append((key, tb_))
                norm(tb_ + ".norm1"); norm(tb_ + ".norm3")
                qkv = pad_head_rows(torch.cat([sd[tb_ + f".attn1.to_{n}.weight"] for n in "qkv"], 0), d, dp)
                P[tb_ + ".qkv.w"] = pack_matrix(qkv, dt, device)
                P[tb_ + ".attn1.to_out.0.w"] = pack_matrix(pad_head_cols(sd[tb_ + ".attn1.to_out.0.weight"], d, dp), dt, device)
                P[tb_ + ".attn1.to_out.0.b"] = f32c(sd[tb_ + ".attn1.to_out.0.bias"], device)
                P[tb_ + ".ff.net.0.proj.w"], P[tb_ + ".ff.net.0.proj.b"] = pack_geglu(
                    sd[tb_ + ".ff.net.0.proj.weight"], sd[tb_ + ".ff.net.0.proj.bias"], dt, device)
                lin(tb_ + ".ff.net.2")
                # class-token side path (fp32): to_v then to_out of attn2 (to_q/to_k never matter for 1 key)
                if one_token:
                    lin(tb_ + ".attn2.to_out.0", L.DC_F32)
        self.P = P
        self._sd = sd              # references only (no copy): split packing of skip-connection convs is lazy
        if not one_token:
            return
        vw = torch.cat([sd[k + ".transformer_blocks.0.attn2.to_v.weight"] for k in self.attns], 0)
        self.cv_off, o = {}, 0
        for k in self.attns:
            self.cv_off[k] = o
            o += sd[k + ".transformer_blocks.0.attn2.to_v.weight"].shape[0]
        self.cv_total = o
        P["attn2v.w"] = pack_matrix(vw, L.DC_F32, device)

    def split_resnet(self, key, C0):
        """Packed halves of a skip-connection ResNet's input convs: `.conv1.wa/.wb` ([Cout, 9*C0] / [Cout, 9*C1], same
        k = tap*C + c order) and `.conv_shortcut.wa/.wb`, for channels [0, C0) and [C0, C0+C1) of the concatenated
        input.  conv(cat(a, b)) = conv_a(a) + conv_b(b): when b is class-independent its half runs once per (image, trial)
        pair instead of once per class (UNetPlan.resnet)."""
        w = self._sd[key + ".conv1.weight"]
        self.once(key + ".conv1.wa", lambda: {key + ".conv1.wa": pack_conv3x3(w, self.dt, self.dev, c_lo=0, c_hi=C0),
                                              key + ".conv1.wb": pack_conv3x3(w, self.dt, self.dev, c_lo=C0)})
        self.split_shortcut(key, C0)

    def split_shortcut(self, key, C0):
        """`.conv_shortcut.wa/.wb`: the 1x1 shortcut's columns for channels [0, C0) / [C0, C0+C1) of the concatenated input."""
        if key + ".conv_shortcut.weight" not in self._sd:
            return
        ws = self._sd[key + ".conv_shortcut.weight"]
        ws = ws.reshape(ws.shape[0], -1)
        self.once(key + ".conv_shortcut.wa", lambda: {key + ".conv_shortcut.wa": pack_matrix(ws[:, :C0], self.dt, self.dev),
                                                      key + ".conv_shortcut.wb": pack_matrix(ws[:, C0:], self.dt, self.dev)})

    def conv2_bs(self, key):
        """`.conv2.bs`: conv2's bias plus the shortcut's, for a conv2 that takes conv_shortcut as its side source."""
        return self.once(key + ".conv2.bs", lambda: (self.P[key + ".conv2.b"] + self.P[key + ".conv_shortcut.b"]).contiguous())

    def tail(self):
        """`conv_out.wt`: conv_out's weights as the tail fold reads them (pack_tail)."""
        return self.once("conv_out.wt", lambda: pack_tail(self._sd["conv_out.weight"], self.dt, self.dev))

    def fold_layernorms(self, tb_):
        """LayerNorm folded into the GEMM that consumes it: y = W (x_hat * g + b) + c = (W diag(g)) x_hat + (W b + c).  Packs
        `<tb>.qkv.wf/.bf` (norm1 -> q/k/v) and `<tb>.ff.net.0.proj.wf/.bf` (norm3 -> GEGLU projection); the kernel then only
        standardises the rows (dc_igemm ln_eps)."""
        sd = self._sd

        def make():
            d = sd[tb_ + ".norm1.weight"].shape[0] // self.heads[tb_.rsplit(".transformer_blocks.", 1)[0]]
            qkv = pad_head_rows(torch.cat([sd[tb_ + f".attn1.to_{n}.weight"] for n in "qkv"], 0).float(), d, site_head_dim(d))
            wf, bf = pack_geglu(sd[tb_ + ".ff.net.0.proj.weight"], sd[tb_ + ".ff.net.0.proj.bias"], self.dt, self.dev,
                                ln_gamma=sd[tb_ + ".norm3.weight"], ln_beta=sd[tb_ + ".norm3.bias"])
            return {tb_ + ".qkv.wf": pack_matrix(qkv, self.dt, self.dev, col_scale=sd[tb_ + ".norm1.weight"]),
                    tb_ + ".qkv.bf": fold_layernorm_bias(qkv, None, sd[tb_ + ".norm1.bias"], self.dev),
                    tb_ + ".ff.net.0.proj.wf": wf, tb_ + ".ff.net.0.proj.bf": bf}
        self.once(tb_ + ".qkv.wf", make)

    def pack_cross(self, fold_ln):
        """attn2 as attention (a context of several tokens; the one-token plan never needs these): per transformer block `<tb>.norm2.g/.b`,
        `<tb>.attn2.to_q.w` and `<tb>.attn2.to_out.0.wc` in the compute dtype with attn1's head padding, and ONE fp32 matrix
        `attn2kv.w` that stacks [to_k ; to_v] of every block of every site (rows `ckv_off[tb]` ... + 2 Cq: K | V of that block), so the
        context side path produces K | V of all of them with one GEMM, as `attn2v.w` stacks to_v for the one-token plan.  fold_ln: also
        `<tb>.attn2.to_q.wf/.bf`, norm2 folded into to_q for the row-standardising GEMM."""
        sd = self._sd

        def widths(key):
            d = sd[key + ".proj_in.weight"].shape[0] // self.heads[key]
            return d, site_head_dim(d)

        def make():
            new, kv, self.ckv_off, o = {}, [], {}, 0
            for key, tb_ in self.tblocks:
                d, dp = widths(key)
                new[tb_ + ".norm2.g"], new[tb_ + ".norm2.b"] = f32c(sd[tb_ + ".norm2.weight"], self.dev), f32c(sd[tb_ + ".norm2.bias"], self.dev)
                new[tb_ + ".attn2.to_q.w"] = pack_matrix(pad_head_rows(sd[tb_ + ".attn2.to_q.weight"], d, dp), self.dt, self.dev)
                new[tb_ + ".attn2.to_out.0.wc"] = pack_matrix(pad_head_cols(sd[tb_ + ".attn2.to_out.0.weight"], d, dp), self.dt, self.dev)
                new[tb_ + ".attn2.to_out.0.bc"] = f32c(sd[tb_ + ".attn2.to_out.0.bias"], self.dev)
                kv += [pad_head_rows(sd[tb_ + ".attn2.to_k.weight"], d, dp), pad_head_rows(sd[tb_ + ".attn2.to_v.weight"], d, dp)]
                self.ckv_off[tb_] = o
                o += 2 * self.heads[key] * dp
            self.ckv_total = o
            return dict(new, **{"attn2kv.w": pack_matrix(torch.cat(kv, 0), L.DC_F32, self.dev)})

        def make_folded(key, tb_):
            d, dp = widths(key)
            wq = pad_head_rows(sd[tb_ + ".attn2.to_q.weight"].float(), d, dp)
            return {tb_ + ".attn2.to_q.wf": pack_matrix(wq, self.dt, self.dev, col_scale=sd[tb_ + ".norm2.weight"]),
                    tb_ + ".attn2.to_q.bf": fold_layernorm_bias(wq, None, sd[tb_ + ".norm2.bias"], self.dev)}
        self.once("attn2kv.w", make)
        for key, tb_ in self.tblocks if fold_ln else ():
            self.once(tb_ + ".attn2.to_q.wf", lambda: make_folded(key, tb_))

    def fold_proj_out(self, key):
        """proj_out folded into the feed-forward's second linear: with h3 = W2 f + b2 + h2 (ff.net.2 + residual) the block's output
        x + Wpo h3 + bpo equals x + [Wpo W2 | Wpo] [f ; h2] + (Wpo b2 + bpo) — ONE GEMM over K = 4C + C with x as its residual instead of
        two (h3 never exists).  Exact algebra; the product matrix is formed in fp64 and rounded once to the compute dtype.
        Packs `<key>.ffpo.w` [C, 5C] and `<key>.ffpo.b`.  The ff.net.2 is the site's LAST block's: proj_out follows that one alone."""
        sd = self._sd

        def make():
            tb_ = f"{key}.transformer_blocks.{self.depth[key] - 1}"
            w2, b2 = sd[tb_ + ".ff.net.2.weight"].double(), sd[tb_ + ".ff.net.2.bias"].double()
            wpo = sd[key + ".proj_out.weight"].double()
            wpo = wpo.reshape(wpo.shape[0], -1)
            return {key + ".ffpo.w": pack_matrix(torch.cat([wpo @ w2, wpo], 1).float(), self.dt, self.dev),
                    key + ".ffpo.b": f32c((sd[key + ".proj_out.bias"].double() + wpo @ b2).float(), self.dev)}
        self.once(key + ".ffpo.w", make)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.P.values())


# ======================================================================================
#                                   UNet plan
# ======================================================================================
class UNetPlan(Plan):
    """Static launch plan of one UNetCondition2D scoring step.

    inputs (plan-owned device buffers, refreshed per micro-batch by the caller):
      lam [n_bj] f32 (what dc_sinusoid embeds: the log-SNR, or the DDPM step for a StableDiffusionUNet);
      ctx [n_ctx, hid] f32 (S = 1: one class token per context) or [n_ctx, S, hid] (S > 1: a prompt of S tokens);
      varlen plans: ctx_len [n_ctx] int32, tokens of each prompt that are attended (1 ... S; S when built);  a0 = conv_in GEMM operand [n_bj, H, W, kin]
      (written by the q_sample op when `score=True`, else by the caller through `a0_view`);
      maps bj_of_unit / ctx_of_unit [U] int32.
    output: pred [U, H, W, out_channels] f32 (NHWC); with score=True also err -> errors buffer.

    The builders below share, on self: pb, weights and its P, sw (the route switches), cfg, G / eps (GroupNorm groups and epsilon),
    tproj (the stacked time_emb_proj output), cvec / ckv (per site: the class vector, S = 1, or the prompt's K | V) and ctx_len.
    """

    def __init__(self, model, weights, n_bj, n_cls, n_ctx, *, share_trunk=True, score=None, device=None, S=1, varlen=False):
        assert S >= 1, S
        if varlen and S == 1:
            raise L.DcamdError("a varlen plan needs prompts of S > 1 tokens: one token is always attended")
        cfg = self.cfg = model.config
        dev = device or weights.dev
        dt = weights.dt
        self.dt, self.n_bj, self.n_cls, self.n_ctx, self.S, self.varlen = dt, n_bj, n_cls, n_ctx, S, bool(varlen)
        self.weights, self.P, self.sw = weights, weights.P, switches()
        self.G, self.eps = cfg.norm_num_groups, cfg.norm_eps
        # StableDiffusionXLUNet: the text_time side path (`aug`, a row per context, added to the time embedding) and sites of several blocks
        text_time = getattr(cfg, "addition_embed_type", None) == "text_time"
        if S == 1 and (text_time or max(weights.depth.values(), default=1) > 1):
            raise L.DcamdError(f"{type(model).__name__}: a context of one token (the class-vector path) is not built for text_time "
                               "conditioning or for sites of several transformer blocks: hand the backbone a prompt of S > 1 tokens")
        U = n_bj * n_cls
        pb = self.pb = PlanBuilder(dev, n_bj, n_cls, n_ctx)
        H = W = cfg.sample_size
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        # ---- inputs ----
        self.lam = score["lam"] if score is not None and "lam" in score else torch.zeros(n_bj, **f32)
        self.ctx = torch.zeros((n_ctx, cfg.encoder_hid_dim) if S == 1 else (n_ctx, S, cfg.encoder_hid_dim), **f32)
        self.bj_of_unit = (torch.arange(U, **i32) // n_cls).contiguous()
        self.ctx_of_unit = score["ctx_of_unit"] if score is not None and "ctx_of_unit" in score else (torch.arange(U, **i32) % n_ctx).contiguous()
        pb.set_map("bj", "unit", self.bj_of_unit)
        pb.set_map("ctx", "unit", self.ctx_of_unit)
        lam = pb.external("lam", self.lam, "bj", 1, 1, 1, L.DC_F32)
        pb.external("ctx", self.ctx, "ctx", 1, S, cfg.encoder_hid_dim, L.DC_F32)
        # prompts of different lengths: every cross-attention site reads the key count of a unit's context through the same map as
        # its K | V.  The context plan is the same: the pad rows of a prompt are projected and never read
        self.ctx_len = torch.full((n_ctx,), S, **i32) if varlen else None
        self.ctx_len_ptr = pb.const(self.ctx_len)
        # text_time: pooled [n_ctx, pooled_dim] and time_ids [n_ctx, 6] f32, inputs of the context plan like ctx (None otherwise)
        self.pooled = torch.zeros(n_ctx, cfg.pooled_dim, **f32) if text_time else None
        self.time_ids = torch.zeros(n_ctx, 6, **f32) if text_time else None
        kin = weights.kin
        if score is not None:
            self.score = score
            a0, noise = pb.score_head(score, cfg.in_channels, H, W, kin, dt, im2col=1)
        else:
            self.a0_buf = torch.zeros(n_bj, H, W, kin, dtype=TORCH_DT[dt], device=dev)
            a0 = pb.external("a0", self.a0_buf, "bj", H, W, kin, dt)
        # ---- fp32 side path: time embedding, stacked time_emb_proj; the class-token vectors / prompt K | V are the context plan's ----
        c, C0 = self.c, cfg.block_out_channels[0]
        self.context_plan(dev)          # (emits into its own builder: the main plan's op order does not depend on where this stands)
        te = pb.sinusoid("temb.sin", lam, C0, cfg.flip_sin_to_cos, cfg.freq_shift)
        te = pb.igemm("temb.l1", te, c("time_embedding.linear_1.w"), 4 * C0, bias=c("time_embedding.linear_1.b"), act=L.ACT_SILU)
        # text_time: temb.l2 runs in the UNIT domain with `aug` as its row vector — the epilogue is act((acc + bias) + rowvec), rows read
        # through bj_of_unit, the vector through ctx_of_unit: SiLU(temb[bj] + aug[ctx]) with no new op.  tproj then has U rows, and every
        # ResNet, whose time vector it is, becomes a per-unit layer: the class-shared trunk ends behind conv_in (inherent to the model)
        te = pb.igemm("temb.l2", te, c("time_embedding.linear_2.w"), 4 * C0, bias=c("time_embedding.linear_2.b"), rowvec=self.aug,
                      act=L.ACT_SILU)                                                                                 # = SiLU(temb (+ aug))
        self.tproj = pb.igemm("tproj", te, c("tproj.w"), weights.tproj_total, bias=c("tproj.b"))
        pred = self.pred = self.walk(a0, share_trunk)
        if pred.dom != "unit":
            raise L.DcamdError("backbone has no class-conditioned layer: nothing to score per class")
        if score is not None:
            pb.score_tail(pred, score, noise, self.bj_of_unit, cfg.in_channels)
        pb.finalize(keep_alive=[pred])
        for builder in (self.ctx_pb, pb):      # a shape libdcamd refuses is an error here, when the plan is built, never at a launch
            builder.check_served(type(model).__name__, f"{n_bj} x {n_cls} units of {H}x{W}, S = {S}")

    def c(self, key):
        """Device pointer of the packed weight P[key], kept alive by the plan."""
        return self.pb.const(self.P[key])

    def context_plan(self, dev):
        """Builds the context plan `ctx_pb` (run by run_ctx): what depends only on the weights and on `ctx`, executed once per
        classify call / forward and NOT once per micro-batch.  S = 1: the class vector of every site into `cvec`; S > 1: K | V of every
        site for the prompts' tokens into `ckv`.  The main plan reads either as 'ctx'-domain externals."""
        pb, P, weights, cfg, S, n_ctx = self.pb, self.P, self.weights, self.cfg, self.S, self.n_ctx
        pc = self.ctx_pb = PlanBuilder(dev, 1, 1, n_ctx)
        cctx = pc.external("ctx", self.ctx, "ctx", 1, S, cfg.encoder_hid_dim, L.DC_F32)
        if "encoder_hid_proj.w" in P:
            hp = pc.igemm("ctx.hid_proj", cctx, pc.const(P["encoder_hid_proj.w"]), cfg.cross_attention_dim,
                          bias=pc.const(P["encoder_hid_proj.b"]))
        else:
            hp = cctx                  # no projection (StableDiffusionUNet): the context rows are the side path's input themselves
        self.cvec, self.ckv, self.aug = {}, {}, None
        aug = None
        if self.pooled is not None:
            # text_time (diffusers, restated): the six size numbers of a context through the sinusoid of width addition_time_embed_dim,
            # [n_ctx, 6 * dim] concatenated BEHIND text_embeds (the GEMM's second K range), add_embedding.linear_1 -> SiLU -> linear_2.
            # It depends on the context row alone: once per call, n_ctx rows, fp32
            dim, T4 = cfg.addition_time_embed_dim, 4 * cfg.block_out_channels[0]
            tid = pc.external("time_ids", self.time_ids, "ctx", 1, 1, 6, L.DC_F32)
            sin = pc.tensor("add.sin", "ctx", 1, 1, 6 * dim, L.DC_F32)
            pc.emit(L.OP_SINUSOID, dict(lam=tid, out=sin, n=6 * n_ctx, dim=dim, flip_sin_to_cos=int(cfg.flip_sin_to_cos),
                                        freq_shift=float(cfg.freq_shift)),
                    [tid], [sin], dict(name="add.sin", family="sinusoid", flops=0.0, bytes=0.0))
            pooled = pc.external("pooled", self.pooled, "ctx", 1, 1, cfg.pooled_dim, L.DC_F32)
            a1 = pc.igemm("add.l1", pooled, pc.const(P["add_embedding.linear_1.w"]), T4, src1=sin,
                          bias=pc.const(P["add_embedding.linear_1.b"]), act=L.ACT_SILU)
            aug = pc.igemm("add.l2", a1, pc.const(P["add_embedding.linear_2.w"]), T4, bias=pc.const(P["add_embedding.linear_2.b"]))
        if S == 1:
            # one key: softmax = 1, attn2 is to_out(to_v(ctx)), a row vector of the attn1.to_out epilogue
            vall = pc.igemm("ctx.to_v", hp, pc.const(P["attn2v.w"]), weights.cv_total)
            cv_t = {}
            for k in weights.attns:
                tbk = k + ".transformer_blocks.0"
                Ck = P[k + ".norm.g"].shape[0]
                cv_t[k] = pc.igemm(k + ".cvec", vall.view(weights.cv_off[k], Ck), pc.const(P[tbk + ".attn2.to_out.0.w"]), Ck,
                                   bias=pc.const(P[tbk + ".attn2.to_out.0.b"]))
            pc.finalize(keep_alive=list(cv_t.values()))
            self.cvec = {k: pb.external(k + ".cvec", pc.tensor_view(t).view(n_ctx, -1), "ctx", 1, 1, t.C, L.DC_F32) for k, t in cv_t.items()}
        else:
            # a prompt of S tokens: K | V of every site from ONE stacked GEMM over the n_ctx * S projected rows (fp32 side path, stored in
            # the compute dtype); the main plan reads them as 'ctx'-domain tensors of 1 x S tokens
            weights.pack_cross(self.sw.ln_fold)
            kvall = pc.igemm("ctx.to_kv", hp, pc.const(P["attn2kv.w"]), weights.ckv_total, out_dt=self.dt)
            pc.finalize(keep_alive=[kvall] + ([aug] if aug is not None else []))
            kvx = pb.external("ctx.kv", pc.tensor_view(kvall), "ctx", 1, S, weights.ckv_total, self.dt)
            for k, tb_ in weights.tblocks:
                heads = weights.heads[k]
                Cq = heads * site_head_dim(P[k + ".norm.g"].shape[0] // heads)
                self.ckv[tb_] = (kvx.view(weights.ckv_off[tb_], Cq), kvx.view(weights.ckv_off[tb_] + Cq, Cq))
            if aug is not None:
                self.aug = pb.external("add.aug", pc.tensor_view(aug).view(n_ctx, -1), "ctx", 1, 1, aug.C, L.DC_F32)

    def walk(self, a0, share_trunk):
        """The main path, conv_in to conv_out; returns the prediction tensor."""
        pb, c, cfg, qs = self.pb, self.c, self.cfg, self.sw.qstats
        boc = cfg.block_out_channels
        # share_trunk=False recomputes the class-independent layers per unit (reference-equivalent
        # executed FLOPs; used for A/B tests): conv_in then reads its operand through bj_of_unit.
        h = pb.igemm("conv_in", a0, c("conv_in.w"), boc[0], bias=c("conv_in.b"),
                     dom=None if share_trunk else "unit", k_real=9 * cfg.in_channels)
        skips = [h]
        for i, kind in enumerate(cfg.down_block_types):
            for j in range(cfg.layers_per_block[i]):
                h = self.resnet(f"down_blocks.{i}.resnets.{j}", h)
                if kind == "CrossAttnDownBlock2D":
                    h = self.transformer(f"down_blocks.{i}.attentions.{j}", h)
                skips.append(h)
            if i != len(boc) - 1:
                key = f"down_blocks.{i}.downsamplers.0.conv"
                h = pb.igemm(key, h, c(key + ".w"), boc[i], taps=9, stride=2, bias=c(key + ".b"))
                skips.append(h)
        h = self.resnet("mid_block.resnets.0", h)
        h = self.transformer("mid_block.attentions.0", h)
        h = self.resnet("mid_block.resnets.1", h)
        rlpb = cfg.layers_per_block[::-1]
        for i, kind in enumerate(cfg.up_block_types):
            for j in range(rlpb[i] + 1):
                h = self.resnet(f"up_blocks.{i}.resnets.{j}", h, skips.pop())
                if kind == "CrossAttnUpBlock2D":
                    h = self.transformer(f"up_blocks.{i}.attentions.{j}", h)
            if i != len(boc) - 1:
                h = pb.upsample_conv(f"up_blocks.{i}.upsamplers.0.conv", h, self.weights, self.sw.up4, qs)
        return self.conv_out(h)

    def gn_conv3(self, gname, cname, x, gamma, beta, groups, Wp, Cout, **kw):
        """GroupNorm + SiLU of the single-source tensor x, then a 3x3 conv of it (bias / row vector / residual / side source
        in kw).  One launch where the wave-specialised conv can normalise its own input (affine from the quad records x's
        producer wrote: no pass over x at all); else the GroupNorm pass and the plain conv."""
        pb, eps = self.pb, self.eps
        dom = pb.dom(x, kw.get("rowvec"), kw.get("residual"), kw["side"][0] if kw.get("side") else None)
        # first choice: x's producer stores the normalised tensor itself (csrc/epi_pn.h) and this conv is the plain halo conv
        y = pb.pn_claim(x, gamma, beta, groups, eps, True)
        if y is not None:
            return pb.igemm(cname, y, Wp, Cout, taps=9, **kw)
        # second: where this conv could in turn normalise its own output for the NEXT GroupNorm, keep it the plain halo conv behind a
        # GroupNorm pass (one pass at the head of a chain of producer-normalised convs) rather than the wave-specialised conv, whose
        # epilogue cannot (conv3_ws.hip: one workgroup per CU, 0.75 against 1.0 PF)
        chain = kw.get("qstats") and pb.pn_capable(x, Cout, dom)
        if not chain and self.sw.gn_ws and dom == x.dom and pb.qstats_ok(x, None, groups, dom) and pb.gn_ws_ok(x, Cout):
            aff = pb.groupnorm_stats(gname, x, gamma, beta, groups, eps)
            return pb.igemm(cname, x, Wp, Cout, taps=9, gn=(aff[0], aff[1], True), **kw)
        y = pb.groupnorm(gname, x, gamma, beta, groups, eps, True)
        return pb.igemm(cname, y, Wp, Cout, taps=9, **kw)

    def resnet(self, key, x0, x1=None):
        pb, c, P, G, qs = self.pb, self.c, self.P, self.G, self.sw.qstats
        Cout = P[key + ".conv1.b"].shape[0]
        shortcut = key + ".conv_shortcut.w" in P
        # a skip connection from the class-shared trunk into a per-class layer: what is linear in cat(x0, x1) splits into an x0 half
        # and an x1 half, and the x1 half runs once per (image, trial) pair instead of once per class
        shared_skip = self.sw.skip_split and x1 is not None and x1.dom == "bj" and x0.dom == "unit" and shortcut
        # conv(cat(h, skip)) = conv_a(h) + conv_b(skip), and GroupNorm never mixes the two halves when its groups do not straddle
        # the seam: then norm1 / conv1 split too.  Exact algebra; only the summation order differs.
        split = shared_skip and x0.C % ((x0.C + x1.C) // G) == 0
        h = self.resnet_conv1(key, x0, x1, split, Cout)      # conv2 normalises it itself where gn_conv3 can (norm2 + SiLU)
        conv2 = dict(gamma=c(key + ".norm2.g"), beta=c(key + ".norm2.b"), groups=G, Wp=c(key + ".conv2.w"), Cout=Cout, qstats=qs)
        # conv_shortcut folded into conv2: the 1x1 over the raw input becomes extra K chunks of conv2's own MFMA loop
        # (conv3_halo side source) — no shortcut launch, no shortcut tensor written and read back
        # (the SHORTCUT of a class-shared skip splits even where a GroupNorm group straddles the seam and norm1 / conv1 cannot:
        #  shortcut(cat(x0, x1)) = Wa x0 + Wb x1 is linear — the x1 half once per pair, the x0 half as conv2's side source)
        fold = (self.sw.short_fold and shortcut and (x1 is None or shared_skip)
                and pb.side_ok(h, x0, Cout, residual=x1 if shared_skip else None))
        ss = None
        if shared_skip if fold else split:       # the skip's half of the shortcut, once per pair
            self.weights.split_shortcut(key, x0.C)
            ss = pb.igemm(key + ".shorts", x1, c(key + ".conv_shortcut.wb"), Cout)
        if fold:
            w2 = c(key + (".conv_shortcut.wa" if shared_skip else ".conv_shortcut.w"))
            return self.gn_conv3(key + ".gn2", key + ".conv2", h, bias=pb.const(self.weights.conv2_bs(key)), residual=ss, side=(x0, w2), **conv2)
        if split:
            sc = pb.igemm(key + ".short", x0, c(key + ".conv_shortcut.wa"), Cout, bias=c(key + ".conv_shortcut.b"), residual=ss)
        elif shortcut:
            sc = pb.igemm(key + ".short", x0, c(key + ".conv_shortcut.w"), Cout, src1=x1, bias=c(key + ".conv_shortcut.b"))
        else:
            assert x1 is None
            sc = x0
        return self.gn_conv3(key + ".gn2", key + ".conv2", h, bias=c(key + ".conv2.b"), residual=sc, **conv2)

    def resnet_conv1(self, key, x0, x1, split, Cout):
        """norm1 + SiLU + conv1 + the time vector of a ResNet over x0 (| the skip x1)."""
        pb, c, P, G, qs = self.pb, self.c, self.P, self.G, self.sw.qstats
        tvec = self.tproj.view(self.weights.tproj_off[key], Cout)
        if split:
            # class-independent skip half, once per (image, trial) pair: its GroupNorm groups are its own, its conv
            # partial sum enters the per-unit conv as a residual read through bj_of_unit
            Ca, Cb = x0.C, x1.C
            cpg = (Ca + Cb) // G
            self.weights.split_resnet(key, Ca)
            g1, b1 = P[key + ".norm1.g"], P[key + ".norm1.b"]
            ts = self.gn_conv3(key + ".gn1s", key + ".conv1s", x1, pb.const(g1[Ca:]), pb.const(b1[Ca:]), Cb // cpg, c(key + ".conv1.wb"), Cout)
            return self.gn_conv3(key + ".gn1", key + ".conv1", x0, pb.const(g1[:Ca]), pb.const(b1[:Ca]), Ca // cpg, c(key + ".conv1.wa"), Cout,
                                 bias=c(key + ".conv1.b"), rowvec=tvec, residual=ts, qstats=qs)
        if x1 is None:
            return self.gn_conv3(key + ".gn1", key + ".conv1", x0, c(key + ".norm1.g"), c(key + ".norm1.b"), G, c(key + ".conv1.w"), Cout,
                                 bias=c(key + ".conv1.b"), rowvec=tvec, qstats=qs)
        h = pb.groupnorm(key + ".gn1", x0, c(key + ".norm1.g"), c(key + ".norm1.b"), G, self.eps, True, x1=x1)
        return pb.igemm(key + ".conv1", h, c(key + ".conv1.w"), Cout, taps=9, bias=c(key + ".conv1.b"), rowvec=tvec, qstats=qs)

    def transformer(self, key, x):
        pb, c, heads = self.pb, self.c, self.weights.heads[key]
        tbk = key + ".transformer_blocks.0"
        d = x.C // heads
        Cq = heads * site_head_dim(d)      # q / k / v / attention width: heads of d channels padded to a served width (160: as they are)
        h = pb.pn_claim(x, c(key + ".norm.g"), c(key + ".norm.b"), self.G, 1e-6, False)
        if h is None:
            h = pb.groupnorm(key + ".gn", x, c(key + ".norm.g"), c(key + ".norm.b"), self.G, 1e-6, False)
        if self.S > 1:
            # the blocks of the site in sequence between one proj_in and one proj_out (one block everywhere but in a StableDiffusionXLUNet)
            depth = self.weights.depth[key]
            for kb in range(depth):
                tbk = f"{key}.transformer_blocks.{kb}"
                h = self.prompt_attention(key, tbk, self.self_attention(key, tbk, h, None, heads, d, Cq, proj_in=kb == 0), heads, d, Cq)
                h = self.feed_forward(key, tbk, x, h, last=kb == depth - 1)
            return h
        elif self.sw.tblock and h.dom == pb.dom(h, self.cvec[key]) and pb.tblock_front_ok(h, heads):
            # proj_in -> LayerNorm -> q/k/v -> attention -> to_out + class vector + residual in ONE launch, the sample on chip
            assert Cq == x.C, "dc_tblock_front takes unpadded heads only"
            h = pb.tblock_front(tbk + ".front", h, c(key + ".proj_in.w"), c(key + ".proj_in.b"), c(tbk + ".norm1.g"), c(tbk + ".norm1.b"),
                                c(tbk + ".qkv.w"), c(tbk + ".attn1.to_out.0.w"), c(tbk + ".attn1.to_out.0.b"), self.cvec[key], heads, 1e-5)
        else:
            h = self.self_attention(key, tbk, h, self.cvec[key], heads, d, Cq)
        return self.feed_forward(key, tbk, x, h)

    def self_attention(self, key, tbk, h, rowvec, heads, d, Cq, proj_in=True):
        """proj_in -> LayerNorm -> q/k/v -> attention -> to_out + residual as a chain of launches.  rowvec: the class vector of a
        one-token context (attn2 of one key is a row vector of this epilogue); None in a prompt plan.  proj_in False: h is the output
        of the site's previous block."""
        pb, c, Cc = self.pb, self.c, h.C
        if proj_in:
            h = pb.igemm(key + ".proj_in", h, c(key + ".proj_in.w"), Cc, bias=c(key + ".proj_in.b"))
        # (q/k/v keeps its LayerNorm launch: measured faster on the 256x256 tile + LayerNorm than on the row-standardising GEMM)
        hn = pb.layernorm(tbk + ".ln1", h, c(tbk + ".norm1.g"), c(tbk + ".norm1.b"), 1e-5)
        qkv = pb.igemm(tbk + ".qkv", hn, c(tbk + ".qkv.w"), 3 * Cq)
        # heads of 160 channels: dc_attention does not serve them; the strip kernel of dc_cross_attention in its self form does
        attend = pb.attention_strip if d == WIDE_HEAD else pb.attention
        o = attend(tbk + ".attn1", qkv.view(0, Cq), qkv.view(Cq, Cq), qkv.view(2 * Cq, Cq), heads, d)
        return pb.igemm(tbk + ".attn_out", o, c(tbk + ".attn1.to_out.0.w"), Cc, bias=c(tbk + ".attn1.to_out.0.b"), rowvec=rowvec, residual=h)

    def prompt_attention(self, key, tbk, h, heads, d, Cq):
        """attn2 over the S > 1 tokens of a prompt, behind the self-attention chain without a class vector (the one-launch front,
        dc_tblock_front, is built around that vector's epilogue and is not used in a prompt plan):
        norm2 -> to_q -> dc_cross_attention against this site's K | V of the context plan -> attn2.to_out + bias + residual.
        Everything in front of the cross-attention is class-independent: in the first block of a class-shared trunk it stays in the
        'bj' domain, and the cross-attention, reading q through bj_of_unit, is the first per-unit op."""
        pb, c = self.pb, self.c
        if self.sw.ln_fold and pb.ln_ok(h, Cq):
            q2 = pb.igemm(tbk + ".attn2.to_q", h, c(tbk + ".attn2.to_q.wf"), Cq, bias=c(tbk + ".attn2.to_q.bf"), ln_eps=1e-5)
        else:
            hn = pb.layernorm(tbk + ".ln2", h, c(tbk + ".norm2.g"), c(tbk + ".norm2.b"), 1e-5)
            q2 = pb.igemm(tbk + ".attn2.to_q", hn, c(tbk + ".attn2.to_q.w"), Cq)
        o2 = pb.cross_attention(tbk + ".attn2", q2, self.ckv[tbk][0], self.ckv[tbk][1], heads, d, kv_len=self.ctx_len_ptr)
        return pb.igemm(tbk + ".attn2_out", o2, c(tbk + ".attn2.to_out.0.wc"), h.C, bias=c(tbk + ".attn2.to_out.0.bc"), residual=h)

    def feed_forward(self, key, tbk, x, h, last=True):
        """norm3 -> GEGLU -> ff.net.2 + residual -> proj_out + the site's input x.  last False (a block with another one behind it):
        it ends at ff.net.2 + residual; proj_out, and its fold into ff.net.2, belong to the site's last block."""
        pb, c, Cc = self.pb, self.c, h.C
        # LayerNorm folded into the consuming GEMM where the activation-stationary kernel can standardise the rows itself
        # (gamma into W's columns, beta into the bias: UNetWeights.fold_layernorms): no LayerNorm launch, no normalised tensor
        if self.sw.ln_fold and pb.ln_ok(h, 8 * Cc, L.ACT_GEGLU):
            self.weights.fold_layernorms(tbk)
            f = pb.igemm(tbk + ".geglu", h, c(tbk + ".ff.net.0.proj.wf"), 8 * Cc, bias=c(tbk + ".ff.net.0.proj.bf"), act=L.ACT_GEGLU, ln_eps=1e-5)
        else:
            hn = pb.layernorm(tbk + ".ln3", h, c(tbk + ".norm3.g"), c(tbk + ".norm3.b"), 1e-5)
            f = pb.igemm(tbk + ".geglu", hn, c(tbk + ".ff.net.0.proj.w"), 8 * Cc, bias=c(tbk + ".ff.net.0.proj.b"), act=L.ACT_GEGLU)
        if not last:
            return pb.igemm(tbk + ".ff_out", f, c(tbk + ".ff.net.2.w"), Cc, bias=c(tbk + ".ff.net.2.b"), residual=h)
        if self.sw.po_fold:
            # ff.net.2 and proj_out as one GEMM over [f | h] (UNetWeights.fold_proj_out): no ff_out tensor, one launch fewer
            self.weights.fold_proj_out(key)
            return pb.igemm(key + ".ff_proj_out", f, c(key + ".ffpo.w"), Cc, src1=h, bias=c(key + ".ffpo.b"), residual=x)
        h = pb.igemm(tbk + ".ff_out", f, c(tbk + ".ff.net.2.w"), Cc, bias=c(tbk + ".ff.net.2.b"), residual=h)
        return pb.igemm(key + ".proj_out", h, c(key + ".proj_out.w"), Cc, bias=c(key + ".proj_out.b"), residual=x)

    def conv_out(self, h):
        """conv_norm_out + SiLU + conv_out, by the first route that serves the shape: tail fold, claimed producer norm, fused prologue,
        GroupNorm pass."""
        pb, c, cfg, G, eps = self.pb, self.c, self.cfg, self.G, self.eps
        Co = cfg.out_channels
        tn_out = 32 if Co <= 32 else 128
        norm = (c("conv_norm_out.g"), c("conv_norm_out.b"))
        if self.sw.tail_fold and Co <= 3 and h.C == 128 and self.dt != L.DC_F32:
            # the last ResNet's conv2 normalises its output and multiplies it by conv_out's weights itself: no normalised tensor, no thin conv
            pred = pb.pn_tail("conv_out", h, *norm, G, eps, True, pb.const(self.weights.tail()), c("conv_out.b"), Co)
            if pred is not None:
                return pred
        gn = None
        hn = pb.pn_claim(h, *norm, G, eps, True)
        if hn is not None:
            pass                  # the last ResNet's conv2 stored conv_norm_out + SiLU of its output: conv_out is a plain thin conv
        elif self.sw.gn_out_fusion and pb.qstats_ok(h, None, G, h.dom) and pb.gn_fusable(h, None, Co, tile_n=tn_out, out_dt=L.DC_F32):
            # conv_norm_out + SiLU inside conv_out's halo load (the thin-output conv reads ~1 GB for 3 channels and its VALU is idle):
            # the affine comes from the last conv's quad records, the normalised tensor never exists, one launch instead of two
            aff = pb.groupnorm_stats("conv_norm_out", h, *norm, G, eps)
            hn, gn = h, (aff[0], aff[1], True)
        else:
            hn = pb.groupnorm("conv_norm_out", h, *norm, G, eps, True)
        return pb.igemm("conv_out", hn, c("conv_out.w"), Co, taps=9, bias=c("conv_out.b"), out_dt=L.DC_F32, tile_n=tn_out, gn=gn)

    def run_ctx(self):
        """Refresh the per-class cross-attention vectors (S = 1) or the per-site K | V of every prompt (S > 1) from `self.ctx` (call
        after changing ctx / weights)."""
        self.ctx_pb.run()
