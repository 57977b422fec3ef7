"""The plan model: a backbone becomes a static launch plan for libdcamd, assembled by a PlanBuilder.

A *plan* is a flat array of `dc_op` records (include/dcamd.h) over one arena allocation.
It is built once per (backbone, dtype, n_bj, n_cls) shape, then replayed with ONE native
call (`dc_run_plan`) per micro-batch — the replacement for the reference's Python double
loop body (diffusion/diffusion_classifier.py:695-714; ~600 eager launches per forward).

Work unit = (image b, trial j, class c).  Tensors live in one of three *domains*:
  'bj'   one sample per (image, trial) pair  — q_sample, time embedding, and every layer
         before the first cross-attention (the class-shared trunk: computed once per pair,
         never per class; exact, because class conditioning enters only through attn2);
  'unit' one sample per (pair, class);
  'ctx'  one row per class (class-token side path).
When a 'unit' op reads a 'bj'/'ctx' tensor the kernel indexes it through an int32 map
(bj_of_unit / ctx_of_unit), so nothing is ever broadcast-materialised and skip
connections are never concatenated in memory.

Here: the dtype tables, `TRef` / `PlanBuilder` (op emission, liveness, ctypes marshalling), the arena offset assignment
(`assign_arena`, pure Python), the plan-level switches (`switches`) and the base class of the plan classes (`Plan`).  The weight
packers live in packing.py; the backbones' plans in engine.py (UNet) and engine_dit / engine_vae / engine_clip / engine_t5.

PyTorch is used for device memory and streams only.
"""
import ctypes as C
import os
from collections import namedtuple

import torch

from . import _lib as L
from . import loss as LS

DT = {"f32": L.DC_F32, "fp32": L.DC_F32, "float32": L.DC_F32, "bf16": L.DC_BF16, "bfloat16": L.DC_BF16,
      "f16": L.DC_F16, "fp16": L.DC_F16, "float16": L.DC_F16}
TORCH_DT = {L.DC_F32: torch.float32, L.DC_BF16: torch.bfloat16, L.DC_F16: torch.float16}
DT_SIZE = {L.DC_F32: 4, L.DC_BF16: 2, L.DC_F16: 2}
FAKE_PTR = 1 << 20      # non-null and 16-byte aligned, for the questions to the library that only look at a pointer (PlanBuilder.probe)


def bke(dt):
    """K granule (elements per 128-byte LDS row) of dc_igemm for a dtype."""
    return 128 // DT_SIZE[dt]


def round_up(a, b):
    return (a + b - 1) // b * b


# ---- plan-level switches ------------------------------------------------------------------------
Switches = namedtuple("Switches", "pn gn_out_fusion skip_split short_fold qstats up4 ln_fold tblock po_fold tail_fold gn_ws")


def switches(env=None):
    """Every plan-level route switch, read from the environment when a plan is built (never at import: A/B runs and tests set a
    variable between two builds).  A route is on unless DCAMD_NO_<its name in capitals> is set, to anything, the empty string included.
      pn             a producer conv is asked to normalise its own output (pn_claim, pn_tail); off: never (A/B runs and tests)
      gn_out_fusion  conv_norm_out + SiLU inside conv_out's halo load
      skip_split     the half of conv1 / conv_shortcut that reads a class-shared skip runs once per (image, trial) pair
      short_fold     conv_shortcut as extra K chunks of conv2 (the halo conv's side source)
      qstats         3x3 convs also emit the (mean, M2) quad statistics of their output, so the GroupNorm that follows streams the
                     tensor once (read + write) instead of twice + write: GroupNorm 8.3 -> ~6 ms per cfg2 step
      up4            nearest-2x upsample + 3x3 conv as four 2x2-tap phases of the low-resolution tensor
      ln_fold        LayerNorm folded into the GEMM that consumes it
      tblock         the attention half of a transformer block (proj_in ... to_out) as one launch where libdcamd serves the shape (tblock.hip)
      po_fold        ff.net.2 and proj_out as one GEMM
      tail_fold      conv_norm_out + SiLU + conv_out inside the last ResNet conv's epilogue (csrc/epi_pn.h, tail fold)
      gn_ws          GroupNorm(+SiLU) applied by the consuming 3x3 conv's loader waves (conv3_ws.hip) from the producer's quad records: no
                     GroupNorm launch, the normalised tensor never exists (off: the GroupNorm pass + the plain conv, for A/B runs).  It
                     reads the quad records, so it is also off when qstats is
    """
    env = os.environ if env is None else env
    on = {name: env.get("DCAMD_NO_" + name.upper()) is None for name in Switches._fields}
    on["gn_ws"] = on["gn_ws"] and on["qstats"]
    return Switches(**on)


# ---- arena --------------------------------------------------------------------------------------
def assign_arena(bases, nops):
    """Arena offsets from liveness: sets `off` of every base (objects with `first`, `last`, `nbytes`; live over ops [first, last],
    last == nops meaning "to the end") and returns the arena size.  Bases are placed in order of `first` (ties: the given order), each
    into the smallest free block that holds it (the remainder stays free), else at the top; at the end of op idx the bases with
    last == idx are freed and neighbouring free blocks coalesce.  A mistake here silently aliases two live activations."""
    order = sorted(bases, key=lambda b: b.first)
    by_last = {}
    for b in order:
        by_last.setdefault(b.last, []).append(b)
    free, top = [], 0   # free: list of (off, size)
    pending = iter(order)
    nxt = next(pending, None)
    for idx in range(nops + 1):
        while nxt is not None and nxt.first == idx:
            need = nxt.nbytes
            best = None
            for i, (o, s) in enumerate(free):
                if s >= need and (best is None or s < free[best][1]):
                    best = i
            if best is not None:
                o, s = free.pop(best)
                nxt.off = o
                if s > need:
                    free.append((o + need, s - need))
            else:
                nxt.off = top
                top += need
            nxt = next(pending, None)
        for b in by_last.get(idx, []):
            free.append((b.off, b.nbytes))
            free.sort()
            merged = []
            for o, s in free:
                if merged and merged[-1][0] + merged[-1][1] == o:
                    merged[-1] = (merged[-1][0], merged[-1][1] + s)
                else:
                    merged.append((o, s))
            free = merged
    return top


class TRef:
    """Handle of a plan tensor [n(dom), H, W, C] (NHWC) or a view of one."""
    __slots__ = ("name", "dom", "H", "W", "C", "dt", "ld", "eoff", "base", "nbytes", "first", "last", "off", "ext", "qs", "prod")

    def __init__(self, name, dom, H, W, C, dt, nbytes=0, ext=None):
        self.name, self.dom, self.H, self.W, self.C, self.dt = name, dom, H, W, C, dt
        self.ld, self.eoff, self.base = C, 0, self
        self.nbytes, self.first, self.last, self.off, self.ext = nbytes, None, None, None, ext
        self.qs = None       # (quad-statistics tensor, parts) written by the producing conv (dc_igemm_params.qstats)
        self.prod = None     # index of the producing dc_igemm op while it can still be asked to normalise this tensor (pn_claim)

    def view(self, coff, C):
        v = TRef(self.name + f"[{coff}:{coff + C}]", self.dom, self.H, self.W, C, self.dt)
        v.ld, v.eoff, v.base = self.ld, self.eoff + coff, self.base
        return v


# op kind -> (the library function that names the kernel chosen for the op's params, the meta key the name is stored under): every
# kind whose entry dc_<op> has a dc_<op>_variant beside it in the header.  bench.py groups timings by an igemm's `family`; the others
# keep the family their builder wrote and get a `variant`.  (DC_OP_CONV3_PN_TAIL's variant takes two structs: finalize() asks it.)
VARIANT_OF = {kind: (fn + "_variant", "family" if kind == L.OP_IGEMM else "variant") for kind, fn in L.OP_ENTRY.items()
              if fn + "_variant" in L.EXPORTS and kind != L.OP_CONV3_PN_TAIL}


class PlanBuilder:
    def __init__(self, device, n_bj, n_cls, n_ctx):
        self.dev = device
        self.n = {"bj": n_bj, "unit": n_bj * n_cls, "ctx": n_ctx}
        self.ops = []        # (kind, struct_cls = L.OP_PARAMS[kind], fields{name: value | TRef | ("ptr", TRef)}, reads, writes)
        self.keep = []       # torch tensors kept alive (weights, maps, inputs)
        self.maps = {}       # (src_dom, dst_dom) -> external int32 TRef
        self.arena = None
        self.arena_bytes = 0
        self.meta = []       # per op: name, kernel family, algorithmic flops / HBM bytes (bench.py roofline)
        self.pn_off = not switches().pn      # A/B runs and tests: never ask a producer to normalise

    # ---- tensors -------------------------------------------------------------------
    def tensor(self, name, dom, H, W, Cc, dt):
        nbytes = self.n[dom] * H * W * Cc * DT_SIZE[dt]
        return TRef(name, dom, H, W, Cc, dt, nbytes=round_up(nbytes, 256))

    def external(self, name, t, dom, H, W, Cc, dt):
        assert t.is_contiguous() and t.device.type == "cuda", name
        self.keep.append(t)
        return TRef(name, dom, H, W, Cc, dt, ext=t)

    def const(self, t):
        """Device pointer of a constant (weight / bias / map) tensor kept alive by the plan."""
        if t is None:
            return None
        assert t.is_contiguous() and t.device.type == "cuda"
        self.keep.append(t)
        return t.data_ptr()

    def set_map(self, src_dom, dst_dom, t):
        self.maps[(src_dom, dst_dom)] = self.const(t)

    def map(self, src, dst_dom):
        if src is None or src.dom == dst_dom:
            return None
        return self.maps[(src.dom, dst_dom)]

    @staticmethod
    def dom(*ts):
        doms = {t.dom for t in ts if t is not None}
        if "unit" in doms or len(doms) > 1:   # bj x ctx -> one sample per (pair, class)
            return "unit"
        return doms.pop()

    def emit(self, kind, fields, reads, writes, meta=None, cls=None):
        """cls: the ctypes class of the op's record when it is not the op's own params struct (a weighted scoring op: the struct with
        the weights block behind it, loss.weighted_params)."""
        idx = len(self.ops)
        self.meta.append(dict(meta or {}, kind=kind))
        for t in reads + writes:
            if t is None:
                continue
            b = t.base
            if b.ext is None:
                if b.first is None:
                    b.first = idx
                b.last = idx
        self.ops.append((kind, cls or L.OP_PARAMS[kind], fields))

    # ---- ops -----------------------------------------------------------------------
    def igemm(self, name, src0, W, Cout, *, taps=1, stride=1, upsample=0, src1=None, bias=None, rowvec=None,
              act=L.ACT_NONE, gate=None, residual=None, out_dt=None, tile_n=128, wdt=None, dom=None, k_real=None, gn=None,
              side=None, ln_eps=0.0, qstats=False, up4=False):
        dom = dom or self.dom(src0, src1, rowvec, gate, residual)
        Hin, Win = (src0.H * 2, src0.W * 2) if upsample else (src0.H, src0.W)
        if taps == 9:
            Hout, Wout = (Hin + 2 - 3) // stride + 1, (Win + 2 - 3) // stride + 1
        else:
            Hout, Wout = Hin, Win
        cout_out = Cout // 2 if act == L.ACT_GEGLU else Cout
        out = self.tensor(name, dom, Hout, Wout, cout_out, src0.dt if out_dt is None else out_dt)
        f = dict(dtype=src0.dt if wdt is None else wdt, taps=taps, stride=stride, upsample=upsample,
                 n_img=self.n[dom], Hin=Hin, Win=Win, Hout=Hout, Wout=Wout,
                 src0=src0, map0=self.map(src0, dom), C0=src0.C, ld0=src0.ld,
                 src1=src1, map1=self.map(src1, dom), C1=src1.C if src1 is not None else 0,
                 ld1=src1.ld if src1 is not None else 0,
                 W=W, Cout=Cout, tile_n=tile_n, bias=bias,
                 rowvec=rowvec, rowvec_map=self.map(rowvec, dom), rowvec_ld=rowvec.ld if rowvec is not None else 0,
                 act=act, gate=gate, gate_map=self.map(gate, dom), gate_ld=gate.ld if gate is not None else 0,
                 residual=residual, res_map=self.map(residual, dom),
                 res_dtype=residual.dt if residual is not None else 0,
                 res_ld=residual.ld if residual is not None else 0,
                 out=out, out_dtype=out.dt, out_ld=out.ld)
        if up4:                  # W is the four-phase form of an upsample conv's weights (pack_up4, dc_igemm_up4_ok)
            assert upsample and taps == 9
            f.update(up4=1)
            k_real = 4 * src0.C
        if ln_eps:               # row LayerNorm (no affine) of the A operand inside the GEMM (dc_igemm_ln_ok)
            f.update(ln_eps=float(ln_eps))
        if side is not None:     # (src2, W2): 1x1 side source summed into the same output (conv_shortcut folded into conv2)
            s2, W2 = side
            assert (s2.H, s2.W) == (Hout, Wout) and s2.dt == src0.dt
            f.update(src2=s2, map2=self.map(s2, dom), W2=W2, C2=s2.C, ld2=s2.ld)
        if gn is not None:       # fused GroupNorm(+SiLU) prologue: (scale, shift, silu) from groupnorm_stats
            assert gn[0].dom == dom and gn[0].C == f["C0"] + f["C1"], "GroupNorm affine must live in the conv's domain"
            f.update(gn_scale=gn[0], gn_shift=gn[1], gn_silu=int(gn[2]))
        if src1 is not None:
            assert src1.dt == src0.dt and (src1.H, src1.W) == (src0.H, src0.W)
        qs = None
        if qstats:
            # the conv also writes (mean, M2) per (sample, part, channel quad) of its output: the GroupNorm that consumes the
            # tensor then streams it once (read + write) instead of sweeping it twice
            parts = int(L.lib().dc_igemm_qstats_parts(self.probe(**f)))
            if parts > 0:
                qs = TRef(name + ".qs", dom, 1, 1, 1, L.DC_F32, nbytes=round_up(self.n[dom] * parts * (Cout // 4) * 2 * 4, 256))
                f.update(qstats=qs)
                out.qs = (qs, parts)
        M = self.n[dom] * Hout * Wout
        kreal = taps * (src0.C + (src1.C if src1 is not None else 0)) if k_real is None else k_real
        es = DT_SIZE[f["dtype"]]
        nsrc = {"bj": self.n["bj"], "unit": self.n["unit"], "ctx": self.n["ctx"]}
        in_bytes = sum(nsrc.get(t.dom, 1) * t.H * t.W * t.C * DT_SIZE[t.dt] for t in (src0, src1, residual) if t is not None)
        meta = dict(name=name, family=f"igemm_{'f32' if f['dtype'] == L.DC_F32 else 'bf16' if f['dtype'] == L.DC_BF16 else 'f16'}_n{tile_n}",
                    flops=2.0 * M * kreal * Cout, bytes=float(in_bytes + kreal * Cout * es + M * cout_out * DT_SIZE[out.dt]),
                    M=M, N=Cout, K=kreal, taps=taps)
        if side is not None:
            meta["flops"] += 2.0 * M * side[0].C * Cout
            meta["K"] = kreal + side[0].C
            meta["bytes"] += float(nsrc.get(side[0].dom, 1) * side[0].H * side[0].W * side[0].C * DT_SIZE[side[0].dt] + side[0].C * Cout * es)
        self.emit(L.OP_IGEMM, f, [src0, src1, rowvec, gate, residual] + (list(gn[:2]) if gn else []) + ([side[0]] if side else []), [out] + ([qs] if qs else []), meta)
        if qstats and gn is None and (qs is not None or (taps == 9 and stride == 1 and not upsample and Hin == 4 and Win == 4)):
            out.prod = len(self.ops) - 1       # (4x4 images: no quad records, but the conv can still normalise its output inside the wave)
        return out

    def upsample_conv(self, key, x, weights, up4, qstats):
        """The 3x3 conv behind a nearest-2x upsample, `key` naming its entries in weights.P.  Nearest-2x upsample + 3x3 conv == four
        2x2-tap convs of the low-resolution tensor (phase-summed weights, packed on first use by weights.up4): 4/9 of the MACs, taken
        where the switch `up4` is on and dc_igemm_up4_ok serves the shape; else the plain upsample route."""
        four = up4 and self.up4_ok(x, x.C)
        W = weights.up4(key) if four else weights.P[key + ".w"]
        return self.igemm(key, x, self.const(W), x.C, taps=9, upsample=1, bias=self.const(weights.P[key + ".b"]), qstats=qstats, up4=four)

    def probe(self, x=None, **fields):
        """dc_igemm_params for a question to the library (dc_igemm_*_ok, dc_igemm_variant; none of them touches memory): FAKE_PTR for
        every plan tensor, and, given x, a plain 3x3 stride-1 conv of x with Cout channels on the 128-wide tile unless `fields` says
        otherwise."""
        if x is not None:
            fields = dict(dict(dtype=x.dt, taps=9, stride=1, upsample=0, n_img=self.n[x.dom], Hin=x.H, Win=x.W, Hout=x.H, Wout=x.W,
                               src0=x, C0=x.C, ld0=x.ld, W=FAKE_PTR, tile_n=128, out=FAKE_PTR, out_dtype=x.dt, out_ld=fields["Cout"]), **fields)
        return L.IgemmParams(**{k: (FAKE_PTR if isinstance(v, TRef) else v) for k, v in fields.items() if v is not None})

    def pn_capable(self, x, Cout, dom):
        """Would a plain 3x3 stride-1 conv of x (single source) be able to normalise its own output (dc_igemm_pn_ok)?"""
        if self.pn_off or Cout % 32:
            return False
        return bool(L.lib().dc_igemm_pn_ok(self.probe(x, Cout=Cout, n_img=self.n[dom], pn_groups=32, pn_eps=1e-5)))

    def _producer(self, x, groups):
        """(index, kind, fields) of the conv op that produced x while it can still be asked for GroupNorm(x) in `groups` groups: x is a
        whole tensor with a recorded producer nobody has claimed yet, and the groups divide its channels.  Else None."""
        if x is None or x.prod is None or x.base is not x or self.pn_off:
            return None
        kind, _, f = self.ops[x.prod]
        if f.get("pn_out") is not None or f["Cout"] % groups:
            return None
        return x.prod, kind, f

    def pn_claim(self, x, gamma, beta, groups, eps, silu):
        """Producer-side GroupNorm (dc_igemm_params.pn_*; csrc/epi_pn.h): ask the 3x3 conv that produced x to ALSO store
        act(GroupNorm(x)) — its accumulators hold every value in fp32 and it writes the statistics anyway — so that the consumer of
        this GroupNorm reads a finished tensor with a plain conv / GEMM and no GroupNorm pass (nor a normalising loader) runs.
        Returns the normalised tensor, or None when the producer cannot (then the caller takes the GroupNorm pass / the fused loader).
        One claim per tensor; whether the raw x is still stored is decided in finalize() (only if something reads it)."""
        prod = self._producer(x, groups)
        if prod is None:
            return None
        idx, _, f = prod
        if not L.lib().dc_igemm_pn_ok(self.probe(**f, pn_groups=groups, pn_eps=float(eps))):
            return None
        dom = x.dom
        y = self.tensor(x.name + ".pn", dom, x.H, x.W, x.C, x.dt)
        # arrival counters of this call site: monotonic, zeroed once here, never part of the (reused) arena
        cnt = self.const(torch.zeros(self.n[dom] * ((f["Cout"] + 127) // 128), dtype=torch.int32, device=self.dev))
        y.first = y.last = idx
        f.update(pn_out=y, pn_gamma=gamma, pn_beta=beta, pn_cnt=cnt, pn_ld=y.ld, pn_groups=groups, pn_silu=int(silu), pn_eps=float(eps))
        self.meta[idx]["bytes"] += float(self.n[dom] * x.H * x.W * x.C * DT_SIZE[x.dt])
        self.meta[idx]["pn"] = True
        x.prod = None
        return y

    def pn_tail(self, name, x, gamma, beta, groups, eps, silu, Wt, bias, Co):
        """Tail fold (dc_conv3_pn_tail; csrc/epi_pn.h): ask the 3x3 conv that produced x to compute act(GroupNorm(x)) AND the bias-only
        3x3 conv of Co <= 3 channels that is its only reader, so that neither x nor the normalised tensor is ever stored.  Wt: that
        conv's weights as pack_tail lays them out.  Returns the fp32 prediction tensor, or None when the library does not serve the
        pair (the caller then takes pn_claim / the fused loader / the GroupNorm pass).  x must be unread so far and stays unreadable."""
        prod = self._producer(x, groups)
        if prod is None:
            return None
        idx, kind, f = prod
        b = x.base
        if kind != L.OP_IGEMM or b.ext is not None or b.first != idx or b.last != idx:
            return None
        dom = x.dom
        pred = self.tensor(name, dom, x.H, x.W, Co, L.DC_F32)
        t = dict(tail_Wt=Wt, tail_bias=bias, tail_pred=pred, tail_Co=Co, tail_pred_ld=pred.ld,
                 pn_gamma=gamma, pn_beta=beta, pn_groups=groups, pn_silu=int(silu), pn_eps=float(eps))
        probe = dict(f, out=None, **t)
        conv_p, tail_p = self._tail_structs(probe, lambda v: FAKE_PTR if isinstance(v, TRef) else v)
        ring_floats = int(L.lib().dc_conv3_pn_tail_ring_floats(conv_p, tail_p))
        if ring_floats <= 0 or not L.lib().dc_conv3_pn_tail_ok(conv_p, tail_p):
            return None
        # ring and arrival counters belong to this call site: never part of the (reused) arena
        t["tail_ring"] = self.const(torch.zeros(ring_floats, dtype=torch.float32, device=self.dev))
        t["pn_cnt"] = self.const(torch.zeros(self.n[dom], dtype=torch.int32, device=self.dev))
        f.update(t, out=None)
        self.ops[idx] = (L.OP_CONV3_PN_TAIL, L.OP_PARAMS[L.OP_CONV3_PN_TAIL], f)
        pred.first = pred.last = idx
        M = self.n[dom] * x.H * x.W
        m = self.meta[idx]
        m.update(kind=L.OP_CONV3_PN_TAIL, tail=True, pn=True)
        # no store of the conv's own output; the folded conv's MACs, its prediction, the ring (written by the conv, read by the combine
        # launch, which also re-reads and re-writes the border pixels: counted as twice the ring) and the packed weights
        m["flops"] += 2.0 * M * x.C * 9 * Co
        m["bytes"] += float(-M * x.C * DT_SIZE[x.dt] + M * Co * 4 + 2 * ring_floats * 4 + 32 * x.C * DT_SIZE[x.dt])
        x.prod = None
        return pred

    @staticmethod
    def _tail_structs(f, ptr):
        """(dc_igemm_params, dc_pn_tail_params) of a DC_OP_CONV3_PN_TAIL op: the conv's pn_* fields travel in the tail struct."""
        conv, tail = L.IgemmParams(), L.PnTailParams()
        for name, ctype in L.IgemmParams._fields_:
            if name in f and f[name] is not None and not name.startswith("pn_"):
                setattr(conv, name, ptr(f[name]) if ctype is L.vp else f[name])
        src = dict(Wt="tail_Wt", bias="tail_bias", pred="tail_pred", ring="tail_ring", gamma="pn_gamma", beta="pn_beta", cnt="pn_cnt",
                   Co="tail_Co", pred_ld="tail_pred_ld", groups="pn_groups", silu="pn_silu", eps="pn_eps")
        for name, ctype in L.PnTailParams._fields_:
            v = f.get(src.get(name))
            if v is not None:
                setattr(tail, name, ptr(v) if ctype is L.vp else v)
        return conv, tail

    def up4_ok(self, src0, Cout):
        """Can the upsample conv of src0 run as four 2x2-tap phases on the low-resolution image (dc_igemm_up4_ok)?"""
        H2, W2 = 2 * src0.H, 2 * src0.W
        return bool(L.lib().dc_igemm_up4_ok(self.probe(src0, Cout=Cout, upsample=1, Hin=H2, Win=W2, Hout=H2, Wout=W2, bias=FAKE_PTR, up4=1)))

    def ln_ok(self, src0, Cout, act=L.ACT_NONE):
        """Can this 1-tap GEMM normalise its input rows itself (dc_igemm_ln_ok)?"""
        cout_out = Cout // 2 if act == L.ACT_GEGLU else Cout
        return bool(L.lib().dc_igemm_ln_ok(self.probe(src0, Cout=Cout, taps=1, act=act, out_ld=cout_out, ln_eps=1e-5)))

    def side_ok(self, src0, s2, Cout, residual=None):
        """Can a 3x3 stride-1 conv of src0 take the 1x1 side source s2 (dc_igemm_side_ok)?"""
        return bool(L.lib().dc_igemm_side_ok(self.probe(src0, Cout=Cout, n_img=self.n[self.dom(src0, s2, residual)], residual=residual,
                                                        res_dtype=src0.dt, res_ld=Cout, src2=s2, W2=FAKE_PTR, C2=s2.C, ld2=s2.ld)))

    def gn_fusable(self, src0, src1, Cout, tile_n=128, out_dt=None):
        """Can a 3x3 stride-1 conv of these sources take the GroupNorm prologue (dc_igemm_gn_fusable)?"""
        return bool(L.lib().dc_igemm_gn_fusable(self.probe(src0, Cout=Cout, n_img=self.n[self.dom(src0, src1)], src1=src1,
                                                           C1=src1.C if src1 is not None else 0, ld1=src1.ld if src1 is not None else 0,
                                                           tile_n=tile_n, out_dtype=src0.dt if out_dt is None else out_dt)))

    def gn_ws_ok(self, x, Cout):
        """Would a 3x3 stride-1 conv of x with a fused GroupNorm prologue run on the wave-specialised halo kernel (conv3_ws.hip: the
        transform is done by loader waves, not in the MFMA waves' stream)?  Asked through dc_igemm_variant."""
        p = self.probe(x, Cout=Cout, gn_scale=FAKE_PTR, gn_shift=FAKE_PTR, gn_silu=1)
        return L.lib().dc_igemm_variant(p).decode().startswith("conv3_ws")

    @staticmethod
    def qstats_ok(x0, x1, groups, dom):
        """Does x0 carry quad statistics its GroupNorm can use (single source, same domain, groups made of whole quads)?"""
        return x1 is None and x0.qs is not None and ((x0.C // groups) % 4 == 0) and x0.dom == dom

    def _groupnorm(self, name, x0, x1, gamma, beta, groups, eps, silu, stats):
        """dc_groupnorm over x0 (| x1).  stats: the statistics-only form, which writes no y but the per-(sample, channel) scale / shift."""
        dom = self.dom(x0, x1)
        Cc = x0.C + (x1.C if x1 is not None else 0)
        assert x0.ld == x0.C and (x1 is None or x1.ld == x1.C)
        n, HW = self.n[dom], x0.H * x0.W
        out = None if stats else self.tensor(name, dom, x0.H, x0.W, Cc, x0.dt)
        splits = L.lib().dc_groupnorm_splits(n, HW, Cc)
        ws = TRef(name + ".ws", dom, 1, 1, 1, L.DC_F32, nbytes=round_up(L.lib().dc_groupnorm_ws_floats(n, groups, splits) * 4, 256))
        f = dict(x=x0, map0=self.map(x0, dom), x1=x1, map1=self.map(x1, dom), y=out, dtype=x0.dt, out_dtype=x0.dt,
                 n=n, HW=HW, C=x0.C, C1=x1.C if x1 is not None else 0, groups=groups, silu=0 if stats else int(silu), splits=splits, eps=eps,
                 gamma=gamma, beta=beta, ws=ws)
        res = [out]
        if stats:
            res = [self.tensor(name + ".scale", dom, 1, 1, Cc, L.DC_F32), self.tensor(name + ".shift", dom, 1, 1, Cc, L.DC_F32)]
            f.update(out_scale=res[0], out_shift=res[1])
        qs = None
        if self.qstats_ok(x0, x1, groups, dom):    # the producer's quad records: the affine is formed without reading the tensor
            qs = x0.qs[0]
            f.update(qstats=qs, qparts=x0.qs[1])
        sweep = 1.0 * n * HW * Cc * DT_SIZE[x0.dt]
        meta = dict(name=name, family="groupnorm_stats", flops=0.0, bytes=0.0 if qs is not None else sweep) if stats else \
            dict(name=name, family="groupnorm", flops=0.0, bytes=2.0 * sweep)
        self.emit(L.OP_GROUPNORM, f, [x0, x1, qs], res + [ws], meta)
        return res

    def groupnorm(self, name, x0, gamma, beta, groups, eps, silu, x1=None):
        return self._groupnorm(name, x0, x1, gamma, beta, groups, eps, silu, False)[0]

    def groupnorm_stats(self, name, x0, gamma, beta, groups, eps, x1=None):
        """Statistics-only GroupNorm: returns the per-(sample, channel) scale / shift tensors for a fused conv prologue."""
        return tuple(self._groupnorm(name, x0, x1, gamma, beta, groups, eps, False, True))

    def layernorm(self, name, x, gamma, beta, eps, scale=None, shift=None):
        assert x.ld == x.C
        assert scale is None or x.dom == "unit" or scale.dom == x.dom, "LayerNorm input must already be per-unit"
        out = self.tensor(name, x.dom, x.H, x.W, x.C, x.dt)
        f = dict(x=x, y=out, dtype=x.dt, out_dtype=x.dt, rows=self.n[x.dom] * x.H * x.W, C=x.C,
                 rows_per_sample=x.H * x.W, mod_ld=scale.ld if scale is not None else 0, eps=eps,
                 gamma=gamma, beta=beta, scale=scale, shift=shift, mod_map=self.map(scale, x.dom))
        self.emit(L.OP_LAYERNORM, f, [x, scale, shift], [out],
                  dict(name=name, family="layernorm", flops=0.0, bytes=2.0 * f["rows"] * x.C * DT_SIZE[x.dt]))
        return out

    def attention(self, name, q, k, v, heads, d):
        """softmax(q k^T / sqrt(d)) v per head, for heads of true width d.  q / k / v hold q.C // heads channels per head: d, or
        padded_head_dim(d) with the pad channels zero (pad_head_rows), which add nothing to the scores and give zero output
        columns.  The scale is that of the true d; the FLOP count is what executes, at the padded width."""
        out = self.tensor(name, q.dom, q.H, q.W, q.C, q.dt)
        dp = q.C // heads
        assert d <= dp and dp * heads == q.C, (d, dp, heads, q.C)
        f = dict(q=q, k=k, v=v, out=out, dtype=q.dt, n=self.n[q.dom], L=q.H * q.W, heads=heads, d=dp,
                 ld_qkv=q.ld, ld_out=out.ld, scale=float(d) ** -0.5)
        Lq = q.H * q.W
        self.emit(L.OP_ATTENTION, f, [q, k, v], [out],
                  dict(name=name, family="attention", flops=4.0 * self.n[q.dom] * heads * Lq * Lq * dp,
                       bytes=4.0 * self.n[q.dom] * Lq * q.C * DT_SIZE[q.dt]))
        return out

    def cross_attention(self, name, q, k, v, heads, d, kv_len=None):
        """softmax(q k^T / sqrt(d)) v per head with keys / values from the 'ctx' domain (k.W tokens per context, picked per unit through
        ctx_of_unit) and queries of q's domain read through its map (bj_of_unit for the class-shared trunk): dc_cross_attention.  Head
        widths as in `attention` (q.C // heads channels per head, the scale of the true d).  The output is per unit.
        kv_len: device pointer (`const`) of an int32 tensor [n_ctx] of keys per context, indexed through the same map as k / v: dc_cross_attention_len
        (only the first kv_len[c] of a context's k.W rows are attended).  The lengths are device data that change between runs, so
        `flops` is computed with S = k.W: the upper bound.  `bytes` (q + out) does not depend on the length."""
        dom = self.dom(q, k)
        out = self.tensor(name, dom, q.H, q.W, q.C, q.dt)
        dp = q.C // heads
        assert d <= dp and dp * heads == q.C and k.C == q.C and v.C == q.C and k.dom == v.dom and k.ld == v.ld, (d, dp, heads, q.C, k.C)
        assert k.dt == q.dt and v.dt == q.dt and k.H == 1
        n, Lq, S = self.n[dom], q.H * q.W, k.W
        f = dict(q=q, k=k, v=v, out=out, q_map=self.map(q, dom), kv_map=self.map(k, dom), dtype=q.dt, n=n, Lq=Lq, S=S, heads=heads,
                 d=dp, ld_q=q.ld, ld_kv=k.ld, ld_out=out.ld, scale=float(d) ** -0.5)
        meta = dict(name=name, family="cross_attention", flops=4.0 * n * heads * Lq * S * dp, bytes=2.0 * n * Lq * q.C * DT_SIZE[q.dt])
        if kv_len is None:
            self.emit(L.OP_CROSS_ATTENTION, f, [q, k, v], [out], meta)
        else:
            self.emit(L.OP_CROSS_ATTENTION_LEN, dict(f, kv_len=kv_len), [q, k, v], [out], meta)
        return out

    def attention_strip(self, name, q, k, v, heads, d):
        """Self-attention as `attention` states it, launched through dc_cross_attention in its self form: q / k / v are the three
        column offsets of one fused QKV tensor, the keys of a sample are its own L rows (Lq = S = L, ld_q = ld_kv, no maps).  For
        heads of 160 channels, which dc_attention does not serve and the strip kernel does (csrc/attention_cross.hip)."""
        out = self.tensor(name, q.dom, q.H, q.W, q.C, q.dt)
        dp, Lq, n = q.C // heads, q.H * q.W, self.n[q.dom]
        assert d <= dp and dp * heads == q.C and k.C == q.C and v.C == q.C and k.dom == q.dom and v.dom == q.dom, (d, dp, heads, q.C, k.C)
        assert k.ld == q.ld and v.ld == q.ld and k.dt == q.dt and v.dt == q.dt
        f = dict(q=q, k=k, v=v, out=out, q_map=None, kv_map=None, dtype=q.dt, n=n, Lq=Lq, S=Lq, heads=heads, d=dp,
                 ld_q=q.ld, ld_kv=k.ld, ld_out=out.ld, scale=float(d) ** -0.5)
        self.emit(L.OP_CROSS_ATTENTION, f, [q, k, v], [out],
                  dict(name=name, family="attention", flops=4.0 * n * heads * Lq * Lq * dp, bytes=4.0 * n * Lq * q.C * DT_SIZE[q.dt]))
        return out

    def tblock_front_ok(self, x, heads):
        """Can ONE launch take proj_in -> LayerNorm -> q/k/v -> attention -> to_out of this block input (dc_tblock_front_ok)?"""
        fn = getattr(L.lib(), "dc_tblock_front_ok", None)
        if fn is None:
            return False
        p = L.TblockFrontParams(dtype=x.dt, n=self.n[x.dom], L=x.H * x.W, C=x.C, heads=heads, ldx=x.ld, ld_out=x.C)
        return int(fn(p)) == 1

    def tblock_front(self, name, x, Wp, bp, ln_g, ln_b, Wqkv, Wo, bo, rowvec, heads, eps):
        """out = to_out(attention(LayerNorm(h))) + bo + rowvec + h with h = proj_in(x) + bp, one workgroup per sample (dc_tblock_front)."""
        assert rowvec is None or self.dom(x, rowvec) == x.dom, "the class vector must not widen the block's domain"
        dom, Lq, Cc = x.dom, x.H * x.W, x.C
        d = Cc // heads
        out = self.tensor(name, dom, x.H, x.W, Cc, x.dt)
        f = dict(x=x, Wp=Wp, bp=bp, ln_g=ln_g, ln_b=ln_b, Wqkv=Wqkv, Wo=Wo, bo=bo, rowvec=rowvec, rowvec_map=self.map(rowvec, dom),
                 rowvec_ld=rowvec.ld if rowvec is not None else 0, out=out, dtype=x.dt, n=self.n[dom], L=Lq, C=Cc, heads=heads,
                 ldx=x.ld, ld_out=out.ld, ln_eps=float(eps), scale=float(d) ** -0.5)
        M, es = self.n[dom] * Lq, DT_SIZE[x.dt]
        self.emit(L.OP_TBLOCK_FRONT, f, [x, rowvec], [out],
                  dict(name=name, family="tblock_front", flops=2.0 * M * Cc * 5 * Cc + 4.0 * self.n[dom] * heads * Lq * Lq * d,
                       bytes=float(2 * M * Cc * es + 5 * Cc * Cc * es), M=M, N=Cc, K=Cc))
        return out

    def sinusoid(self, name, lam, dim, flip, shift):
        out = self.tensor(name, lam.dom, 1, 1, dim, L.DC_F32)
        f = dict(lam=lam, out=out, n=self.n[lam.dom], dim=dim, flip_sin_to_cos=int(flip), freq_shift=float(shift))
        self.emit(L.OP_SINUSOID, f, [lam], [out], dict(name=name, family="sinusoid", flops=0.0, bytes=0.0))
        return out

    def qsample(self, name, x_ptr, eps, alpha, sigma, img_of_bj, Cin, H, W, ld, dt, im2col, patch=0):
        g = patch if int(im2col) == 2 else 1
        out = self.tensor(name, "bj", H // g, W // g, ld, dt)
        f = dict(x=x_ptr, eps=eps, alpha=alpha, sigma=sigma, img_of_bj=img_of_bj, out=out, out_dtype=dt,
                 n_bj=self.n["bj"], C=Cin, H=H, W=W, ld=ld, im2col=int(im2col), patch=int(patch))
        self.emit(L.OP_QSAMPLE, f, [eps, alpha, sigma], [out],
                  dict(name=name, family="qsample", flops=0.0,
                       bytes=float(self.n["bj"] * (2 * Cin * H * W * 4 + (H // g) * (W // g) * ld * DT_SIZE[dt]))))
        return out

    # ---- the two ends of a scoring plan (UNetPlan, DiTPlan) -------------------------------------
    def score_head(self, score, Cin, H, W, ld, dt, im2col, patch=0):
        """score = dict(x=[B,C,H,W] f32 buffer, eps=[n_bj,C,H,W], alpha, sigma, img_of_bj, out_index, errors, v_param, loss, huber_delta; optionally pixel_w, trial_w, T, cells: the loss weights).  Emits q_sample,
        which writes the first GEMM's operand: returns (that operand, the (eps, alpha, sigma) externals score_tail takes back)."""
        noise = tuple(self.external(k, score[k], "bj", 1, 1, 1, L.DC_F32) for k in ("eps", "alpha", "sigma"))
        a0 = self.qsample("a0", self.const(score["x"]), *noise, self.const(score["img_of_bj"]), Cin, H, W, ld, dt, im2col=im2col, patch=patch)
        return a0, noise

    def score_tail(self, pred, score, noise, bj_of_unit, Cin, patch=0):
        """eps-MSE of the prediction into score["errors"] (dc_eps_mse) and, right after it and only where the plan owns evidence
        accumulators (evidence.py), its per-pixel form into them (dc_err_map)."""
        g = patch if patch > 1 else 1
        px = self.n["unit"] * pred.H * g * pred.W * g
        f = dict(pred=pred, eps=noise[0], x=self.const(score["x"]), alpha=noise[1], sigma=noise[2], bj_of_unit=self.const(bj_of_unit),
                 img_of_bj=self.const(score["img_of_bj"]), out_index=self.const(score["out_index"]), n_units=self.n["unit"], C=Cin,
                 H=pred.H * g, W=pred.W * g, ld=pred.ld, v_param=int(score["v_param"]), patch=int(patch),
                 loss=int(score["loss"]), huber_delta=float(score["huber_delta"]))      # the scoring loss (loss.py), for both ops
        weighted = score.get("pixel_w") is not None or score.get("trial_w") is not None
        if weighted:       # the loss weights: the flag in `loss` and the block behind both structs (dcamd.h DC_LOSS_WEIGHTED)
            f.update(loss=f["loss"] | L.LOSS_WEIGHTED, pixel_w=self.const(score.get("pixel_w")), trial_w=self.const(score.get("trial_w")),
                     w_T=int(score["T"]), w_cells=int(score["cells"]))
        cls_of = (lambda kind: LS.weighted_params(L.OP_PARAMS[kind])) if weighted else (lambda kind: None)
        self.emit(L.OP_EPS_MSE, dict(f, out=self.const(score["errors"])), [pred, *noise], [],
                  dict(name="eps_mse", family="eps_mse", flops=0.0, bytes=8.0 * Cin * px), cls=cls_of(L.OP_EPS_MSE))
        if score.get("emap_acc") is not None:
            acc = score["emap_acc"]
            self.emit(L.OP_ERR_MAP, dict(f, acc=self.const(acc), bad=self.const(score["emap_bad"]), T=int(score["emap_T"]), cells=acc.shape[0] - 1),
                      [pred, *noise], [], dict(name="err_map", family="err_map", flops=0.0, bytes=(8.0 * Cin + 8.0) * px),
                      cls=cls_of(L.OP_ERR_MAP))

    # ---- finalize: liveness-based arena + ctypes records ----------------------------
    def finalize(self, keep_alive=()):
        """keep_alive: tensors that must survive to the end of the plan (outputs)."""
        nops = len(self.ops)
        for t in keep_alive:
            t.base.last = nops
        # a producer-normalised conv whose raw output nobody reads stores only the normalised tensor
        for i, (kind, _, f) in enumerate(self.ops):
            if kind == L.OP_IGEMM and f.get("pn_out") is not None and isinstance(f.get("out"), TRef):
                b = f["out"].base
                if b.ext is None and b.first == i and b.last == i:
                    self.meta[i]["bytes"] -= float(self.n[b.dom] * b.H * b.W * b.C * DT_SIZE[b.dt])
                    f["out"] = None
        bases = {}
        for _, _, f in self.ops:
            for v in f.values():
                if isinstance(v, TRef) and v.base.ext is None:
                    bases[id(v.base)] = v.base
        top = assign_arena(list(bases.values()), nops)
        self.arena_bytes = top
        self.arena = torch.empty(max(top, 256), dtype=torch.uint8, device=self.dev)
        base_ptr = self.arena.data_ptr()
        assert base_ptr % 256 == 0

        def ptr(v):
            if v is None:
                return None
            if isinstance(v, TRef):
                b = v.base
                p0 = b.ext.data_ptr() if b.ext is not None else base_ptr + b.off
                return p0 + v.eoff * DT_SIZE[v.dt]
            return v

        self.structs = []
        arr = (L.Op * nops)()
        for i, (kind, cls, f) in enumerate(self.ops):
            if kind == L.OP_CONV3_PN_TAIL:      # two structs behind one op record
                conv, tail = self._tail_structs(f, ptr)
                s = cls(C.pointer(conv), C.pointer(tail))
                self.structs.append((s, conv, tail))
                self.meta[i]["family"] = L.lib().dc_conv3_pn_tail_variant(conv, tail).decode()
            else:
                s = cls()
                for name, ctype in cls._fields_:
                    if name in f:
                        setattr(s, name, ptr(f[name]) if ctype is L.vp else f[name])
                self.structs.append(s)
                if kind in VARIANT_OF:          # the kernel libdcamd picks for this shape
                    fn, key = VARIANT_OF[kind]
                    self.meta[i][key] = getattr(L.lib(), fn)(s).decode()
            arr[i].kind = kind
            arr[i].params = C.cast(C.pointer(s), C.c_void_p)
        self.op_array = arr
        self.nops = nops
        self.ptr_of = ptr
        return self

    def check_served(self, who, what):
        """Raises DcamdError for the first op the library refuses (finalize() named every op's kernel)."""
        for m in self.meta:
            if m.get("variant") == "invalid" or m["family"] == "invalid":
                raise L.DcamdError(f"{who}: libdcamd refuses {m['name']} at {what}")

    def run(self):
        L.check(L.lib().dc_run_plan(self.op_array, self.nops, L.stream_ptr()), "dc_run_plan")

    def run_timed(self):
        """Same launches with a HIP event pair around every op (on the launch stream); returns ms per op."""
        ms = (C.c_float * self.nops)()
        L.check(L.lib().dc_run_plan_timed(self.op_array, self.nops, L.stream_ptr(), ms), "dc_run_plan_timed")
        return list(ms)

    def tensor_view(self, t):
        """torch view of an arena/external tensor (tests and the plain forward read results through it)."""
        n = self.n[t.dom]
        assert t.ld == t.C and t.eoff == 0
        if t.base.ext is not None:
            return t.base.ext
        nel = n * t.H * t.W * t.C
        off = t.base.off
        return self.arena[off:off + nel * DT_SIZE[t.dt]].view(TORCH_DT[t.dt]).view(n, t.H, t.W, t.C)


class Plan:
    """What the plan classes share.  A subclass builds `self.pb` (a finalized PlanBuilder) and names its result tensor `self.pred` (the
    scoring backbones) or `self.out` (the encoders and the VAE halves)."""

    def run(self):
        self.pb.run()

    def run_timed(self):
        return self.pb.run_timed()

    @property
    def arena_bytes(self):
        return self.pb.arena_bytes

    def pred_view(self):
        return self.pb.tensor_view(self.pred)

    def out_view(self):
        return self.pb.tensor_view(self.out)
