"""Counters with the interface of reference `utils/metrics.py` (Metric / Accuracy / Precision /
Recall / F1: `update((pred, batch))`, `sync_across_processes(accelerator)`, `get_output()`,
`set_device`, `reset`), fed by `DiffusionClassifier.evaluate` (reference
diffusion_classifier.py:565-568, :639-643).  The cross-rank sum of the int64 counters is the
reference's only explicit collective (`accelerator.reduce`, utils/metrics.py:56-58): here it is
an all-reduce(SUM) over `torch.distributed` (RCCL on ROCm) when no accelerate object is given.
Binary metrics treat class 1 as positive, like the reference.
"""
import torch
import torch.distributed as dist


class Metric(torch.nn.Module):
    counters = ()

    def __init__(self, name, device=torch.device("cpu")):
        super().__init__()
        self.name = name
        self.device = device
        self.required_output_keys = ()
        self.reset()

    def reset(self):
        for c in self.counters:
            setattr(self, c, torch.tensor(0, dtype=torch.int64, device=self.device))

    def set_device(self, device):
        self.device = device
        for c in self.counters:
            setattr(self, c, getattr(self, c).to(device))

    def _count(self, **masks):
        for c, m in masks.items():
            setattr(self, c, getattr(self, c) + m.sum().to(self.device))

    def update(self, output):
        raise NotImplementedError

    def compute(self):
        raise NotImplementedError

    def get_output(self, reduce=True):
        return self.compute()

    def sync_across_processes(self, accelerator=None):
        for c in self.counters:
            v = getattr(self, c)
            if accelerator is not None and hasattr(accelerator, "reduce"):
                v = accelerator.reduce(v)
            elif dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                v = v.clone()
                dist.all_reduce(v, op=dist.ReduceOp.SUM)
            setattr(self, c, v)

    def __call__(self, output):
        self.update(output)
        return self.compute()

    @staticmethod
    def _pair(output, device):
        y_pred, batch = output
        return y_pred.to(device), batch["prompt"].to(device)

    @staticmethod
    def _ratio(num, den):
        return 0.0 if den == 0 else num.float() / den.float()


class Accuracy(Metric):
    counters = ("correct", "total")

    def update(self, output):
        y_pred, y_true = self._pair(output, self.device)
        self._count(correct=(y_pred == y_true), total=torch.ones_like(y_true, dtype=torch.bool))

    def compute(self):
        return {self.name: self.correct / self.total}


class Precision(Metric):
    counters = ("tp", "fp")

    def __init__(self, name="precision", device=torch.device("cpu")):
        super().__init__(name, device)

    def update(self, output):
        y_pred, y_true = self._pair(output, self.device)
        self._count(tp=(y_pred == 1) & (y_true == 1), fp=(y_pred == 1) & (y_true == 0))

    def compute(self):
        return {self.name: self._ratio(self.tp, self.tp + self.fp)}


class Recall(Metric):
    counters = ("tp", "fn")

    def __init__(self, name="recall", device=torch.device("cpu")):
        super().__init__(name, device)

    def update(self, output):
        y_pred, y_true = self._pair(output, self.device)
        self._count(tp=(y_pred == 1) & (y_true == 1), fn=(y_pred == 0) & (y_true == 1))

    def compute(self):
        return {self.name: self._ratio(self.tp, self.tp + self.fn)}


class F1(Metric):
    counters = ("tp", "fp", "fn")

    def __init__(self, name="f1", device=torch.device("cpu")):
        super().__init__(name, device)

    def update(self, output):
        y_pred, y_true = self._pair(output, self.device)
        self._count(tp=(y_pred == 1) & (y_true == 1), fp=(y_pred == 1) & (y_true == 0), fn=(y_pred == 0) & (y_true == 1))

    def compute(self):
        return {self.name: self._ratio(2 * self.tp, 2 * self.tp + self.fp + self.fn)}


class _HistogramMetric(Metric):
    """Metrics on a continuous score: the state is int64 histograms over a FIXED binning, so ranks combine by the same
    all-reduce(SUM) as the scalar counters, whatever order the images came in.  Fed (labels, batch, ClassPosterior) by `evaluate`."""
    wants_posterior = True
    shape = ()

    def reset(self):
        for c in self.counters:
            setattr(self, c, torch.zeros(self.shape, dtype=torch.int64, device=self.device))

    @staticmethod
    def _triple(output, device):
        y_pred, batch, post = output
        return y_pred.to(device).view(-1), batch["prompt"].to(device).view(-1), post


class AUROC(_HistogramMetric):
    """Binary area under the ROC curve, class 1 positive, score = probs[:, 1], from `hist[label, bin]` over `bins` equal bins of
    [0, 1] (bin = floor(score * bins); score 1 falls into the last bin; a NaN score — an image without a valid posterior — into bin 0).
    A (positive, negative) pair inside one bin counts half, so the result is exact for scores that differ by bin, and off by at most
    sum_bin pos[bin] * neg[bin] / (2 P N) otherwise."""
    counters = ("hist",)

    def __init__(self, name="auroc", bins=1024, device=torch.device("cpu")):
        self.bins = int(bins)
        assert self.bins >= 1
        self.shape = (2, self.bins)
        super().__init__(name, device)

    def update(self, output):
        _, y_true, post = self._triple(output, self.device)
        score = post.probs[:, 1].to(self.device, torch.float32)
        b = torch.floor(torch.nan_to_num(score, nan=0.0) * self.bins).clamp(0, self.bins - 1).to(torch.int64)
        for lab in (0, 1):
            self.hist[lab] += torch.bincount(b[y_true == lab], minlength=self.bins)

    def compute(self):
        neg, pos = self.hist[0].to(torch.float64), self.hist[1].to(torch.float64)
        P, N = pos.sum(), neg.sum()
        if P == 0 or N == 0:
            return {self.name: float("nan")}
        below = torch.cumsum(neg, 0) - neg                       # negatives in lower bins
        return {self.name: ((pos * (below + 0.5 * neg)).sum() / (P * N)).item()}


class SelectiveAccuracy(_HistogramMetric):
    """Accuracy on the most confident `coverage` share of the images (rejection of uncertain cases).  Confidence `by`: "margin_z"
    (default), "margin", "max_prob" or "entropy" (negated: low entropy is confident).  State: `correct[bin]` / `total[bin]` over a fixed
    monotone binning of the fp32 confidence — the top `bits` bits of its order-preserving integer key (sign, exponent and the leading
    mantissa bits: 2^(bits - 9) bins per octave) — with a bin of its own for +inf above and for NaN below everything.  The k = ceil(coverage
    * n) most confident images are whole bins from the top; the bin the cut falls into contributes its accuracy for the remainder."""
    counters = ("correct", "total")

    def __init__(self, name, coverage, by="margin_z", bits=12, device=torch.device("cpu")):
        assert 0.0 < float(coverage) <= 1.0 and by in ("margin_z", "margin", "max_prob", "entropy") and 9 <= int(bits) <= 24
        self.coverage, self.by, self.bits = float(coverage), by, int(bits)
        self.shape = ((1 << self.bits) + 2,)                     # [0] NaN | finite and -inf, ascending | [-1] +inf
        super().__init__(name, device)

    def confidence(self, post):
        if self.by == "max_prob":
            return post.probs.max(dim=1).values
        if self.by == "entropy":
            return -post.entropy
        return getattr(post, self.by)

    def bin_of(self, conf):
        conf = conf.to(torch.float32) + 0.0                      # -0 -> +0
        u = conf.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        key = torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)      # monotone in the value
        b = (key >> (32 - self.bits)) + 1
        b = torch.where(conf == float("inf"), torch.full_like(b, self.shape[0] - 1), b)
        return torch.where(torch.isnan(conf), torch.zeros_like(b), b)

    def update(self, output):
        y_pred, y_true, post = self._triple(output, self.device)
        b = self.bin_of(self.confidence(post).to(self.device))
        self.total += torch.bincount(b, minlength=self.shape[0])
        self.correct += torch.bincount(b[y_pred == y_true], minlength=self.shape[0])

    def compute(self):
        import math
        n = int(self.total.sum())
        if n == 0:
            return {self.name: float("nan")}
        k = max(1, min(n, math.ceil(self.coverage * n - 1e-9)))
        tot = torch.flip(self.total, (0,)).to(torch.float64)     # most confident bin first
        cor = torch.flip(self.correct, (0,)).to(torch.float64)
        before = torch.cumsum(tot, 0) - tot
        take = (k - before).clamp(min=0).minimum(tot)            # images taken from each bin
        frac = torch.where(tot > 0, take / tot.clamp(min=1), torch.zeros_like(tot))
        return {self.name: ((cor * frac).sum() / k).item()}
