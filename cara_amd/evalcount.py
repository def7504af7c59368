"""The counting of ``cara_eval_accumulate`` (include/cara_hip.h) in plain torch, on whatever device the logits are on.

Not a forward: the model has no CPU path.  This is only what happens to a batch of logits once it exists -- rows scored,
top-1 hits, top-5 hits, the sum of the per-row cross-entropy, rows with an invalid label -- so that the shard and
all-reduce logic of ``CaraEngine.evaluate`` can be tested under gloo without a GPU, and so that the kernel has a yardstick
that shares no code with it.  Everything is computed in fp64 from the fp32 logits.

State: ``float64 [5] = (n, top1, top5, loss_sum, bad_labels)``, the kernel's five words (counts are exact in fp64 up to
2^53).  Tie rule, as in the kernel: the label's position in a stable descending sort of its row,
``rank = #{c: l[c] > l[y]} + #{c < y: l[c] == l[y]}``; top-1 is ``rank == 0`` (numpy.argmax's lowest index), top-5 is
``rank < 5``.  A row whose label is outside ``[0, classes)`` adds to the last word only.
"""
from __future__ import annotations

import math

import torch

STATE_WORDS = 5
N, TOP1, TOP5, LOSS, BAD = range(STATE_WORDS)


def new_state(device="cpu") -> torch.Tensor:
    return torch.zeros(STATE_WORDS, dtype=torch.float64, device=device)


def accumulate(state: torch.Tensor, logits: torch.Tensor, labels: torch.Tensor, n_valid: int = None) -> torch.Tensor:
    """Add the first ``n_valid`` rows (default: all) of ``logits`` [B, classes] / ``labels`` int64 [B] into ``state``."""
    n_valid = logits.shape[0] if n_valid is None else int(n_valid)
    if not 0 <= n_valid <= logits.shape[0] or labels.shape[0] != logits.shape[0]:
        raise ValueError("n_valid must lie in [0, B] and labels must hold B entries")
    l = logits[:n_valid].to(torch.float64)
    y = labels[:n_valid].to(torch.int64)
    classes = l.shape[1]
    ok = (y >= 0) & (y < classes)
    l, y = l[ok], y[ok]
    state[BAD] += float((~ok).sum())
    if l.shape[0] == 0:
        return state
    v = l.gather(1, y.view(-1, 1))
    cols = torch.arange(classes, device=l.device).view(1, -1)
    rank = (l > v).sum(1) + ((l == v) & (cols < y.view(-1, 1))).sum(1)
    state[N] += float(l.shape[0])
    state[TOP1] += float((rank == 0).sum())
    state[TOP5] += float((rank < 5).sum())
    state[LOSS] += (torch.logsumexp(l, dim=1) - v.view(-1)).sum()
    return state


COMBINE_MODES = ("prob", "logit")


def combine_views(logits: torch.Tensor, V: int, mode: str = "prob") -> torch.Tensor:
    """The V views' logits of every sample as one row: ``cara_eval_combine_views`` in plain torch, fp64 from the fp32 logits.
    ``logits`` [S*V, classes], the views of sample ``s`` in rows ``s*V .. s*V+V-1`` -> fp64 [S, classes], which ``accumulate`` /
    ``accumulate_report`` then score.  ``"prob"``: ``log(mean_v softmax(l_v))`` -- the loss of the row is ``-log pbar[y]``, its
    confidence ``max pbar``; a class with probability zero in every view gives ``-inf``, not NaN.  ``"logit"``: ``mean_v l_v``."""
    V = int(V)
    if mode not in COMBINE_MODES:
        raise ValueError(f"combine must be one of {COMBINE_MODES}, not {mode!r}")
    if logits.ndim != 2 or V < 1 or logits.shape[0] % V:
        raise ValueError("combine_views takes logits [S*V, classes] with V >= 1")
    l = logits.to(torch.float64).view(logits.shape[0] // V, V, logits.shape[1])
    if mode == "logit":
        return l.mean(dim=1)
    logp = torch.log_softmax(l, dim=2)
    top = logp.max(dim=1, keepdim=True).values
    # (where every view says -inf the shift would be inf - inf: shift by 0 there, the sum of the exponentials is 0, its log -inf)
    shift = torch.where(torch.isinf(top), torch.zeros_like(top), top)
    return (shift + torch.log(torch.exp(logp - shift).sum(dim=1, keepdim=True))).squeeze(1) - math.log(V)


def result(state) -> dict:
    """``dict(top1, top5, loss, n)`` of a state (a tensor or five numbers), the form ``CaraEngine.evaluate`` returns."""
    n, t1, t5, loss, bad = [float(v) for v in state]
    if bad:
        raise ValueError(f"{int(bad)} label(s) outside [0, classes)")
    d = max(n, 1.0)
    return {"top1": t1 / d, "top5": t5 / d, "loss": loss / d, "n": int(n)}


# ---- the evaluation report of ``cara_eval_accumulate_report``: confusion matrix and calibration bins ----------------------------
# A report is four fp64 tensors, the kernel's regions in the kernel's order: ``confusion`` [classes, classes] (row = label, column =
# predicted class), ``bin_count`` [bins], ``bin_hits`` [bins], ``bin_conf`` [bins].  ``pred`` = the lowest class index whose logit
# equals the row maximum (the top-1 tie rule), ``conf`` = the top softmax probability, ``bin = min(bins - 1, floor(conf * bins))``.
REPORT_KEYS = ("confusion", "bin_count", "bin_hits", "bin_conf")


def report_words(classes: int, bins: int) -> int:
    return int(classes) * int(classes) + 3 * int(bins)


def new_report(classes: int, bins: int, device="cpu") -> dict:
    if classes < 1 or bins < 1:
        raise ValueError("a report needs at least one class and one bin")
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=device)   # noqa: E731
    return {"confusion": z(classes, classes), "bin_count": z(bins), "bin_hits": z(bins), "bin_conf": z(bins)}


def report_vector(report: dict) -> torch.Tensor:
    """the report as one fp64 vector in the kernel's layout (what is all-reduced behind the five state words)"""
    return torch.cat([report[k].reshape(-1).to(torch.float64) for k in REPORT_KEYS])


def report_from_vector(vec, classes: int, bins: int) -> dict:
    """``report_vector`` undone: views into ``vec`` (a tensor of ``report_words(classes, bins)`` fp64 words)"""
    vec = torch.as_tensor(vec, dtype=torch.float64)
    if vec.ndim != 1 or vec.shape[0] != report_words(classes, bins):
        raise ValueError(f"a report of {classes} classes and {bins} bins holds {report_words(classes, bins)} words, not {tuple(vec.shape)}")
    cc = classes * classes
    return {"confusion": vec[:cc].view(classes, classes), "bin_count": vec[cc:cc + bins], "bin_hits": vec[cc + bins:cc + 2 * bins],
            "bin_conf": vec[cc + 2 * bins:]}


def accumulate_report(state: torch.Tensor, report: dict, logits: torch.Tensor, labels: torch.Tensor, n_valid: int = None):
    """``accumulate`` into ``state`` and, for the same rows, the confusion cell and the confidence bin into ``report``
    (``new_report(logits.shape[1], bins)``).  A row with a label outside ``[0, classes)`` touches nothing in ``report``.
    Everything in fp64 from the fp32 logits: ``conf = exp(max - logsumexp)``.  -> (state, report)"""
    accumulate(state, logits, labels, n_valid)
    n_valid = logits.shape[0] if n_valid is None else int(n_valid)
    classes, bins = logits.shape[1], report["bin_count"].shape[0]
    if tuple(report["confusion"].shape) != (classes, classes):
        raise ValueError(f"the report's confusion matrix is {tuple(report['confusion'].shape)}, the logits have {classes} classes")
    l = logits[:n_valid].to(torch.float64)
    y = labels[:n_valid].to(torch.int64)
    ok = (y >= 0) & (y < classes)
    l, y = l[ok], y[ok]
    if l.shape[0] == 0:
        return state, report
    top = l.max(dim=1).values
    cols = torch.arange(classes, device=l.device).view(1, -1).expand_as(l)
    pred = torch.where(l == top.view(-1, 1), cols, torch.full_like(cols, classes)).min(dim=1).values   # lowest index on ties
    conf = torch.exp(top - torch.logsumexp(l, dim=1))
    which = torch.clamp(torch.floor(conf * bins).to(torch.int64), max=bins - 1)
    ones = torch.ones_like(conf)
    report["confusion"].view(-1).index_add_(0, y * classes + pred, ones)
    report["bin_count"].index_add_(0, which, ones)
    report["bin_hits"].index_add_(0, which, (pred == y).to(torch.float64))
    report["bin_conf"].index_add_(0, which, conf)
    return state, report


def report_result(state, report: dict) -> dict:
    """``result(state)`` plus what the report holds, the form ``CaraEngine.evaluate(report=True)`` returns (CPU tensors):
    ``confusion`` int64 [C, C]; ``support`` int64 [C], the row sums; ``per_class`` fp64 [C], the recall ``diag / support`` (NaN
    without support); ``precision`` fp64 [C], the diagonal over the column sums (NaN for a class never predicted);
    ``mean_per_class``, the mean of ``per_class`` over the classes with support; ``ece = sum_b n_b / n |hits_b / n_b - conf_b / n_b|``
    over the non-empty bins; ``calibration = {"count", "hits", "confidence"}``, each of length ``bins``, as accumulated."""
    out = result(state)
    confusion = report["confusion"].detach().cpu().round().to(torch.int64)
    count = report["bin_count"].detach().cpu().round().to(torch.int64)
    hits = report["bin_hits"].detach().cpu().round().to(torch.int64)
    conf = report["bin_conf"].detach().cpu().to(torch.float64).clone()
    support, predicted, diag = confusion.sum(1), confusion.sum(0), confusion.diagonal().to(torch.float64)
    nan = torch.full_like(diag, float("nan"))
    per_class = torch.where(support > 0, diag / support.clamp(min=1), nan)
    precision = torch.where(predicted > 0, diag / predicted.clamp(min=1), nan)
    seen, filled = support > 0, count > 0
    gap = ((hits[filled].to(torch.float64) - conf[filled]) / count[filled]).abs()
    ece = float((count[filled].to(torch.float64) / max(out["n"], 1) * gap).sum())
    out.update(confusion=confusion, support=support, per_class=per_class, precision=precision,
               mean_per_class=float(per_class[seen].mean()) if bool(seen.any()) else float("nan"), ece=ece,
               calibration={"count": count, "hits": hits, "confidence": conf})
    return out



# ---- per-sample records of ``cara_eval_predict``: top-k classes and probabilities, loss and rank of every row ---------------------
# The contract of include/cara_hip.h taken literally, in fp64 from the fp32 logits; the ordering is a stable sort of ``-x``.
NO_FINITE_MAX = -3.0e38   # the kernels' floor of a row maximum (as the fp32 value nearest to it): below it a row matches no class


def predict_rows(logits: torch.Tensor, labels, k: int):
    """``logits`` [B, classes] (fp32 values), ``labels`` int64 [B] or None, ``k`` >= 1 -> ``(idx int32 [B, k], prob fp64 [B, k],
    loss fp64 [B], rank int32 [B])``, the last two None without labels.  ``idx[:, j]`` = the class at position ``j`` of the stable
    descending sort of the row (ties to the lowest index, ``-inf`` last in index order); slots ``j >= classes``: index -1,
    probability 0.  ``prob = exp(l[idx] - m) / sum exp(l - m)``; ``loss = m + log(sum) - l[label]``; ``rank`` as in ``accumulate``.
    A label outside ``[0, classes)``: rank -1, loss NaN.  A row without a finite maximum (nothing at or above the fp32 -3e38, or a
    NaN): index 0 then -1, every probability and the loss NaN."""
    k = int(k)
    if logits.ndim != 2 or logits.shape[1] < 1 or k < 1:
        raise ValueError("predict_rows takes logits [B, classes >= 1] and k >= 1")
    l = logits.detach().to(torch.float64).cpu()
    B, classes = l.shape
    kk = min(k, classes)
    order = torch.argsort(-l, dim=1, stable=True)[:, :kk]
    m = l.max(dim=1, keepdim=True).values
    floor = float(torch.tensor(NO_FINITE_MAX, dtype=torch.float32))
    degenerate = ~(m[:, 0] >= floor)                                   # (a NaN maximum compares false: degenerate)
    # (the kernels' maximum never falls below the floor; where the row has a class at or above it, it is the row's own maximum)
    shift = torch.where(degenerate.view(-1, 1), torch.zeros_like(m), m)
    s = torch.exp(l - shift).sum(dim=1, keepdim=True)
    idx = torch.full((B, k), -1, dtype=torch.int32)
    prob = torch.zeros(B, k, dtype=torch.float64)
    idx[:, :kk] = order.to(torch.int32)
    prob[:, :kk] = torch.exp(l.gather(1, order) - shift) / s
    idx[degenerate, 0] = 0
    idx[degenerate, 1:] = -1
    prob[degenerate] = float("nan")
    if labels is None:
        return idx, prob, None, None
    y = labels.detach().to(torch.int64).cpu()
    if y.shape != (B,):
        raise ValueError("labels must hold one entry per row")
    ok = (y >= 0) & (y < classes)
    ys = torch.where(ok, y, torch.zeros_like(y)).view(-1, 1)
    v = l.gather(1, ys)
    cols = torch.arange(classes).view(1, -1)
    rank = ((l > v).sum(1) + ((l == v) & (cols < ys)).sum(1)).to(torch.int32)
    loss = (shift + torch.log(s) - v)[:, 0]
    rank[~ok] = -1
    loss[~ok | degenerate] = float("nan")
    return idx, prob, loss, rank


class Predictions:
    """The table a ``CaraEngine.predict`` pass fills: ``topk`` int32 [N, k] and ``prob`` fp32 [N, k] (``cara_eval_predict``'s
    top-k classes and their softmax probabilities, best first), ``loss`` fp32 [N] and ``rank`` int32 [N] (None for a pass without
    labels), ``labels`` int64 [N] (the labels the pass read, None without) -- tensors on the device of the pass (or on the CPU:
    ``load``).  Row ``i`` of a ``ResidentSplit`` is sample ``i`` in file order.  Every helper below makes at most ONE host read."""

    def __init__(self, topk, prob, loss=None, rank=None, labels=None):
        if topk.ndim != 2 or prob.shape != topk.shape or (loss is None) != (rank is None):
            raise ValueError("Predictions: topk and prob are [N, k], loss and rank come together")
        self.topk, self.prob, self.loss, self.rank, self.labels = topk, prob, loss, rank, labels

    def __len__(self) -> int:
        return int(self.topk.shape[0])

    @property
    def k(self) -> int:
        return int(self.topk.shape[1])

    def _need_labels(self, what):
        from ._lib import CaraError
        if self.rank is None:
            raise CaraError(f"Predictions.{what}: the pass had no labels")

    def counts(self) -> dict:
        """``dict(top1, top5, loss, n)``, the form and -- in its integers -- the values of ``CaraEngine.evaluate`` on the same pass;
        the loss is the fp64 sum of the fp32 per-row terms.  A row with ``rank == -1`` (a label outside the classes) raises."""
        from ._lib import CaraError
        self._need_labels("counts")
        r = self.rank
        good = r >= 0
        words = torch.stack([good.sum().double(), (r == 0).sum().double(), (good & (r < 5)).sum().double(),
                             torch.where(good, self.loss.double(), torch.zeros((), dtype=torch.float64, device=r.device)).sum(),
                             (~good).sum().double()]).tolist()          # the only host read
        n, t1, t5, loss, bad = words
        if bad:
            raise CaraError(f"predict: {int(bad)} label(s) outside the classes of the head")
        d = max(n, 1.0)
        return {"top1": t1 / d, "top5": t5 / d, "loss": loss / d, "n": int(n)}

    def confusion(self, classes: int) -> torch.Tensor:
        """CPU int64 [classes, classes], row = label, column = ``topk[:, 0]``: ``evaluate(report=True)["confusion"]``"""
        self._need_labels("confusion")
        classes = int(classes)
        y, p = self.labels.to(torch.int64), self.topk[:, 0].to(torch.int64)
        ok = (y >= 0) & (y < classes) & (p >= 0) & (p < classes)
        cell = torch.where(ok, y * classes + p, torch.full_like(y, classes * classes))
        return torch.bincount(cell, minlength=classes * classes + 1)[:classes * classes].view(classes, classes).cpu()

    def errors(self) -> torch.Tensor:
        """CPU int64: the indices of the samples whose label is not the first slot (``rank != 0``), ascending"""
        self._need_labels("errors")
        return (self.rank != 0).cpu().nonzero()[:, 0]

    def confident(self, threshold: float):
        """``(indices, classes)``, CPU int64: the samples whose top probability is at least ``threshold`` and the class they are
        given -- pseudo-labels"""
        both = torch.stack([(self.prob[:, 0] >= float(threshold)).to(torch.int32), self.topk[:, 0]]).cpu()
        keep = both[0].nonzero()[:, 0]
        return keep, both[1][keep].to(torch.int64)

    def _words(self):
        """every column as int32 words of ONE [N, W] tensor (floats and int64 labels as their bits) and the column ranges"""
        cols = [("topk", self.topk.view(len(self), -1)), ("prob", self.prob.view(torch.int32))]
        if self.rank is not None:
            cols += [("loss", self.loss.view(torch.int32).view(-1, 1)), ("rank", self.rank.view(-1, 1))]
        if self.labels is not None:
            cols.append(("labels", self.labels.to(torch.int64).contiguous().view(torch.int32).view(-1, 2)))
        return torch.cat([c for _, c in cols], dim=1), [(n, c.shape[1]) for n, c in cols]

    def save(self, path: str, names=None) -> str:
        """write the table as an ``.npz`` (``topk``, ``prob`` and, when the pass had labels, ``loss``, ``rank``, ``labels``;
        ``names``: one string per row, or ``ResidentSplit.imlist``'s ``(path, label)`` pairs, stored as ``names``) -> the file name"""
        import numpy as np
        if names is not None and len(names) != len(self):
            raise ValueError(f"save: {len(names)} names for {len(self)} rows")
        words, cols = self._words()
        words = words.cpu().numpy()                                       # the only host read
        out, at = {}, 0
        kinds = {"prob": np.float32, "loss": np.float32, "labels": np.int64}
        for name, width in cols:
            a = np.ascontiguousarray(words[:, at:at + width]).view(kinds.get(name, np.int32))
            out[name] = a if name in ("topk", "prob") else a.reshape(-1)
            at += width
        if names is not None:
            out["names"] = np.array([n if isinstance(n, str) else n[0] for n in names], dtype=str)
        path = path if path.endswith(".npz") else path + ".npz"
        with open(path, "wb") as fh:
            np.savez(fh, **out)
        return path

    @classmethod
    def load(cls, path: str):
        """-> ``(Predictions on the CPU, names or None)`` of a file ``save`` wrote"""
        import numpy as np
        with np.load(path) as z:
            t = {n: torch.from_numpy(z[n]) for n in z.files if n != "names"}
            names = [str(n) for n in z["names"]] if "names" in z.files else None
        return cls(t["topk"], t["prob"], t.get("loss"), t.get("rank"), t.get("labels")), names
