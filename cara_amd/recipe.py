"""The reference's fine-tuning recipe as a host-side helper (``image_classification/vit_cp.py``).

* ``CosineLRScheduler``: timm 0.4.12 semantics for the arguments the reference passes
  (``vit_cp.py:187``: t_initial=100, warmup_t=10, lr_min=1e-5, warmup_lr_init=1e-6, decay_rate=0.1,
  single cycle, no warm-up prefix), stepped as the reference does: ``sched.step(epoch)`` after every
  BATCH (``vit_cp.py:55-56``), so the LR is a function of the epoch index only.
* ``fit``: the loop of ``vit_cp.py:19-70`` -- AdamW over the parameters whose name contains "CP" or
  "head" (``:175-185``), evaluation at epochs 10, 20, ... (``:57``), scheduler dropped from epoch
  50 on (``:58-59``), and the reference's quirk that ``test()`` switches to eval mode and nothing
  switches back (``:75``; DropPath is therefore only active for epochs 0-10).
The arithmetic of every step runs in libcara_hip.so through ``CaraEngine.train_step``.
"""
from __future__ import annotations

import math
from typing import Callable, Iterable, Optional

import torch

from ._lib import CaraError
from .feed import Feed
from .loss import BCE, Distill, check_distill, check_loss


class CosineLRScheduler:
    def __init__(self, optimizer, t_initial: int, lr_min: float = 0.0, warmup_t: int = 0, warmup_lr_init: float = 0.0,
                 decay_rate: float = 1.0, cycle_limit: int = 1):
        self.opt = optimizer
        self.t_initial, self.lr_min, self.warmup_t, self.warmup_lr_init = t_initial, lr_min, warmup_t, warmup_lr_init
        self.decay_rate, self.cycle_limit = decay_rate, cycle_limit
        self.base = [g["lr"] for g in optimizer.param_groups]
        if warmup_t:
            self.warmup_steps = [(b - warmup_lr_init) / warmup_t for b in self.base]
            self._set([warmup_lr_init] * len(self.base))   # timm initialises the groups to warmup_lr_init
        else:
            self.warmup_steps = [1.0] * len(self.base)

    def _set(self, lrs):
        for g, lr in zip(self.opt.param_groups, lrs):
            g["lr"] = lr

    def lr_at(self, t: int):
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * s for s in self.warmup_steps]
        i = t // self.t_initial
        t_curr = t - self.t_initial * i
        gamma = self.decay_rate ** i
        if i < self.cycle_limit:
            return [self.lr_min * gamma + 0.5 * (b * gamma - self.lr_min * gamma) * (1 + math.cos(math.pi * t_curr / self.t_initial))
                    for b in self.base]
        return [self.lr_min * (self.decay_rate ** self.cycle_limit)] * len(self.base)

    def step(self, epoch: int):
        self._set(self.lr_at(epoch))


def trainable_parameters(model):
    """vit_cp.py:175-183: train names containing "CP" or "head", freeze the rest."""
    out = []
    for n, p in model.named_parameters():
        if "CP" in n or "head" in n:
            out.append(p)
        else:
            p.requires_grad = False
    return out


@torch.no_grad()
def evaluate(model, batches: Iterable) -> float:
    """vit_cp.py:73-82: eval mode (and it stays on), top-1 accuracy."""
    model.eval()
    hit = tot = 0
    for x, y in batches:
        out = model(x)
        hit += (out.argmax(dim=1).view(-1) == y).sum().item()
        tot += y.numel()
    return hit / max(tot, 1)


def checkpoint_name(dataset: str, acc: float, seed: int, directory: str = ".") -> str:
    """File name of the reference's best-accuracy checkpoint (vit_cp.py:65)."""
    import os
    return os.path.join(directory, f"vit_{dataset}_{round(acc, 5)}_seed_{seed}.pt")


def save_checkpoint(model, path: str, weights=None) -> None:
    """vit_cp.py:66: ``th.save(vit.state_dict(), name)`` -- the WHOLE state dict (frozen backbone, 12 CP_* tensors,
    head), keys of timm 0.4.12, tensors on the CPU so that the file loads anywhere.
    ``weights`` (a ``ParamEma``, e.g. ``CaraEngine.make_ema``): the same keys, with the entry of every averaged parameter taken
    from its shadow -- ``load_checkpoint`` then gives the model that ``evaluate(..., weights=)`` scored."""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    if weights is not None:
        names = {id(p): n for n, p in model.named_parameters()}
        for p, s in zip(weights.params, weights.tensors):
            n = names.get(id(p))
            if n is None or n not in sd or sd[n].shape != s.shape:
                raise CaraError("save_checkpoint: weights must average parameters of this model (CaraEngine.make_ema)")
            sd[n] = s.detach().cpu()
    torch.save(sd, path)


def load_checkpoint(model, path: str) -> None:
    """vit_cp.py:170 (``--evaluate``): ``vit.load_state_dict(th.load(path))``, strict, after ``cara()`` and
    ``reset_classifier()``.  The engine notices the in-place change of the backbone parameters and re-ingests them."""
    sd = torch.load(path, map_location="cpu")
    model.load_state_dict(sd)


def evaluate_only(model, path: str, test_batches: Iterable) -> float:
    """The ``--evaluate`` flow of vit_cp.py:168-173: load, test, return the accuracy."""
    load_checkpoint(model, path)
    return evaluate(model, test_batches)


KEEP_AHEAD = 64   # steps of keep tables per draw of fit(patch_drop=)


class GraphedTrainStep:
    """``CaraEngine.train_step`` captured into a hipGraph and replayed (``cara_vit_forward`` / ``cara_vit_backward`` only enqueue
    work on the caller's stream, include/cara_hip.h; the optimiser must be ``cara_amd.optim.AdamW(capturable=True)``: its step count
    and learning rates live in device memory).  The first call with a new key runs eagerly (weights ingested, workspaces sized), the
    second captures, later ones copy the inputs into the graph's static buffers, upload { step, lr } and replay.  What a capture
    cannot hold runs eagerly, every time: more than one rank (the all-reduce) and the exact weight-dropout mode (a fresh host-side
    seed per step).  Same switch as ``bench.py --graph``.
    Two forms.  ``step(images, labels)`` captures ``train_step``: the batch and its labels are the static inputs.  ``step(split,
    item)`` captures ``train_step_resident`` on a ``data.ResidentSplit``: ``item`` is what ``train_rows`` yields -- an index vector,
    or a tuple of it and its tables (``feed.Feed``) -- and the static inputs are the index vector and the tables present, nothing
    else: per sample and replay 8 bytes of ``rows``, 20 of ``boxes``, 32 of ``mix``, 64 of ``aug``, 4 K of ``keep``, 64 of ``ra``, no
    image.  One graph per (form, split, which tables, every input's shape, train / eval mode, precision, smoothing, clip): another K
    of ``keep`` captures another graph.  ``label_smoothing`` and ``clip_grad`` are the steps' (the two launches of ``cara_grad_clip``
    are captured with the step).  An accumulation window (``accumulate`` with k > 1) spans several replays and is refused.
    ``ema`` (``CaraEngine.make_ema(..., capturable=True)``): the average's launch is captured behind the optimiser's; its weight
    lives in device memory and ``ema.advance()`` runs before every step, as ``optimizer.advance()`` does.
    ``class_weight`` / ``logit_bias`` (``train_step``'s): the graph captures the two tensors' addresses, so they are held here and in
    every entry and their identity is part of the key; a replay re-reads their contents, as it re-reads a mix table -- an in-place
    change takes effect at the next call (and is checked there, on the host, before the replay).
    ``sam_rho`` (``train_step``'s): both passes of the SAM step, the measuring launches and the two launches that move the weights and
    put them back are captured in the ONE graph; the value is part of the key (``("sam_rho", rho)``), and the engine's SAM buffers
    are never replaced, so the graph's addresses stay good.
    ``loss`` (``train_step``'s: a ``loss.BCE`` or ``loss.Focal``): the object -- and with it a BCE's ``pos_weight`` tensor, whose address
    the graph captures -- is held here and in every entry; its settings and that tensor's identity are part of the key, and a replay
    re-reads the tensor's contents as it re-reads ``class_weight`` (checked on the host before the replay).
    ``distill`` (``train_step``'s: a ``loss.Distill``): the teacher pass is captured with the rest of the step.  What keeps the
    graph's addresses good is that every entry HOLDS the object (and with it a tensor teacher or the teacher model),
    ``engine.teacher_logits`` and a model teacher's workspace.  The object's identity is also named in the key; since the object
    is fixed for the life of this ``GraphedTrainStep`` that only labels the entry, it tells no two entries apart.  A tensor teacher is
    a static input of the caller's: the graph holds its address and every replay re-reads its contents."""

    def __init__(self, engine, optimizer, label_smoothing: float = 0.0, clip_grad=None, ema=None, class_weight=None, logit_bias=None,
                 sam_rho=None, loss=None, distill=None):
        if not getattr(optimizer, "capturable", False):
            raise CaraError("GraphedTrainStep needs cara_amd.optim.AdamW(capturable=True)")
        if ema is not None and not getattr(ema, "capturable", False):
            raise CaraError("GraphedTrainStep needs CaraEngine.make_ema(..., capturable=True)")
        self.eng, self.opt, self.ema = engine, optimizer, ema
        self.label_smoothing = engine._smoothing(label_smoothing) if label_smoothing else 0.0
        self.clip_grad = engine._max_norm(clip_grad)
        self.class_weight, self.logit_bias = class_weight, logit_bias
        self.sam_rho = engine._sam_rho(sam_rho)
        self.loss = check_loss(loss, class_weight, logit_bias)
        self.distill = check_distill(distill, loss, class_weight, logit_bias)
        self._graphs = {}   # key -> "warm", then (graph, source, static inputs, loss, held): source is the split, None for images

    def _kw(self):
        # (a step without smoothing, without a clip and without an average is called exactly as before)
        kw = {"label_smoothing": self.label_smoothing} if self.label_smoothing else {}
        if self.clip_grad is not None:
            kw["clip_grad"] = self.clip_grad
        if self.ema is not None:
            kw["ema"] = self.ema
        if self.class_weight is not None:
            kw["class_weight"] = self.class_weight
        if self.logit_bias is not None:
            kw["logit_bias"] = self.logit_bias
        if self.sam_rho is not None:
            kw["sam_rho"] = self.sam_rho
        if self.loss is not None:
            kw["loss"] = self.loss
        if self.distill is not None:
            kw["distill"] = self.distill
        return kw

    def __call__(self, x, y, group=None, accumulate=None, keep=None):
        """``(images, labels)``, or ``(split, item)`` with ``item`` an index vector or a tuple of it and its tables in ``Feed``'s
        order; ``keep=`` hands a patch-dropout table (device int32 [batch, K]) to the image form, and to a resident item without
        one.  Everything is refused here, not inside a capture."""
        if self.eng._window(accumulate)[1] > 1:
            raise CaraError("GraphedTrainStep: accumulate with k > 1 is not supported (the window spans several graph replays)")
        eng, kw = self.eng, self._kw()
        if self.class_weight is not None or self.logit_bias is not None or self.loss is not None:
            head = eng._model().head
            if not hasattr(head, "weight"):
                raise CaraError("the classifier head must be a Linear (num_classes > 0)")
            eng._class_vectors(self.class_weight, self.logit_bias, head.weight.shape[0], head.weight.device)
            if self.loss is not None:
                self.loss.check_pos_weight(head.weight.shape[0], head.weight.device, eng.__dict__.setdefault("_class_vec_ok", {}))
        if hasattr(x, "pixels"):
            feed = Feed.of(y)
            if feed.keep is None and keep is not None:
                feed = feed._replace(keep=keep)
            _, dev = eng._resident_args(x, feed)
            eng._teacher_of(self.distill, dev, feed.rows.shape[0], keep=feed.keep)
            names = tuple(feed.tables())
            # (the split itself is part of the key, not its id(): the entry then keeps it -- and the address the graph reads -- alive)
            return self._run(lambda s: eng.train_step_resident(x, s[0], self.opt, group=group, **dict(zip(names, s[1:])), **kw),
                             feed.static(), ("resident", x, names), group)
        if self.distill is not None:
            eng._teacher_of(self.distill, x.device, x.shape[0], keep=keep)
        if keep is None:
            return self._run(lambda s: eng.train_step(s[0], s[1], self.opt, group=group, **kw), (x, y), ("images", None, ()), group)
        if x.ndim != 4 or x.shape[2] != x.shape[3]:
            raise CaraError("images must be [B, C, H, H]")
        eng._check_table("keep", keep, x.shape[0], x.device, eng._patches(x.shape[2]))
        return self._run(lambda s: eng.train_step(s[0], s[1], self.opt, group=group, keep=s[2], **kw), (x, y, keep),
                         ("images", None, ("keep",)), group)

    def _distill_held(self):
        """what a captured distilled step reads besides the engine's own buffers: the object (its tensor teacher or the teacher model),
        the engine's teacher-logits buffer and a model teacher's workspace of the captured shape"""
        d = self.distill
        if d is None:
            return None
        teng = getattr(d.teacher, "_cara_engine", None)
        return (d, self.eng.teacher_logits, None if teng is None else teng._ws[teng._last_key]["ws"])

    def _run(self, step, live, key, group):
        """warm, capture, replay: ``step(inputs)`` is the eager step on a tuple shaped like ``live``, this call's inputs;
        ``key = (form, source, table names)`` is completed with the shapes and the settings that change the launches"""
        from . import dist as cdist
        eng, model = self.eng, self.eng._model()
        self.opt.advance()
        if self.ema is not None:
            self.ema.advance()
        if cdist.world_size(group) > 1 or (eng.weight_dropout == "exact" and model.training):
            return step(live)
        key = (*key, tuple(tuple(t.shape) for t in live), bool(model.training), eng.precision, self.label_smoothing, self.clip_grad)
        if self.class_weight is not None or self.logit_bias is not None:
            key = (*key, id(self.class_weight), id(self.logit_bias))
        if self.sam_rho is not None:
            key = (*key, ("sam_rho", self.sam_rho))
        if self.loss is not None:
            key = (*key, ("loss", *self.loss.key()))
        if self.distill is not None:
            key = (*key, ("distill", id(self.distill)))
        ent = self._graphs.get(key)
        if ent is None:
            self._graphs[key] = "warm"
            return step(live)
        dev = live[0].device
        if ent == "warm":
            static = tuple(t.clone() for t in live)
            torch.cuda.synchronize(dev)
            gr = torch.cuda.CUDAGraph()
            gen = eng._device_generator(dev)
            if gen is not None:
                gr.register_generator_state(gen)
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                with torch.cuda.graph(gr, stream=side):
                    loss = step(static)
            torch.cuda.current_stream(dev).wait_stream(side)
            # (the last element keeps what the engine would replace at an eager step of another batch size in between -- its dlogits
            # buffer and the workspace of this shape -- as ``loss`` keeps its loss buffer: the graph holds their addresses)
            ent = self._graphs[key] = (gr, key[1], static, loss, (eng._dlogits, eng._ws[eng._last_key]["ws"], self.class_weight, self.logit_bias,
                                                                   self.loss, getattr(self.loss, "pos_weight", None), self._distill_held()))
            # (the capture itself ran nothing: fall through to the replay, which is this call's step)
        gr, _, static, loss = ent[:4]
        for s, t in zip(static, live):
            s.copy_(t)
        gr.replay()
        return loss


def fit(model, train_batches: Callable[[int], Iterable], test_batches: Optional[Callable[[], Iterable]] = None,
        epochs: int = 100, lr: float = 1e-3, weight_decay: float = 1e-4, group=None, reference_eval_quirk: bool = True,
        on_eval: Optional[Callable[..., None]] = None, save_best: Optional[dict] = None, seed: Optional[int] = None,
        graph: bool = False, eval_mode: str = "reference", feed: str = "batches", label_smoothing: float = 0.0, clip_grad=None,
        accum_steps: int = 1, ema_decay: Optional[float] = None, ema_warmup: bool = False, patch_drop=None,
        eval_metric: str = "top1", class_weight=None, logit_bias=None, eval_views=None, eval_combine: str = "prob", sam_rho=None, loss=None,
        save_predictions: Optional[str] = None, distill=None):
    """``train_batches(epoch)`` yields (images, labels) already on the device (per-rank shard under
    data parallelism).  Returns (best accuracy, optimizer).

    ``save_best = {"dataset": name, "seed": s, "dir": path}``: keep the state dict of the best evaluation so far on
    disk as the reference does (vit_cp.py:61-66: save on improvement, delete the previous file); the path of the
    file is left in ``save_best["path"]``.  Rank 0 only under data parallelism.
    Data parallel (``torch.distributed`` initialised, more than one rank in ``group``): the trainable parameters are
    broadcast from rank 0 once, and every rank draws its own DropPath / weight-dropout masks from private streams
    seeded with (``seed``, rank); ``seed = None`` derives it from ``torch.initial_seed()`` (what the reference's
    ``torch.manual_seed(args.seed)`` set, vit_cp.py:139-144), so runs with different global seeds stay uncorrelated.
    Single process: the masks come from torch's global generators, exactly as in the reference, unless a ``seed`` is
    passed explicitly.
    ``graph = True``: the step is replayed from a hipGraph (``GraphedTrainStep``; the host then issues one launch per step
    instead of ~600: for boxes where several ranks share few cores).  Eager is the default: the step is GPU-bound.
    ``eval_mode = "sharded"``: ``test_batches`` is a ``data.ResidentSplit`` (or a callable returning batches in the form of
    its ``eval_shard``) and the evaluation epochs run ``CaraEngine.evaluate`` on it -- every rank scores its own part of
    the split on the device and all of them get the global top-1 accuracy.  ``"reference"`` (default): ``evaluate`` below
    over ``test_batches()``, on every rank.
    ``feed = "resident"``: ``train_batches`` is ``(split, rows_of)`` -- a ``data.ResidentSplit`` on the model's device and its
    ``train_rows(...)`` (``get_data(resident_feed=True)`` returns the pair) -- and every step is ``CaraEngine.train_step_resident``
    on an index vector: the same samples in the same order as ``split.train_batches(...)`` with the same seed, without the
    normalised fp32 batch.  An index outside the split is counted on the device, not read; the count is looked at where the
    evaluation epochs read from the device anyway and once more after the last epoch, and a non-zero one raises.
    ``rows_of`` yields index vectors, or tuples of one and its tables in ``feed.Feed``'s order (``train_rows(..., augment=, mix=,
    color=, patch_drop=, rand=)``: None for a table not asked for in front of one that is); the tables present are
    ``train_step_resident``'s keyword arguments of those names.  A crop box outside its image, and an entry of ``mix``, ``aug``,
    ``keep`` or ``ra`` that the kernel refuses (``data.check_mix`` ...), is counted like a bad row.
    ``label_smoothing`` in [0, 1): every step's loss is the smoothed cross-entropy (both feeds).
    ``clip_grad = max_norm``: every optimiser step clips the global gradient norm first (``train_step(..., clip_grad=)``; both
    feeds, eager and graphed).  ``accum_steps = k`` > 1: ``k`` consecutive batches of an epoch form a window -- one optimiser step,
    one all-reduce and one scheduler step per window on the sum of their gradients (``train_step(..., accumulate=(i, k))``), an
    effective batch of ``k`` batches.  The batches of a window are held until it is complete, and a trailing incomplete window at
    the end of an epoch is DROPPED without being run: ``drop_last`` at window granularity.  Not with ``graph = True``.
    ``ema_decay = d``: an exponential moving average of the trainable tensors (``CaraEngine.make_ema(d, warmup=ema_warmup)``, built
    after the broadcast; one more launch per optimiser step, every feed, eager and graphed).  The evaluation epochs then score
    BOTH the raw parameters and the average -- ``eval_mode = "sharded"`` hands the shadows to ``CaraEngine.evaluate(weights=)``,
    ``"reference"`` runs the module forward with every averaged parameter's ``.data`` swapped for its shadow and restored
    afterwards -- and call ``on_eval(epoch, raw_accuracy, averaged_accuracy)``; the AVERAGED accuracy is the one that is compared,
    returned and named in the checkpoint file, and ``save_best`` writes the averaged weights (``save_checkpoint(weights=)``).
    The average is left in ``model._cara_engine.ema``.  ``ema_decay = None``: nothing of this runs and ``on_eval(epoch, accuracy)``
    is called as before.
    ``patch_drop`` (a ``data.PatchDropout``; the ``"batches"`` feed): every training step runs on the kept patch tokens of a table
    drawn on the host from a generator seeded by (seed, epoch, rank) on the stream of ``data.keep_seed`` -- one generator per epoch,
    drawn ``KEEP_AHEAD`` steps at a time (the feed does not say how many batches an epoch has), checked (``data.check_keep``) and
    uploaded once per draw; each step gets a [batch, K] view (``train_step(..., keep=)``).  Every micro-batch of an accumulation
    window has its own rows, every rank its own stream, and the graphed step takes the table as a static input.  The evaluation
    epochs see every patch.  The resident feed carries its table itself: ``train_rows(..., patch_drop=)``.
    ``eval_metric = "mean_per_class"`` (``eval_mode = "sharded"`` only): the evaluation epochs call
    ``CaraEngine.evaluate(report=True)`` and the mean per-class accuracy (the mean recall over the classes the split holds) is the
    number that is compared, returned, passed to ``on_eval`` and named in the ``save_best`` file -- with ``ema_decay`` for the raw
    and the averaged pass alike.  ``"top1"`` (default): the top-1 accuracy, with the calls that were always made.
    ``class_weight`` / ``logit_bias`` (fp32 [classes], host or device, e.g. ``data.balanced_class_weight`` / ``data.logit_prior`` of
    ``data.class_counts(split, classes)``): moved to the model's device once, and every training step of either feed, eager or
    graphed, runs the weighted, logit-adjusted loss (``train_step(..., class_weight=, logit_bias=)``).  The evaluation epochs are
    unchanged: they score the raw logits.
    ``eval_views`` (a ``data.EvalViews``; ``eval_mode = "sharded"`` only, ``test_batches`` a ``ResidentSplit`` of any stored size) and
    ``eval_combine`` (``"prob"`` / ``"logit"``): the evaluation epochs score every test image through those views
    (``CaraEngine.evaluate(views=, combine=)``: centre crop, flips, five / ten crops) -- the raw and the averaged pass alike, with
    either ``eval_metric``.  None (default): the calls that were always made.
    ``sam_rho`` (a number >= 0): every training step of either feed is a sharpness-aware one (``train_step(..., sam_rho=)``: two
    forward/backward passes per micro-step, the optimiser steps on the gradient at the perturbed weights) -- with ``accum_steps``,
    ``clip_grad`` and ``ema_decay``, eager or graphed (both passes in the one graph).  Not with ``weight_dropout = "exact"``.
    ``loss`` (a ``loss.BCE`` or ``loss.Focal``): every training step of either feed, eager or graphed, trains on that sigmoid loss
    (``train_step(..., loss=)``); a BCE's ``pos_weight`` (host or device) is moved to the model's device once.  Not beside
    ``class_weight`` / ``logit_bias``.  ``evaluate`` is untouched: the evaluation epochs score the raw logits, and the loss they
    report stays the softmax cross-entropy, whatever the training loss is.
    ``save_predictions`` (a file name; ``eval_mode = "sharded"`` only): every evaluation that becomes the best so far -- the one
    ``save_best`` keeps the weights of -- is followed by one ``CaraEngine.predict`` pass with the same ``eval_views`` /
    ``eval_combine`` and the same weights (the average with ``ema_decay``), and rank 0 writes its table there
    (``evalcount.Predictions.save``, with the split's file names when the source is a ``ResidentSplit``): when ``fit`` returns
    the file holds the per-sample predictions of the returned best pass.
    ``distill`` (a ``loss.Distill``): every training step of either feed, eager or graphed, is a distilled one (``train_step(...,
    distill=)``).  ``Distill("ema", ...)`` with ``ema_decay = d`` is the mean teacher: the string is replaced by the average this
    call trains with.  Not beside ``loss``, ``class_weight`` or ``logit_bias``.  The evaluation epochs are untouched."""
    check_loss(loss, class_weight, logit_bias)
    check_distill(distill, loss, class_weight, logit_bias)
    if distill is not None and distill.kind() == "fit" and ema_decay is None:
        raise CaraError("fit: Distill('ema') names the average fit trains with: it needs ema_decay")
    if save_predictions is not None and eval_mode != "sharded":
        raise CaraError("fit: save_predictions is written by CaraEngine.predict: it needs eval_mode = 'sharded'")
    if eval_views is not None and eval_mode != "sharded":
        raise CaraError("fit: eval_views are read by CaraEngine.evaluate(views=): they need eval_mode = 'sharded'")
    if eval_metric not in ("top1", "mean_per_class"):
        raise CaraError(f"eval_metric must be 'top1' or 'mean_per_class', not {eval_metric!r}")
    if eval_metric == "mean_per_class" and eval_mode != "sharded":
        raise CaraError("fit: eval_metric = 'mean_per_class' is computed by CaraEngine.evaluate(report=True): it needs eval_mode = 'sharded'")
    if patch_drop is not None and feed != "batches":
        raise CaraError("fit: patch_drop is the 'batches' feed's; the resident feed carries its table itself (train_rows(..., patch_drop=))")
    if patch_drop is not None and not callable(getattr(patch_drop, "draw", None)):
        raise CaraError("fit: patch_drop must be a data.PatchDropout (anything with draw(P, B, steps, generator))")
    if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1:
        raise CaraError(f"accum_steps must be an integer >= 1, not {accum_steps!r}")
    if graph and accum_steps > 1:
        raise CaraError("fit: accum_steps > 1 cannot run with graph = True (an accumulation window spans several graph replays)")
    if eval_mode not in ("reference", "sharded"):
        raise CaraError(f"eval_mode must be 'reference' or 'sharded', not {eval_mode!r}")
    if feed not in ("batches", "resident"):
        raise CaraError(f"feed must be 'batches' or 'resident', not {feed!r}")
    from . import dist as cdist
    eng = model._cara_engine
    smooth = {"label_smoothing": eng._smoothing(label_smoothing)} if label_smoothing else {}
    if clip_grad is not None:
        smooth["clip_grad"] = eng._max_norm(clip_grad)
    if sam_rho is not None:
        smooth["sam_rho"] = eng._sam_rho(sam_rho)
    if class_weight is not None or logit_bias is not None:
        if not hasattr(model.head, "weight"):
            raise CaraError("the classifier head must be a Linear (num_classes > 0)")
        hdev = model.head.weight.device
        for name, t in (("class_weight", class_weight), ("logit_bias", logit_bias)):
            if t is None:
                continue
            if not torch.is_tensor(t):
                raise CaraError(f"fit: {name} must be an fp32 [classes] tensor, not {type(t).__name__}")
            smooth[name] = t.detach().to(hdev).contiguous()
        eng._class_vectors(smooth.get("class_weight"), smooth.get("logit_bias"), model.head.weight.shape[0], hdev)
    if loss is not None:
        if not hasattr(model.head, "weight"):
            raise CaraError("the classifier head must be a Linear (num_classes > 0)")
        hdev = model.head.weight.device
        if loss.pos_weight is not None and loss.pos_weight.device != hdev:
            loss = BCE(loss.target_threshold, loss.pos_weight.detach().to(hdev).contiguous(), loss.sum_classes)
        loss.check_pos_weight(model.head.weight.shape[0], hdev, eng.__dict__.setdefault("_class_vec_ok", {}))
        smooth["loss"] = loss
    model.train()
    params = trainable_parameters(model)
    if cdist.world_size(group) > 1:
        cdist.broadcast_parameters(params, group=group)
    if cdist.world_size(group) > 1 or seed is not None:
        run_seed = int(seed) if seed is not None else int(torch.initial_seed() % (1 << 40))
        model._cara_engine.seed_rank_streams(run_seed, cdist.get_rank(group))
    if seed is None:
        seed = int(torch.initial_seed() % (1 << 31))   # (only names the checkpoint file below, like args.seed in vit_cp.py:65)
    # vit_cp.py:185's torch.optim.AdamW, as one HIP launch over the 14 trainable tensors (cara_amd/optim.py: same arithmetic)
    from .optim import AdamW
    opt = AdamW(params, lr=lr, weight_decay=weight_decay, capturable=graph)
    sched = CosineLRScheduler(opt, t_initial=100, warmup_t=10, lr_min=1e-5, warmup_lr_init=1e-6, decay_rate=0.1)
    ema = None
    if ema_decay is not None:
        ema = eng.ema = eng.make_ema(ema_decay, warmup=ema_warmup, capturable=graph)
        smooth["ema"] = ema
    if distill is not None:
        if distill.kind() == "fit":
            distill = Distill(ema, distill.alpha, distill.temperature, distill.hard)
        smooth["distill"] = distill
    gstep = GraphedTrainStep(eng, opt, **smooth) if graph else None
    best = 0.0
    scored = {"report": True} if eval_metric == "mean_per_class" else {}
    if eval_views is not None:
        scored.update(views=eval_views, combine=eval_combine)
    if feed == "resident":
        split, rows_of = train_batches
        train_batches = lambda epoch: ((split, rows) for rows in rows_of(epoch))   # noqa: E731

        def step(split, item, opt, group=None, **win):
            f = Feed.of(item)
            return eng.train_step_resident(split, f.rows, opt, group=group, **f.tables(), **smooth, **win)
    else:
        def step(x, y, opt, group=None, **win):
            return eng.train_step(x, y, opt, group=group, **smooth, **win)
    drawn = {"epoch": None}

    def keep_of(epoch, x):
        """the next step's [batch, K] view of the epoch's keep table ({} without a patch dropout)"""
        if patch_drop is None:
            return {}
        from .data import check_keep, keep_seed
        if x.ndim != 4 or x.shape[2] != x.shape[3]:
            raise CaraError("images must be [B, C, H, H]")
        B, P = x.shape[0], (x.shape[2] // model.patch_embed.proj.kernel_size[0]) ** 2
        if getattr(patch_drop, "grid", None) not in (None, P):
            raise CaraError(f"fit: patch_drop was built for a grid of {patch_drop.grid} patches, the images have {P}")
        if drawn["epoch"] != epoch:
            drawn.update(epoch=epoch, gen=torch.Generator().manual_seed(keep_seed(seed, epoch, cdist.get_rank(group))), table=None, next=0)
        t = drawn["table"]
        if t is None or drawn["next"] >= t.shape[0] or t.shape[1] != B:
            t = patch_drop.draw(P, B, KEEP_AHEAD, drawn["gen"])
            check_keep(t, B, P)
            t = drawn["table"] = t.contiguous().to(x.device)
            drawn["next"] = 0
        drawn["next"] += 1
        return {"keep": t[drawn["next"] - 1]}

    def check_rows(upto):
        # (data parallel: a rank that raised alone would leave the others waiting in the next all-reduce.  train_rows range-checks
        # an epoch's indices on the host before it uploads them, on every rank, so only a hand-made feed can get here)
        bad = eng.resident_bad_rows() if feed == "resident" else 0
        if bad:
            raise CaraError(f"fit: {bad} row index(es) outside the training split (or crop boxes outside their image, or mix entries "
                            f"with a partner outside the batch, a rectangle outside the output or a weight outside [0, 1], or aug entries "
                            f"data.check_aug refuses, or keep entries outside the patch grid, or ra entries data.check_ra refuses) reached "
                            f"the device up to epoch {upto}")
    for epoch in range(epochs):
        window = []
        for x, y in train_batches(epoch):
            kept = keep_of(epoch, x) if feed == "batches" else {}
            if accum_steps > 1:
                window.append((x, y, kept))
                if len(window) < accum_steps:
                    continue                    # (what is left in `window` when the epoch ends is dropped)
                for i, (wx, wy, wk) in enumerate(window):
                    step(wx, wy, opt, group=group, accumulate=(i, accum_steps), **wk)
                window = []
            elif gstep is not None:
                gstep(x, y, group=group, **kept)
            else:
                step(x, y, opt, group=group, **kept)
            if sched is not None:
                sched.step(epoch)
        if epoch % 10 == 0 and epoch != 0:
            if epoch >= 50:
                sched = None
            check_rows(epoch)
            if test_batches is not None:
                if eval_mode == "sharded":
                    acc = eng.evaluate(test_batches, group=group, **scored)[eval_metric]
                else:
                    acc = evaluate(model, test_batches())
                raw = acc
                if ema is not None:
                    if eval_mode == "sharded":
                        acc = eng.evaluate(test_batches, group=group, weights=ema, **scored)[eval_metric]
                    else:
                        with ema.swapped_in():
                            acc = evaluate(model, test_batches())
                if acc > best and save_best is not None and cdist.get_rank(group) == 0:
                    import os
                    old = save_best.get("path")
                    if old and os.path.exists(old):
                        os.remove(old)
                    save_best["path"] = checkpoint_name(save_best.get("dataset", "task"), acc, save_best.get("seed", seed),
                                                        save_best.get("dir", "."))
                    save_checkpoint(model, save_best["path"], weights=ema)
                if acc > best and save_predictions is not None:
                    # (every rank takes part in the pass's all-reduce; the pass that was just scored: views and weights alike)
                    table = eng.predict(test_batches, group=group, weights=ema,
                                        **({"views": eval_views, "combine": eval_combine} if eval_views is not None else {}))
                    if cdist.get_rank(group) == 0:
                        table.save(save_predictions, names=getattr(test_batches, "imlist", None))
                best = max(best, acc)
                if on_eval:
                    on_eval(epoch, acc) if ema is None else on_eval(epoch, raw, acc)
                if not reference_eval_quirk:
                    model.train()
    check_rows(epochs - 1)   # one host read per fit: the epochs after the last evaluation, or a fit shorter than 11 epochs
    return best, opt
