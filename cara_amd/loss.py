"""The sigmoid losses of the fused train step (``cara_sigmoid_loss``, include/cara_hip.h): small value objects handed to
``CaraEngine.train_step(..., loss=)``, ``train_step_resident``, ``recipe.GraphedTrainStep`` and ``recipe.fit``.  They hold settings
only; the arithmetic is the kernel's.  Every value the C entry refuses is refused here first, on the host, before a step launches
anything.  ``loss=None`` is the softmax cross-entropy the step always ran.  ``Distill`` is the value object of ``distill=``: knowledge
distillation on that softmax cross-entropy (``cara_distill_loss``) against a teacher whose forward the step runs itself."""
from __future__ import annotations

import math

import torch

from ._lib import CaraError


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise CaraError(f"{name} must be a number, not {v!r}")
    return float(v)


def _flag(name, v):
    if not isinstance(v, (bool, int)) or v not in (0, 1):
        raise CaraError(f"{name} must be True or False, not {v!r}")
    return bool(v)


class SigmoidLoss:
    """what the step reads of either loss: the head arguments of ``cara_sigmoid_loss`` behind ``smoothing``"""
    target_threshold = None
    gamma = 0.0
    alpha = None
    pos_weight = None
    sum_classes = False

    def c_args(self):
        """(target_threshold, gamma, alpha) as the C entry takes them: a negative number for None"""
        return (-1.0 if self.target_threshold is None else self.target_threshold, self.gamma, -1.0 if self.alpha is None else self.alpha)

    def key(self):
        """what changes the launches of a captured step: the settings and the ADDRESS of the weight vector (its contents are re-read)"""
        return (type(self).__name__, self.target_threshold, self.gamma, self.alpha, id(self.pos_weight) if self.pos_weight is not None else None,
                self.sum_classes)

    def check_pos_weight(self, ncls, dev, seen):
        """``pos_weight`` of a step, refused here -- before anything is launched -- unless it is None or a contiguous fp32 [ncls] tensor
        on ``dev`` with finite values >= 0.  The values cost a host read: one per tensor, remembered in ``seen`` by (address,
        version), so a steady step reads nothing."""
        t = self.pos_weight
        if t is None:
            return
        if t.dtype != torch.float32 or t.ndim != 1 or t.shape[0] != ncls or t.device != dev or not t.is_contiguous():
            raise CaraError(f"pos_weight must be a contiguous fp32 [{ncls}] tensor -- one entry per class of the head -- on the model's device")
        key = (t.data_ptr(), t._version)
        if seen.get("pos_weight") != key:
            if bool((~torch.isfinite(t) | (t < 0)).any()):
                raise CaraError("pos_weight must be finite and >= 0 in every class")
            seen["pos_weight"] = key


class BCE(SigmoidLoss):
    """Binary cross-entropy on the step's soft target ``q`` (both Mixup / CutMix labels, label smoothing): per class
    ``torch.nn.functional.binary_cross_entropy_with_logits(z, q, pos_weight=pos_weight)``, averaged over the batch and over the classes
    -- or summed over the classes with ``sum_classes`` -- which is timm's ``BinaryCrossEntropy``.
    ``target_threshold`` (None, or a number in [0, 1)): the target becomes ``q > target_threshold`` (timm's ``--bce-target-thresh``).
    ``pos_weight`` (None, or an fp32 [classes] tensor, finite and >= 0): the weight of each class's positive term.  The step reads it
    on the model's device; ``recipe.fit`` moves a host tensor there once."""

    def __init__(self, target_threshold=None, pos_weight=None, sum_classes=False):
        if target_threshold is not None:
            target_threshold = _number("target_threshold", target_threshold)
            if not (0.0 <= target_threshold < 1.0):                       # (a NaN fails the comparison)
                raise CaraError(f"target_threshold must be None or a number in [0, 1), not {target_threshold!r}")
        if pos_weight is not None and not torch.is_tensor(pos_weight):
            raise CaraError(f"pos_weight must be None or an fp32 [classes] tensor, not {type(pos_weight).__name__}")
        self.target_threshold, self.pos_weight, self.sum_classes = target_threshold, pos_weight, _flag("sum_classes", sum_classes)

    def __repr__(self):
        return f"BCE(target_threshold={self.target_threshold!r}, pos_weight={'None' if self.pos_weight is None else '...'}, sum_classes={self.sum_classes})"


class Focal(SigmoidLoss):
    """The sigmoid focal loss (Lin et al.; torchvision's ``sigmoid_focal_loss``) on the step's soft target ``q``:
    ``alpha_t (1 - p_t) ** gamma * ce`` per class, with ``1 - p_t = q (1 - p) + (1 - q) p`` and ``alpha_t = alpha q + (1 - alpha)(1 - q)``,
    averaged over the batch and summed over the classes (``sum_classes=True``, the default: torchvision's ``reduction="sum"`` divided
    by the batch) or averaged over them too.  ``gamma``: 0, or a finite number >= 1 -- the backward holds ``(1 - p_t) ** (gamma - 1)``,
    which a gamma in (0, 1) makes infinite at a saturated logit.  ``alpha``: None (no class balance), or a number in [0, 1].
    ``Focal(gamma=0, alpha=None)`` is ``BCE()``."""

    def __init__(self, gamma=2.0, alpha=0.25, sum_classes=True):
        gamma = _number("gamma", gamma)
        if not (gamma == 0.0 or (1.0 <= gamma < math.inf)):               # (a NaN fails both)
            raise CaraError(f"gamma must be 0 or a finite number >= 1, not {gamma!r}")
        if alpha is not None:
            alpha = _number("alpha", alpha)
            if not (0.0 <= alpha <= 1.0):
                raise CaraError(f"alpha must be None or a number in [0, 1], not {alpha!r}")
        self.gamma, self.alpha, self.sum_classes = gamma, alpha, _flag("sum_classes", sum_classes)

    def __repr__(self):
        return f"Focal(gamma={self.gamma!r}, alpha={self.alpha!r}, sum_classes={self.sum_classes})"


class Distill:
    """Knowledge distillation in the fused step (``cara_distill_loss``): handed to ``train_step(..., distill=)``,
    ``train_step_resident``, ``recipe.GraphedTrainStep`` and ``recipe.fit``.  On the step's soft target ``q`` and with the teacher's
    logits ``t`` of the same input:
    soft (``hard=False``): ``(1 - alpha) * cross_entropy(z, q) + alpha * T**2 * kl_div(log_softmax(z / T), softmax(t / T),
    reduction="batchmean")`` (Hinton et al.);  hard (``hard=True``, DeiT): the cross-entropy on ``(1 - alpha) q + alpha
    onehot(argmax t)``, ties to the lowest class; ``temperature`` is then not read.
    ``teacher`` is one of
    * a ``ParamEma`` of the training engine (``CaraEngine.make_ema``) -- the mean teacher: the step's own forward on the average;
    * another ``cara()`` model on the same device with the same image size and class count -- its rank, ``cp_length``, depth, dim and
      precision are its own: the pass runs through its engine, in eval semantics whatever its ``training`` flag says;
    * a device fp32 [batch, classes] tensor of recorded logits (contiguous, on the step's device): no teacher pass;
    * the string ``"ema"``, for ``recipe.fit(ema_decay=...)`` alone, which puts the average it trains with in its place.
    ``alpha`` in [0, 1], ``temperature`` finite and > 0 (and not below 2.94e-39, where the fp32 1 / T overflows).  The teacher gets no
    gradient and its pass runs before the student's."""

    def __init__(self, teacher, alpha=0.5, temperature=1.0, hard=False):
        alpha, temperature = _number("alpha", alpha), _number("temperature", temperature)
        if not (0.0 <= alpha <= 1.0):                                        # (a NaN fails the comparison)
            raise CaraError(f"alpha must be a number in [0, 1], not {alpha!r}")
        hard = _flag("hard", hard)
        # (the kernel multiplies by the fp32 1 / T: a T whose reciprocal overflows there would make every tempered logit inf or NaN)
        t32 = torch.tensor(temperature, dtype=torch.float32)    # (what the entry gets)
        if not hard and not (0.0 < temperature < math.inf and bool(torch.isfinite(t32)) and bool(torch.isfinite(1.0 / t32))):
            raise CaraError(f"temperature must be a number > 0 that is finite in fp32 and whose fp32 reciprocal is finite, not {temperature!r}")
        from .ema import ParamEma
        if not (torch.is_tensor(teacher) or isinstance(teacher, ParamEma) or getattr(teacher, "_cara_engine", None) is not None
                or (isinstance(teacher, str) and teacher == "ema")):
            raise CaraError("teacher must be a ParamEma of the engine, a cara() model, an fp32 [batch, classes] tensor of logits or, "
                            f"for recipe.fit, the string 'ema', not {teacher!r}")
        self.teacher, self.alpha, self.temperature, self.hard = teacher, alpha, temperature, hard

    def kind(self):
        """"tensor", "ema", "model" or "fit" (the unresolved string)"""
        from .ema import ParamEma
        t = self.teacher
        return "tensor" if torch.is_tensor(t) else "ema" if isinstance(t, ParamEma) else "fit" if isinstance(t, str) else "model"

    def c_args(self):
        """(alpha, temperature, hard) as the C entry takes them"""
        return self.alpha, self.temperature, int(self.hard)

    def __repr__(self):
        return f"Distill({self.kind()} teacher, alpha={self.alpha!r}, temperature={self.temperature!r}, hard={self.hard})"


def check_distill(distill, loss=None, class_weight=None, logit_bias=None):
    """``distill=`` of a step: None or a ``Distill``; not beside ``loss=`` (the sigmoid losses) or ``class_weight`` / ``logit_bias``"""
    if distill is None:
        return None
    if not isinstance(distill, Distill):
        raise CaraError(f"distill must be None or a cara_amd.loss.Distill, not {distill!r}")
    if loss is not None or class_weight is not None or logit_bias is not None:
        raise CaraError("distill= cannot run beside loss=, class_weight or logit_bias: the distilled loss is the softmax cross-entropy's")
    return distill


def check_loss(loss, class_weight=None, logit_bias=None):
    """``loss=`` of a step: None, a ``BCE`` or a ``Focal``; not beside the softmax loss's ``class_weight`` / ``logit_bias``"""
    if loss is None:
        return None
    if not isinstance(loss, SigmoidLoss) or type(loss) is SigmoidLoss:
        raise CaraError(f"loss must be None, a cara_amd.loss.BCE or a cara_amd.loss.Focal, not {loss!r}")
    if class_weight is not None or logit_bias is not None:
        raise CaraError("loss= cannot run beside class_weight / logit_bias: those belong to the softmax cross-entropy (a BCE takes pos_weight)")
    return loss
