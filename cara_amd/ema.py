"""Exponential moving average of the trainable tensors of a fine-tuning run as ONE HIP launch per optimiser step.

``ParamEma`` keeps a shadow copy of every parameter it is given and moves it towards the parameter by ``1 - decay`` at each
``update()`` (``cara_ema_update``, include/cara_hip.h: torch.lerp's two-branch arithmetic in fp32, pointers and sizes of up to 32
tensors by value in the kernel arguments, as ``cara_adamw_step`` does).  The model is then scored on the shadows
(``CaraEngine.evaluate(..., weights=ema)``: the same forward reads them in place of the CP tensors and the head -- no copy) and the
checkpoint written from them (``recipe.save_checkpoint(..., weights=ema)``).  Not in the reference's loop
(``image_classification/vit_cp.py:45-66`` scores the raw iterate); off unless asked for.  Device tensors only: there is no CPU path.

Decay schedule (this project's definition): ``decay_at(t) = decay``, and with ``warmup`` ``min(decay, (1 + t) / (10 + t))``, ``t``
the number of updates already made; the kernel gets ``float32(1 - decay_at(t))``.

Skipped steps: under ``precision = "fp16"`` a step whose gradients overflowed leaves the parameters as they are, and the average is
updated all the same -- it keeps approaching the unchanged parameters, and the update count moves on.  No skip word is read.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

from . import _lib as L
from ._lib import CaraError


def decay_at(decay: float, warmup: bool, t: int) -> float:
    """decay used by update number ``t`` (0-based: ``t`` updates were made before it)"""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def weight_at(decay: float, warmup: bool, t: int) -> float:
    """``float32(1 - decay_at(t))``: the weight the kernel is given, as a Python float"""
    return C.c_float(1.0 - decay_at(decay, warmup, t)).value


class ParamEma:
    def __init__(self, params, decay: float = 0.9998, warmup: bool = False, capturable: bool = False):
        params = list(params)
        if not params:
            raise CaraError("ParamEma needs at least one parameter")
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 <= decay <= 1.0):   # (a NaN fails the comparison)
            raise CaraError(f"ParamEma: decay must be a number in [0, 1], not {decay!r}")
        self._check(params)
        self.params = params
        self.decay, self.warmup = float(decay), bool(warmup)
        with torch.no_grad():
            self.tensors = [p.detach().clone(memory_format=torch.contiguous_format) for p in params]
        self.num_updates = 0
        # capturable = True: the weight lives in a device float, so that a launch captured into a hipGraph follows the warm-up.
        # update() then only enqueues; advance() -- once before every step / graph replay, outside the captured region, as
        # AdamW.advance -- moves the count on and fills the float (a fill launch: stream-ordered, its value in its arguments).
        self.capturable = bool(capturable)
        self._w_dev = None
        self._plan = None    # (parameter addresses, [(ntensors, ema[], param[], n[])]) of the last update

    @staticmethod
    def _check(params):
        dev = params[0].device if torch.is_tensor(params[0]) else None
        for p in params:
            if not torch.is_tensor(p) or not p.is_cuda or p.dtype != torch.float32 or p.is_sparse:
                raise CaraError("cara_amd.ema.ParamEma averages dense fp32 tensors on the GPU (no CPU path)")
            if not p.is_contiguous():
                raise CaraError("cara_amd.ema.ParamEma needs contiguous tensors")
            if p.device != dev:
                raise CaraError("cara_amd.ema.ParamEma: all tensors on one device")
            if p.numel() == 0:
                raise CaraError("cara_amd.ema.ParamEma: empty tensor")

    def decay_at(self, t: int) -> float:
        return decay_at(self.decay, self.warmup, t)

    def weight_at(self, t: int) -> float:
        return weight_at(self.decay, self.warmup, t)

    def advance(self):
        """capturable mode: next update -- its weight -> device, count + 1 (call before update() / graph.replay())"""
        if not self.capturable:
            raise CaraError("advance() belongs to ParamEma(capturable=True)")
        dev = self.tensors[0].device
        if self._w_dev is None or self._w_dev.device != dev:
            self._w_dev = torch.zeros(1, device=dev)
        self._w_dev.fill_(self.weight_at(self.num_updates))
        self.num_updates += 1

    @torch.no_grad()
    def update(self):
        """shadow <- shadow + (1 - decay)(parameter - shadow) for every tensor: one launch per 32 tensors, nothing read on the host"""
        if self.capturable:
            if self._w_dev is None:
                raise CaraError("ParamEma(capturable=True): call advance() before update()")
            weight, wdev = 0.0, self._w_dev.data_ptr()
        else:
            if torch.cuda.is_current_stream_capturing():
                raise CaraError("a captured update needs ParamEma(capturable=True): the weight would be frozen into the graph")
            weight, wdev = self.weight_at(self.num_updates), None
            self.num_updates += 1
        dev = self.tensors[0].device
        # the three host arrays of every launch are kept while no tensor moves (the checks and the arrays are most of a call's host
        # time: 14 tensors); a parameter whose storage was replaced is checked again
        key = tuple(p.data_ptr() for p in self.params)
        if self._plan is None or self._plan[0] != key:
            self._check(self.params)
            pairs = list(zip(self.tensors, self.params))
            if any(p.shape != s.shape or p.device != dev for s, p in pairs):
                raise CaraError("ParamEma: a parameter changed its shape or device since the average was made")
            launches = []
            for i in range(0, len(pairs), L.ADAMW_MAX_TENSORS):
                part = pairs[i:i + L.ADAMW_MAX_TENSORS]
                k = len(part)
                launches.append((k, (C.c_void_p * k)(*[s.data_ptr() for s, _ in part]), (C.c_void_p * k)(*[q.data_ptr() for _, q in part]),
                                 (C.c_size_t * k)(*[s.numel() for s, _ in part])))
            self._plan = (key, launches)
        fn = L.lib().cara_ema_update
        with torch.cuda.device(dev):
            st = L.stream(dev)
            for k, e, p, n in self._plan[1]:
                L.check(fn(k, e, p, n, weight, wdev, st), "cara_ema_update")

    @torch.no_grad()
    def copy_to(self, params=None):
        """shadows -> ``params`` (default: the averaged parameters themselves), in place"""
        params = self.params if params is None else list(params)
        if len(params) != len(self.tensors) or any(p.shape != s.shape for p, s in zip(params, self.tensors)):
            raise CaraError("copy_to: the targets must match the averaged tensors one by one")
        for p, s in zip(params, self.tensors):
            p.copy_(s)

    @contextlib.contextmanager
    def swapped_in(self):
        """``with ema.swapped_in():`` -- inside the block every averaged parameter's ``.data`` IS its shadow (no copy), restored
        afterwards: how a forward that reads the module's own parameters is run on the average (evaluation, not the hot path)"""
        saved = [p.data for p in self.params]
        try:
            for p, s in zip(self.params, self.tensors):
                p.data = s
            yield self
        finally:
            for p, d in zip(self.params, saved):
                p.data = d

    def state_dict(self) -> dict:
        return {"shadow": [s.detach().clone() for s in self.tensors], "num_updates": int(self.num_updates), "decay": self.decay,
                "warmup": self.warmup}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        shadow = list(sd["shadow"])
        if len(shadow) != len(self.tensors) or any(tuple(a.shape) != tuple(b.shape) for a, b in zip(shadow, self.tensors)):
            raise CaraError("ParamEma.load_state_dict: the saved shadows do not match the averaged tensors")
        for s, src in zip(self.tensors, shadow):
            s.copy_(src)     # (in place: a captured launch and an engine that was handed the shadows keep their addresses)
        self.num_updates, self.decay, self.warmup = int(sd["num_updates"]), float(sd["decay"]), bool(sd["warmup"])
