"""``Feed``: one step's index vector and the tables that ride with it on the resident training path.

The order ``rows, boxes, mix, aug, keep, ra`` is the contract between ``data.ResidentSplit.train_rows`` (which yields it),
``recipe.fit`` / ``recipe.GraphedTrainStep`` (which carry it) and ``CaraEngine.train_step_resident`` (whose keyword arguments
the table names are).  Everything that depends on that order asks this module."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from ._lib import CaraError

# per table: its column count (None: keep's K is free, 1 <= K <= the patches P of the grid) and what the engine says to anything
# that is not such a device int32 [batch, columns] tensor
TABLES = {
    "boxes": (5, "boxes must be a contiguous int32 [batch, 5] tensor (x0, y0, w, h, flip) on the model's device"),
    "mix": (8, "mix must be a contiguous int32 [batch, 8] tensor (partner, cx0, cy0, cw, ch, blend bits, target bits, 0) on the "
               "model's device"),
    "aug": (16, "aug must be a contiguous int32 [batch, 16] tensor (op0, f0, op1, f1, op2, f2, ex0, ey0, ew, eh, emode, eseed, 0, 0, 0, "
                "0) on the model's device"),
    "keep": (None, "keep must be a contiguous int32 [batch, K] tensor of patch indices on the model's device, 1 <= K <= {P} "
                   "(data.PatchDropout.draw, data.check_keep)"),
    "ra": (16, "ra must be a contiguous int32 [batch, 16] tensor (op0, arg0, op1, arg1, op2, arg2, m00, m01, m02, m10, m11, m12, fill, 0, "
               "0, 0) on the model's device"),
}


class Feed(NamedTuple):
    """``rows`` (device int64 [batch]) and, each None or a device int32 [batch, columns] table: ``boxes`` (crop and flip),
    ``mix`` (Mixup / CutMix), ``aug`` (colour jitter / erase), ``keep`` (patch dropout), ``ra`` (RandAugment)"""
    rows: Optional[torch.Tensor]
    boxes: Optional[torch.Tensor] = None
    mix: Optional[torch.Tensor] = None
    aug: Optional[torch.Tensor] = None
    keep: Optional[torch.Tensor] = None
    ra: Optional[torch.Tensor] = None

    @classmethod
    def of(cls, item) -> "Feed":
        """a bare index vector, or a tuple / list of it and up to five tables in field order (the ones left out are None)"""
        if not isinstance(item, (tuple, list)):
            return cls(item)
        if not 1 <= len(item) <= len(cls._fields):
            raise CaraError(f"a feed item is rows or (rows, {', '.join(cls._fields[1:])}) cut anywhere behind rows, not {len(item)} entries")
        return cls(*item)

    def item(self):
        """what ``train_rows`` yields: the tuple cut behind its last table, the bare ``rows`` when there is none"""
        last = max(i for i, t in enumerate(self) if i == 0 or t is not None)
        return self.rows if last == 0 else tuple(self[:last + 1])

    def tables(self) -> dict:
        """{name: table} of the tables present: the keyword arguments of ``train_step_resident``"""
        return {n: t for n, t in zip(self._fields[1:], self[1:]) if t is not None}

    def static(self) -> tuple:
        """``rows`` and the tables present, in field order: what a captured step copies before a replay"""
        return (self.rows, *self.tables().values())
