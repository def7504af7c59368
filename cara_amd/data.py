"""VTAB-1k input pipeline, MI355X-first.

The reference (``/root/reference/image_classification/vtab.py:36-107``) decodes every image again in
every epoch with 4 DataLoader workers: ``ImageFilelist`` over ``impath label`` lines, ``Resize((224,224),
bicubic)`` + ``ToTensor`` + ImageNet ``Normalize``, ``DataLoader(batch 64, shuffle, drop_last)`` for
training and ``DataLoader(batch 256)`` for evaluation.  At 5 000+ images/s per GPU that feed is the
bottleneck, and a VTAB-1k task is 1 000 training images: 150 MB as resized uint8 pixels.  So the whole split is
decoded ONCE (same arithmetic: PIL bicubic resize of the RGB image) into one device-resident uint8 tensor, and an epoch
is an index permutation plus ``index_select`` and the /255 + per-channel normalise of the drawn batch on the GPU.  Under
data parallelism every rank holds the split and takes the rank-strided part of the same epoch-seeded
permutation (``dist.epoch_shard``), which is ``drop_last`` per rank like the reference loader.

No torchvision here (not installed): the three transforms are restated on PIL + torch and checked
against an independent numpy computation in tests/test_data.py.
"""
from __future__ import annotations

import math
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dist as D
from .feed import Feed

# vtab.py:9-31
DATASET_NAMES = ("cifar", "caltech101", "dtd", "oxford_flowers102", "oxford_iiit_pet", "svhn", "sun397",
                 "patch_camelyon", "eurosat", "resisc45", "diabetic_retinopathy", "clevr_count", "clevr_dist",
                 "dmlab", "kitti", "dsprites_loc", "dsprites_ori", "smallnorb_azi", "smallnorb_ele")
CLASSES_NUM = (100, 102, 47, 102, 37, 10, 397, 2, 10, 45, 5, 8, 6, 6, 4, 16, 16, 18, 9)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def get_classes_num(dataset_name: str) -> int:
    """vtab.py:32-34 (KeyError on an unknown name, like the reference's dict lookup)."""
    return dict(zip(DATASET_NAMES, CLASSES_NUM))[dataset_name]


def read_filelist(flist: str) -> List[Tuple[str, int]]:
    """vtab.py:40-50: one ``impath label`` pair per line, split on whitespace (a line with any other
    number of fields raises ValueError, as the reference's tuple unpacking does)."""
    out = []
    with open(flist, "r") as fh:
        for line in fh.readlines():
            impath, imlabel = line.strip().split()
            out.append((impath, int(imlabel)))
    return out


def decode_image_u8(path: str, size: int = 224) -> torch.Tensor:
    """vtab.py:36-37 + the Resize of :91: RGB -> bicubic resize to size x size (PIL semantics, as torchvision applies
    to PIL images).  uint8 [3,size,size]."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB").resize((size, size), Image.BICUBIC)
        a = np.asarray(im, dtype=np.uint8)
    return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous()


def normalize_u8(x: torch.Tensor) -> torch.Tensor:
    """ToTensor + Normalize of vtab.py:92-94 on uint8 [..., 3, H, W] (any device): /255, (x - mean) / std, fp32.
    The same fp32 operations in the same order on the CPU and on the GPU (equal to within one ulp: the GPU's fp32
    division is not correctly rounded in every case)."""
    mean = torch.tensor(IMAGENET_MEAN, device=x.device).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=x.device).view(3, 1, 1)
    return x.to(torch.float32).div_(255.0).sub_(mean).div_(std)


def decode_image(path: str, size: int = 224) -> torch.Tensor:
    """The whole transform of vtab.py:91-94 for one file: fp32 [3,size,size]."""
    return normalize_u8(decode_image_u8(path, size))


class RandomResizedCropFlip:
    """Crop boxes for the augmented resident feed: the published definition of torchvision's ``RandomResizedCrop.get_params``
    plus a coin flip, restated (torchvision is not installed).  Per sample, up to ten tries of an area ``Hs * Ws * U(scale)``
    and an aspect ratio ``exp(U(log ratio))``, ``w = round(sqrt(area * r))``, ``h = round(sqrt(area / r))``; the first try with
    ``0 < w <= Ws`` and ``0 < h <= Hs`` is taken at a uniform integer offset.  If none fits: the centre crop of the whole image
    clamped to the ratio bounds.  ``size`` is the side the crop is resized to (the model's input); the boxes do not depend on it
    -- the kernel that reads them resamples to the model's own size.  No antialiasing; Mixup / CutMix is ``MixupCutmix`` and
    colour jitter / Random Erasing ``ColorJitterErase`` below."""

    TRIES = 10

    def __init__(self, size: int, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip: float = 0.5):
        if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]) or not (0.0 <= flip <= 1.0) or int(size) <= 0:
            raise ValueError("RandomResizedCropFlip: size > 0, 0 < scale[0] <= scale[1], 0 < ratio[0] <= ratio[1], flip in [0, 1]")
        self.size, self.scale, self.ratio, self.flip = int(size), (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1])), float(flip)

    def draw(self, Hs: int, Ws: int, n: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """int32 [n, 5] = (x0, y0, w, h, flip) in the pixels of an ``Hs`` x ``Ws`` source, on the host.  A fixed number of
        variates per sample (ten tries of four, one flip), so sample ``i`` of a table does not depend on ``n``."""
        T = self.TRIES
        u = torch.rand(n, T, 4, generator=generator, dtype=torch.float64)
        coin = torch.rand(n, generator=generator, dtype=torch.float64)
        area = Hs * Ws * (self.scale[0] + (self.scale[1] - self.scale[0]) * u[..., 0])
        lo, hi = math.log(self.ratio[0]), math.log(self.ratio[1])
        r = torch.exp(lo + (hi - lo) * u[..., 1])
        w = torch.round(torch.sqrt(area * r)).to(torch.int64)
        h = torch.round(torch.sqrt(area / r)).to(torch.int64)
        ok = (w > 0) & (w <= Ws) & (h > 0) & (h <= Hs)
        first = torch.where(ok.any(1), ok.to(torch.int64).argmax(1), torch.zeros(n, dtype=torch.int64))
        pick = lambda t: t.gather(1, first[:, None])[:, 0]   # noqa: E731
        w, h = pick(w), pick(h)
        x0 = torch.floor(pick(u[..., 2]) * (Ws - w + 1).clamp(min=1)).to(torch.int64)
        y0 = torch.floor(pick(u[..., 3]) * (Hs - h + 1).clamp(min=1)).to(torch.int64)
        # the fallback: whole image, centre crop clamped to the ratio bounds
        in_ratio = Ws / Hs
        if in_ratio < self.ratio[0]:
            fw, fh = Ws, int(round(Ws / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            fw, fh = int(round(Hs * self.ratio[1])), Hs
        else:
            fw, fh = Ws, Hs
        fw, fh = min(max(fw, 1), Ws), min(max(fh, 1), Hs)
        none = ~ok.any(1)
        w, h = torch.where(none, torch.full_like(w, fw), w), torch.where(none, torch.full_like(h, fh), h)
        x0 = torch.where(none, torch.full_like(x0, (Ws - fw) // 2), x0).clamp_(min=0)
        y0 = torch.where(none, torch.full_like(y0, (Hs - fh) // 2), y0).clamp_(min=0)
        x0, y0 = torch.minimum(x0, Ws - w), torch.minimum(y0, Hs - h)
        return torch.stack([x0, y0, w, h, (coin < self.flip).to(torch.int64)], 1).to(torch.int32).contiguous()


def check_boxes(boxes: torch.Tensor, Hs: int, Ws: int) -> None:
    """ValueError unless ``boxes`` is an int32 [..., 5] table whose every box lies inside an ``Hs`` x ``Ws`` image"""
    if not torch.is_tensor(boxes) or boxes.dtype != torch.int32 or boxes.ndim < 1 or boxes.shape[-1] != 5:
        raise ValueError("boxes must be an int32 [..., 5] tensor (x0, y0, w, h, flip)")
    b = boxes.reshape(-1, 5).to(torch.int64)
    x0, y0, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    bad = (w < 1) | (h < 1) | (x0 < 0) | (y0 < 0) | (x0 + w > Ws) | (y0 + h > Hs)
    if bool(bad.any()):
        raise ValueError(f"{int(bad.sum())} crop box(es) outside the {Hs} x {Ws} source, the first: {boxes.reshape(-1, 5)[int(bad.to(torch.int64).argmax())].tolist()}")


EVAL_MAX_VIEWS = 16   # CARA_EVAL_MAX_VIEWS of include/cara_hip.h: the views cara_eval_combine_views takes per sample


class EvalViews:
    """The views every test image is scored through (``CaraEngine.evaluate(views=)``): a host int32 [V, 5] table of
    ``(x0, y0, w, h, flip)`` boxes in source pixels, the same for every sample, made for a source size by ``table(Hs, Ws)``.
    ``size`` is the side every view is resized to, the model's input.  The resampling is the crop kernel's
    (``cara_im2col_patches_u8_rows_crop``, ``resized_crop_reference``): bilinear with half-pixel centres and NO antialias filter --
    a strong downscale aliases where PIL's or torchvision's antialiased resize would not -- and a box of side ``size`` is the
    source's exact bytes.
    ``resize(size)``: the whole image (the identity on a split of ``size``).  ``center(size, crop_pct)``: the centred square of
    side ``round(min(Hs, Ws) * crop_pct)``, timm's resize / centre-crop protocol when the split was decoded at ``size / crop_pct``
    (256 -> ``(16, 16, 224, 224, 0)``).  ``flip=True`` on either adds the mirrored view behind it.  ``five_crop``: the four corners
    (top-left, top-right, bottom-left, bottom-right) and the centre at that side; ``ten_crop``: those and then their mirror images.
    ``EvalViews(table)``: a hand-made table."""

    def __init__(self, table, size: Optional[int] = None):
        t = torch.as_tensor(table)
        if t.dtype not in (torch.int32, torch.int64) or t.ndim != 2 or t.shape[1] != 5 or t.shape[0] < 1:
            raise ValueError("EvalViews takes an integer [V, 5] table (x0, y0, w, h, flip), V >= 1")
        self.size = None if size is None else int(size)
        self._fixed, self._make, self.V = t.to(torch.int32).cpu().contiguous(), None, int(t.shape[0])

    @classmethod
    def _of(cls, size, V, make) -> "EvalViews":
        if int(size) <= 0:
            raise ValueError("EvalViews: size > 0")
        self = cls.__new__(cls)
        self.size, self._fixed, self._make, self.V = int(size), None, make, V
        return self

    @staticmethod
    def _side(Hs, Ws, crop_pct):
        if not 0.0 < float(crop_pct) <= 1.0:
            raise ValueError("EvalViews: 0 < crop_pct <= 1")
        return max(1, int(math.floor(min(Hs, Ws) * float(crop_pct) + 0.5)))

    @staticmethod
    def _with_flips(boxes, flip):
        return boxes + [(x0, y0, w, h, 1) for x0, y0, w, h, _ in boxes] if flip else boxes

    @classmethod
    def resize(cls, size: int, flip: bool = False) -> "EvalViews":
        return cls._of(size, 2 if flip else 1, lambda Hs, Ws: cls._with_flips([(0, 0, Ws, Hs, 0)], flip))

    @classmethod
    def center(cls, size: int, crop_pct: float = 0.875, flip: bool = False) -> "EvalViews":
        def make(Hs, Ws):
            s = cls._side(Hs, Ws, crop_pct)
            return cls._with_flips([((Ws - s) // 2, (Hs - s) // 2, s, s, 0)], flip)
        cls._side(1, 1, crop_pct)
        return cls._of(size, 2 if flip else 1, make)

    @classmethod
    def five_crop(cls, size: int, crop_pct: float = 0.875, _flip: bool = False) -> "EvalViews":
        def make(Hs, Ws):
            s = cls._side(Hs, Ws, crop_pct)
            return cls._with_flips([(0, 0, s, s, 0), (Ws - s, 0, s, s, 0), (0, Hs - s, s, s, 0), (Ws - s, Hs - s, s, s, 0),
                                    ((Ws - s) // 2, (Hs - s) // 2, s, s, 0)], _flip)
        cls._side(1, 1, crop_pct)
        return cls._of(size, 10 if _flip else 5, make)

    @classmethod
    def ten_crop(cls, size: int, crop_pct: float = 0.875) -> "EvalViews":
        return cls.five_crop(size, crop_pct, _flip=True)

    def table(self, Hs: int, Ws: int) -> torch.Tensor:
        """host int32 [V, 5] for an ``Hs`` x ``Ws`` source; ValueError for a box outside it or more than ``EVAL_MAX_VIEWS`` views"""
        t = self._fixed if self._make is None else torch.tensor(self._make(int(Hs), int(Ws)), dtype=torch.int32)
        check_views(t, Hs, Ws)
        return t.contiguous()


def check_views(table: torch.Tensor, Hs: int, Ws: int) -> None:
    """ValueError unless ``table`` is an int32 [V, 5] table of 1 <= V <= ``EVAL_MAX_VIEWS`` boxes inside an ``Hs`` x ``Ws`` image"""
    if not torch.is_tensor(table) or table.dtype != torch.int32 or table.ndim != 2 or table.shape[1] != 5 or table.shape[0] < 1:
        raise ValueError("a view table is an int32 [V, 5] tensor (x0, y0, w, h, flip), V >= 1")
    if table.shape[0] > EVAL_MAX_VIEWS:
        raise ValueError(f"{table.shape[0]} views: cara_eval_combine_views takes at most {EVAL_MAX_VIEWS} per sample")
    check_boxes(table, Hs, Ws)


def resized_crop_reference(pixels_u8: torch.Tensor, rows, boxes, size, dtype=torch.float64) -> torch.Tensor:
    """What ``cara_im2col_patches_u8_rows_crop`` samples, before normalisation, in torch ops on the CPU: [B,C,Hi,Wi] of
    ``dtype`` with ``size`` = Hi or (Hi, Wi).  Output pixel (oy, ox) of sample b: ``ox' = flip ? Wi-1-ox : ox``,
    ``sx = max((ox' + 0.5) * (w / Wi) - 0.5, 0)``, ``ix0 = min(int(sx), w-1)``, ``ix1 = min(ix0+1, w-1)``, ``fx = sx - ix0``, the
    same for y, ``v = (1-fy) ((1-fx) u00 + fx u01) + fy ((1-fx) u10 + fx u11)`` on the bytes at (y0+iy*, x0+ix*) of image
    ``rows[b]``: bilinear ``interpolate(align_corners=False, antialias=False)`` of the box, then a horizontal flip."""
    Hi, Wi = (size, size) if isinstance(size, int) else size
    px = pixels_u8.cpu()
    rows = torch.as_tensor(rows).cpu().tolist()
    boxes = torch.as_tensor(boxes).cpu().tolist()
    out = torch.empty(len(rows), px.shape[1], Hi, Wi, dtype=dtype)

    def axis(n_out, n_box, flip):
        o = torch.arange(n_out, dtype=dtype)
        if flip:
            o = n_out - 1 - o
        s = ((o + 0.5) * (torch.tensor(n_box, dtype=dtype) / n_out) - 0.5).clamp_(min=0)
        i0 = s.to(torch.int64).clamp_(max=n_box - 1)
        return i0, (i0 + 1).clamp_(max=n_box - 1), s - i0.to(dtype)
    for b, (r, (x0, y0, w, h, flip)) in enumerate(zip(rows, boxes)):
        src = px[r, :, y0:y0 + h, x0:x0 + w].to(dtype)
        iy0, iy1, fy = axis(Hi, h, False)
        ix0, ix1, fx = axis(Wi, w, flip != 0)
        fy = fy[:, None]
        top = (1 - fx) * src[:, iy0][:, :, ix0] + fx * src[:, iy0][:, :, ix1]
        bot = (1 - fx) * src[:, iy1][:, :, ix0] + fx * src[:, iy1][:, :, ix1]
        out[b] = (1 - fy) * top + fy * bot
    return out


def box_seed(seed: int, epoch: int, rank: int, stream: int = 0x27D4EB2F) -> int:
    """32-bit seed (torch's host generator keeps no more) of the generator that draws the crop boxes of one rank's epoch: each
    of seed, epoch and rank enters through an odd multiplier, so changing one of them alone always changes the value, and a
    bijective finaliser (murmur3's) spreads neighbouring values.  ``stream``: the constant of this random stream (``mix_seed``
    has another)"""
    x = (int(seed) * 0x9E3779B1 + int(epoch) * 0x85EBCA77 + int(rank) * 0xC2B2AE3D + int(stream)) & 0xffffffff
    x = ((x ^ (x >> 16)) * 0x85EBCA6B) & 0xffffffff
    x = ((x ^ (x >> 13)) * 0xC2B2AE35) & 0xffffffff
    return x ^ (x >> 16)


def mix_seed(seed: int, epoch: int, rank: int) -> int:
    """``box_seed`` of the stream that draws the Mixup / CutMix tables: another constant, so the same (seed, epoch, rank) gives a
    generator that is not the boxes'"""
    return box_seed(seed, epoch, rank, stream=0x165667B1)


def _f32_bits(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).contiguous().view(torch.int32)


def _bits_f32(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.int32).contiguous().view(torch.float32)


def identity_mix(B: int, steps: Optional[int] = None) -> torch.Tensor:
    """int32 [B, 8] (or [steps, B, 8]) table that mixes nothing: partner = the sample itself, no rectangle, m = t = 0"""
    t = torch.zeros(B, 8, dtype=torch.int32)
    t[:, 0] = torch.arange(B, dtype=torch.int32)
    return t if steps is None else t.expand(steps, B, 8).contiguous()


class MixupCutmix:
    """Mix tables for the resident feed: the published definition of timm's ``Mixup`` in batch mode (``mode="batch"``,
    ``correct_lam=True``), restated (timm is not installed).  Per batch: with probability ``1 - prob`` the identity table.
    Otherwise CutMix is chosen if ``rand < switch_prob`` and both alphas are positive (with one positive alpha: that method),
    ``lam ~ Beta(alpha, alpha)`` of the chosen method, and every sample ``i`` is mixed with ``partner = B - 1 - i`` (timm's
    ``x.flip(0)``).
      Mixup:  ``x_i (1 - m) + x_partner m`` with ``m = t = 1 - lam``, no rectangle.
      CutMix: ``r = sqrt(1 - lam)``, ``ch = int(Hi r)``, ``cw = int(Wi r)``, centre ``(cy, cx)`` a uniform integer in [0, Hi) x
              [0, Wi), edges ``clip(c -/+ side // 2, 0, Hi or Wi)`` (timm's ``rand_bbox``); the rectangle is the partner's
              pixels, ``t = area / (Hi Wi)`` of the clipped rectangle (``correct_lam``: lam = 1 - t) and ``m = 0``.
    The target of sample ``i`` is ``(1 - t) onehot(y_i) + t onehot(y_partner)``, smoothed by the loss (``soft_target``).
    A row of the table is ``(partner, cx0, cy0, cw, ch, bits of fp32 m, bits of fp32 t, 0)``: include/cara_hip.h,
    ``cara_im2col_patches_u8_rows_mix``.  ``size`` = Hi or (Hi, Wi): the model's input, in whose pixels the rectangle is."""

    def __init__(self, size, mixup_alpha: float = 0.8, cutmix_alpha: float = 1.0, prob: float = 1.0, switch_prob: float = 0.5):
        Hi, Wi = (size, size) if isinstance(size, int) else size
        if int(Hi) <= 0 or int(Wi) <= 0 or mixup_alpha < 0 or cutmix_alpha < 0 or (mixup_alpha == 0 and cutmix_alpha == 0) \
                or not (0.0 <= prob <= 1.0) or not (0.0 <= switch_prob <= 1.0):
            raise ValueError("MixupCutmix: size > 0, alphas >= 0 and not both 0, prob and switch_prob in [0, 1]")
        self.Hi, self.Wi = int(Hi), int(Wi)
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob = float(mixup_alpha), float(cutmix_alpha), float(prob), float(switch_prob)

    def draw(self, B: int, steps: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """int32 [steps, B, 8] on the host.  A fixed number of variates of ``generator`` per batch -- one, the seed of that batch's
        own generator (the Beta draw rejects a varying number of its variates) -- so batch ``k`` does not depend on ``steps``."""
        Hi, Wi = self.Hi, self.Wi
        out = identity_mix(B, steps)
        for k in range(steps):
            g = torch.Generator().manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=generator)))
            u = torch.rand(4, generator=g, dtype=torch.float64).tolist()
            if not u[0] < self.prob:
                continue
            cutmix = self.cutmix_alpha > 0 and (self.mixup_alpha == 0 or u[1] < self.switch_prob)
            alpha = self.cutmix_alpha if cutmix else self.mixup_alpha
            x, y = torch._standard_gamma(torch.full((2,), alpha, dtype=torch.float64), generator=g).tolist()
            lam = x / (x + y) if x + y > 0 else 0.5
            row = out[k]
            row[:, 0] = B - 1 - torch.arange(B, dtype=torch.int32)
            if cutmix:
                r = math.sqrt(1.0 - lam)
                ch, cw = int(Hi * r), int(Wi * r)
                cy, cx = min(int(u[2] * Hi), Hi - 1), min(int(u[3] * Wi), Wi - 1)
                y0, y1 = min(max(cy - ch // 2, 0), Hi), min(max(cy + ch // 2, 0), Hi)
                x0, x1 = min(max(cx - cw // 2, 0), Wi), min(max(cx + cw // 2, 0), Wi)
                row[:, 1], row[:, 2], row[:, 3], row[:, 4] = x0, y0, x1 - x0, y1 - y0
                row[:, 6] = _f32_bits(torch.tensor((x1 - x0) * (y1 - y0) / (Hi * Wi), dtype=torch.float64))
            else:
                row[:, 5] = row[:, 6] = _f32_bits(torch.tensor(1.0 - lam, dtype=torch.float64))
        return out


def check_mix(mix: torch.Tensor, B: int, Hi: int, Wi: int) -> None:
    """ValueError unless ``mix`` is an int32 [..., B, 8] table whose every partner is in [0, B), whose every rectangle lies inside
    the ``Hi`` x ``Wi`` output and whose every m and t is in [0, 1] (the companion of ``check_boxes``)"""
    if not torch.is_tensor(mix) or mix.dtype != torch.int32 or mix.ndim < 2 or mix.shape[-1] != 8 or mix.shape[-2] != B:
        raise ValueError("mix must be an int32 [..., batch, 8] tensor (partner, cx0, cy0, cw, ch, blend bits, target bits, 0)")
    t = mix.reshape(-1, 8).cpu()
    w = t.to(torch.int64)
    m, tg = _bits_f32(t[:, 5]), _bits_f32(t[:, 6])
    bad = (w[:, 0] < 0) | (w[:, 0] >= B) | (w[:, 1] < 0) | (w[:, 2] < 0) | (w[:, 3] < 0) | (w[:, 4] < 0) | (w[:, 1] + w[:, 3] > Wi) \
        | (w[:, 2] + w[:, 4] > Hi) | ~((m >= 0) & (m <= 1)) | ~((tg >= 0) & (tg <= 1))
    if bool(bad.any()):
        i = int(bad.to(torch.int64).argmax())
        raise ValueError(f"{int(bad.sum())} mix entry(ies) with a partner outside [0, {B}), a rectangle outside the {Hi} x {Wi} output "
                         f"or a weight outside [0, 1], the first: {t[i, :5].tolist()} m {float(m[i])} t {float(tg[i])}")


def mix_reference(pixels_u8: torch.Tensor, rows, boxes, mix, size, dtype=torch.float64) -> torch.Tensor:
    """What ``cara_im2col_patches_u8_rows_mix`` samples, before normalisation, in torch ops on the CPU: with ``x =
    resized_crop_reference(pixels, rows, boxes, size)`` (``boxes`` None: every sample its whole image, which must have the
    output's size) and row ``i`` of ``mix`` = (p, cx0, cy0, cw, ch, m, t, 0): ``out[i] = x[i] + m (x[p] - x[i])``, then
    ``out[i][:, cy0:cy0+ch, cx0:cx0+cw] = x[p][...]``.  [B,C,Hi,Wi] of ``dtype``."""
    Hi, Wi = (size, size) if isinstance(size, int) else size
    rows = torch.as_tensor(rows).cpu()
    if boxes is None:
        if tuple(pixels_u8.shape[2:]) != (Hi, Wi):
            raise ValueError("without boxes the split must have the output's size")
        boxes = torch.tensor([[0, 0, Wi, Hi, 0]] * len(rows), dtype=torch.int32)
    mix = torch.as_tensor(mix).cpu()
    check_mix(mix, len(rows), Hi, Wi)
    x = resized_crop_reference(pixels_u8, rows, boxes, (Hi, Wi), dtype)
    m = _bits_f32(mix[:, 5]).to(dtype)
    out = torch.empty_like(x)
    for i, (p, cx0, cy0, cw, ch) in enumerate(mix[:, :5].tolist()):
        out[i] = x[i] + m[i] * (x[p] - x[i])
        out[i][:, cy0:cy0 + ch, cx0:cx0 + cw] = x[p][:, cy0:cy0 + ch, cx0:cx0 + cw]
    return out


def soft_target(labels: torch.Tensor, mix, classes: int, smoothing: float = 0.0) -> torch.Tensor:
    """The target ``cara_cross_entropy_mix`` trains on, float64 [B, classes]: ``q = (1 - eps) ((1 - t) onehot(y) + t
    onehot(y[partner])) + eps / classes`` -- torch's ``label_smoothing`` of timm's ``mixup_target``.  ``mix`` None: t = 0."""
    y = labels.detach().cpu().long()
    B = y.shape[0]
    eye = torch.eye(classes, dtype=torch.float64)
    if mix is None:
        partner, t = torch.arange(B), torch.zeros(B, dtype=torch.float64)
    else:
        mix = torch.as_tensor(mix).cpu()
        partner, t = mix[:, 0].long(), _bits_f32(mix[:, 6]).double()
    t = t[:, None]
    return (1.0 - smoothing) * ((1.0 - t) * eye[y] + t * eye[y[partner]]) + smoothing / classes


def class_counts(split_or_labels, classes: int) -> torch.Tensor:
    """Images per class, int64 [classes] on the host, of a ``ResidentSplit`` (its ``labels`` are read once) or a label tensor: what
    ``balanced_class_weight`` and ``logit_prior`` are made from.  A label outside [0, classes) raises ``ValueError``."""
    labels = getattr(split_or_labels, "labels", split_or_labels)
    y = torch.as_tensor(labels).detach().cpu().reshape(-1).long()
    if not isinstance(classes, int) or isinstance(classes, bool) or classes < 1:
        raise ValueError(f"class_counts: classes must be an integer >= 1, not {classes!r}")
    if y.numel() and (int(y.min()) < 0 or int(y.max()) >= classes):
        raise ValueError(f"class_counts: labels span [{int(y.min())}, {int(y.max())}], outside [0, {classes})")
    return torch.bincount(y, minlength=classes)


def _counts64(counts, who: str) -> torch.Tensor:
    n = torch.as_tensor(counts).detach().cpu().reshape(-1).double()
    if n.numel() == 0 or not bool(torch.isfinite(n).all()) or bool((n < 0).any()) or not float(n.sum()) > 0:
        raise ValueError(f"{who}: counts must be non-negative with a positive total")
    return n


def balanced_class_weight(counts, power: float = 1.0, dtype=torch.float32) -> torch.Tensor:
    """Class weights for ``train_step(class_weight=)``, fp32 [classes]: ``w_c`` proportional to ``max(n_c, 1) ** -power`` and scaled
    so that ``sum_c n_c w_c == sum_c n_c`` -- the mean weight over the training samples is 1, so the loss (a sum over the batch
    divided by the batch size) keeps its scale.  ``power = 1`` is inverse frequency, ``0.5`` the usual softened form, ``0`` all
    ones.  An absent class gets the weight of a class with one image.  Computed in float64 and rounded once to ``dtype`` (fp32 is
    what the step takes: the identity then holds to that rounding, 2^-24 of the total).  Negative counts or a total that is not
    positive raise ``ValueError``."""
    n = _counts64(counts, "balanced_class_weight")
    if isinstance(power, bool) or not isinstance(power, (int, float)) or not power >= 0.0 or power == float("inf"):
        raise ValueError(f"balanced_class_weight: power must be a finite number >= 0, not {power!r}")
    raw = n.clamp_min(1.0) ** -float(power)
    return (raw * (n.sum() / (n * raw).sum())).to(dtype)


def logit_prior(counts, tau: float = 1.0) -> torch.Tensor:
    """The bias of logit-adjusted training (Menon et al., 2021) for ``train_step(logit_bias=)``, fp32 [classes]:
    ``tau * log((n_c + 1) / (N + classes))`` -- the add-one smoothing keeps the bias of an absent class finite.  Negative counts
    or a total that is not positive raise ``ValueError``."""
    n = _counts64(counts, "logit_prior")
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not abs(tau) < float("inf"):
        raise ValueError(f"logit_prior: tau must be a finite number, not {tau!r}")
    return (float(tau) * torch.log((n + 1.0) / (n.sum() + n.numel()))).float()


def aug_seed(seed: int, epoch: int, rank: int) -> int:
    """``box_seed`` of the stream that draws the colour-jitter / erase tables (a third constant)"""
    return box_seed(seed, epoch, rank, stream=0x2545F491)


AUG_NONE, AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION = 0, 1, 2, 3
AUG_ERASE_STREAM = 0x45524153                 # the counter hash's stream of the erase noise (feed.hip)
GRAY_WEIGHTS = (0.2989, 0.587, 0.114)         # torchvision's rgb_to_grayscale; the kernel holds them as fp32


def identity_aug(B: int, steps: Optional[int] = None) -> torch.Tensor:
    """int32 [B, 16] (or [steps, B, 16]) table that changes nothing: no colour op, no erase rectangle"""
    return torch.zeros((B, 16) if steps is None else (steps, B, 16), dtype=torch.int32)


class ColorJitterErase:
    """Colour-jitter / Random-Erasing tables for the resident feed, restated from the published definitions (neither torchvision
    nor timm is installed).
    torchvision's ``ColorJitter(brightness, contrast, saturation)`` (no hue): per sample a factor uniform in
    ``[max(0, 1 - j), 1 + j]`` for every ``j > 0`` and a uniform random order of the three ops; each op is ``_blend``:
    ``clamp(f x + (1 - f) d)`` with ``d`` = 0 (brightness), the image's mean gray (contrast) or the pixel's gray (saturation).
    timm's ``RandomErasing(probability, min_area, max_area, min_aspect, max_aspect, mode, max_count=1)``: with probability
    ``erase_prob``, up to ten attempts of ``area = Hi Wi U(erase_scale)``, ``aspect = exp(U(log erase_ratio))``, ``h =
    round(sqrt(area aspect))``, ``w = round(sqrt(area / aspect))``; the first with ``w < Wi`` and ``h < Hi`` is taken at a uniform
    integer offset (``top`` in [0, Hi - h], ``left`` in [0, Wi - w]); none fits: nothing erased.  ``erase_mode``: "pixel" (a standard
    normal per element of the normalised image) or "const" (zeros).
    A row of the table is ``(op0, f0 bits, op1, f1 bits, op2, f2 bits, ex0, ey0, ew, eh, emode, eseed, 0, 0, 0, 0)``:
    include/cara_hip.h, ``cara_im2col_patches_u8_rows_aug``.  ``size`` = Hi or (Hi, Wi): the model's input."""

    TRIES = 10

    def __init__(self, size, brightness: float = 0.4, contrast: float = 0.4, saturation: float = 0.4, erase_prob: float = 0.25,
                 erase_scale=(0.02, 1.0 / 3.0), erase_ratio=(0.3, 3.3), erase_mode: str = "pixel"):
        Hi, Wi = (size, size) if isinstance(size, int) else size
        if int(Hi) <= 0 or int(Wi) <= 0 or min(brightness, contrast, saturation) < 0 or not (0.0 <= erase_prob <= 1.0) \
                or not (0 < erase_scale[0] <= erase_scale[1] <= 1) or not (0 < erase_ratio[0] <= erase_ratio[1]) \
                or erase_mode not in ("pixel", "const"):
            raise ValueError("ColorJitterErase: size > 0, jitters >= 0, erase_prob in [0, 1], 0 < erase_scale[0] <= erase_scale[1] <= 1, "
                             "0 < erase_ratio[0] <= erase_ratio[1], erase_mode 'pixel' or 'const'")
        self.Hi, self.Wi = int(Hi), int(Wi)
        self.jitter = (float(brightness), float(contrast), float(saturation))
        self.erase_prob, self.erase_mode = float(erase_prob), erase_mode
        self.erase_scale, self.erase_ratio = (float(erase_scale[0]), float(erase_scale[1])), (float(erase_ratio[0]), float(erase_ratio[1]))

    def draw(self, B: int, steps: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """int32 [steps, B, 16] on the host.  One variate of ``generator`` per batch -- the seed of that batch's own generator, as
        in ``MixupCutmix.draw`` -- so batch ``k`` does not depend on ``steps``."""
        Hi, Wi, T = self.Hi, self.Wi, self.TRIES
        out = identity_aug(B, steps)
        for k in range(steps):
            g = torch.Generator().manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=generator)))
            uf = torch.rand(B, 3, generator=g, dtype=torch.float64)
            order = torch.rand(B, 3, generator=g, dtype=torch.float64).argsort(1)      # a uniform permutation per sample
            ue = torch.rand(B, T, 4, generator=g, dtype=torch.float64)
            coin = torch.rand(B, generator=g, dtype=torch.float64)
            seeds = torch.randint(0, 2 ** 32, (B,), generator=g, dtype=torch.int64)
            row = out[k]
            j = torch.tensor(self.jitter, dtype=torch.float64)
            lo = (1.0 - j).clamp(min=0.0)
            f = lo + (1.0 + j - lo) * uf                                                # [B, 3]: brightness, contrast, saturation
            ops = torch.where(j > 0, torch.arange(1, 4), torch.zeros(3, dtype=torch.int64)).expand(B, 3)
            row[:, 0:6:2] = ops.gather(1, order).to(torch.int32)
            row[:, 1:6:2] = torch.where(ops.gather(1, order) > 0, _f32_bits(f.gather(1, order)), torch.zeros(B, 3, dtype=torch.int32))
            area = Hi * Wi * (self.erase_scale[0] + (self.erase_scale[1] - self.erase_scale[0]) * ue[..., 0])
            la, lb = math.log(self.erase_ratio[0]), math.log(self.erase_ratio[1])
            aspect = torch.exp(la + (lb - la) * ue[..., 1])
            h = torch.round(torch.sqrt(area * aspect)).to(torch.int64)
            w = torch.round(torch.sqrt(area / aspect)).to(torch.int64)
            fits = (w < Wi) & (h < Hi) & (w > 0) & (h > 0)
            first = fits.to(torch.int64).argmax(1)
            pick = lambda t: t.gather(1, first[:, None])[:, 0]   # noqa: E731
            w, h = pick(w), pick(h)
            top = torch.floor(pick(ue[..., 2]) * (Hi - h + 1).clamp(min=1)).to(torch.int64).clamp(min=0)
            left = torch.floor(pick(ue[..., 3]) * (Wi - w + 1).clamp(min=1)).to(torch.int64).clamp(min=0)
            on = fits.any(1) & (coin < self.erase_prob)
            zero = torch.zeros(B, dtype=torch.int64)
            row[:, 6] = torch.where(on, torch.minimum(left, Wi - w), zero).to(torch.int32)
            row[:, 7] = torch.where(on, torch.minimum(top, Hi - h), zero).to(torch.int32)
            row[:, 8] = torch.where(on, w, zero).to(torch.int32)
            row[:, 9] = torch.where(on, h, zero).to(torch.int32)
            row[:, 10] = 1 if self.erase_mode == "pixel" else 0
            row[:, 11] = torch.where(seeds >= 2 ** 31, seeds - 2 ** 32, seeds).to(torch.int32)
        return out


def check_aug(aug: torch.Tensor, B: int, Hi: int, Wi: int) -> None:
    """ValueError unless ``aug`` is an int32 [..., B, 16] table the kernel accepts: every op in [0, 3], no non-zero op twice in a row,
    every factor of a non-zero op finite and >= 0, every erase rectangle inside the ``Hi`` x ``Wi`` output, every emode 0 or 1,
    the last four words 0 (the companion of ``check_mix``)"""
    if not torch.is_tensor(aug) or aug.dtype != torch.int32 or aug.ndim < 2 or aug.shape[-1] != 16 or aug.shape[-2] != B:
        raise ValueError("aug must be an int32 [..., batch, 16] tensor (op0, f0, op1, f1, op2, f2, ex0, ey0, ew, eh, emode, eseed, 0, 0, 0, 0)")
    t = aug.reshape(-1, 16).cpu()
    w = t.to(torch.int64)
    ops, f = w[:, 0:6:2], _bits_f32(t[:, 1:6:2])
    bad = ((ops < 0) | (ops > 3)).any(1)
    for code in (1, 2, 3):
        bad |= (ops == code).sum(1) > 1
    bad |= ((ops != 0) & ~((f >= 0) & torch.isfinite(f))).any(1)
    bad |= (w[:, 6] < 0) | (w[:, 7] < 0) | (w[:, 8] < 0) | (w[:, 9] < 0) | (w[:, 6] + w[:, 8] > Wi) | (w[:, 7] + w[:, 9] > Hi)
    bad |= ((w[:, 10] != 0) & (w[:, 10] != 1)) | (w[:, 12:] != 0).any(1)
    if bool(bad.any()):
        i = int(bad.to(torch.int64).argmax())
        raise ValueError(f"{int(bad.sum())} aug entry(ies) with an unknown or repeated op, a factor that is negative or not finite, an erase "
                         f"rectangle outside the {Hi} x {Wi} output, an emode outside {{0, 1}} or a non-zero pad word, the first: "
                         f"{t[i].tolist()}")


def erase_noise(index, eseed: int):
    """(u1, arg, z): the pixel-mode erase value of element ``index`` (its position in [B,C,Hi,Wi], any integer array) in the kernel's
    formula: two draws of the counter hash, ``u1 = ((h1 >> 8) + 1) 2^-24``, ``u2 = (h2 >> 8) 2^-24`` (exact), ``arg`` = the fp32
    product ``6.2831855f u2``; ``z = sqrt(-2 log(u1)) cos(arg)`` in float64 on those fp32 arguments.  numpy arrays."""
    import numpy as np
    from .dropout import keep_hash_np
    i = np.asarray(index).astype(np.uint32)
    seed = int(eseed) & 0xffffffff
    h1 = keep_hash_np(i * np.uint32(2), seed, AUG_ERASE_STREAM)
    h2 = keep_hash_np(i * np.uint32(2) + np.uint32(1), seed, AUG_ERASE_STREAM)
    u1 = ((h1 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (h2 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    arg = np.float32(6.2831855) * u2
    return u1, arg, np.sqrt(-2.0 * np.log(u1)) * np.cos(arg.astype(np.float64))


def color_chain_reference(x: torch.Tensor, row) -> torch.Tensor:
    """the colour chain of one table row on one unmixed image ``x`` [3,Hi,Wi] on the 0..255 scale, in ``x``'s dtype: each slot
    ``clamp(f x + (1 - f) d, 0, 255)`` with the fp32 factor and the fp32 gray weights the kernel holds"""
    wr, wg, wb = (float(torch.tensor(v, dtype=torch.float32)) for v in GRAY_WEIGHTS)
    gray = lambda t: wr * t[0] + wg * t[1] + wb * t[2]   # noqa: E731
    row = torch.as_tensor(row).to(torch.int32)
    for k in range(3):
        op = int(row[2 * k])
        if op == AUG_NONE:
            continue
        f = float(_bits_f32(row[2 * k + 1:2 * k + 2])[0])
        d = 0.0 if op == AUG_BRIGHTNESS else (gray(x).mean() if op == AUG_CONTRAST else gray(x)[None])
        x = (f * x + (1.0 - f) * d).clamp(0.0, 255.0)
    return x


def aug_reference(pixels_u8: torch.Tensor, rows, boxes, mix, aug, size, dtype=torch.float64) -> torch.Tensor:
    """What ``cara_im2col_patches_u8_rows_aug`` computes before its one rounding to 16 bits, in torch ops on the CPU: the
    NORMALISED image [B,3,Hi,Wi] of ``dtype``.  ``y[i] = color_chain_reference(resized_crop_reference(...)[i], aug[i])``; the mix of
    ``mix_reference`` on ``y`` (``mix`` None: none; ``boxes`` None: whole images of the output's size); ``(v / 255 - mean) / std``; the
    erase rectangle of ``aug[i]`` filled with 0 or with ``erase_noise``.  Named functions are evaluated in float64 on the fp32
    arguments the kernel's formula gives them."""
    Hi, Wi = (size, size) if isinstance(size, int) else size
    rows = torch.as_tensor(rows).cpu()
    B = len(rows)
    if boxes is None:
        if tuple(pixels_u8.shape[2:]) != (Hi, Wi):
            raise ValueError("without boxes the split must have the output's size")
        boxes = torch.tensor([[0, 0, Wi, Hi, 0]] * B, dtype=torch.int32)
    mix = identity_mix(B) if mix is None else torch.as_tensor(mix).cpu()
    aug = torch.as_tensor(aug).cpu()
    check_mix(mix, B, Hi, Wi)
    check_aug(aug, B, Hi, Wi)
    if pixels_u8.shape[1] != 3:
        raise ValueError("the colour ops are defined on three channels")
    x = resized_crop_reference(pixels_u8, rows, boxes, (Hi, Wi), dtype)
    y = torch.stack([color_chain_reference(x[i], aug[i]) for i in range(B)])
    return _mix_normalize_erase(y, mix, aug, Hi, Wi, dtype)


def _mix_normalize_erase(y: torch.Tensor, mix, aug, Hi: int, Wi: int, dtype) -> torch.Tensor:
    """the tail of ``aug_reference`` (and ``ra_reference``) on the unmixed images ``y`` [B,3,Hi,Wi] after their own chains"""
    B = y.shape[0]
    m = _bits_f32(mix[:, 5]).to(dtype)
    out = torch.empty_like(y)
    for i, (p, cx0, cy0, cw, ch) in enumerate(mix[:, :5].tolist()):
        out[i] = y[i] + m[i] * (y[p] - y[i])
        out[i][:, cy0:cy0 + ch, cx0:cx0 + cw] = y[p][:, cy0:cy0 + ch, cx0:cx0 + cw]
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    out = (out / 255.0 - mean) / std
    index = torch.arange(B * 3 * Hi * Wi).view(B, 3, Hi, Wi)
    for i, (ex0, ey0, ew, eh, emode, eseed) in enumerate(aug[:, 6:12].tolist()):
        if ew == 0 or eh == 0:
            continue
        sl = (slice(None), slice(ey0, ey0 + eh), slice(ex0, ex0 + ew))
        out[i][sl] = torch.from_numpy(erase_noise(index[i][sl].numpy(), eseed)[2]).to(dtype) if emode else 0.0
    return out


def ra_seed(seed: int, epoch: int, rank: int) -> int:
    """``box_seed`` of the stream that draws the RandAugment tables (a fifth constant)"""
    return box_seed(seed, epoch, rank, stream=0x3C6EF372)


RA_NONE, RA_POSTERIZE, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_INVERT, RA_AUTOCONTRAST, RA_EQUALIZE = range(7)
RA_ARG_MAX = (0, 8, 256, 255, 0, 0, 0)        # the largest argument of each lookup op
RA_MATRIX_MAX = 32768.0
RA_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
          "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
_RA_LOOKUP = {"Posterize": RA_POSTERIZE, "Solarize": RA_SOLARIZE, "SolarizeAdd": RA_SOLARIZE_ADD, "Invert": RA_INVERT,
              "AutoContrast": RA_AUTOCONTRAST, "Equalize": RA_EQUALIZE}
_RA_JITTER = {"Color": AUG_SATURATION, "Contrast": AUG_CONTRAST, "Brightness": AUG_BRIGHTNESS}
_RA_GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")


def identity_ra(B: int, steps: Optional[int] = None) -> torch.Tensor:
    """int32 [B, 16] (or [steps, B, 16]) table that changes nothing: no lookup op, the identity matrix (1, 0, 0, 0, 1, 0), fill 0"""
    t = torch.zeros((B, 16) if steps is None else (steps, B, 16), dtype=torch.int32)
    t[..., 6] = t[..., 10] = 0x3f800000
    return t


def ra_level_arg(op: str, level: float, sign: int = 1, increasing: bool = True):
    """the argument of one op at level L in [0, 10] (timm's ``_LEVEL_DENOM`` = 10), restated: Rotate -> degrees ``+-30 L/10``; ShearX /
    ShearY -> ``+-0.3 L/10``; TranslateXRel / TranslateYRel -> ``+-0.45 L/10`` of the size; Posterize -> bits kept ``4 - int(4 L/10)``
    (not increasing: ``int(4 L/10)``); Solarize -> threshold ``256 - int(256 L/10)`` (not increasing: ``int(256 L/10)``); SolarizeAdd ->
    ``int(110 L/10)``; Color / Contrast / Brightness -> factor ``max(0.1, 1 +- 0.9 L/10)`` (not increasing: ``0.1 + 1.8 L/10``);
    AutoContrast, Equalize, Invert -> None"""
    x = float(level) / 10.0
    if op == "Rotate":
        return sign * 30.0 * x
    if op in ("ShearX", "ShearY"):
        return sign * 0.3 * x
    if op in ("TranslateXRel", "TranslateYRel"):
        return sign * 0.45 * x
    if op == "Posterize":
        return 4 - int(4 * x) if increasing else int(4 * x)
    if op == "Solarize":
        return 256 - int(256 * x) if increasing else min(256, int(256 * x))
    if op == "SolarizeAdd":
        return min(255, int(110 * x))
    if op in _RA_JITTER:
        return max(0.1, 1.0 + sign * 0.9 * x) if increasing else 0.1 + 1.8 * x
    if op in ("AutoContrast", "Equalize", "Invert"):
        return None
    raise ValueError(f"unknown RandAugment op {op!r} (one of {RA_OPS})")


def ra_op_matrix(op: str, arg: float, Hi: int, Wi: int):
    """the 3 x 3 float64 output-to-input matrix of one geometric op on a ``Hi`` x ``Wi`` image, in PIL's ``Image.transform(AFFINE)``
    convention (evaluated at pixel centres): Rotate by ``arg`` degrees about (Wi / 2, Hi / 2) as ``Image.rotate`` builds it; ShearX
    (1, arg, 0; 0, 1, 0); ShearY (1, 0, 0; arg, 1, 0); TranslateXRel (1, 0, arg Wi; 0, 1, 0); TranslateYRel (1, 0, 0; 0, 1, arg Hi)"""
    import numpy as np
    m = np.eye(3)
    if op == "Rotate":
        t = -math.radians(arg)
        c, s, cx, cy = math.cos(t), math.sin(t), Wi / 2.0, Hi / 2.0
        m[0] = (c, s, cx - (c * cx + s * cy))
        m[1] = (-s, c, cy - (-s * cx + c * cy))
    elif op == "ShearX":
        m[0, 1] = arg
    elif op == "ShearY":
        m[1, 0] = arg
    elif op == "TranslateXRel":
        m[0, 2] = arg * Wi
    elif op == "TranslateYRel":
        m[1, 2] = arg * Hi
    else:
        raise ValueError(f"{op!r} is no geometric op")
    return m


class RandAugment:
    """RandAugment tables for the resident feed (timm's ``rand-m9-mstd0.5-inc1``), restated from the published definitions (timm is
    not installed): per sample ``n`` ops drawn uniformly (with replacement) from ``ops``, each applied with probability ``prob`` at the
    level ``clip(N(m, mstd), 0, 10)`` through ``ra_level_arg`` (a fair sign where the map says +-).
    ``draw`` gives two tables: ``ra`` int32 [steps, B, 16], rows ``(op0, arg0, op1, arg1, op2, arg2, m00, m01, m02, m10, m11, m12,
    fill, 0, 0, 0)`` of ``cara_im2col_patches_u8_rows_ra`` (include/cara_hip.h), and ``slots`` int32 [steps, B, 6], the jitter slots
    ``(op0, f0, op1, f1, op2, f2)`` of the ``aug`` row.  The geometric ops of a sample compose in drawn order into ONE output-to-input
    matrix (float64, rounded once to fp32): one resampling, not one per op.  Posterize, Solarize, SolarizeAdd, Invert, AutoContrast
    and Equalize fill the lookup slots in drawn order; Color / Contrast / Brightness become the saturation / contrast / brightness
    slots of the aug row.
    Known departures from PIL's order of application: (1) the geometry always comes first, whatever was drawn; (2) the jitter slots
    run after the lookup slots; (3) the fill pixels pass through the lookup slots (PIL fills after them when the geometric op comes
    last); (4) a second AutoContrast / Equalize of a sample is dropped (one statistic slot per row), and so is a repeated Color /
    Contrast / Brightness (``check_aug``: a jitter op at most once per row).  Not built: Sharpness, PIL's random choice of
    interpolation (always bilinear).  ``size`` = Hi or (Hi, Wi): the model's input.  ``n`` <= 3: a row has three slots of each kind."""

    def __init__(self, size, n: int = 2, m: float = 9, mstd: float = 0.5, prob: float = 0.5, increasing: bool = True,
                 fill=(124, 116, 104), ops=None):
        Hi, Wi = (size, size) if isinstance(size, int) else size
        ops = tuple(RA_OPS if ops is None else ops)
        if int(Hi) <= 0 or int(Wi) <= 0 or not (1 <= int(n) <= 3) or not (0 <= m <= 10) or mstd < 0 or not (0.0 <= prob <= 1.0) \
                or len(fill) != 3 or any(not (0 <= int(v) <= 255) for v in fill) or not ops or any(o not in RA_OPS for o in ops):
            raise ValueError(f"RandAugment: size > 0, 1 <= n <= 3, 0 <= m <= 10, mstd >= 0, prob in [0, 1], fill three bytes, ops from {RA_OPS}")
        self.Hi, self.Wi, self.n, self.m, self.mstd, self.prob = int(Hi), int(Wi), int(n), float(m), float(mstd), float(prob)
        self.increasing, self.ops = bool(increasing), ops
        self.fill = (int(fill[0]) << 16) | (int(fill[1]) << 8) | int(fill[2])

    def row(self, drawn):
        """(ra row, jitter slots) as two lists of ints from ``[(op name, level, sign), ...]`` in drawn order (the applied ops only)"""
        import numpy as np
        mat, lookup, jitter = np.eye(3), [], []
        for op, level, sign in drawn:
            arg = ra_level_arg(op, level, sign, self.increasing)
            if op in _RA_GEOMETRIC:
                mat = mat @ ra_op_matrix(op, arg, self.Hi, self.Wi)     # (the later op maps the output first)
            elif op in _RA_LOOKUP:
                code = _RA_LOOKUP[op]
                if code >= RA_AUTOCONTRAST and any(c >= RA_AUTOCONTRAST for c, _ in lookup):
                    continue
                lookup.append((code, 0 if arg is None else int(arg)))
            elif all(c != _RA_JITTER[op] for c, _ in jitter):
                jitter.append((_RA_JITTER[op], int(np.array([arg], dtype=np.float32).view(np.int32)[0])))
        lookup += [(0, 0)] * (3 - len(lookup))
        jitter += [(0, 0)] * (3 - len(jitter))
        words = [int(w) for w in np.ascontiguousarray(mat[:2].astype(np.float32)).view(np.int32).reshape(-1)]
        return [v for s in lookup for v in s] + words + [self.fill, 0, 0, 0], [v for s in jitter for v in s]

    def draw(self, B: int, steps: int, generator: Optional[torch.Generator] = None):
        """(ra int32 [steps, B, 16], slots int32 [steps, B, 6]) on the host.  One variate of ``generator`` per batch -- the seed of that
        batch's own generator, as in ``MixupCutmix.draw`` -- so batch ``k`` does not depend on ``steps``."""
        ra, slots = identity_ra(B, steps), torch.zeros(steps, B, 6, dtype=torch.int32)
        for k in range(steps):
            g = torch.Generator().manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=generator)))
            which = torch.randint(0, len(self.ops), (B, self.n), generator=g).tolist()
            coin = torch.rand(B, self.n, generator=g, dtype=torch.float64).tolist()
            level = (self.m + self.mstd * torch.randn(B, self.n, generator=g, dtype=torch.float64)).clamp_(0.0, 10.0).tolist()
            sign = torch.rand(B, self.n, generator=g, dtype=torch.float64).tolist()
            rows = [self.row([(self.ops[which[b][j]], level[b][j], 1 if sign[b][j] < 0.5 else -1) for j in range(self.n) if coin[b][j] < self.prob])
                    for b in range(B)]
            ra[k] = torch.tensor([r for r, _ in rows], dtype=torch.int32)
            slots[k] = torch.tensor([s for _, s in rows], dtype=torch.int32)
        return ra, slots


def check_ra(ra: torch.Tensor, B: int) -> None:
    """ValueError unless ``ra`` is an int32 [..., B, 16] table the kernel accepts: every op in [0, 6], every argument in its op's range
    (``RA_ARG_MAX``; 0 for no op), at most one statistic op (autocontrast, equalize) in a row, every matrix word a finite fp32 of
    magnitude <= 32768, fill <= 0xFFFFFF, the last three words 0 (the companion of ``check_aug``)"""
    if not torch.is_tensor(ra) or ra.dtype != torch.int32 or ra.ndim < 2 or ra.shape[-1] != 16 or ra.shape[-2] != B:
        raise ValueError("ra must be an int32 [..., batch, 16] tensor (op0, arg0, op1, arg1, op2, arg2, m00, m01, m02, m10, m11, m12, fill, 0, 0, 0)")
    t = ra.reshape(-1, 16).cpu()
    w = t.to(torch.int64)
    ops, args, m = w[:, 0:6:2], w[:, 1:6:2], _bits_f32(t[:, 6:12])
    bad = ((ops < 0) | (ops > 6)).any(1)
    top = torch.tensor(RA_ARG_MAX)[ops.clamp(0, 6)]
    bad |= ((args < 0) | (args > top)).any(1)
    bad |= (ops >= RA_AUTOCONTRAST).sum(1) > 1
    bad |= (~(m.abs() <= RA_MATRIX_MAX)).any(1)
    bad |= (w[:, 12] < 0) | (w[:, 12] > 0xFFFFFF) | (w[:, 13:] != 0).any(1)
    if bool(bad.any()):
        i = int(bad.to(torch.int64).argmax())
        raise ValueError(f"{int(bad.sum())} ra entry(ies) with an unknown op, an argument outside its range, two statistic ops, a matrix "
                         f"word that is not finite or above {RA_MATRIX_MAX:g} in magnitude, a fill above 0xFFFFFF or a non-zero pad word, "
                         f"the first: {t[i].tolist()}")


def ra_lut(hist, op: int):
    """the 256-entry table of a statistic op from a 256-bin histogram (integers): autocontrast -- lo, hi the first / last non-zero
    bin, identity if hi <= lo, else ``clamp(255 (i - lo) // (hi - lo), 0, 255)`` and 0 below lo; equalize -- ``step = (sum h - h[hi])
    // 255``, identity if hi <= lo or step == 0, else ``min(255, (step // 2 + sum_{j<i} h[j]) // step)``.  numpy int64 [256]."""
    import numpy as np
    h = np.asarray(hist, dtype=np.int64)
    i = np.arange(256, dtype=np.int64)
    nz = np.nonzero(h)[0]
    if len(nz) < 2:
        return i
    lo, hi = int(nz[0]), int(nz[-1])
    if op == RA_AUTOCONTRAST:
        return np.where(i < lo, 0, np.clip((255 * (i - lo)) // (hi - lo), 0, 255))
    step = (int(h.sum()) - int(h[hi])) // 255
    if step == 0:
        return i
    before = np.concatenate([[0], np.cumsum(h)[:-1]])
    return np.minimum(255, (step // 2 + before) // step)


def ra_lookup_reference(q, row):
    """the lookup slots of one ra row on the quantised image ``q`` (integer array [3,Hi,Wi]) -> (image, tables or None): the
    statistic slot's tables are int64 [3, 256], of the histograms as they stand before that slot"""
    import numpy as np
    q = np.asarray(q).astype(np.int64)
    tables = None
    for k in range(3):
        op, arg = int(row[2 * k]), int(row[2 * k + 1])
        if op == RA_POSTERIZE:
            q = q & ~((1 << (8 - arg)) - 1)
        elif op == RA_SOLARIZE:
            q = np.where(q < arg, q, 255 - q)
        elif op == RA_SOLARIZE_ADD:
            q = np.where(q < 128, np.minimum(q + arg, 255), q)
        elif op == RA_INVERT:
            q = 255 - q
        elif op in (RA_AUTOCONTRAST, RA_EQUALIZE):
            tables = np.stack([ra_lut(np.bincount(q[c].reshape(-1), minlength=256), op) for c in range(3)])
            q = np.stack([tables[c][q[c]] for c in range(3)])
    return q, tables


def ra_geometry_reference(pixels_u8: torch.Tensor, r: int, box, row, Hi: int, Wi: int, dtype=torch.float64) -> torch.Tensor:
    """the geometry of one ra row on image ``r`` of the split through ``box`` = (x0, y0, w, h, flip): [3,Hi,Wi] of ``dtype`` on the
    0..255 scale, in the kernel's formula with the fp32 matrix words the row holds -- ``u = m00 x + m01 y + m02``, ``v = m10 x + m11 y +
    m12`` at ``x = ox + 0.5``, ``y = oy + 0.5``; the fill byte unless ``0 <= u < Wi`` and ``0 <= v < Hi``; inside, ``uf = flip ? Wi - u : u``,
    ``s = max(uf w / Wi - 0.5, 0)``, ``i0 = min(int(s), w - 1)``, ``i1 = min(i0 + 1, w - 1)``, ``f = s - i0``, the same for v, bilinear"""
    x0, y0, w, h, flip = (int(v) for v in box)
    row = torch.as_tensor(row).to(torch.int32)
    m = _bits_f32(row[6:12]).to(dtype)
    src = pixels_u8[r, :, y0:y0 + h, x0:x0 + w].to(dtype)
    y, x = torch.meshgrid(torch.arange(Hi, dtype=dtype) + 0.5, torch.arange(Wi, dtype=dtype) + 0.5, indexing="ij")
    u = m[0] * x + m[1] * y + m[2]
    v = m[3] * x + m[4] * y + m[5]
    inside = (u >= 0) & (u < Wi) & (v >= 0) & (v < Hi)
    uf = Wi - u if flip else u

    def axis(t, n_box, n_out):
        s = (t * n_box / n_out - 0.5).clamp(min=0)
        s = torch.where(inside, s, torch.zeros_like(s))
        i0 = s.to(torch.int64).clamp(max=n_box - 1)
        return i0, (i0 + 1).clamp(max=n_box - 1), s - i0.to(dtype)
    ix0, ix1, fx = axis(uf, w, Wi)
    iy0, iy1, fy = axis(v, h, Hi)
    top = (1 - fx) * src[:, iy0, ix0] + fx * src[:, iy0, ix1]
    bot = (1 - fx) * src[:, iy1, ix0] + fx * src[:, iy1, ix1]
    val = (1 - fy) * top + fy * bot
    fill = int(row[12])
    fills = torch.tensor([(fill >> 16) & 255, (fill >> 8) & 255, fill & 255], dtype=dtype).view(3, 1, 1)
    return torch.where(inside[None], val, fills.expand_as(val))


def ra_reference(pixels_u8: torch.Tensor, rows, boxes, mix, aug, ra, size, dtype=torch.float64, parts: bool = False):
    """What ``cara_im2col_patches_u8_rows_ra`` computes before its one rounding to 16 bits, in torch / numpy ops on the CPU: the
    NORMALISED image [B,3,Hi,Wi] of ``dtype``.  Per sample ``ra_geometry_reference``; where the row has a lookup slot, ``rint`` (half to
    even) and ``ra_lookup_reference``; then ``color_chain_reference`` with the ``aug`` row (``aug`` None: none), the mix (``mix`` None:
    none), the normalisation and the erase of ``aug_reference``.  ``parts``: also the unquantised geometry values and the statistic
    tables, ``(out, geometry [B,3,Hi,Wi], [tables or None] * B)``."""
    Hi, Wi = (size, size) if isinstance(size, int) else size
    rows = torch.as_tensor(rows).cpu()
    B = len(rows)
    px = pixels_u8.cpu()
    if boxes is None:
        if tuple(px.shape[2:]) != (Hi, Wi):
            raise ValueError("without boxes the split must have the output's size")
        boxes = torch.tensor([[0, 0, Wi, Hi, 0]] * B, dtype=torch.int32)
    boxes = torch.as_tensor(boxes).cpu()
    mix = identity_mix(B) if mix is None else torch.as_tensor(mix).cpu()
    aug = identity_aug(B) if aug is None else torch.as_tensor(aug).cpu()
    ra = torch.as_tensor(ra).cpu()
    check_boxes(boxes, px.shape[2], px.shape[3])
    check_mix(mix, B, Hi, Wi)
    check_aug(aug, B, Hi, Wi)
    check_ra(ra, B)
    if px.shape[1] != 3:
        raise ValueError("the RandAugment ops are defined on three channels")
    geo = torch.stack([ra_geometry_reference(px, int(rows[i]), boxes[i].tolist(), ra[i], Hi, Wi, dtype) for i in range(B)])
    y, tables = [], []
    for i in range(B):
        v, t = geo[i], None
        if bool((ra[i, 0:6:2] != 0).any()):
            q, t = ra_lookup_reference(torch.round(v).clamp(0, 255).to(torch.int64).numpy(), ra[i].tolist())
            v = torch.from_numpy(q).to(dtype)
        tables.append(t)
        y.append(color_chain_reference(v, aug[i]))
    out = _mix_normalize_erase(torch.stack(y), mix, aug, Hi, Wi, dtype)
    return (out, geo, tables) if parts else out


def keep_seed(seed: int, epoch: int, rank: int) -> int:
    """``box_seed`` of the stream that draws the patch-dropout tables (a fourth constant)"""
    return box_seed(seed, epoch, rank, stream=0x5BD1E995)


def identity_keep(B: int, P: int, steps: Optional[int] = None) -> torch.Tensor:
    """int32 [B, P] (or [steps, B, P]) table that keeps every patch in its place"""
    t = torch.arange(P, dtype=torch.int32).expand(B, P).contiguous()
    return t if steps is None else t.expand(steps, B, P).contiguous()


class PatchDropout:
    """Keep tables for a patch dropout: the published definition of timm's ``PatchDropout`` (the FLIP trick), restated (timm is
    not installed).  On a grid of ``P`` patches ``K = max(1, int(P * (1 - prob)))`` are kept per sample: each sample independently
    keeps the first ``K`` entries of ``argsort(randn(P))``, sorted ascending with ``ordered=True`` (timm's default is unordered).
    The kept tokens are gathered behind the position embedding, so token ``1 + j`` of sample ``b`` is patch ``keep[b][j]`` with
    ITS row of ``pos_embed``; the cls token stays.  Training steps only: an evaluation sees every patch.
    ``size`` / ``patch`` (optional): the model's input and patch size, from which ``grid`` = P follows -- what ``train_rows`` and
    ``recipe.fit`` ask for, in the way ``MixupCutmix`` carries ``Hi`` / ``Wi``; or pass ``grid=`` itself."""

    def __init__(self, prob: float, ordered: bool = False, size=None, patch: int = 16, grid: Optional[int] = None):
        if not isinstance(prob, (int, float)) or not (0.0 <= prob < 1.0):   # (a NaN fails the comparison)
            raise ValueError("PatchDropout: prob must be a number in [0, 1)")
        self.prob, self.ordered = float(prob), bool(ordered)
        if grid is None and size is not None:
            Hi, Wi = (size, size) if isinstance(size, int) else size
            if int(patch) <= 0 or int(Hi) <= 0 or int(Wi) <= 0 or Hi % patch or Wi % patch:
                raise ValueError("PatchDropout: size must be a positive multiple of patch")
            grid = (int(Hi) // int(patch)) * (int(Wi) // int(patch))
        if grid is not None and int(grid) < 1:
            raise ValueError("PatchDropout: grid must be >= 1")
        self.grid = None if grid is None else int(grid)

    def num_keep(self, P: int) -> int:
        return max(1, int(P * (1.0 - self.prob)))

    def draw(self, P: int, B: int, steps: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """int32 [steps, B, K] on the host, from one ``randn`` of ``generator`` for the whole table"""
        K = self.num_keep(P)
        noise = torch.randn(steps * B * P, generator=generator).reshape(steps, B, P)
        keep = torch.argsort(noise, dim=-1)[..., :K]
        if self.ordered:
            keep = keep.sort(dim=-1).values
        return keep.to(torch.int32).contiguous()


def check_keep(keep: torch.Tensor, B: int, P: int) -> None:
    """ValueError unless ``keep`` is an int32 [..., B, K] table, 1 <= K <= P, whose every entry is in [0, P) and whose rows hold no
    patch twice (the companion of ``check_boxes``; the device checks the range only)"""
    if not torch.is_tensor(keep) or keep.dtype != torch.int32 or keep.ndim < 2 or keep.shape[-2] != B or not (1 <= keep.shape[-1] <= P):
        raise ValueError(f"keep must be an int32 [..., batch, K] tensor of patch indices, batch = {B}, 1 <= K <= {P}")
    t = keep.reshape(-1, keep.shape[-1]).cpu().to(torch.int64)
    bad = (t < 0) | (t >= P)
    if bool(bad.any()):
        raise ValueError(f"{int(bad.sum())} keep entry(ies) outside [0, {P}), the first: {int(t[bad][0])}")
    s = t.sort(dim=-1).values
    dup = (s[:, 1:] == s[:, :-1]).any(dim=-1)
    if bool(dup.any()):
        i = int(dup.to(torch.int64).argmax())
        raise ValueError(f"{int(dup.sum())} keep row(s) hold a patch twice, the first: {t[i].tolist()}")


def keep_reference(tokens_or_rows: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """Host gather for the tests: ``tokens_or_rows`` [B, P, ...] (patch rows, or patch tokens with their positions added) ->
    [B, K, ...], entry ``[b, j]`` = ``tokens_or_rows[b, keep[b][j]]``"""
    idx = keep.to(tokens_or_rows.device, torch.int64)
    B, K = idx.shape
    return tokens_or_rows[torch.arange(B, device=idx.device).reshape(B, 1).expand(B, K), idx]


class _Drawer(NamedTuple):
    """what ``ResidentSplit.train_rows`` knows of one of its table drawers"""
    arg: str                    # train_rows' argument
    field: str                  # the Feed field its table fills
    attrs: Optional[tuple]      # the int attributes that, with a callable ``draw``, make an object such a drawer (None: not asked)
    refusal: str                # ... and what anything else is told
    seed: Callable              # (seed, epoch, rank) -> the seed of its generator: every drawer has a stream of its own
    draw: Callable              # (drawer, Hs, Ws, steps, B, generator) -> its host table for an epoch of steps x B samples
    width: object               # the columns of that int32 [steps, B, columns] table ("K": the drawer's own)
    check: Callable             # (table, drawer, Hs, Ws, B): raises on an entry the kernel would refuse


# in the order they draw
_DRAWERS = (
    _Drawer("patch_drop", "keep", ("grid",), "patch_drop must be a PatchDropout with its grid (PatchDropout(prob, size=, patch=) or grid=)",
            keep_seed, lambda d, Hs, Ws, steps, B, g: d.draw(d.grid, B, steps, g), "K",
            lambda t, d, Hs, Ws, B: check_keep(t, B, d.grid)),
    _Drawer("augment", "boxes", None, "", box_seed, lambda d, Hs, Ws, steps, B, g: d.draw(Hs, Ws, steps * B, g).reshape(steps, B, 5), 5,
            lambda t, d, Hs, Ws, B: check_boxes(t, Hs, Ws)),
    _Drawer("mix", "mix", ("Hi", "Wi"), "mix must be a MixupCutmix (anything with draw(B, steps, generator), Hi and Wi)",
            mix_seed, lambda d, Hs, Ws, steps, B, g: d.draw(B, steps, g), 8, lambda t, d, Hs, Ws, B: check_mix(t, B, d.Hi, d.Wi)),
    _Drawer("color", "aug", ("Hi", "Wi"), "color must be a ColorJitterErase (anything with draw(B, steps, generator), Hi and Wi)",
            aug_seed, lambda d, Hs, Ws, steps, B, g: d.draw(B, steps, g), 16, lambda t, d, Hs, Ws, B: check_aug(t, B, d.Hi, d.Wi)),
    # (its draw gives a pair: the table and the int32 [steps, B, 6] jitter slots that replace aug's)
    _Drawer("rand", "ra", ("Hi", "Wi"), "rand must be a RandAugment (anything with draw(B, steps, generator), Hi and Wi)",
            ra_seed, lambda d, Hs, Ws, steps, B, g: d.draw(B, steps, g), 16, lambda t, d, Hs, Ws, B: check_ra(t, B)),
)


class ResidentSplit:
    """One file list decoded once and kept on ``device`` as the resized uint8 pixels ``pixels`` [N,3,size,size]
    (150 KB per image: the 73k-image dsprites test split is 11 GB, not 44) plus ``labels`` int64 [N]; a batch is
    normalised to fp32 when it is drawn.  The split is decoded and uploaded in chunks, so the host never holds more
    than one chunk.  ``len()`` and ``[i]`` behave like the reference's ``ImageFilelist``."""

    def __init__(self, root: str, flist: str, device="cuda", size: int = 224, workers: int = 8, chunk: int = 2048):
        self.root, self.imlist = root, read_filelist(flist)
        paths = [os.path.join(root, p) for p, _ in self.imlist]
        self.pixels = torch.empty(len(paths), 3, size, size, dtype=torch.uint8, device=device)
        for c0 in range(0, len(paths), chunk):
            part = paths[c0:c0 + chunk]
            if workers > 1 and len(part) > 1:
                with ThreadPoolExecutor(max_workers=workers) as ex:   # PIL releases the GIL while decoding/resizing
                    decoded = list(ex.map(lambda p: decode_image_u8(p, size), part))
            else:
                decoded = [decode_image_u8(p, size) for p in part]
            self.pixels[c0:c0 + len(part)].copy_(torch.stack(decoded))
        self.labels = torch.tensor([l for _, l in self.imlist], dtype=torch.int64, device=device)

    @classmethod
    def from_tensors(cls, pixels: torch.Tensor, labels: torch.Tensor) -> "ResidentSplit":
        """A split over pixels that are resident already: uint8 [N,3,size,size] and int64 [N] on one device (synthetic
        splits of tests and tools; nothing is decoded, ``imlist`` holds empty paths)."""
        if pixels.dtype != torch.uint8 or pixels.ndim != 4 or labels.dtype != torch.int64 or labels.shape != pixels.shape[:1]:
            raise ValueError("from_tensors takes uint8 [N,C,H,W] pixels and int64 [N] labels")
        self = cls.__new__(cls)
        self.root, self.pixels, self.labels = "", pixels.contiguous(), labels.to(pixels.device)
        self.imlist = [("", int(l)) for l in labels.tolist()]
        return self

    @property
    def images(self) -> torch.Tensor:
        """The whole split normalised, fp32 [N,3,size,size] (materialised: for small splits and tests)."""
        return normalize_u8(self.pixels)

    def __len__(self) -> int:
        return len(self.imlist)

    def __getitem__(self, i: int):
        return normalize_u8(self.pixels[i]), int(self.labels[i])

    # ---- loaders -----------------------------------------------------------------------------------
    def train_batches(self, batch_size: int = 64, seed: int = 0, rank: Optional[int] = None,
                      world: Optional[int] = None) -> Callable[[int], Iterator[Tuple[torch.Tensor, torch.Tensor]]]:
        """``f(epoch)`` -> iterator of (images, labels) on the device: shuffle + drop_last per rank
        (vtab.py:84-88), rank-strided shard of one epoch-seeded permutation under data parallelism.
        The shape ``recipe.fit`` expects for ``train_batches``."""
        rank = D.get_rank() if rank is None else rank
        world = D.world_size() if world is None else world

        def epoch_iter(epoch: int):
            for idx in D.epoch_shard(len(self), epoch, rank, world, batch_size, seed):
                idx = idx.to(self.pixels.device)
                yield normalize_u8(self.pixels.index_select(0, idx)), self.labels.index_select(0, idx)
        return epoch_iter

    def train_rows(self, batch_size: int = 64, seed: int = 0, rank: Optional[int] = None,
                   world: Optional[int] = None, augment=None, mix=None, color=None,
                   patch_drop=None, rand=None) -> Callable[[int], Iterator[torch.Tensor]]:
        """``f(epoch)`` -> iterator of int64 [batch_size] index vectors on the device: the indices ``train_batches`` draws
        (``dist.epoch_shard``), in the same order, for ``CaraEngine.train_step_resident`` -- which reads the uint8 pixels
        and the labels of those rows itself, so no fp32 batch is written.  An epoch's indices are range-checked on the host
        and uploaded once as one [steps, batch_size] tensor; every step gets a row view of it.
        With a drawer, the iterator yields ``Feed(rows, boxes, mix, aug, keep, ra).item()`` instead: the tuple cut behind the last table
        asked for, None for one in front of it that is not (``cara_amd.feed``).  Every table is an int32 [batch_size, columns] view of
        one [steps, batch_size, columns] upload per epoch, drawn on the host from a generator seeded by (seed, epoch, rank) on a
        stream of its drawer's own and checked before the upload, like the indices:
        ``augment`` (a ``RandomResizedCropFlip``, or anything with its ``draw``) -> ``boxes``, 5 columns (``box_seed``, ``check_boxes``);
        ``mix`` (a ``MixupCutmix``, or anything with its ``draw``, ``Hi`` and ``Wi``) -> ``mix``, 8 columns (``mix_seed``, ``check_mix``);
        ``color`` (a ``ColorJitterErase``, or anything with its ``draw``, ``Hi`` and ``Wi``) -> ``aug``, 16 columns (``aug_seed``, ``check_aug``);
        ``patch_drop`` (a ``PatchDropout`` that knows its ``grid``, or anything with its ``draw`` and ``grid``) -> ``keep``, K columns
        (``keep_seed``, ``check_keep``);
        ``rand`` (a ``RandAugment``, or anything with its ``draw``, ``Hi`` and ``Wi``) -> ``ra``, 16 columns (``ra_seed``, ``check_ra``), and
        an ``aug`` that carries the jitter slots ``rand`` drew (``check_aug``).  With ``color`` too, ``color`` must only erase (its three
        jitters 0): as in timm, auto-augment replaces colour jitter."""
        drawers = {"augment": augment, "mix": mix, "color": color, "patch_drop": patch_drop, "rand": rand}
        for s in sorted(_DRAWERS, key=lambda s: Feed._fields.index(s.field), reverse=True):   # (the last table's drawer first)
            d = drawers[s.arg]
            if d is not None and s.attrs is not None and not (callable(getattr(d, "draw", None))
                                                              and all(isinstance(getattr(d, a, None), int) for a in s.attrs)):
                raise ValueError(s.refusal)
            if s.arg == "rand" and d is not None and color is not None and any(float(j) != 0.0 for j in getattr(color, "jitter", (1.0,))):
                raise ValueError("rand replaces colour jitter: pass a color that only erases (brightness = contrast = saturation = 0)")
        rank = D.get_rank() if rank is None else rank
        world = D.world_size() if world is None else world

        def epoch_iter(epoch: int):
            idx = D.epoch_shard(len(self), epoch, rank, world, batch_size, seed)
            if not idx:
                return
            table = torch.stack(idx)
            if int(table.min()) < 0 or int(table.max()) >= len(self):
                raise ValueError(f"epoch {epoch}: a drawn index is outside [0, {len(self)})")
            (steps, B), (Hs, Ws) = table.shape, self.pixels.shape[2:]
            host = {}
            for s in _DRAWERS:
                d = drawers[s.arg]
                if d is None:
                    continue
                t = s.draw(d, Hs, Ws, steps, B, torch.Generator().manual_seed(s.seed(seed, epoch, rank)))
                t, slots = t if s.field == "ra" else (t, None)
                if not torch.is_tensor(t) or t.ndim != 3 or tuple(t.shape[:2]) != (steps, B) or s.width not in ("K", t.shape[2]) \
                        or (s.field == "ra" and (not torch.is_tensor(slots) or tuple(slots.shape) != (steps, B, 6))):
                    raise ValueError(f"rand.draw did not give an int32 {(steps, B, 16)} table and int32 {(steps, B, 6)} jitter slots"
                                     if s.field == "ra" else
                                     f"{s.arg}.draw gave {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}, "
                                     f"not an int32 {(steps, B, s.width)} table")
                s.check(t, d, Hs, Ws, B)
                host[s.field] = t
                if slots is not None:   # (as in timm, auto-augment replaces colour jitter: aug keeps its erase columns only)
                    host["aug"] = host["aug"].clone() if "aug" in host else identity_aug(B, steps)
                    host["aug"][..., :6] = slots
                    check_aug(host["aug"], B, d.Hi, d.Wi)
            dev = {n: t.contiguous().to(self.pixels.device) for n, t in host.items()}
            table = table.to(self.pixels.device)
            for step in range(steps):
                yield Feed(table[step], **{n: t[step] for n, t in dev.items()}).item()
        return epoch_iter

    def eval_batches(self, batch_size: int = 256) -> Callable[[], Iterator[Tuple[torch.Tensor, torch.Tensor]]]:
        """In file order, last batch partial (vtab.py:96-100: shuffle False, no drop_last)."""
        def it():
            for i in range(0, len(self), batch_size):
                yield normalize_u8(self.pixels[i:i + batch_size]), self.labels[i:i + batch_size]
        return it

    def eval_shard(self, batch_size: int = 256, rank: Optional[int] = None,
                   world: Optional[int] = None) -> Iterator[Tuple[torch.Tensor, torch.Tensor, int]]:
        """This rank's part of the split (``dist.eval_shard``: contiguous, file order) as ``(pixels_u8, labels, n_valid)``:
        the resident uint8 pixels themselves, not normalised -- ``CaraEngine.evaluate`` hands them to the uint8 forward.
        Every batch has ``batch_size`` rows: the last one of a shard is padded (with copies of its first row and label)
        and says so in ``n_valid``, so a pass uses one batch shape and one workspace."""
        rank = D.get_rank() if rank is None else rank
        world = D.world_size() if world is None else world
        mine = D.eval_shard(len(self), rank, world, batch_size)
        for i in range(mine.start, mine.stop, batch_size):
            j = min(i + batch_size, mine.stop)
            px, y = self.pixels[i:j], self.labels[i:j]
            if j - i < batch_size:
                pad = batch_size - (j - i)
                px = torch.cat([px, px[:1].expand(pad, -1, -1, -1)])
                y = torch.cat([y, y[:1].expand(pad)])
            yield px, y, j - i

    def eval_view_shard(self, views_table: torch.Tensor, batch_size: int = 256, rank: Optional[int] = None,
                        world: Optional[int] = None) -> Iterator[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]]:
        """This rank's part of the split (``dist.eval_shard``) seen through the V views of ``views_table`` (host int32 [V, 5],
        ``EvalViews.table``), by index: ``(rows int64 [S*V], boxes int32 [S*V, 5], labels int64 [S], n_valid_samples)`` with
        ``S = batch_size // V`` whole samples per batch and view ``v`` of sample ``s`` in row ``s*V + v`` -- what
        ``cara_vit_forward_u8_rows_crop`` and ``cara_eval_combine_views`` read.  Every batch has the same shape: the last one of a
        shard is padded with copies of its first sample and says so in ``n_valid``.  ``rows`` and ``labels`` are built on the
        device, ``boxes`` is ONE device tensor uploaded before the first batch and yielded every time: no host upload per batch.
        The table is checked against the split's size, and ``V <= batch_size``, here -- before the first batch exists."""
        check_views(views_table, *self.pixels.shape[2:])
        V = int(views_table.shape[0])
        S = int(batch_size) // V
        if S < 1:
            raise ValueError(f"batch_size {batch_size} holds no whole sample of {V} views")
        rank = D.get_rank() if rank is None else rank
        world = D.world_size() if world is None else world
        mine = D.eval_shard(len(self), rank, world, S)
        dev = self.pixels.device

        def batches():
            boxes = views_table.repeat(S, 1).contiguous().to(dev)
            for i in range(mine.start, mine.stop, S):
                j = min(i + S, mine.stop)
                idx = torch.arange(i, i + S, dtype=torch.int64, device=dev)
                if j - i < S:
                    idx = torch.where(idx < j, idx, torch.full_like(idx, i))
                yield idx.repeat_interleave(V), boxes, self.labels.index_select(0, idx), j - i
        return batches()


def get_data(name: str, evaluate: bool = True, batch_size: int = 64, root: Optional[str] = None, device="cuda",
             seed: int = 0, workers: int = 8, shard_eval: bool = False, resident_feed: bool = False, augment=None,
             train_size: Optional[int] = None, mix=None, color=None, patch_drop=None, rand=None, test_size: Optional[int] = None):
    """Drop-in for ``vtab.get_data`` (vtab.py:88-107): the same split files -- ``train800val200.txt`` /
    ``test.txt`` when ``evaluate`` else ``train800.txt`` / ``val200.txt`` -- under ``./data/vtab-1k/<name>``.
    Returns (train_batches, test_batches) in the form ``recipe.fit`` takes instead of two DataLoaders.
    ``shard_eval = True``: the second value is the test ``ResidentSplit`` itself, the form ``fit(eval_mode="sharded")`` and
    ``CaraEngine.evaluate`` take (every rank then scores its own part, ``ResidentSplit.eval_shard``).
    ``resident_feed = True``: the first value is ``(train split, its train_rows(batch_size, seed=seed))``, the form
    ``fit(feed="resident")`` takes: the steps read the split's uint8 pixels by index instead of a normalised fp32 batch.
    ``augment`` / ``train_size`` (with ``resident_feed``): the training split is decoded at ``train_size`` (default 224, the
    model's size) and its ``train_rows`` yields ``(rows, boxes)`` drawn by ``augment`` -- "resize 256, random-resized-crop
    224" is ``train_size=256, augment=RandomResizedCropFlip(224)``.
    ``test_size`` (with ``shard_eval``): the test split is decoded at that size instead of the model's and read through the crop
    boxes of an ``EvalViews`` -- "resize 256, centre-crop 224" is ``test_size=256`` and ``fit(..., eval_views=EvalViews.center(224))``.
    ``mix`` / ``color`` / ``patch_drop`` / ``rand`` (with ``resident_feed``): handed to ``train_rows``, which then yields tuples."""
    if (augment is not None or train_size is not None or mix is not None or color is not None or patch_drop is not None
            or rand is not None) and not resident_feed:
        raise ValueError("augment / train_size / mix / color / patch_drop / rand belong to the resident feed: pass resident_feed=True")
    if train_size is not None and train_size != 224 and augment is None:
        raise ValueError("a training split of another size than the model's is read through crop boxes: pass augment")
    if test_size is not None and test_size != 224 and not shard_eval:
        raise ValueError("a test split of another size than the model's is read through view boxes: pass shard_eval=True and "
                         "evaluate with views")
    root = root if root is not None else "./data/vtab-1k/" + name
    tr, te = ("train800val200.txt", "test.txt") if evaluate else ("train800.txt", "val200.txt")
    train = ResidentSplit(root, os.path.join(root, tr), device=device, workers=workers, size=224 if train_size is None else train_size)
    test = ResidentSplit(root, os.path.join(root, te), device=device, workers=workers, size=224 if test_size is None else test_size)
    if resident_feed:
        feed = (train, train.train_rows(batch_size, seed=seed, augment=augment, mix=mix, color=color, patch_drop=patch_drop, rand=rand))
    else:
        feed = train.train_batches(batch_size, seed=seed)
    return feed, (test if shard_eval else test.eval_batches(256))
