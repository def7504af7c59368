"""Host side of the augmented resident feed: the sampling oracle of the GPU tests against torch's own bilinear resize, the
box draw (RandomResizedCropFlip), ResidentSplit.train_rows with and without an augment, and the refusals.  CPU only."""
import math

import pytest
import torch
import torch.nn.functional as F

from cara_amd import dist as D
from cara_amd._lib import CaraError
from cara_amd.data import RandomResizedCropFlip, ResidentSplit, box_seed, check_boxes, resized_crop_reference

HS, WS = 40, 52
N, BATCH = 37, 8


def _image():
    return torch.randint(0, 256, (1, 3, HS, WS), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)


# full image, same size at an offset, 1x1, touching the bottom-right corner, w != h
BOXES = [(0, 0, WS, HS), (7, 5, 32, 32), (20, 11, 1, 1), (WS - 17, HS - 9, 17, 9), (3, 2, 45, 13)]


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("size", [32, (24, 48)])
def test_reference_is_torch_bilinear_resize_of_the_crop_then_flip(size, flip):
    px = _image()
    boxes = torch.tensor([b + (flip,) for b in BOXES], dtype=torch.int32)
    got = resized_crop_reference(px, [0] * len(BOXES), boxes, size)
    out = (size, size) if isinstance(size, int) else size
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(BOXES), 3) + out
    for i, (x0, y0, w, h) in enumerate(BOXES):
        crop = px[:, :, y0:y0 + h, x0:x0 + w].to(torch.float64)
        want = F.interpolate(crop, size=out, mode="bilinear", align_corners=False, antialias=False)[0]
        if flip:
            want = torch.flip(want, dims=[2])
        err = ((got[i] - want).abs() / want.abs().clamp(min=1.0)).max().item()
        assert err <= 1e-12, (BOXES[i], err)
    # a box of the output's size is the bytes themselves; a 1x1 box a constant image
    same = resized_crop_reference(px, [0], torch.tensor([[2, 5, out[1], out[0], flip]], dtype=torch.int32), size)[0]
    want = px[0, :, 5:5 + out[0], 2:2 + out[1]].to(torch.float64)
    assert torch.equal(same, torch.flip(want, dims=[2]) if flip else want)
    assert torch.equal(got[2], px[0, :, 11, 20].to(torch.float64).view(3, 1, 1).expand(3, *out))


@pytest.mark.parametrize("Hs,Ws", [(HS, WS), (256, 256)])
def test_draw_gives_boxes_inside_the_source_within_the_bounds(Hs, Ws):
    aug = RandomResizedCropFlip(224)
    n = 4096
    boxes = aug.draw(Hs, Ws, n, torch.Generator().manual_seed(1))
    assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (n, 5) and boxes.is_contiguous()
    check_boxes(boxes, Hs, Ws)
    x0, y0, w, h, flip = boxes.to(torch.float64).unbind(1)
    assert bool(((x0 >= 0) & (y0 >= 0) & (w >= 1) & (h >= 1) & (x0 + w <= Ws) & (y0 + h <= Hs)).all())
    # rounding w and h to integers moves each by at most 0.5: the bounds on area share and ratio, widened by exactly that
    area_lo, area_hi = (w - 0.5).clamp(min=0) * (h - 0.5).clamp(min=0), (w + 0.5) * (h + 0.5)
    assert bool((area_hi >= 0.08 * Hs * Ws).all()) and bool((area_lo <= 1.0 * Hs * Ws).all())
    assert bool(((w + 0.5) / (h - 0.5).clamp(min=1e-9) >= 3 / 4).all()) and bool(((w - 0.5) / (h + 0.5) <= 4 / 3).all())
    assert set(flip.tolist()) == {0.0, 1.0}
    assert abs(flip.sum().item() - n / 2) <= 4 * math.sqrt(n * 0.25)       # 4 sigma of a fair coin over n draws
    # the offsets use the room they have, and the boxes vary
    assert len({tuple(b) for b in boxes[:, :4].tolist()}) > n // 2
    # deterministic given the generator; another seed gives another table
    assert torch.equal(boxes, aug.draw(Hs, Ws, n, torch.Generator().manual_seed(1)))
    assert not torch.equal(boxes, aug.draw(Hs, Ws, n, torch.Generator().manual_seed(2)))
    # flip = 0 / 1 are respected
    assert not RandomResizedCropFlip(224, flip=0.0).draw(Hs, Ws, 64, torch.Generator().manual_seed(3))[:, 4].any()
    assert RandomResizedCropFlip(224, flip=1.0).draw(Hs, Ws, 64, torch.Generator().manual_seed(3))[:, 4].all()


def test_draw_falls_back_to_the_clamped_centre_crop():
    """ratio 3 at the whole image's area: w = round(sqrt(40 * 52 * 3)) = 79 > 52 in every try, so all ten fail; the source's
    own ratio 1.3 is below the bound, so the fallback is the full width and h = round(52 / 3) = 17, centred"""
    scale, ratio = (1.0, 1.0), (3.0, 3.0)
    w_try = round(math.sqrt(HS * WS * scale[0] * ratio[0]))
    assert w_try == 79 and w_try > WS                                    # no try can be accepted: area and ratio are constants
    boxes = RandomResizedCropFlip(32, scale=scale, ratio=ratio).draw(HS, WS, 50, torch.Generator().manual_seed(0))
    assert boxes[:, :4].tolist() == [[0, (HS - 17) // 2, WS, 17]] * 50
    check_boxes(boxes, HS, WS)
    # the other side: ratio 1/3 on the same source -> full height, w = round(40 / 3) = 13
    boxes = RandomResizedCropFlip(32, scale=(1.0, 1.0), ratio=(1 / 3, 1 / 3)).draw(HS, WS, 5, torch.Generator().manual_seed(0))
    assert round(math.sqrt(HS * WS * 3)) > HS
    assert boxes[:, :4].tolist() == [[(WS - 13) // 2, 0, 13, HS]] * 5
    # an area above the image with a ratio the image has: the whole image
    boxes = RandomResizedCropFlip(32, scale=(2.0, 2.0), ratio=(1.0, 1.0)).draw(48, 48, 5, torch.Generator().manual_seed(0))
    assert boxes[:, :4].tolist() == [[0, 0, 48, 48]] * 5


def _split(Hs=8, Ws=8):
    px = (torch.arange(N, dtype=torch.uint8) + 1).reshape(N, 1, 1, 1).expand(N, 3, Hs, Ws).contiguous()
    return ResidentSplit.from_tensors(px, torch.arange(N) + 100)


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_train_rows_with_and_without_an_augment(rank, world):
    split = _split(HS, WS)
    aug = RandomResizedCropFlip(32)
    tables = {}
    for epoch in range(2):
        shard = D.epoch_shard(N, epoch, rank, world, BATCH, 3)
        plain = list(split.train_rows(BATCH, seed=3, rank=rank, world=world, augment=None)(epoch))
        assert len(plain) == len(shard) >= 2
        for rows, idx in zip(plain, shard):
            assert torch.is_tensor(rows) and rows.dtype == torch.int64 and torch.equal(rows, idx)
        got = list(split.train_rows(BATCH, seed=3, rank=rank, world=world, augment=aug)(epoch))
        assert len(got) == len(shard)
        for (rows, boxes), idx in zip(got, shard):
            assert torch.equal(rows, idx) and rows.is_contiguous()
            assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (BATCH, 5) and boxes.is_contiguous()
        # one upload each per epoch: every step's tensors are views of one index table and one box table
        assert len({r.untyped_storage().data_ptr() for r, _ in got}) == 1 and len({b.untyped_storage().data_ptr() for _, b in got}) == 1
        assert [b.storage_offset() for _, b in got] == [i * BATCH * 5 for i in range(len(got))]
        table = torch.stack([b for _, b in got])
        check_boxes(table, HS, WS)
        # the table is the draw of the generator seeded by (seed, epoch, rank)
        want = aug.draw(HS, WS, len(got) * BATCH, torch.Generator().manual_seed(box_seed(3, epoch, rank)))
        assert torch.equal(table.reshape(-1, 5), want)
        tables[epoch] = table
    assert not torch.equal(tables[0], tables[1])
    other_seed = torch.stack([b for _, b in split.train_rows(BATCH, seed=4, rank=rank, world=world, augment=aug)(0)])
    other_rank = torch.stack([b for _, b in split.train_rows(BATCH, seed=3, rank=rank + 2, world=world + 2, augment=aug)(0)])
    assert not torch.equal(other_seed, tables[0])
    assert not torch.equal(other_rank[:1], tables[0][:1])
    assert len({box_seed(s, e, r) for s in (0, 3, 4) for e in (0, 1, 99) for r in (0, 1, 7)}) == 27


def test_a_box_outside_the_source_is_refused_before_upload():
    split = _split(HS, WS)

    class OneBad:
        def draw(self, Hs, Ws, n, generator):
            boxes = torch.tensor([[0, 0, Ws, Hs, 0]] * n, dtype=torch.int32)
            boxes[n // 2] = torch.tensor([Ws - 3, 0, 4, 4, 1], dtype=torch.int32)       # one pixel past the right edge
            return boxes
    with pytest.raises(ValueError, match="outside the 40 x 52 source"):
        next(split.train_rows(BATCH, augment=OneBad())(0))
    for bad in ([-1, 0, 4, 4, 0], [0, -1, 4, 4, 0], [0, 0, 0, 4, 0], [0, 0, 4, 0, 0], [0, HS - 3, 4, 4, 0], [0, 0, WS + 1, 4, 0]):
        with pytest.raises(ValueError, match="outside"):
            check_boxes(torch.tensor([[0, 0, WS, HS, 0], bad], dtype=torch.int32), HS, WS)
    with pytest.raises(ValueError, match="int32"):
        check_boxes(torch.zeros(2, 5), HS, WS)
    with pytest.raises(ValueError, match="int32"):
        check_boxes(torch.zeros(2, 4, dtype=torch.int32), HS, WS)
    check_boxes(torch.tensor([[WS - 1, HS - 1, 1, 1, 7]], dtype=torch.int32), HS, WS)


def test_step_and_fit_refuse_boxes_that_are_no_box_table():
    from cara_amd import cara, create_model
    from cara_amd.recipe import fit
    m = create_model("vit_base_patch16_224_in21k", drop_path_rate=0.0, depth=1, img_size=32, num_classes=10)
    m = cara({"model": m, "rank": 4, "scale": 0.1, "l_mu": 1.5, "l_std": 0.1})
    split = ResidentSplit.from_tensors(torch.zeros(6, 3, 48, 48, dtype=torch.uint8), torch.arange(6))
    rows = torch.arange(4)
    good = torch.tensor([[0, 0, 32, 32, 0]] * 4, dtype=torch.int32)
    for boxes in (good.float(), good.to(torch.int64), good[:, :4].contiguous(), good.reshape(-1), good.t(), good.tolist()):
        with pytest.raises(CaraError, match="boxes must be"):
            m._cara_engine.train_step_resident(split, rows, None, boxes=boxes)
        with pytest.raises(CaraError, match="boxes must be"):
            m._cara_engine.forward_resident(split, rows, boxes=boxes)
        with pytest.raises(CaraError, match="boxes must be"):
            fit(m, (split, lambda epoch, boxes=boxes: iter([(rows, boxes)])), None, epochs=1, feed="resident")


def test_get_data_passes_the_augment_and_the_training_size_on(tmp_path):
    import os

    from PIL import Image

    from cara_amd.data import get_data, normalize_u8
    root = str(tmp_path)
    g = torch.Generator().manual_seed(0)
    for name, n in (("train800val200.txt", 5), ("test.txt", 3)):
        with open(os.path.join(root, name), "w") as fh:
            for i in range(n):
                fn = f"{name[:2]}{i}.png"
                Image.fromarray(torch.randint(0, 256, (12, 10, 3), generator=g, dtype=torch.uint8).numpy()).save(os.path.join(root, fn))
                fh.write(f"{fn} {i % 3}\n")
    kw = dict(batch_size=2, root=root, device="cpu", seed=1, workers=1)
    (plain, plain_rows), _ = get_data("cifar", resident_feed=True, augment=None, train_size=None, **kw)
    (split, rows_of), test = get_data("cifar", resident_feed=True, augment=RandomResizedCropFlip(224), train_size=256, **kw)
    assert tuple(plain.pixels.shape) == (5, 3, 224, 224) and tuple(split.pixels.shape) == (5, 3, 256, 256) and callable(test)
    ep, ep_plain = list(rows_of(0)), list(plain_rows(0))
    assert len(ep) == len(ep_plain) == 2
    for (rows, boxes), want in zip(ep, ep_plain):
        assert torch.is_tensor(want) and torch.equal(rows, want) and tuple(boxes.shape) == (2, 5)
    (tx, ty), = list(test())
    assert tuple(tx.shape) == (3, 3, 224, 224)                          # the test split keeps the model's size
    with pytest.raises(ValueError, match="resident"):
        get_data("cifar", augment=RandomResizedCropFlip(224), **kw)
    with pytest.raises(ValueError, match="augment"):
        get_data("cifar", resident_feed=True, train_size=256, **kw)
    assert normalize_u8(split.pixels[:1]).shape == (1, 3, 256, 256)
