"""Host side of the mixed resident feed: the definitions (data.soft_target against torch's label_smoothing, data.mix_reference
against x (1 - m) + x.flip(0) m and the pasted rectangle), the table draw (data.MixupCutmix), data.check_mix, that the loss bound
of tests/mix_model.py is neither vacuous nor wrong, ResidentSplit.train_rows(mix=) and the refusals.  CPU only."""
import math

import pytest
import torch
import torch.nn.functional as F

from cara_amd._lib import CaraError
from cara_amd.data import (MixupCutmix, RandomResizedCropFlip, ResidentSplit, box_seed, check_mix, identity_mix, mix_reference,
                           mix_seed, resized_crop_reference, soft_target)
from oracle import small_kernels as K
from tests import mix_model as M
from tests import small_kernels_common as S

HS, WS, OUT = 40, 52, 32


def bits(x):
    return int(torch.tensor(x, dtype=torch.float32).view(torch.int32))


def table(rows):
    """int32 [B, 8] from rows (partner, cx0, cy0, cw, ch, m, t)"""
    return torch.tensor([[p, x, y, w, h, bits(m), bits(t), 0] for p, x, y, w, h, m, t in rows], dtype=torch.int32)


# ---- definitions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_soft_target_without_a_partner_is_torchs_label_smoothing(eps):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(7, 13, generator=g, dtype=torch.float64) * 3
    y = torch.randint(0, 13, (7,), generator=g)
    for mix in (None, table([(6 - i, 0, 0, 0, 0, 0.0, 0.0) for i in range(7)])):
        q = soft_target(y, mix, 13, eps)
        assert q.dtype == torch.float64 and torch.allclose(q.sum(1), torch.ones(7, dtype=torch.float64), atol=1e-15)
        got = -(q * F.log_softmax(logits, 1)).sum(1)
        want = F.cross_entropy(logits, y, label_smoothing=eps, reduction="none")
        assert float((got - want).abs().max()) <= 1e-12


def test_soft_target_without_smoothing_is_the_two_cross_entropies():
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(6, 10, generator=g, dtype=torch.float64) * 3
    y = torch.randint(0, 10, (6,), generator=g)
    t = [0.0, 0.3, 1.0, 0.5, 0.25, 0.75]
    mix = table([(5 - i, 0, 0, 0, 0, 0.0, t[i]) for i in range(6)])
    q = soft_target(y, mix, 10, 0.0)
    got = -(q * F.log_softmax(logits, 1)).sum(1)
    tt = torch.tensor(t, dtype=torch.float32).double()
    want = (1 - tt) * F.cross_entropy(logits, y, reduction="none") + tt * F.cross_entropy(logits, y.flip(0), reduction="none")
    assert float((got - want).abs().max()) <= 1e-12
    # and with both: timm's mixup_target then torch's smoothing
    q = soft_target(y, mix, 10, 0.1)
    want = 0.9 * ((1 - tt)[:, None] * torch.eye(10, dtype=torch.float64)[y] + tt[:, None] * torch.eye(10, dtype=torch.float64)[y.flip(0)]) + 0.01
    assert float((q - want).abs().max()) <= 1e-15


def _pixels():
    return torch.randint(0, 256, (4, 3, HS, WS), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)


ROWS = [2, 0, 3, 2, 1, 0]
BOXES = [(0, 0, WS, HS, 0), (11, 9, 13, 13, 1), (3, 2, 45, 13, 0), (WS - 9, HS - 37, 9, 37, 1), (7, 5, OUT, OUT, 1), (20, 1, 31, 33, 0)]


@pytest.mark.parametrize("m", [0.0, 0.25, 1.0])
def test_mix_reference_with_a_mixup_table_is_the_blend_with_the_flipped_batch(m):
    px, boxes = _pixels(), torch.tensor(BOXES, dtype=torch.int32)
    x = resized_crop_reference(px, ROWS, boxes, OUT)
    got = mix_reference(px, ROWS, boxes, table([(5 - i, 0, 0, 0, 0, m, m) for i in range(6)]), OUT)
    mm = float(torch.tensor(m, dtype=torch.float32))
    want = x * (1 - mm) + x.flip(0) * mm
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12 * 255
    if m == 0.0:
        assert torch.equal(got, x)


def test_mix_reference_with_a_cutmix_table_is_the_pasted_rectangle():
    px, boxes = _pixels(), torch.tensor(BOXES, dtype=torch.int32)
    x = resized_crop_reference(px, ROWS, boxes, OUT)
    rects = [(0, 0, OUT, OUT), (0, 0, 5, 7), (OUT - 3, OUT - 9, 3, 9), (13, 2, 1, 1), (4, 4, 0, 9), (6, 0, 20, OUT)]
    got = mix_reference(px, ROWS, boxes, table([(5 - i, *r, 0.0, r[2] * r[3] / OUT ** 2) for i, r in enumerate(rects)]), OUT)
    for i, (x0, y0, w, h) in enumerate(rects):
        want = x[i].clone()
        want[:, y0:y0 + h, x0:x0 + w] = x[5 - i][:, y0:y0 + h, x0:x0 + w]
        assert torch.equal(got[i], want), i
    assert torch.equal(got[0], x[5]) and torch.equal(got[4], x[4])
    # without boxes: a split of the output's size, read whole
    sq = px[:, :, :OUT, :OUT].contiguous()
    got = mix_reference(sq, ROWS, None, table([(5 - i, 0, 0, 16, 16, 0.0, 0.25) for i in range(6)]), OUT)
    want = sq[ROWS].double()
    want[:, :, :16, :16] = sq[ROWS].double().flip(0)[:, :, :16, :16]
    assert torch.equal(got, want)
    with pytest.raises(ValueError, match="size"):
        mix_reference(px, ROWS, None, identity_mix(6), OUT)


# ---- the draw --------------------------------------------------------------------------------------------------------------
def _unpack(t):
    f = lambda c: t[..., c].contiguous().view(torch.float32)   # noqa: E731
    return t[..., 0], t[..., 1:5].to(torch.int64), f(5), f(6)


def test_draw_gives_timms_batch_mode_tables():
    B, steps, Hi, Wi = 6, 4096, 32, 48
    mc = MixupCutmix((Hi, Wi), switch_prob=0.3)
    t = mc.draw(B, steps, torch.Generator().manual_seed(1))
    assert t.dtype == torch.int32 and tuple(t.shape) == (steps, B, 8) and t.is_contiguous()
    check_mix(t, B, Hi, Wi)
    # deterministic per generator, another seed another table; batch k does not depend on steps
    assert torch.equal(t, mc.draw(B, steps, torch.Generator().manual_seed(1)))
    assert not torch.equal(t, mc.draw(B, steps, torch.Generator().manual_seed(2)))
    assert torch.equal(t[:7], mc.draw(B, 7, torch.Generator().manual_seed(1)))
    partner, rect, m, tg = _unpack(t)
    assert torch.equal(partner, (B - 1 - torch.arange(B, dtype=torch.int32)).expand(steps, B)) and not t[..., 7].any()
    # one draw per batch: every row of a batch has the batch's rectangle and weights
    assert bool((rect == rect[:, :1]).all()) and bool((m == m[:, :1]).all()) and bool((tg == tg[:, :1]).all())
    x0, y0, w, h = rect[:, 0].unbind(1)
    m, tg = m[:, 0], tg[:, 0]
    assert bool(((x0 >= 0) & (y0 >= 0) & (w >= 0) & (h >= 0) & (x0 + w <= Wi) & (y0 + h <= Hi)).all())
    cut = m == 0                                      # (Mixup's m = 1 - lam is 0 with probability 0)
    # CutMix: m = 0 and t exactly the clipped rectangle's share; Mixup: m == t in (0, 1] and no rectangle
    assert torch.equal(tg[cut], ((w * h)[cut].double() / (Hi * Wi)).float())
    assert bool((w[~cut] == 0).all()) and bool((h[~cut] == 0).all()) and torch.equal(m[~cut], tg[~cut])
    assert bool(((m >= 0) & (m <= 1) & (tg >= 0) & (tg <= 1)).all())
    n_cut = int(cut.sum())
    assert abs(n_cut - 0.3 * steps) <= 4 * math.sqrt(steps * 0.3 * 0.7), n_cut       # 4 sigma of a 0.3 coin over the batches
    # the rectangles use the room they have; the Beta(0.8, 0.8) blends spread over (0, 1) (a rectangle is clipped at the edges,
    # so its share seldom comes near 1)
    assert len({tuple(r) for r in rect[:, 0][cut].tolist()}) > n_cut // 2
    assert float(tg[cut].min()) < 0.1 and float(m[~cut].min()) < 0.1 and float(m[~cut].max()) > 0.9
    assert abs(float(m[~cut].double().mean()) - 0.5) < 4 * math.sqrt(1 / (4 * 2.6) / (steps * 0.7))      # var Beta(a, a) = 1 / (4 (2a + 1))


def test_draw_respects_prob_and_single_methods():
    B, steps = 4, 64
    ident = identity_mix(B, steps)
    assert torch.equal(MixupCutmix(32, prob=0.0).draw(B, steps, torch.Generator().manual_seed(3)), ident)
    assert torch.equal(ident[5], torch.tensor([[i, 0, 0, 0, 0, 0, 0, 0] for i in range(B)], dtype=torch.int32))
    half = MixupCutmix(32, prob=0.5).draw(B, 4096, torch.Generator().manual_seed(3))
    n_id = int((half == identity_mix(B, 4096)).all(-1).all(-1).sum())
    assert abs(n_id - 2048) <= 4 * math.sqrt(4096 * 0.25)
    only_mixup = _unpack(MixupCutmix(32, cutmix_alpha=0.0).draw(B, steps, torch.Generator().manual_seed(3)))
    assert not only_mixup[1].any() and bool((only_mixup[2] > 0).all())
    only_cutmix = _unpack(MixupCutmix(32, mixup_alpha=0.0).draw(B, steps, torch.Generator().manual_seed(3)))
    assert not only_cutmix[2].any() and only_cutmix[1][..., 2:].any()
    for bad in (dict(mixup_alpha=0.0, cutmix_alpha=0.0), dict(prob=1.5), dict(switch_prob=-0.1), dict(mixup_alpha=-1.0)):
        with pytest.raises(ValueError, match="MixupCutmix"):
            MixupCutmix(32, **bad)
    with pytest.raises(ValueError, match="MixupCutmix"):
        MixupCutmix(0)


def test_check_mix_refuses_what_the_kernel_refuses():
    B, Hi, Wi = 4, 32, 48
    good = (1, 3, 2, 10, 12, 0.5, 0.25)
    check_mix(table([good] * B), B, Hi, Wi)
    check_mix(table([(B - 1, 0, 0, Wi, Hi, 1.0, 1.0), (0, Wi, Hi, 0, 0, 0.0, 0.0)] * 2), B, Hi, Wi)
    nan = float("nan")
    for bad in ((B, 3, 2, 10, 12, 0.5, 0.25), (-1, 3, 2, 10, 12, 0.5, 0.25),
                (1, -1, 2, 10, 12, 0.5, 0.25), (1, 3, -1, 10, 12, 0.5, 0.25), (1, Wi - 9, 2, 10, 12, 0.5, 0.25), (1, 3, Hi - 11, 10, 12, 0.5, 0.25),
                (1, 3, 2, -1, 12, 0.5, 0.25), (1, 3, 2, 10, -1, 0.5, 0.25),
                (1, 3, 2, 10, 12, 1.5, 0.25), (1, 3, 2, 10, 12, nan, 0.25), (1, 3, 2, 10, 12, -0.1, 0.25),
                (1, 3, 2, 10, 12, 0.5, 2.0), (1, 3, 2, 10, 12, 0.5, nan)):
        with pytest.raises(ValueError, match="mix entry"):
            check_mix(table([good, bad, good, good]), B, Hi, Wi)
    for wrong in (table([good] * B).float(), table([good] * B)[:, :7], table([good] * (B + 1)), table([good] * B).tolist()):
        with pytest.raises(ValueError, match="int32"):
            check_mix(wrong, B, Hi, Wi)


# ---- the loss bound --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", S.XENT_C)
@pytest.mark.parametrize("B", S.XENT_B)
def test_loss_bound_holds_the_fp32_restatement_and_not_a_slip(B, Cn):
    worst = 0.0
    for eps in (0.0, 0.1):
        for t in (0.0, 0.3, 1.0):
            for same in (True, False):
                for scale in ((1.0, 1.0), (0.25, 512.0)):
                    l, y, mix = M.loss_case(B, Cn, t, same)
                    model = M.xent_mix(l, y, mix, eps, *scale)
                    term, loss, dl = M.xent_mix_f32(l, y, mix, eps, *scale)
                    for name, got in (("terms", term), ("loss", loss), ("dlogits", dl)):
                        ok, ratio = K.hold_f32(got, *model[name])
                        assert ok.all(), (name, eps, t, same, scale, ratio)
                        worst = max(worst, ratio)
                    # q is the definition's
                    assert float((model["q"] - soft_target(y, mix, Cn, float(torch.tensor(eps, dtype=torch.float32)))).abs().max()) <= 1e-15
    print(f"B {B} C {Cn}: the fp32 restatement uses at most {worst:.3f} of the bound")
    assert worst > 1e-3                   # not vacuous: a restatement in fp32 does use the bound
    # ... and not wrong: what a slip gives is outside it.  eps / (C - 1) for eps / C; the partner's weight forgotten in the loss
    if Cn > 2:
        l, y, mix = M.loss_case(B, Cn, 0.3, False)
        model = M.xent_mix(l, y, mix, 0.1)
        slip = M.xent_mix(l, y, mix, 0.1 * Cn / (Cn - 1))["dlogits"][0].float()
        assert not K.hold_f32(slip, *model["dlogits"])[0].all()
        forgot = M.xent_mix_f32(l, y, table([(int(r[0]), 0, 0, 0, 0, 0.0, 0.0) for r in mix.tolist()]), 0.1)[0]
        if B > 1:
            assert not K.hold_f32(forgot, *model["terms"])[0].all()


def test_loss_model_without_smoothing_and_partner_is_the_small_kernels_xent():
    for B in S.XENT_B:
        for Cn in S.XENT_C:
            l, y = S.xent_inputs(B, Cn)
            a, b = M.xent_mix(l, y, None, 0.0, 0.25, 512.0), K.xent(l, y, 0.25, 512.0)
            for name in ("terms", "loss", "dlogits"):
                assert torch.allclose(a[name][0], b[name][0], rtol=1e-14, atol=1e-300), name
                assert bool((a[name][1] >= b[name][1] * (1 - 1e-12)).all())      # (never tighter than xent's own bound)


# ---- the feed --------------------------------------------------------------------------------------------------------------
N, BATCH = 37, 8


def _split(Hs=HS, Ws=WS):
    px = (torch.arange(N, dtype=torch.uint8) + 1).reshape(N, 1, 1, 1).expand(N, 3, Hs, Ws).contiguous()
    return ResidentSplit.from_tensors(px, torch.arange(N) + 100)


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_train_rows_with_a_mix(rank, world):
    split, aug, mc = _split(), RandomResizedCropFlip(32), MixupCutmix(32)
    tables = {}
    for epoch in range(2):
        plain = list(split.train_rows(BATCH, seed=3, rank=rank, world=world)(epoch))
        boxed = list(split.train_rows(BATCH, seed=3, rank=rank, world=world, augment=aug)(epoch))
        got = list(split.train_rows(BATCH, seed=3, rank=rank, world=world, augment=aug, mix=mc)(epoch))
        assert len(got) == len(plain) >= 2
        for (rows, boxes, mix), want_rows, (_, want_boxes) in zip(got, plain, boxed):
            assert torch.equal(rows, want_rows) and torch.equal(boxes, want_boxes)          # rows and boxes are what they were
            assert mix.dtype == torch.int32 and tuple(mix.shape) == (BATCH, 8) and mix.is_contiguous()
        # one upload per epoch: every step's table is a view of one tensor
        assert len({m.untyped_storage().data_ptr() for _, _, m in got}) == 1
        assert [m.storage_offset() for _, _, m in got] == [i * BATCH * 8 for i in range(len(got))]
        table_ = torch.stack([m for _, _, m in got])
        check_mix(table_, BATCH, 32, 32)
        assert torch.equal(table_, mc.draw(BATCH, len(got), torch.Generator().manual_seed(mix_seed(3, epoch, rank))))
        tables[epoch] = table_
    assert not torch.equal(tables[0], tables[1])
    # a stream of its own: never the boxes' seed
    assert all(mix_seed(s, e, r) != box_seed(s, e, r) for s in (0, 3, 4) for e in (0, 1, 99) for r in (0, 1, 7))
    assert len({mix_seed(s, e, r) for s in (0, 3, 4) for e in (0, 1, 99) for r in (0, 1, 7)}) == 27
    # without an augment the boxes are None; the split then has the model's size
    sq = _split(32, 32)
    for rows, boxes, mix in sq.train_rows(BATCH, seed=3, mix=mc)(0):
        assert boxes is None and tuple(mix.shape) == (BATCH, 8) and rows.dtype == torch.int64


def test_a_mix_entry_outside_is_refused_before_upload():
    class OneBad:
        Hi = Wi = 32

        def draw(self, B, steps, generator):
            t = identity_mix(B, steps)
            t[steps // 2, 1, 0] = B
            return t
    with pytest.raises(ValueError, match="mix entry"):
        next(_split().train_rows(BATCH, mix=OneBad())(0))
    with pytest.raises(ValueError, match="MixupCutmix"):
        _split().train_rows(BATCH, mix=identity_mix(BATCH))

    class NoSize:                                            # a drawer that does not say whose pixels its rectangles are in
        def draw(self, B, steps, generator):
            return identity_mix(B, steps)
    with pytest.raises(ValueError, match="MixupCutmix"):
        _split().train_rows(BATCH, mix=NoSize())

    class WrongShape(OneBad):
        def draw(self, B, steps, generator):
            return identity_mix(B, steps + 1)
    with pytest.raises(ValueError, match="mix.draw gave"):
        next(_split().train_rows(BATCH, mix=WrongShape())(0))


def test_steps_and_fit_refuse_what_is_no_mix_table_and_a_smoothing_outside_0_1():
    from cara_amd import cara, create_model
    from cara_amd.recipe import fit
    m = create_model("vit_base_patch16_224_in21k", drop_path_rate=0.0, depth=1, img_size=32, num_classes=10)
    m = cara({"model": m, "rank": 4, "scale": 0.1, "l_mu": 1.5, "l_std": 0.1})
    eng = m._cara_engine
    split = ResidentSplit.from_tensors(torch.zeros(6, 3, 48, 48, dtype=torch.uint8), torch.arange(6))
    rows = torch.arange(4)
    boxes = torch.tensor([[0, 0, 32, 32, 0]] * 4, dtype=torch.int32)
    good = identity_mix(4)
    for mix in (good.float(), good.to(torch.int64), good[:, :7].contiguous(), good.reshape(-1), good.t(), good.tolist(),
                identity_mix(8)[::2]):
        with pytest.raises(CaraError, match="mix must be"):
            eng.train_step_resident(split, rows, None, boxes=boxes, mix=mix)
        with pytest.raises(CaraError, match="mix must be"):
            eng.forward_resident(split, rows, boxes=boxes, mix=mix)
        with pytest.raises(CaraError, match="mix must be"):
            fit(m, (split, lambda epoch, mix=mix: iter([(rows, boxes, mix)])), None, epochs=1, feed="resident")
    for eps in (-0.1, 1.0, 1.5, float("nan"), "0.1", None):
        with pytest.raises(CaraError, match="label_smoothing"):
            eng.train_step_resident(split, rows, None, boxes=boxes, mix=good, label_smoothing=eps)
        with pytest.raises(CaraError, match="label_smoothing"):
            eng.train_step(torch.zeros(4, 3, 32, 32), torch.arange(4), None, label_smoothing=eps)
        if eps is not None:                                   # (fit's default means "none")
            with pytest.raises(CaraError, match="label_smoothing"):
                fit(m, (split, lambda epoch: iter([(rows, boxes, good)])), None, epochs=1, feed="resident", label_smoothing=eps)
    # what is a table and a smoothing gets as far as the device check
    with pytest.raises(CaraError, match="GPU only"):
        eng.train_step_resident(split, rows, None, boxes=boxes, mix=good, label_smoothing=0.1)


def test_get_data_passes_the_mix_on(tmp_path):
    import os

    from PIL import Image

    from cara_amd.data import get_data
    root = str(tmp_path)
    g = torch.Generator().manual_seed(0)
    for name, n in (("train800val200.txt", 5), ("test.txt", 3)):
        with open(os.path.join(root, name), "w") as fh:
            for i in range(n):
                fn = f"{name[:2]}{i}.png"
                Image.fromarray(torch.randint(0, 256, (12, 10, 3), generator=g, dtype=torch.uint8).numpy()).save(os.path.join(root, fn))
                fh.write(f"{fn} {i % 3}\n")
    kw = dict(batch_size=2, root=root, device="cpu", seed=1, workers=1)
    (split, rows_of), _ = get_data("cifar", resident_feed=True, mix=MixupCutmix(224), **kw)
    ep = list(rows_of(0))
    assert len(ep) == 2 and all(len(item) == 3 and item[1] is None and tuple(item[2].shape) == (2, 8) for item in ep)
    with pytest.raises(ValueError, match="resident"):
        get_data("cifar", mix=MixupCutmix(224), **kw)
