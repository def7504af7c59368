"""Host side of the jittered resident feed, no device: data.aug_reference against a plain-torch restatement of torchvision's three
adjust functions, the numpy fp32 restatement of the chain and of the tree (tests/aug_model.py) inside the bounds derived there --
and slipped restatements outside them --, ColorJitterErase.draw, check_aug, and the pixel-mode noise on the restatement."""
import itertools
import math

import numpy as np
import pytest
import torch

from cara_amd import data as D
from tests import aug_model as G

BR, CO, SA = 1, 2, 3
HI = WI = 32


def _pixels(n=4, size=40, seed=3):
    return torch.randint(0, 256, (n, 3, size, size), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


BOXES = [(0, 0, 40, 40, 0), (11, 9, 13, 13, 1), (3, 2, 35, 13, 0), (8, 8, 32, 32, 1)]
ROWS = [2, 0, 3, 2]


# ---- the reference against plain torch -------------------------------------------------------------------------------------------
def _gray(img):
    w = [float(torch.tensor(v, dtype=torch.float32)) for v in D.GRAY_WEIGHTS]
    return (w[0] * img[0] + w[1] * img[1] + w[2] * img[2]).unsqueeze(0)


def _blend(img1, img2, ratio):
    """torchvision.transforms._functional_tensor._blend on a float image with bound 1.0"""
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 1.0)


def adjust_brightness(img, f):
    return _blend(img, torch.zeros_like(img), f)


def adjust_contrast(img, f):
    return _blend(img, torch.mean(_gray(img), dim=(-3, -2, -1), keepdim=True), f)


def adjust_saturation(img, f):
    return _blend(img, _gray(img), f)


ADJUST = {BR: adjust_brightness, CO: adjust_contrast, SA: adjust_saturation}


@pytest.mark.parametrize("order", list(itertools.permutations((BR, CO, SA))))
def test_reference_is_torchvisions_adjust_functions_on_the_unit_scale(order):
    """the gray weights are the three fp32 values the kernel holds, in both"""
    px = _pixels()
    f = (0.6, 1.4, 1.7)
    aug = G.table([G.row(list(zip(order, f[i:] + f[:i]))) for i in (0, 1, 2, 0)])
    got = D.aug_reference(px, ROWS, torch.tensor(BOXES, dtype=torch.int32), None, aug, HI)
    x = D.resized_crop_reference(px, ROWS, torch.tensor(BOXES, dtype=torch.int32), HI) / 255.0
    mean = torch.tensor(D.IMAGENET_MEAN, dtype=torch.float32).double().view(3, 1, 1)
    std = torch.tensor(D.IMAGENET_STD, dtype=torch.float32).double().view(3, 1, 1)
    for b in range(4):
        img = x[b]
        for op, fb in G.row_slots(aug[b]):
            img = ADJUST[op](img, float(fb))
        assert float((got[b] - (img - mean) / std).abs().max()) < 1e-12, b


def test_reference_mixes_after_the_chain_and_erases_after_the_normalisation():
    px = _pixels()
    bx = torch.tensor(BOXES, dtype=torch.int32)
    aug = G.table([G.row([(CO, 1.3)], erase=(3, 4, 5, 6), emode=0), G.row([(BR, 0.5)]), G.row([], erase=(0, 0, 32, 2), emode=1, eseed=9), G.row([(SA, 0.2)])])
    mix = torch.tensor([[1, 0, 0, 0, 0, G.bits(0.25), 0, 0], [0, 2, 2, 8, 8, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int32)
    got = D.aug_reference(px, ROWS, bx, mix, aug, HI)
    colour = aug.clone()
    colour[:, 6:] = 0
    y = D.aug_reference(px, ROWS, bx, None, colour, HI)
    want0 = y[0] + 0.25 * (y[1] - y[0])                 # (the normalisation is affine: blending after it is the same to rounding)
    inside = torch.zeros(3, 32, 32, dtype=torch.bool)
    inside[:, 4:10, 3:8] = True
    assert float((got[0] - want0)[~inside].abs().max()) < 1e-12 and not got[0][inside].any()
    want1 = y[1].clone()
    want1[:, 2:10, 2:10] = y[0][:, 2:10, 2:10]
    assert float((got[1] - want1).abs().max()) < 1e-12
    assert torch.equal(got[2][:, 2:], y[2][:, 2:]) and abs(float(got[2][:, :2].mean())) < 0.3 and torch.equal(got[3], y[3])
    idx = torch.arange(4 * 3 * 32 * 32).view(4, 3, 32, 32)[2][:, :2].numpy()
    assert np.array_equal(got[2][:, :2].numpy(), D.erase_noise(idx, 9)[2])
    with pytest.raises(ValueError):
        D.aug_reference(px[:, :1], ROWS, bx, None, aug, HI)
    with pytest.raises(ValueError):
        D.aug_reference(px, ROWS, None, None, aug, HI)


# ---- the fp32 restatement inside the derived bounds ------------------------------------------------------------------------------
def _images(kind):
    px = _pixels(seed=11)
    if kind == "bright":
        px = (200 + px.to(torch.int32) * 56 // 256).to(torch.uint8)
    return G.crop_f32(px, ROWS, BOXES, HI, WI)


def test_fma32_is_one_rounding():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(20000).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 4)) for _ in range(3))
    from fractions import Fraction
    got = G.fma32(a, b, c)
    for i in range(0, 20000, 37):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.nextafter(got[i], np.float32(-np.inf))
        hi = np.nextafter(got[i], np.float32(np.inf))
        assert abs(exact - Fraction(float(got[i]))) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi)))), i
    # what rounding the float64 sum to nearest first gets wrong: a b = 1 + 2^-11 + 2^-24 is a tie of two fp32 values, broken by c
    a = np.float32(1 + 2 ** -12)
    assert G.fma32(a, a, np.float32(2 ** -80)) == np.float32(1 + 2 ** -11 + 2 ** -23) and G.fma32(a, a, np.float32(-2 ** -80)) == np.float32(1 + 2 ** -11)
    assert np.float32(np.float64(a) * np.float64(a) + 2.0 ** -80) == np.float32(np.float64(a) * np.float64(a) - 2.0 ** -80)


def test_the_restated_crop_is_the_reference_to_rounding():
    u = _images("bytes")
    x = D.resized_crop_reference(_pixels(seed=11), ROWS, torch.tensor(BOXES, dtype=torch.int32), HI).numpy()
    assert float(np.abs(u - x).max()) < G.E_CROP_BYTES


FACTORS = [(0.6, 1.0, 1.4), (1.4, 0.6, 1.0), (1.0, 1.4, 0.6), (1.6, 0.0, 2.0)]


@pytest.mark.parametrize("kind", ["bytes", "bright"])
@pytest.mark.parametrize("order", list(itertools.permutations((BR, CO, SA))))
def test_chain_restatement_inside_the_derived_bound_and_slips_outside(order, kind):
    u = _images(kind)
    held = {"no clamp": True, "bf16 weights": True}
    worst = 0.0
    for b, f in enumerate(FACTORS):
        r = G.row(list(zip(order, f)))
        v, e, M64, eM = G.chain_bound(u[b], r)
        got, M32 = G.chain_f32(u[b], r)
        assert abs(float(M32) - M64) <= eM
        err = np.abs(got.astype(np.float64) - v)
        assert (err <= e).all(), (b, float((err - e).max()))
        worst = max(worst, float((err / np.maximum(e, 1e-300)).max()))
        for slip in held:
            s, _ = G.chain_f32(u[b], r, slip=slip)
            held[slip] &= bool((np.abs(s.astype(np.float64) - v) <= e).all())
    print(f"order {order} [{kind}]: worst |restatement - float64| / bound {worst:.3f}")
    assert 0.0 < worst <= 1.0
    assert not held["bf16 weights"]                              # gray weights rounded to 8 bits
    if kind == "bright":
        assert not held["no clamp"]                              # (1.4 x 200 leaves the range: the clamp is part of every slot)


def test_a_fused_slot_is_another_restatement_and_a_slot_is_exact_where_stated():
    u = _images("bytes")
    r = G.row([(SA, 0.6), (BR, 1.4), (CO, 0.7)])
    a, _ = G.chain_f32(u[0], r)
    b, _ = G.chain_f32(u[0], r, slip="fused")
    assert (a != b).any() and float(np.abs(a - b).max()) < 1e-3
    for op in (BR, CO, SA):
        same, _ = G.chain_f32(u[1], G.row([(op, 1.0)]))
        assert np.array_equal(same.view(np.int32), u[1].view(np.int32)), op
    black, _ = G.chain_f32(u[1], G.row([(BR, 0.0)]))
    assert not black.any()
    flat, M = G.chain_f32(u[1], G.row([(CO, 0.0)]))
    assert (flat == M).all() and 0 < M < 255
    grey, _ = G.chain_f32(u[1], G.row([(SA, 0.0)]))
    assert np.array_equal(grey[0], G.gray_f32(u[1])) and np.array_equal(grey[0], grey[2])


@pytest.mark.parametrize("n", [1, 63, 1024, 4097, 9216, 50176])
def test_tree_mean_inside_gamma_of_its_longest_path_and_a_running_sum_outside(n):
    rng = np.random.default_rng(n)
    g = (rng.random(n) * 255).astype(np.float32)
    exact = math.fsum(float(v) for v in g) / n
    got = float(G.tree_mean(g))
    m = G.mean_path(n) - 3                                       # (the gray values are given: their three roundings are not in it)
    assert abs(got - exact) <= G.gamma(m) * exact
    assert G.mean_path(n) == -(-n // 4096) + 28
    if n == 50176:    # 224 x 224, a flat image: one running sum stagnates (every addend rounds up once the sum passes 2^23), the tree does not
        flat = np.full(n, 254.7, dtype=np.float32)
        assert abs(float(G.sequential_mean(flat)) - float(flat[0])) > G.gamma(m) * 254.7
        assert abs(float(G.tree_mean(flat)) - float(flat[0])) <= G.gamma(m) * 254.7


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
def test_draw_is_deterministic_independent_of_steps_and_in_range():
    c = D.ColorJitterErase(32)
    a = c.draw(5, 7, torch.Generator().manual_seed(4))
    b = c.draw(5, 3, torch.Generator().manual_seed(4))
    assert a.dtype == torch.int32 and tuple(a.shape) == (7, 5, 16) and torch.equal(a[:3], b) and torch.equal(a, c.draw(5, 7, torch.Generator().manual_seed(4)))
    assert not torch.equal(a, c.draw(5, 7, torch.Generator().manual_seed(5)))
    D.check_aug(a, 5, 32, 32)
    t = D.ColorJitterErase((24, 40), brightness=0.4, contrast=1.5, saturation=0.0, erase_prob=1.0, erase_mode="const").draw(64, 32, torch.Generator().manual_seed(1))
    D.check_aug(t, 64, 24, 40)
    r = t.reshape(-1, 16)
    ops, f = r[:, 0:6:2], D._bits_f32(r[:, 1:6:2])
    assert set(ops.reshape(-1).tolist()) == {0, BR, CO} and bool(((ops == 0).sum(1) == 1).all())        # saturation 0: its slot is empty
    fb, fc = f[ops == BR], f[ops == CO]
    assert 0.6 <= float(fb.min()) < 0.65 and 1.35 < float(fb.max()) <= 1.4 + 1e-6 and 0.0 <= float(fc.min()) < 0.1 and 2.4 < float(fc.max()) <= 2.5
    assert bool((f[ops == 0] == 0).all()) and bool((r[:, 10] == 0).all()) and bool((r[:, 12:] == 0).all())
    w, h = r[:, 8], r[:, 9]
    assert bool((w > 0).all()) and bool((h > 0).all()) and bool((w < 40).all()) and bool((h < 24).all())
    assert bool((r[:, 6] + w <= 40).all()) and bool((r[:, 7] + h <= 24).all()) and int(r[:, 6].min()) == 0 and int(r[:, 7].min()) == 0
    area = (w * h).double() / (24 * 40)
    assert 0.01 < float(area.min()) and float(area.max()) < 0.36 and len(set(r[:, 11].tolist())) > 2000
    assert int((r[:, 6] + w).max()) == 40 and int((r[:, 7] + h).max()) == 24                             # (offsets reach the far edges)


def test_all_six_permutations_occur_and_the_erase_share_is_the_probability():
    c = D.ColorJitterErase(32, erase_prob=0.25)
    t = c.draw(4, 4096, torch.Generator().manual_seed(2)).reshape(-1, 16)
    orders = {}
    for o in map(tuple, t[:, 0:6:2].tolist()):
        orders[o] = orders.get(o, 0) + 1
    n = t.shape[0]
    assert len(orders) == 6 and all(abs(k / n - 1 / 6) < 4 * math.sqrt(5 / 36 / n) for k in orders.values()), orders
    share = float((t[:, 8] > 0).double().mean())
    print(f"erase share {share:.4f} of {n} samples")
    assert abs(share - 0.25) < 4 * math.sqrt(0.25 * 0.75 / n)
    assert bool(((t[:, 8] > 0) == (t[:, 9] > 0)).all()) and bool((t[:, 10] == 1).all())
    none = D.ColorJitterErase(32, 0, 0, 0, erase_prob=0.0).draw(4, 3, torch.Generator().manual_seed(2))
    assert not none[..., :10].any() and not none[..., 12:].any()
    for bad in (dict(brightness=-0.1), dict(erase_prob=1.5), dict(erase_scale=(0.0, 0.3)), dict(erase_ratio=(2.0, 1.0)), dict(erase_mode="rand")):
        with pytest.raises(ValueError):
            D.ColorJitterErase(32, **bad)


def test_check_aug_refuses_every_violation_of_the_rule():
    good = G.table([G.row([(SA, 0.5), (BR, 2.0)], erase=(3, 4, 29, 28), emode=1, eseed=0xffffffff), G.row([])])
    D.check_aug(good, 2, 32, 32)
    D.check_aug(good.expand(3, 2, 16), 2, 32, 32)
    D.check_aug(G.table([[0, G.bits(float("nan")), 0, -1, 0, G.bits(-3.0)] + [0] * 10] * 2), 2, 32, 32)      # factors of op 0 are not read
    nan, inf = float("nan"), float("inf")
    e = (3, 4, 5, 6)
    for entry in (G.row([(4, 1.0)]), G.row([(-1, 1.0)]), G.row([(BR, 1.0), (BR, 1.0)]), G.row([(CO, 1.0), (SA, 1.0), (CO, 1.0)]), G.row([(BR, -0.5)]),
                  G.row([(CO, nan)]), G.row([(SA, inf)]), G.row([(SA, -inf)]), G.row([], (-1, 4, 5, 6)), G.row([], (3, -1, 5, 6)),
                  G.row([], (3, 4, -5, 6)), G.row([], (3, 4, 5, -6)), G.row([], (28, 4, 5, 6)), G.row([], (3, 27, 5, 6)), G.row([], (1, 1, 2 ** 31 - 1, 1)),
                  G.row([], e, emode=2), G.row([], e, emode=-1), G.row([], e, pad=(1, 0, 0, 0)), G.row([], e, pad=(0, 0, 0, 7))):
        t = good.clone()
        t[1] = torch.tensor(entry, dtype=torch.int32)
        with pytest.raises(ValueError):
            D.check_aug(t, 2, 32, 32)
    for t in (good.long(), good[:, :8].contiguous(), good[:1], good.float(), good.tolist()):
        with pytest.raises(ValueError):
            D.check_aug(t, 2, 32, 32)
    assert D.aug_seed(1, 2, 3) not in (D.mix_seed(1, 2, 3), D.box_seed(1, 2, 3)) and D.aug_seed(1, 2, 3) != D.aug_seed(1, 2, 4)
    assert not D.identity_aug(3).any() and tuple(D.identity_aug(3, 2).shape) == (2, 3, 16)


# ---- pixel mode ------------------------------------------------------------------------------------------------------------------
def test_erase_noise_is_a_standard_normal_and_a_function_of_index_and_seed():
    n = 1 << 16
    idx = np.arange(n) + 12345
    u1, arg, z = D.erase_noise(idx, 0xdeadbeef)
    assert u1.min() > 0 and u1.max() <= 1 and arg.dtype == np.float32 and arg.min() >= 0 and arg.max() < 6.2831855
    assert np.isfinite(z).all()
    mean, var = float(z.mean()), float(z.var())
    print(f"erase noise over 2^16 elements: mean {mean:.5f} variance {var:.5f}")
    assert abs(mean) < 4 / math.sqrt(n) and abs(var - 1) < 4 * math.sqrt(2 / n)
    again = D.erase_noise(idx, 0xdeadbeef)[2]
    assert np.array_equal(z.view(np.int64), again.view(np.int64))
    assert np.array_equal(D.erase_noise(idx[100:200], 0xdeadbeef - (1 << 32))[2], z[100:200])       # (the table holds the seed as an int32)
    other = D.erase_noise(idx, 0xdeadbeee)[2]
    assert (other != z).mean() > 0.999 and abs(float(np.corrcoef(z, other)[0, 1])) < 4 / math.sqrt(n)
    # the two draws of an element are the hash at 2 i and 2 i + 1 on the erase stream
    from cara_amd.dropout import keep_hash_np
    h1 = keep_hash_np(np.uint32(2 * 777), 5, D.AUG_ERASE_STREAM)
    assert D.erase_noise(np.array([777]), 5)[0][0] == (float(h1 >> np.uint32(8)) + 1) * 2.0 ** -24


def test_the_feed_yields_the_fourth_table():
    px = _pixels(n=12, size=32)
    split = D.ResidentSplit.from_tensors(px, torch.arange(12))
    c = D.ColorJitterErase(32)
    feed = split.train_rows(4, seed=5, rank=0, world=1, color=c)
    items = list(feed(0))
    assert len(items) == 3 and all(len(i) == 4 and i[1] is None and i[2] is None and tuple(i[3].shape) == (4, 16) for i in items)
    again = list(feed(0))
    assert all(torch.equal(a[3], b[3]) and torch.equal(a[0], b[0]) for a, b in zip(items, again)) and not torch.equal(items[0][3], list(feed(1))[0][3])
    both = list(split.train_rows(4, seed=5, rank=0, world=1, mix=D.MixupCutmix(32), color=c)(0))
    assert all(len(i) == 4 and tuple(i[2].shape) == (4, 8) and torch.equal(i[3], j[3]) for i, j in zip(both, items))
    plain = list(split.train_rows(4, seed=5, rank=0, world=1, mix=D.MixupCutmix(32))(0))
    assert all(len(i) == 3 and torch.equal(i[2], j[2]) for i, j in zip(plain, both))

    class Bad:
        Hi = Wi = 32

        def draw(self, B, steps, generator):
            t = D.identity_aug(B, steps)
            t[0, 0, 0] = 7
            return t
    with pytest.raises(ValueError):
        list(split.train_rows(4, color=Bad(), rank=0, world=1)(0))
    with pytest.raises(ValueError):
        split.train_rows(4, color=object(), rank=0, world=1)
    with pytest.raises(ValueError):
        D.get_data("cifar", color=c)
