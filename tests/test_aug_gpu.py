"""GPU side of the jittered resident feed.  cara_im2col_patches_u8_rows_aug: an all-zero table bitwise against the calls without
one, single ops at f == 1, the contrast statistic bitwise against the numpy restatement of its tree (tests/aug_model.py), the chain
and its mixes against data.aug_reference in float64 within the bound derived there, the erase rectangle element by element, every
guard.  Whole model: train_step_resident / GraphedTrainStep / fit with an aug table against the calls without one (bitwise) and
against fp32 autograd of the oracle's as-written model on the float64 definition.  Helpers of tests/test_augmented_feed_gpu.py and
tests/test_mix_gpu.py; every test on both operand builds."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import aug_model as G
from tests import mix_model as M
from tests import test_augmented_feed_gpu as A
from tests import test_mix_gpu as T
from tests.test_augmented_feed_gpu import DEV, SENTINEL, L

pytestmark = pytest.mark.gpu
OPERANDS = ["bf16", "fp16"]
HS = WS = 40
N_SPLIT, OUT = 6, 32
ROWS = [2, 0, 5, 2, 4]                         # B = 5 (a sample is 3072 elements, 12 waves at four per lane; 5 is no multiple of 4 workgroups)
B5 = len(ROWS)
SAME = [(0, 0, OUT, OUT, 0), (WS - OUT, HS - OUT, OUT, OUT, 1), (5, 3, OUT, OUT, 0), (0, HS - OUT, OUT, OUT, 1), (WS - OUT, 0, OUT, OUT, 0)]
SCALED = [(0, 0, WS, HS, 0), (11, 9, 13, 13, 1), (3, 2, 35, 13, 0), (WS - 9, HS - 37, 9, 37, 1), (4, 1, 31, 33, 1)]
GUARD = 12345.0                                # fp32 value of the guard words around the statistic scratch
BR, CO, SA = 1, 2, 3


@functools.lru_cache(maxsize=None)
def _source_cpu(kind="bytes"):
    """eight images of 40 x 40 of which the split is the middle six.  "bytes": every byte value in every channel; "bright": bytes
    in [200, 255] (a brightness factor above 1 clamps them); "zero": image 0 of the split is all zero"""
    g = torch.Generator().manual_seed(23)
    px = torch.randint(0, 256, (N_SPLIT + 2, 3, HS, WS), generator=g, dtype=torch.uint8)
    if kind == "bytes":
        px.view(N_SPLIT + 2, 3, -1)[:, :, :256] = torch.arange(256, dtype=torch.uint8)
    elif kind == "bright":
        px = (200 + px.to(torch.int32) * 56 // 256).to(torch.uint8)
    elif kind == "zero":
        px[1] = 0
    return px


def _split_px(kind="bytes"):
    return _source_cpu(kind).to(DEV)[1:1 + N_SPLIT]


def _square(kind="bytes"):
    """the same split cut to the output's size (read without boxes): host and device"""
    sq = _source_cpu(kind)[:, :, 3:3 + OUT, 5:5 + OUT].contiguous()
    return sq[1:1 + N_SPLIT], sq.to(DEV)[1:1 + N_SPLIT]


def _aug_patches(lib, dt, px, rows, boxes, mix, aug, p, bad=None, out=OUT, n_split=N_SPLIT):
    """cara_im2col_patches_u8_rows_aug into a buffer between two sentinel guards, its statistic scratch between two guard words
    (all checked here) -> ([B, patches, 3 p p] of dt, stat fp32 [B] on the host: GUARD where nothing was written)"""
    B = len(rows)
    idx = torch.tensor(rows, device=DEV)
    bx = None if boxes is None else torch.tensor(boxes, dtype=torch.int32, device=DEV)
    mx = None if mix is None else mix.to(DEV)
    ag = aug.to(DEV)
    mean, std = A._norm()
    nel = B * 3 * out * out
    buf = torch.full((nel + 128,), SENTINEL, dtype=torch.int16, device=DEV)
    got = buf[64:64 + nel]
    nst = int(lib.cara_aug_stat_bytes(B)) // 4
    assert nst == B * (1 + G.GROUPS)
    sbuf = torch.full((nst + 2,), GUARD, device=DEV)
    P = L().ptr
    L().check(lib.cara_im2col_patches_u8_rows_aug(P(px), n_split, px.shape[2], px.shape[3], P(idx), P(bx), P(mx), P(ag), P(sbuf[1:]), P(mean),
                                                  P(std), P(got), P(bad) if bad is not None else None, B, 3, out, out, p, L().stream()),
              "cara_im2col_patches_u8_rows_aug")
    torch.cuda.synchronize()
    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + nel:] == SENTINEL).all())
    assert float(sbuf[0]) == GUARD and float(sbuf[-1]) == GUARD
    return got.view(dt).view(B, (out // p) ** 2, 3 * p * p), sbuf[1:1 + B].cpu()


def _zeros(B=B5):
    from cara_amd.data import identity_aug
    return identity_aug(B)


_same = T._same
PARTNERS = [3, 4, 0, 3, 1]                       # with partner == i (sample 3)
MIXED = T.table([(3, 0, 0, 0, 0, 0.25, 0.25), (4, 6, 3, 13, 11, 0.0, 0.1), (0, 0, 0, 0, 0, 0.5, 0.5), (3, 0, 0, 0, 0, 0.0, 0.0), (1, 0, 5, OUT, 9, 0.0, 0.2)])


# ---- 1. the identity table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("p", [16, 8])
def test_an_all_zero_table_gives_the_patch_rows_of_the_call_without_it(p, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    _, sq = _square()
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for boxes in (SAME, SCALED):
        crop = A._crop_patches(lib, dt, px, ROWS, boxes, p, out=OUT, n_split=N_SPLIT)
        got, stat = _aug_patches(lib, dt, px, ROWS, boxes, None, _zeros(), p, bad)
        assert _same(got, crop) and bool((stat == GUARD).all())
        assert _same(_aug_patches(lib, dt, px, ROWS, boxes, T._identity(B5), _zeros(), p, bad)[0], crop)
        want = T._mix_patches(lib, dt, px, ROWS, boxes, MIXED, p, out=OUT, n_split=N_SPLIT)
        assert _same(_aug_patches(lib, dt, px, ROWS, boxes, MIXED, _zeros(), p, bad)[0], want) and not _same(want, crop)
    # without boxes, with and without a mix table
    want = T._mix_patches(lib, dt, sq, ROWS, None, MIXED, p, out=OUT, n_split=N_SPLIT)
    assert _same(_aug_patches(lib, dt, sq, ROWS, None, MIXED, _zeros(), p, bad)[0], want)
    want = T._mix_patches(lib, dt, sq, ROWS, None, T._identity(B5), p, out=OUT, n_split=N_SPLIT)
    assert _same(_aug_patches(lib, dt, sq, ROWS, None, None, _zeros(), p, bad)[0], want)
    assert int(bad) == 0


# ---- 2. single ops ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
def test_each_op_at_factor_one_is_the_identity_and_brightness_zero_is_black(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    plain = A._crop_patches(lib, dt, px, ROWS, SCALED, 16, out=OUT, n_split=N_SPLIT)
    for op in (BR, CO, SA):
        for slot in range(3):
            ops = [(0, 0.0)] * slot + [(op, 1.0)]
            got, _ = _aug_patches(lib, dt, px, ROWS, SCALED, None, G.table([G.row(ops)] * B5), 16)
            assert _same(got, plain), (op, slot)
    got, _ = _aug_patches(lib, dt, px, ROWS, SCALED, None, G.table([G.row([(BR, 1.0), (CO, 1.0), (SA, 1.0)])] * B5), 16)
    assert _same(got, plain)
    # brightness 0: the normalised value of a zero byte, which the crop kernel gives for an all-zero image
    zpx = _source_cpu("zero").to(DEV)[1:1 + N_SPLIT]
    black = A._crop_patches(lib, dt, zpx, [0] * B5, SCALED, 16, out=OUT, n_split=N_SPLIT)
    assert len({int(v) for v in black.view(torch.int16).unique()}) == 3
    got, _ = _aug_patches(lib, dt, px, ROWS, SCALED, None, G.table([G.row([(BR, 0.0)])] * B5), 16)
    assert _same(got, black)


# ---- 3. the statistic ----------------------------------------------------------------------------------------------------------
STAT_ROWS = [G.row([(CO, 0.7)]), G.row([(BR, 1.6), (CO, 1.3)]), G.row([(SA, 0.5), (CO, 0.6), (BR, 1.2)]), G.row([(BR, 0.8), (SA, 1.4)]),
             G.row([(BR, 1.6), (SA, 1.5), (CO, 1.1)])]


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("kind,boxes,out", [("bytes", SAME, OUT), ("bytes", SCALED, OUT), ("bright", SCALED, OUT), ("bytes", SCALED, 96)])
def test_the_contrast_statistic_is_bitwise_the_restated_tree(kind, boxes, out, operands):
    """contrast first, after a clamping brightness, after saturation, after both; flips and scaled boxes; sample 3 has no contrast
    op: its word is neither written nor read (the guards beside stat are checked in _aug_patches).  out = 96: 9 216 pixels, every
    thread of the 16 workgroups adds two or three."""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    aug = G.table(STAT_ROWS)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, stat = _aug_patches(lib, dt, _split_px(kind), ROWS, boxes, None, aug, 16, bad, out=out)
    u = G.crop_f32(_source_cpu(kind)[1:1 + N_SPLIT], ROWS, boxes, out, out)
    if kind == "bright":
        assert float((u[1] * np.float32(1.6)).min()) > 255.0           # (the clamp is active everywhere)
    for b in range(B5):
        want = G.stat_f32(u[b], STAT_ROWS[b])
        if want is None:
            assert float(stat[b]) == GUARD, b
        else:
            assert stat[b].numpy().view(np.int32) == np.float32(want).view(np.int32), (b, float(stat[b]), float(want))
    assert int(bad) == 0


# ---- 4. the chain ----------------------------------------------------------------------------------------------------------------
FACTORS = [(0.6, 1.0, 1.4), (1.4, 0.6, 1.0), (1.0, 1.4, 0.6), (0.6, 0.6, 1.4), (1.4, 1.4, 0.6)]
ORDERS = list(itertools.permutations((BR, CO, SA)))


def _reference(kind, boxes, mix, aug, out=OUT):
    from cara_amd.data import aug_reference
    return aug_reference(_source_cpu(kind)[1:1 + N_SPLIT], ROWS, torch.tensor(boxes, dtype=torch.int32), mix, aug, out)


def _chain_errors(kind, boxes, aug):
    """the derived bound of every unmixed, un-normalised element: the crop's E_CROP_BYTES carried through the chain"""
    from cara_amd.data import resized_crop_reference
    x = resized_crop_reference(_source_cpu(kind)[1:1 + N_SPLIT], ROWS, torch.tensor(boxes, dtype=torch.int32), OUT).numpy()
    return np.stack([G.chain_bound(x[b], aug[b], e0=G.E_CROP_BYTES)[1] for b in range(B5)])


def _std():
    from cara_amd.data import IMAGENET_STD
    return np.array(IMAGENET_STD, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)


def _hold(got, ref, e, dt, what):
    """|got - ref| <= e + half a 16-bit spacing (taken at |ref| + e); -> the worst excess over half a spacing as a share of e"""
    ref, e = torch.as_tensor(ref, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64)
    err = (got.cpu().to(torch.float64) - ref).abs()
    half = A._spacing(ref.abs() + e, dt) / 2
    share = float(((err - half).clamp(min=0) / e).max())
    print(f"{what}: max |got - ref| {float(err.max()):.3e}, largest e {float(e.max()):.3e}, worst excess over half a spacing / e {share:.3f}")
    assert bool((err <= e + half).all()), what
    return share


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("p", [16, 8])
def test_all_six_orders_within_the_derived_chain_bound(p, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    worst = 0.0
    for order in ORDERS:
        aug = G.table([G.row(list(zip(order, f))) for f in FACTORS])
        got = A._unpatch(_aug_patches(lib, dt, px, ROWS, SCALED, None, aug, p)[0], p, OUT)
        e = G.normalized_bound(_chain_errors("bytes", SCALED, aug), _std())
        worst = max(worst, _hold(got, _reference("bytes", SCALED, None, aug), e, dt, f"order {order} p {p} [{operands}]"))
    print(f"chain p {p} [{operands}]: worst excess over half a 16-bit spacing as a share of e: {worst:.3f}")


# ---- 5. the partner ------------------------------------------------------------------------------------------------------------
COLOR_ROWS = [G.row([(CO, 1.4), (SA, 0.6)]), G.row([(BR, 0.6)]), G.row([(SA, 1.4), (BR, 1.2), (CO, 0.7)]), G.row([]), G.row([(CO, 0.6), (BR, 1.4)])]


@pytest.mark.parametrize("operands", OPERANDS)
def test_a_partner_brings_its_own_chain(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    aug = G.table(COLOR_ROWS)
    own, _ = _aug_patches(lib, dt, px, ROWS, SCALED, None, aug, 16)
    full = T.table([(q, 0, 0, OUT, OUT, 0.0, 1.0) for q in PARTNERS])
    got, _ = _aug_patches(lib, dt, px, ROWS, SCALED, full, aug, 16)
    assert _same(got, own[PARTNERS]) and not _same(got, own)
    # Mixup m = 0.5, different colour rows on both sides: (1 - m) e_i + m e_p, the blend's three roundings of values <= 255 (mix_model)
    half = T.table([(q, 0, 0, 0, 0, 0.5, 0.5) for q in PARTNERS])
    got = A._unpatch(_aug_patches(lib, dt, px, ROWS, SCALED, half, aug, 16)[0], 16, OUT)
    eb = _chain_errors("bytes", SCALED, aug)
    e = G.normalized_bound(0.5 * eb + 0.5 * eb[PARTNERS] + 3 * 255 * G.U, _std())
    _hold(got, _reference("bytes", SCALED, half, aug), e, dt, f"mixup of two chains [{operands}]")


# ---- 6. / 7. the erase rectangle -------------------------------------------------------------------------------------------------
RECTS = [(0, 5, 7, 9), (OUT - 7, 5, 7, 9), (5, 0, 9, 7), (5, OUT - 7, 9, 7), (13, 17, 1, 1), (6, 3, 13, 11), (0, 0, 1, OUT), (OUT - 1, 0, 1, OUT),
         (3, 3, 0, 9), (0, 0, OUT, OUT), (0, OUT - 1, OUT, 1), (17, 0, 5, 0), (1, 1, OUT - 2, OUT - 2), (2, 9, 3, 4), (30, 30, 2, 2)]


def _inside(rect):
    x0, y0, w, h = rect
    m = torch.zeros(3, OUT, OUT, dtype=torch.bool)
    m[:, y0:y0 + h, x0:x0 + w] = True
    return m


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("p", [16, 8])
def test_const_erase_zeroes_the_rectangle_and_nothing_else(p, operands):
    """each edge, 1 x 1, edges inside a lane's four pixels (x 6 .. 18, 2 .. 4), the whole output, empty ones -- over a jittered
    and mixed batch"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    plain = A._unpatch(_aug_patches(lib, dt, px, ROWS, SCALED, MIXED, G.table(COLOR_ROWS), p)[0], p, OUT).cpu()
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s in range(0, len(RECTS), B5):
        rects = RECTS[s:s + B5]
        aug = G.table([COLOR_ROWS[i][:6] + G.row([], erase=r, eseed=77)[6:] for i, r in enumerate(rects)])
        got = A._unpatch(_aug_patches(lib, dt, px, ROWS, SCALED, MIXED, aug, p, bad)[0], p, OUT).cpu()
        for i, r in enumerate(rects):
            inside = _inside(r)
            assert not got[i][inside].view(torch.int16).any(), r
            assert torch.equal(got[i][~inside].view(torch.int16), plain[i][~inside].view(torch.int16)), r
    assert int(bad) == 0


@pytest.mark.parametrize("operands", OPERANDS)
def test_pixel_erase_is_the_stated_noise(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    rects = [RECTS[5], RECTS[9], RECTS[0], RECTS[12], RECTS[4]]
    colour = G.table(COLOR_ROWS)
    plain = A._unpatch(_aug_patches(lib, dt, px, ROWS, SCALED, MIXED, colour, 16)[0], 16, OUT).cpu()

    def run(seeds):
        aug = G.table([COLOR_ROWS[i][:6] + G.row([], erase=r, emode=1, eseed=s)[6:] for i, (r, s) in enumerate(zip(rects, seeds))])
        return aug, A._unpatch(_aug_patches(lib, dt, px, ROWS, SCALED, MIXED, aug, 16)[0], 16, OUT).cpu()
    seeds = [1, 0xfffffffe, 12345, 0x80000000, 7]
    aug, got = run(seeds)
    ref = _reference("bytes", SCALED, MIXED, aug)
    inside = torch.stack([_inside(r) for r in rects])
    assert torch.equal(got[~inside].view(torch.int16), plain[~inside].view(torch.int16))
    x = ref[inside]
    lo, hi = A._neighbours(x, dt)
    g = got[inside].to(torch.float64)
    ok = (g == lo) | (g == hi)
    nearest = torch.where((x - lo) <= (hi - x), lo, hi)
    print(f"pixel erase [{operands}]: {int((~ok).sum())} of {ok.numel()} elements are no neighbour of the float64 value, "
          f"{int((g != nearest).sum())} ({float((g != nearest).double().mean()):.2e}) are not the nearer one; mean {float(g.mean()):.4f} var {float(g.var()):.4f}")
    assert ok.all(), ok.logical_not().nonzero()[:20].tolist()
    assert torch.equal(run(seeds)[1].view(torch.int16), got.view(torch.int16))                     # the same seeds: the same bits
    other = run([s + 1 for s in seeds])[1]
    assert torch.equal(other[~inside].view(torch.int16), got[~inside].view(torch.int16))
    assert float((other[inside] != got[inside]).double().mean()) > 0.99


# ---- 8. what is refused ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
def test_what_the_aug_kernel_refuses_is_zeroed_counted_once_and_never_read(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    good = [COLOR_ROWS[i][:6] + G.row([], erase=(4, 6, 9, 11), emode=i % 2, eseed=5)[6:] for i in range(B5)]
    mix = T.table([(q, 4, 6, 9, 11, m, m) for q, m in zip(PARTNERS, [0.0, 0.5, 0.0, 0.25, 0.0])])
    want, _ = _aug_patches(lib, dt, px, ROWS, SCALED, mix, G.table(good), 16)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    nan, inf = float("nan"), float("inf")
    e = (4, 6, 9, 11)
    entries = [G.row([(4, 1.0)], e), G.row([(-1, 1.0)], e), G.row([(2 ** 31 - 1, 1.0)], e), G.row([(BR, 1.0), (BR, 0.5)], e),
               G.row([(SA, 1.0), (CO, 1.0), (SA, 1.0)], e), G.row([(BR, -0.1)], e), G.row([(CO, nan)], e), G.row([(SA, inf)], e),
               G.row([(0, 0.0), (0, 0.0), (BR, -1.0)], e),
               G.row([], (-1, 6, 9, 11)), G.row([], (4, -1, 9, 11)), G.row([], (OUT - 8, 6, 9, 11)), G.row([], (4, OUT - 10, 9, 11)),
               G.row([], (4, 6, -9, 11)), G.row([], (4, 6, 9, -1)), G.row([], (1, 6, 2 ** 31 - 1, 11)), G.row([], (4, 2 ** 31 - 1, 9, 1)),
               G.row([], e, emode=2), G.row([], e, emode=-1),
               G.row([], e, pad=(1, 0, 0, 0)), G.row([], e, pad=(0, 0, 0, -1)), G.row([], e, pad=(0, 2, 0, 0)), G.row([], e, pad=(0, 0, 3, 0))]
    total = 0
    # sample 2 is nobody's partner: only it goes bad
    assert 2 not in [q for i, q in enumerate(PARTNERS) if i != 2]
    for entry in entries:
        rows_ = list(good)
        rows_[2] = entry
        got, _ = _aug_patches(lib, dt, px, ROWS, SCALED, mix, G.table(rows_), 16, bad)
        total += 1
        assert int(bad) == total, entry
        assert not got[2].view(torch.int16).any(), entry
        assert _same(got[[0, 1, 3, 4]], want[[0, 1, 3, 4]]), entry
    # a factor is not read where its op is 0
    rows_ = list(good)
    rows_[3] = [0, G.bits(nan), 0, G.bits(-1.0), 0, -1] + good[3][6:]
    assert _same(_aug_patches(lib, dt, px, ROWS, SCALED, mix, G.table(rows_), 16, bad)[0], want) and int(bad) == total
    # a bad partner row (sample 4 is sample 1's partner): both, once each; a bad source row of a partner likewise
    rows_ = list(good)
    rows_[4] = entries[0]
    got, _ = _aug_patches(lib, dt, px, ROWS, SCALED, mix, G.table(rows_), 16, bad)
    total += 2
    assert int(bad) == total and not got[1].view(torch.int16).any() and not got[4].view(torch.int16).any()
    assert _same(got[[0, 2, 3]], want[[0, 2, 3]])
    got, _ = _aug_patches(lib, dt, px, ROWS[:4] + [N_SPLIT], SCALED, mix, G.table(good), 16, bad)
    total += 2
    assert int(bad) == total and not got[1].view(torch.int16).any() and not got[4].view(torch.int16).any()
    assert _same(got[[0, 2, 3]], want[[0, 2, 3]])
    # a NULL counter is allowed
    rows_ = list(good)
    rows_[2] = entries[5]
    got, _ = _aug_patches(lib, dt, px, ROWS, SCALED, mix, G.table(rows_), 16, None)
    assert not got[2].view(torch.int16).any() and _same(got[[0, 1, 3, 4]], want[[0, 1, 3, 4]])
    # the refusals: status 1, nothing launched (the output, the scratch and the counter stay as they are)
    P = L().ptr
    idx = torch.tensor(ROWS, device=DEV)
    bx = torch.tensor(SCALED, dtype=torch.int32, device=DEV)
    mx, ag = mix.to(DEV), G.table(good).to(DEV)
    mean, std = A._norm()
    out = torch.full((B5 * 4 * 40 * 40,), SENTINEL, dtype=torch.int16, device=DEV)
    stat = torch.full((B5 * (1 + G.GROUPS) + 1,), GUARD, device=DEV)
    a = dict(pixels=P(px), n=N_SPLIT, Hs=HS, Ws=WS, rows=P(idx), boxes=P(bx), mix=P(mx), aug=P(ag), stat=P(stat), mean=P(mean), std=P(std),
             out=P(out), B=B5, C=3, Hi=OUT, Wi=OUT, p=16)

    def call(**kw):
        v = dict(a, **kw)
        return lib.cara_im2col_patches_u8_rows_aug(v["pixels"], v["n"], v["Hs"], v["Ws"], v["rows"], v["boxes"], v["mix"], v["aug"], v["stat"],
                                                   v["mean"], v["std"], v["out"], P(bad), v["B"], v["C"], v["Hi"], v["Wi"], v["p"], L().stream())
    for name in ("pixels", "rows", "stat", "mean", "std", "out"):
        assert call(**{name: None}) == 1, name
    assert call(stat=P(stat.view(torch.int8)[2:])) == 1                                # the scratch is fp32 words
    assert call(boxes=None) == 1                                                        # no boxes: the split must have the output's size
    assert call(C=1) == 1 and call(C=4) == 1                                            # the colour ops are defined on three channels
    assert call(n=0) == 1 and call(Hs=0) == 1 and call(Ws=-4) == 1 and call(B=0) == 1
    assert call(p=6, Hi=36, Wi=36) == 1 and call(p=2) == 1 and call(p=0) == 1 and call(Hi=40) == 1 and call(Wi=40) == 1
    assert call(B=2 ** 20, Hi=32, Wi=32) == 1                                           # 2 B C Hi Wi > 2^32
    torch.cuda.synchronize()
    assert int(bad) == total and bool((out == SENTINEL).all()) and bool((stat == GUARD).all())


# ---- whole model -----------------------------------------------------------------------------------------------------------------
DEPTH, N_MODEL, SRC, IMG, BATCH = A.DEPTH, A.N_MODEL, A.SRC, A.IMG, A.BATCH
STEP_ROWS = [G.row([(CO, 1.3), (SA, 0.7), (BR, 1.1)], erase=(3, 5, 11, 9), emode=1, eseed=99), G.row([(BR, 0.8)]),
             G.row([(SA, 1.4), (CO, 0.6)], erase=(20, 0, 12, 32), emode=0), G.row([], erase=(0, 28, 32, 4), emode=1, eseed=3)]


def _one_step(precision, split, idx, dp, boxes=None, mix=None, aug=None, eps=0.0, opt=True):
    from cara_amd.optim import AdamW
    m = A._model(precision).train()
    eng = m._cara_engine
    o = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4) if opt else None
    kw = {k: v for k, v in (("boxes", boxes), ("mix", mix), ("aug", aug)) if v is not None}
    if eps:
        kw["label_smoothing"] = eps
    loss = eng.train_step_resident(split, idx, o, droppath=dp, **kw).clone()
    assert eng.resident_bad_rows() == 0
    return loss, eng._flat_grad.clone(), A._trainable(m), m


@pytest.mark.parametrize("precision", OPERANDS)
def test_step_with_an_all_zero_aug_table_is_bitwise_the_step_without(precision):
    from cara_amd.data import identity_aug
    idx = torch.tensor([7, 0, 7, 11], device=DEV)
    boxes = A._same_size_boxes(BATCH, seed=1).to(DEV)
    mix = T.table([(3 - i, 2, 3, 9, 11, 0.0, 0.1) if i % 2 else (3 - i, 0, 0, 0, 0, 0.3, 0.3) for i in range(BATCH)]).to(DEV)
    dp = T._dp(2)
    zero = identity_aug(BATCH).to(DEV)
    A._assert_same_step(_one_step(precision, A._split(), idx, dp, boxes, mix, zero, 0.1), _one_step(precision, A._split(), idx, dp, boxes, mix, None, 0.1))
    A._assert_same_step(_one_step(precision, A._split(), idx, dp, boxes, None, zero), _one_step(precision, A._split(), idx, dp, boxes))


@pytest.mark.parametrize("precision", OPERANDS)
def test_augmented_step_against_the_oracle(precision):
    """jittered, erased, mixed and smoothed: the loss and every CP / head gradient against fp32 autograd of the oracle's as-written
    model fed aug_reference with soft_target, at the bars the mixed step's test holds (tests/mix_model.LOSS_BAR, grad_bar)"""
    import torch.nn.functional as F
    from cara_amd.data import aug_reference, soft_target
    from oracle import cara_oracle as O
    from tests.test_model_gpu import grad_bar, rel
    eps = 0.1
    rows = [7, 0, 3, 11]
    px, labels = A._split_cpu()
    boxes = torch.tensor([(0, 0, SRC, SRC, 0), (5, 9, 30, 37, 1), (16, 16, IMG, IMG, 0), (3, 2, 41, 20, 1)], dtype=torch.int32)
    mix = T.table([(3, 0, 0, 0, 0, 0.3, 0.3), (2, 4, 8, 20, 16, 0.0, 20 * 16 / IMG ** 2), (1, 0, 0, 0, 0, 0.75, 0.75), (0, 11, 0, 9, 32, 0.0, 9 / 32)])
    aug = G.table(STEP_ROWS)
    idx, dp = torch.tensor(rows, device=DEV), T._dp(5)
    loss, flat, _, m = _one_step(precision, A._split(), idx, dp, boxes.to(DEV), mix.to(DEV), aug.to(DEV), eps, opt=False)
    plain = _one_step(precision, A._split(), idx, dp, boxes.to(DEV), mix.to(DEV), None, eps, opt=False)[0]
    assert not torch.equal(loss, plain)
    x = aug_reference(px, rows, boxes, mix, aug, IMG).float()
    q = soft_target(labels[rows], mix, 100, float(torch.tensor(eps, dtype=torch.float32))).float()
    w, cp = A._weights()
    cps = {k: v.clone().requires_grad_(True) for k, v in cp.items()}
    cps["CP_A1"], cps["CP_P1"] = cp["CP_A1"][:3 * DEPTH].clone().requires_grad_(True), cp["CP_P1"][:9 * DEPTH].clone().requires_grad_(True)
    ww = dict(w)
    ww["head.weight"], ww["head.bias"] = w["head.weight"].clone().requires_grad_(True), w["head.bias"].clone().requires_grad_(True)
    rlogits = O.vit_cara_forward(x, ww, cps, s=0.1, depth=DEPTH, drop_path_keep=dp.cpu())
    rloss = -(q * F.log_softmax(rlogits, 1)).sum(1).mean()
    rloss.backward()
    worst = max(rel(getattr(m, n).grad, cps[n].grad) for n in O.CP_NAMES)
    rh = max(rel(m.head.weight.grad, ww["head.weight"].grad), rel(m.head.bias.grad, ww["head.bias"].grad))
    print(f"augmented step [{precision}]: loss {loss.item():.5f} vs oracle {rloss.item():.5f}; worst CP-gradient rel-L2 {worst:.2e}, head {rh:.2e}")
    assert abs(loss.item() - rloss.item()) < M.LOSS_BAR[precision] * max(1.0, abs(rloss.item())), (loss.item(), rloss.item())
    assert worst < grad_bar(precision) and rh < grad_bar(precision)
    assert bool(flat[:-1].any())


@pytest.mark.parametrize("precision", OPERANDS)
def test_graph_replay_rereads_the_aug_table(precision):
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    split = A._split()
    g = torch.Generator().manual_seed(8)
    rows = [torch.randint(0, N_MODEL, (BATCH,), generator=g).to(DEV) for _ in range(4)]
    boxes = [A._same_size_boxes(BATCH, seed=20 + i).to(DEV) for i in range(4)]
    mixes = [T.table([(3 - i, 0, 0, 0, 0, 0.2 * k + 0.1, 0.2 * k + 0.1) for i in range(BATCH)]).to(DEV) for k in range(4)]
    augs = [G.table([STEP_ROWS[(i + k) % BATCH][:11] + [k] + [0, 0, 0, 0] for i in range(BATCH)]).to(DEV) for k in range(4)]
    rows[3], boxes[3], mixes[3] = rows[2], boxes[2], mixes[2]          # the last replay differs from the one before in its aug table alone
    out = {}
    for mode in ("eager", "graph"):
        m = A._model(precision, drop_path_rate=0.0).train()
        eng = m._cara_engine
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        gstep = GraphedTrainStep(eng, opt, label_smoothing=0.1) if mode == "graph" else None
        losses = []
        for it in range(4):                             # warm, capture + replay, replay, replay
            opt.param_groups[0]["lr"] = 1e-3 * (0.7 ** it)
            if gstep is not None:
                loss = gstep(split, (rows[it], boxes[it], mixes[it], augs[it]))
            else:
                opt.advance()
                loss = eng.train_step_resident(split, rows[it], opt, boxes=boxes[it], mix=mixes[it], aug=augs[it], label_smoothing=0.1)
            losses.append(loss.item())
        if gstep is not None:
            (ent,) = gstep._graphs.values()
            assert ent[1] is split and sum(t.numel() * t.element_size() for t in ent[2]) == (8 + 20 + 32 + 64) * BATCH
        assert eng.resident_bad_rows() == 0 and eng.skipped_steps == 0
        out[mode] = (losses, A._trainable(m))
    print(f"[{precision}] losses eager {out['eager'][0]} graph {out['graph'][0]}")
    assert out["graph"][0] == out["eager"][0] and len(set(out["eager"][0])) == 4
    for n in out["eager"][1]:
        assert torch.equal(out["graph"][1][n], out["eager"][1][n]), n


@pytest.mark.parametrize("precision", OPERANDS)
def test_fit_over_rows_boxes_mix_and_aug_tables(precision):
    from cara_amd.data import ColorJitterErase, MixupCutmix, RandomResizedCropFlip
    from cara_amd.recipe import fit
    split = A._split()
    m = A._model(precision)
    start = A._trainable(m)
    feed = split.train_rows(BATCH, seed=5, rank=0, world=1, augment=RandomResizedCropFlip(IMG), mix=MixupCutmix(IMG),
                            color=ColorJitterErase(IMG, erase_prob=0.5))
    seen = [item for e in range(2) for item in feed(e)]
    assert len(seen) == 6 and all(len(item) == 4 for item in seen) and len({tuple(item[3].reshape(-1).tolist()) for item in seen}) == 6
    assert any(int(item[3][:, 8].max()) > 0 for item in seen)
    fit(m, (split, feed), None, epochs=2, lr=1e-3, seed=5, feed="resident", label_smoothing=0.1)
    eng = m._cara_engine
    assert torch.isfinite(eng._loss_buf[0]) and float(eng._loss_buf[0]) > 0 and eng.resident_bad_rows() == 0
    after = A._trainable(m)
    assert all(torch.isfinite(after[n]).all() for n in after) and any(not torch.equal(after[n], start[n]) for n in after)
