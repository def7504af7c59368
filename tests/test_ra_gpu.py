"""GPU side of the RandAugment feed.  cara_im2col_patches_u8_rows_ra: an identity table bitwise against the calls without one; every
lookup op alone, every two-slot order of a statistic and a fixed op, the geometry alone and with slots bitwise against the numpy
restatement of tests/ra_model.py, the byte tables in the scratch too; a poisoned scratch; partners; kept rows; every guard.  Whole
model: train_step_resident / GraphedTrainStep / fit with an ra table against the calls without one (bitwise) and against fp32
autograd of the oracle's as-written model on data.ra_reference.  Every test on both operand builds."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import aug_model as G
from tests import mix_model as M
from tests import ra_model as R
from tests import test_aug_gpu as TA
from tests import test_augmented_feed_gpu as A
from tests import test_mix_gpu as T
from tests.test_augmented_feed_gpu import DEV, SENTINEL, L

pytestmark = pytest.mark.gpu
OPERANDS = ["bf16", "fp16"]
HS, WS = 37, 41
N_SPLIT, OUT = 6, 32
ROWS = [2, 0, 5, 2, 4]                         # B = 5
B5 = len(ROWS)
SAME = [(0, 0, OUT, OUT, 0), (WS - OUT, HS - OUT, OUT, OUT, 1), (5, 3, OUT, OUT, 0), (0, HS - OUT, OUT, OUT, 1), (WS - OUT, 0, OUT, OUT, 0)]
SCALED = [(0, 0, WS, HS, 0), (11, 9, 13, 13, 1), (3, 2, 35, 13, 0), (WS - 9, 0, 9, HS, 1), (4, 1, 31, 33, 1)]
GROUPS = 8                                     # RA_GROUPS of feed.hip
GUARD = 0x5b
_same = T._same


@functools.lru_cache(maxsize=None)
def _source_cpu():
    """eight images of 37 x 41 of which the split is the middle six; every byte value in every channel"""
    g = torch.Generator().manual_seed(29)
    px = torch.randint(0, 256, (N_SPLIT + 2, 3, HS, WS), generator=g, dtype=torch.uint8)
    px.view(N_SPLIT + 2, 3, -1)[:, :, :256] = torch.arange(256, dtype=torch.uint8)
    return px


def _split_cpu():
    return _source_cpu()[1:1 + N_SPLIT]


def _split_px():
    return _source_cpu().to(DEV)[1:1 + N_SPLIT]


def _square():
    sq = _source_cpu()[:, :, 3:3 + OUT, 5:5 + OUT].contiguous()
    return sq[1:1 + N_SPLIT], sq.to(DEV)[1:1 + N_SPLIT]


def _norm_cpu():
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD
    return np.array(IMAGENET_MEAN, dtype=np.float32), np.array(IMAGENET_STD, dtype=np.float32)


def _ra_patches(lib, dt, px, rows, boxes, mix, aug, ra, p, bad=None, out=OUT, n_split=N_SPLIT, keep=None, poison=None):
    """cara_im2col_patches_u8_rows_ra into a buffer between two sentinel guards, its scratch between two guard bytes runs (all checked
    here) -> ([B, patches or K, 3 p p] of dt, the byte tables uint8 [B,3,256] on the host: `poison` or GUARD where nothing was written)"""
    B = len(rows)
    idx = torch.tensor(rows, device=DEV)
    bx = None if boxes is None else torch.tensor(boxes, dtype=torch.int32, device=DEV)
    mx = None if mix is None else mix.to(DEV)
    ag = None if aug is None else aug.to(DEV)
    rt = None if ra is None else ra.to(DEV)
    kp = None if keep is None else torch.tensor(keep, dtype=torch.int32, device=DEV)
    K = 0 if keep is None else kp.shape[1]
    mean, std = A._norm()
    per = K if keep is not None else (out // p) ** 2
    nel = B * per * 3 * p * p
    buf = torch.full((nel + 128,), SENTINEL, dtype=torch.int16, device=DEV)
    got = buf[64:64 + nel]
    nst = int(lib.cara_ra_stat_bytes(B))
    assert nst == B * 768 * (1 + 4 * GROUPS)
    sbuf = torch.full((nst + 128,), GUARD if poison is None else poison, dtype=torch.uint8, device=DEV)
    sbuf[:64] = GUARD
    sbuf[64 + nst:] = GUARD
    stat = torch.full((int(lib.cara_aug_stat_bytes(B)) // 4,), TA.GUARD, device=DEV)
    P = L().ptr
    L().check(lib.cara_im2col_patches_u8_rows_ra(P(px), n_split, px.shape[2], px.shape[3], P(idx), P(bx), P(mx), P(ag), P(stat) if aug is not None else None,
                                                 P(rt), P(sbuf[64:]) if ra is not None else None, P(kp), K, P(mean), P(std), P(got),
                                                 P(bad) if bad is not None else None, B, 3, out, out, p, L().stream()),
              "cara_im2col_patches_u8_rows_ra")
    torch.cuda.synchronize()
    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + nel:] == SENTINEL).all())
    assert bool((sbuf[:64] == GUARD).all()) and bool((sbuf[64 + nst:] == GUARD).all())
    return got.view(dt).view(B, per, 3 * p * p), sbuf[64:64 + B * 768].view(B, 3, 256).cpu()


def _ident(B=B5):
    from cara_amd.data import identity_ra
    return identity_ra(B)


def _model_rows(px_cpu, rows, boxes, mix, aug, ra, p, dt, out=OUT, keep=None):
    mean, std = _norm_cpu()
    img, tables, _ = R.feed_f32(px_cpu, rows, boxes, None if mix is None else mix.tolist(), None if aug is None else aug.tolist(), ra.tolist(),
                                out, out, mean, std)
    return R.patch_rows(img, p, dt, keep), tables


def _check_tables(lut, tables, blank=GUARD):
    for b, t in enumerate(tables):
        if t is None:
            assert bool((lut[b] == blank).all()), b          # no statistic slot: nothing written
        else:
            assert (lut[b].numpy().astype(np.int64) == t).all(), b


MIXED = T.table([(3, 0, 0, 0, 0, 0.25, 0.25), (4, 6, 3, 13, 11, 0.0, 0.1), (0, 0, 0, 0, 0, 0.5, 0.5), (3, 0, 0, 0, 0, 0.0, 0.0), (1, 0, 5, OUT, 9, 0.0, 0.2)])
KEEP = [[3, 0], [1, 2], [0, 3], [2, 2 ^ 1], [1, 0]]    # p = 16: a grid of four patches, K = 2


# ---- 1. the identity table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("p", [16, 8])
def test_an_identity_table_gives_the_patch_rows_of_the_call_without_it(p, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    _, sq = _square()
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    aug = G.table(TA.COLOR_ROWS[:4] + [G.row([(TA.CO, 0.6), (TA.BR, 1.4)], erase=(4, 6, 9, 11), emode=1, eseed=5)])
    for boxes in (SAME, SCALED):
        crop = A._crop_patches(lib, dt, px, ROWS, boxes, p, out=OUT, n_split=N_SPLIT)
        got, lut = _ra_patches(lib, dt, px, ROWS, boxes, None, None, _ident(), p, bad)
        assert _same(got, crop) and bool((lut == GUARD).all())
        assert _same(_ra_patches(lib, dt, px, ROWS, boxes, None, None, None, p, bad)[0], crop)          # no table: the call without
        want = T._mix_patches(lib, dt, px, ROWS, boxes, MIXED, p, out=OUT, n_split=N_SPLIT)
        assert _same(_ra_patches(lib, dt, px, ROWS, boxes, MIXED, None, _ident(), p, bad)[0], want) and not _same(want, crop)
        want, _ = TA._aug_patches(lib, dt, px, ROWS, boxes, MIXED, aug, p, out=OUT, n_split=N_SPLIT)
        assert _same(_ra_patches(lib, dt, px, ROWS, boxes, MIXED, aug, _ident(), p, bad)[0], want)
        assert _same(_ra_patches(lib, dt, px, ROWS, boxes, MIXED, aug, None, p, bad)[0], want)
        want, _ = TA._aug_patches(lib, dt, px, ROWS, boxes, None, aug, p, out=OUT, n_split=N_SPLIT)
        assert _same(_ra_patches(lib, dt, px, ROWS, boxes, None, aug, _ident(), p, bad)[0], want)
    if p == 16:
        dense, _ = TA._aug_patches(lib, dt, px, ROWS, SCALED, MIXED, aug, p, out=OUT, n_split=N_SPLIT)
        want = torch.stack([dense[b][torch.tensor(KEEP[b], device=DEV)] for b in range(B5)])
        assert _same(_ra_patches(lib, dt, px, ROWS, SCALED, MIXED, aug, _ident(), p, bad, keep=KEEP)[0], want)
        assert _same(_ra_patches(lib, dt, px, ROWS, SCALED, MIXED, aug, None, p, bad, keep=KEEP)[0], want)
    # without boxes
    want = T._mix_patches(lib, dt, sq, ROWS, None, MIXED, p, out=OUT, n_split=N_SPLIT)
    assert _same(_ra_patches(lib, dt, sq, ROWS, None, MIXED, None, _ident(), p, bad)[0], want)
    assert int(bad) == 0


# ---- 2. the ops and the geometry, to the bit ----------------------------------------------------------------------------------------
def _rot(deg, cx=OUT / 2, cy=OUT / 2):
    t = -math.radians(deg)
    c, s = math.cos(t), math.sin(t)
    return (c, s, cx - (c * cx + s * cy), -s, c, cy - (-s * cx + c * cy))


FIXED = [(R.POSTERIZE, 3), (R.SOLARIZE, 100), (R.SOLARIZE_ADD, 60), (R.INVERT, 0)]
SINGLE = [[(R.POSTERIZE, 3)], [(R.SOLARIZE, 100)], [(R.SOLARIZE_ADD, 60)], [(R.INVERT, 0)], [(R.AUTOCONTRAST, 0)],
          [(R.EQUALIZE, 0)], [(R.POSTERIZE, 0)], [(R.POSTERIZE, 8)], [(R.SOLARIZE, 0)], [(R.SOLARIZE, 256)]]
ORDERS = [[(s, 0), f] for s in (R.AUTOCONTRAST, R.EQUALIZE) for f in FIXED] + [[f, (s, 0)] for s in (R.AUTOCONTRAST, R.EQUALIZE) for f in FIXED]
MATRICES = [_rot(20), (1, 0.3, 0, 0, 1, 0), (1, 0, 5, 0, 1, -3), (1, 0, -2.25, 0.1, 0.9, 1.5), (0, 1, 0, -1, 0, OUT)]
FILL = 0x7C7468


def _tables():
    """[(name, ra table of five rows)]"""
    out = [("single %d" % i, R.table([R.row(s) for s in SINGLE[i:i + 5]])) for i in (0, 5)]
    out += [("orders %d" % i, R.table([R.row(s) for s in (ORDERS + ORDERS[:4])[i:i + 5]])) for i in (0, 5, 10, 15)]
    out.append(("geometry", R.table([R.row([], m, FILL) for m in MATRICES])))
    slots = [[(R.EQUALIZE, 0), (R.POSTERIZE, 4)], [(R.SOLARIZE, 128), (R.AUTOCONTRAST, 0), (R.INVERT, 0)], [(R.INVERT, 0)],
             [(R.SOLARIZE_ADD, 110), (R.POSTERIZE, 2), (R.EQUALIZE, 0)], [(R.AUTOCONTRAST, 0)]]
    out.append(("geometry and slots", R.table([R.row(s, m, FILL) for s, m in zip(slots, MATRICES)])))
    return out


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("p,out", [(16, OUT), (8, OUT), (16, 64)])
def test_ops_and_geometry_are_bitwise_the_restatement(p, out, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px, cpu = _split_px(), _split_cpu()
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for name, ra in _tables():
        if out != OUT and not name.startswith(("geometry", "orders 0")):
            continue
        if out != OUT:      # (the rotations and the quarter turn about the larger image's centre)
            ra = ra.clone()
            for b in (0, 4):
                if not R.is_identity(ra[b].tolist()):
                    ra[b, 6:12] = torch.tensor(R.row([], _rot(20, out / 2, out / 2) if b == 0 else (0, 1, 0, -1, 0, out))[6:12], dtype=torch.int32)
        for boxes in (SAME, SCALED):
            got, lut = _ra_patches(lib, dt, px, ROWS, boxes, None, None, ra, p, bad, out=out)
            want, tables = _model_rows(cpu, ROWS, boxes, None, None, ra, p, dt, out=out)
            differ = got.cpu().view(torch.int16) != want.view(torch.int16)
            print(f"{name} p {p} out {out} [{operands}] boxes {'same' if boxes is SAME else 'scaled'}: {int(differ.sum())} of {differ.numel()} differ")
            assert not differ.any(), (name, differ.nonzero()[:10].tolist())
            _check_tables(lut, tables)
    assert int(bad) == 0


@pytest.mark.parametrize("operands", OPERANDS)
def test_a_poisoned_scratch_changes_nothing(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    for name, ra in _tables()[2:4] + _tables()[-1:]:
        clean, lut = _ra_patches(lib, dt, px, ROWS, SCALED, MIXED, None, ra, 16)
        dirty, lut_ff = _ra_patches(lib, dt, px, ROWS, SCALED, MIXED, None, ra, 16, poison=0xFF)
        assert _same(clean, dirty), name
        written = (lut != GUARD).flatten(1).any(1)
        assert bool((lut[written] == lut_ff[written]).all()) and bool((lut_ff[~written] == 0xFF).all()), name


# ---- 3. partners, the jitter chain behind the ra row, kept rows ------------------------------------------------------------------------
PARTNER_RA = [R.row([(R.EQUALIZE, 0)], _rot(-15), FILL), R.row([(R.INVERT, 0), (R.AUTOCONTRAST, 0)]), R.row([], (1, 0, 4, 0, 1, 0), 0x102030),
              R.row([(R.SOLARIZE, 90)], (1, 0.2, 0, 0, 1, 0), FILL), R.row()]
PARTNER_AUG = [G.row([(TA.CO, 1.3), (TA.SA, 0.7)]), G.row([(TA.BR, 0.8)], erase=(3, 5, 11, 9)), G.row([(TA.SA, 1.4), (TA.CO, 0.6), (TA.BR, 1.2)]),
               G.row([]), G.row([(TA.CO, 0.6)], erase=(20, 0, 12, 32))]


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("p", [16, 8])
def test_a_partner_brings_its_own_row_tables_and_chain(p, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px, cpu = _split_px(), _split_cpu()
    ra = R.table(PARTNER_RA)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for aug in (None, G.table(PARTNER_AUG)):
        got, lut = _ra_patches(lib, dt, px, ROWS, SCALED, MIXED, aug, ra, p, bad)
        want, tables = _model_rows(cpu, ROWS, SCALED, MIXED, aug, ra, p, dt)
        differ = got.cpu().view(torch.int16) != want.view(torch.int16)
        print(f"partners p {p} [{operands}] aug {aug is not None}: {int(differ.sum())} of {differ.numel()} differ")
        assert not differ.any(), differ.nonzero()[:10].tolist()
        _check_tables(lut, tables)
        # and the mix matters: sample 1 has sample 4's pixels in its rectangle, sample 0 a quarter of sample 3
        alone, _ = _ra_patches(lib, dt, px, ROWS, SCALED, None, aug, ra, p, bad)
        assert not _same(alone[0], got[0]) and not _same(alone[1], got[1]) and _same(alone[3], got[3])
    assert int(bad) == 0


@pytest.mark.parametrize("operands", OPERANDS)
def test_kept_rows_are_the_dense_rows_and_the_histogram_is_of_the_whole_image(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    ra, aug = R.table(PARTNER_RA), G.table(PARTNER_AUG)
    for p, keep in ((16, KEEP), (8, [[15, 0, 7], [1, 2, 3], [9, 9 + 1, 4], [12, 5, 6], [0, 15, 8]])):
        dense, lut = _ra_patches(lib, dt, px, ROWS, SCALED, MIXED, aug, ra, p)
        kept, lut_k = _ra_patches(lib, dt, px, ROWS, SCALED, MIXED, aug, ra, p, keep=keep)
        want = torch.stack([dense[b][torch.tensor(keep[b], device=DEV)] for b in range(B5)])
        assert _same(kept, want) and torch.equal(lut, lut_k)


# ---- 4. what the kernel refuses --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
def test_what_the_ra_kernel_refuses_is_zeroed_counted_once_and_never_read(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _split_px()
    good = list(PARTNER_RA)
    partners = [3, 4, 0, 3, 1]
    mix = T.table([(q, 4, 6, 9, 11, m, m) for q, m in zip(partners, [0.0, 0.5, 0.0, 0.25, 0.0])])
    aug = G.table(PARTNER_AUG)
    want, _ = _ra_patches(lib, dt, px, ROWS, SCALED, mix, aug, R.table(good), 16)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    nan, inf = float("nan"), float("inf")
    entries = [R.row([(7, 0)]), R.row([(-1, 0)]), R.row([(2 ** 31 - 1, 0)]), R.row([(0, 1)]), R.row([(R.POSTERIZE, 9)]), R.row([(R.POSTERIZE, -1)]),
               R.row([(R.SOLARIZE, 257)]), R.row([(R.SOLARIZE_ADD, 256)]), R.row([(R.INVERT, 1)]), R.row([(R.AUTOCONTRAST, 1)]),
               R.row([(R.EQUALIZE, -2 ** 31)]), R.row([(R.EQUALIZE, 0), (R.AUTOCONTRAST, 0)]), R.row([(R.EQUALIZE, 0), (R.INVERT, 0), (R.EQUALIZE, 0)]),
               R.row(matrix=(nan, 0, 0, 0, 1, 0)), R.row(matrix=(1, 0, inf, 0, 1, 0)), R.row(matrix=(1, 0, 0, 0, 1, -inf)),
               R.row(matrix=(1, 0, 32769, 0, 1, 0)), R.row(matrix=(1, 0, 0, -4e4, 1, 0)), R.row(fill=0x1000000), R.row(fill=-1),
               R.row(pad=(1, 0, 0)), R.row(pad=(0, -1, 0)), R.row(pad=(0, 0, 2))]
    total = 0
    assert 2 not in [q for i, q in enumerate(partners) if i != 2]      # sample 2 is nobody's partner: only it goes bad
    for entry in entries:
        rows_ = list(good)
        rows_[2] = entry
        got, _ = _ra_patches(lib, dt, px, ROWS, SCALED, mix, aug, R.table(rows_), 16, bad)
        total += 1
        assert int(bad) == total, entry
        assert not got[2].view(torch.int16).any(), entry
        assert _same(got[[0, 1, 3, 4]], want[[0, 1, 3, 4]]), entry
    # the largest matrix words are taken: everything falls outside, the image is the fill
    rows_ = list(good)
    rows_[2] = R.row([], (32768, 0, 0, 0, -32768, 0), 0x102030)
    got, _ = _ra_patches(lib, dt, px, ROWS, SCALED, mix, aug, R.table(rows_), 16, bad)
    assert int(bad) == total and got[2].view(torch.int16).any() and _same(got[[0, 1, 3, 4]], want[[0, 1, 3, 4]])
    # a bad partner row (sample 4 is sample 1's partner): both, once each; then a bad source row and a bad box of a sample with a
    # statistic slot
    rows_ = list(good)
    rows_[4] = entries[0]
    got, _ = _ra_patches(lib, dt, px, ROWS, SCALED, mix, aug, R.table(rows_), 16, bad)
    total += 2
    assert int(bad) == total and not got[1].view(torch.int16).any() and not got[4].view(torch.int16).any()
    assert _same(got[[0, 2, 3]], want[[0, 2, 3]])
    rows_ = list(good)
    rows_[2] = R.row([(R.EQUALIZE, 0)], _rot(5), FILL)                 # (sample 2 is nobody's partner; its pre-pass then reads no pixel)
    for outside in (N_SPLIT, -1, 2 ** 40):
        got, _ = _ra_patches(lib, dt, px, ROWS[:2] + [outside] + ROWS[3:], SCALED, mix, aug, R.table(rows_), 16, bad)
        total += 1
        assert int(bad) == total and not got[2].view(torch.int16).any() and _same(got[[0, 1, 3, 4]], want[[0, 1, 3, 4]])
    boxes_ = list(SCALED)
    boxes_[2] = (WS - 34, 2, 35, 13, 0)
    got, _ = _ra_patches(lib, dt, px, ROWS, boxes_, mix, aug, R.table(rows_), 16, bad)
    total += 1
    assert int(bad) == total and not got[2].view(torch.int16).any() and _same(got[[0, 1, 3, 4]], want[[0, 1, 3, 4]])
    # a NULL counter is allowed
    rows_ = list(good)
    rows_[2] = entries[5]
    got, _ = _ra_patches(lib, dt, px, ROWS, SCALED, mix, aug, R.table(rows_), 16, None)
    assert not got[2].view(torch.int16).any() and _same(got[[0, 1, 3, 4]], want[[0, 1, 3, 4]])
    # the refusals: status 1, nothing launched (the output, the scratch and the counter stay as they are)
    P = L().ptr
    idx = torch.tensor(ROWS, device=DEV)
    bx = torch.tensor(SCALED, dtype=torch.int32, device=DEV)
    mx, ag, rt = mix.to(DEV), aug.to(DEV), R.table(good).to(DEV)
    mean, std = A._norm()
    out = torch.full((B5 * 4 * 40 * 40,), SENTINEL, dtype=torch.int16, device=DEV)
    stat = torch.full((B5 * (1 + G.GROUPS) + 1,), TA.GUARD, device=DEV)
    scr = torch.full((int(lib.cara_ra_stat_bytes(B5)) + 8,), GUARD, dtype=torch.uint8, device=DEV)
    kp = torch.tensor(KEEP, dtype=torch.int32, device=DEV)
    a = dict(pixels=P(px), n=N_SPLIT, Hs=HS, Ws=WS, rows=P(idx), boxes=P(bx), mix=P(mx), aug=P(ag), stat=P(stat), ra=P(rt), scr=P(scr), keep=None, K=0,
             mean=P(mean), std=P(std), out=P(out), B=B5, C=3, Hi=OUT, Wi=OUT, p=16)

    def call(**kw):
        v = dict(a, **kw)
        return lib.cara_im2col_patches_u8_rows_ra(v["pixels"], v["n"], v["Hs"], v["Ws"], v["rows"], v["boxes"], v["mix"], v["aug"], v["stat"], v["ra"],
                                                  v["scr"], v["keep"], v["K"], v["mean"], v["std"], v["out"], P(bad), v["B"], v["C"], v["Hi"], v["Wi"],
                                                  v["p"], L().stream())
    for name in ("pixels", "rows", "stat", "scr", "mean", "std", "out"):
        assert call(**{name: None}) == 1, name
    assert call(scr=P(scr[2:])) == 1                                                    # the scratch holds int32 partials
    assert call(boxes=None) == 1                                                        # no boxes: the split must have the output's size
    assert call(C=1) == 1 and call(C=4) == 1 and call(C=1, aug=None, stat=None) == 1    # fill and tables are of three channels
    assert call(n=0) == 1 and call(Hs=0) == 1 and call(Ws=-4) == 1 and call(B=0) == 1
    assert call(p=6, Hi=36, Wi=36) == 1 and call(p=2) == 1 and call(p=0) == 1 and call(Hi=40) == 1 and call(Wi=40) == 1
    assert call(keep=P(kp), K=0) == 1 and call(keep=P(kp), K=5) == 1
    assert int(lib.cara_ra_stat_bytes(0)) == 0 and int(lib.cara_ra_stat_bytes(-3)) == 0
    torch.cuda.synchronize()
    assert int(bad) == total and bool((out == SENTINEL).all()) and bool((stat == TA.GUARD).all()) and bool((scr == GUARD).all())


# ---- whole model -----------------------------------------------------------------------------------------------------------------
DEPTH, N_MODEL, SRC, IMG, BATCH = A.DEPTH, A.N_MODEL, A.SRC, A.IMG, A.BATCH


def _step_ra(img=IMG):
    return R.table([R.row([(R.EQUALIZE, 0), (R.POSTERIZE, 5)], _rot(12, img / 2, img / 2), FILL), R.row([(R.SOLARIZE, 140)]),
                    R.row([], (1, 0.15, -2, 0, 1, 0), FILL), R.row([(R.INVERT, 0), (R.AUTOCONTRAST, 0)], (1, 0, 0, 0.1, 1, 1.5), 0x101010)])


STEP_AUG = [G.row([(TA.CO, 1.3), (TA.SA, 0.7)], erase=(3, 5, 11, 9), emode=1, eseed=99), G.row([(TA.BR, 0.8)]),
            G.row([(TA.SA, 1.4)], erase=(20, 0, 12, 32), emode=0), G.row([])]


def _one_step(precision, split, idx, dp, boxes=None, mix=None, aug=None, ra=None, eps=0.0, opt=True):
    from cara_amd.optim import AdamW
    m = A._model(precision).train()
    eng = m._cara_engine
    o = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4) if opt else None
    kw = {k: v for k, v in (("boxes", boxes), ("mix", mix), ("aug", aug), ("ra", ra)) if v is not None}
    if eps:
        kw["label_smoothing"] = eps
    loss = eng.train_step_resident(split, idx, o, droppath=dp, **kw).clone()
    assert eng.resident_bad_rows() == 0
    return loss, eng._flat_grad.clone(), A._trainable(m), m


@pytest.mark.parametrize("precision", OPERANDS)
def test_step_with_an_identity_ra_table_is_bitwise_the_step_without(precision):
    from cara_amd.data import identity_ra
    idx = torch.tensor([7, 0, 7, 11], device=DEV)
    boxes = A._same_size_boxes(BATCH, seed=1).to(DEV)
    mix = T.table([(3 - i, 2, 3, 9, 11, 0.0, 0.1) if i % 2 else (3 - i, 0, 0, 0, 0, 0.3, 0.3) for i in range(BATCH)]).to(DEV)
    aug = G.table(STEP_AUG).to(DEV)
    dp = T._dp(2)
    ident = identity_ra(BATCH).to(DEV)
    A._assert_same_step(_one_step(precision, A._split(), idx, dp, boxes, mix, aug, ident, 0.1), _one_step(precision, A._split(), idx, dp, boxes, mix, aug, None, 0.1))
    A._assert_same_step(_one_step(precision, A._split(), idx, dp, boxes, None, None, ident), _one_step(precision, A._split(), idx, dp, boxes))


@pytest.mark.parametrize("precision", OPERANDS)
def test_randaugmented_step_against_the_oracle(precision):
    """affine, lookups, jitter, erase, mix and smoothing: the loss and every CP / head gradient against fp32 autograd of the oracle's
    as-written model fed ra_reference with soft_target, at the bars the mixed step's test holds (tests/mix_model.LOSS_BAR, grad_bar)"""
    import torch.nn.functional as F
    from cara_amd.data import ra_reference, soft_target
    from oracle import cara_oracle as O
    from tests.test_model_gpu import grad_bar, rel
    eps = 0.1
    rows = [7, 0, 3, 11]
    px, labels = A._split_cpu()
    boxes = torch.tensor([(0, 0, SRC, SRC, 0), (5, 9, 30, 37, 1), (16, 16, IMG, IMG, 0), (3, 2, 41, 20, 1)], dtype=torch.int32)
    mix = T.table([(3, 0, 0, 0, 0, 0.3, 0.3), (2, 4, 8, 20, 16, 0.0, 20 * 16 / IMG ** 2), (1, 0, 0, 0, 0, 0.75, 0.75), (0, 11, 0, 9, 32, 0.0, 9 / 32)])
    aug, ra = G.table(STEP_AUG), _step_ra()
    idx, dp = torch.tensor(rows, device=DEV), T._dp(5)
    loss, flat, _, m = _one_step(precision, A._split(), idx, dp, boxes.to(DEV), mix.to(DEV), aug.to(DEV), ra.to(DEV), eps, opt=False)
    plain = _one_step(precision, A._split(), idx, dp, boxes.to(DEV), mix.to(DEV), aug.to(DEV), None, eps, opt=False)[0]
    assert not torch.equal(loss, plain)
    x = ra_reference(px, rows, boxes, mix, aug, ra, IMG).float()
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
    print(f"randaugmented step [{precision}]: loss {loss.item():.5f} vs oracle {rloss.item():.5f}; worst CP-gradient rel-L2 {worst:.2e}, head {rh:.2e}")
    assert abs(loss.item() - rloss.item()) < M.LOSS_BAR[precision] * max(1.0, abs(rloss.item())), (loss.item(), rloss.item())
    assert worst < grad_bar(precision) and rh < grad_bar(precision)
    assert bool(flat[:-1].any())


@pytest.mark.parametrize("precision", OPERANDS)
def test_graph_replay_rereads_the_ra_table(precision):
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    split = A._split()
    g = torch.Generator().manual_seed(8)
    rows = [torch.randint(0, N_MODEL, (BATCH,), generator=g).to(DEV) for _ in range(4)]
    boxes = [A._same_size_boxes(BATCH, seed=20 + i).to(DEV) for i in range(4)]
    base = _step_ra().tolist()
    ras = [R.table([base[(i + k) % BATCH] for i in range(BATCH)]).to(DEV) for k in range(4)]
    rows[3], boxes[3] = rows[2], boxes[2]          # the last replay differs from the one before in its ra table alone
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
                loss = gstep(split, (rows[it], boxes[it], None, None, None, ras[it]))
            else:
                opt.advance()
                loss = eng.train_step_resident(split, rows[it], opt, boxes=boxes[it], ra=ras[it], label_smoothing=0.1)
            losses.append(loss.item())
        if gstep is not None:
            (ent,) = gstep._graphs.values()
            assert ent[1] is split and sum(t.numel() * t.element_size() for t in ent[2]) == (8 + 20 + 64) * BATCH
        assert eng.resident_bad_rows() == 0 and eng.skipped_steps == 0
        out[mode] = (losses, A._trainable(m))
    print(f"[{precision}] losses eager {out['eager'][0]} graph {out['graph'][0]}")
    assert out["graph"][0] == out["eager"][0] and len(set(out["eager"][0])) == 4
    for n in out["eager"][1]:
        assert torch.equal(out["graph"][1][n], out["eager"][1][n]), n


@pytest.mark.parametrize("precision", OPERANDS)
def test_fit_over_the_six_element_tuples(precision):
    from cara_amd.data import ColorJitterErase, MixupCutmix, RandAugment, RandomResizedCropFlip
    from cara_amd.recipe import fit
    split = A._split()
    m = A._model(precision)
    start = A._trainable(m)
    erase = ColorJitterErase(IMG, 0.0, 0.0, 0.0, erase_prob=0.5)
    feed = split.train_rows(BATCH, seed=5, rank=0, world=1, augment=RandomResizedCropFlip(IMG), mix=MixupCutmix(IMG), color=erase,
                            rand=RandAugment(IMG, prob=0.9))
    seen = [item for e in range(2) for item in feed(e)]
    assert len(seen) == 6 and all(len(item) == 6 and item[4] is None for item in seen)
    assert len({tuple(item[5].reshape(-1).tolist()) for item in seen}) == 6
    assert any(int(item[5][:, 0:6:2].max()) > 0 for item in seen) and any(int(item[3][:, 0:6:2].max()) > 0 for item in seen)
    with pytest.raises(ValueError):
        split.train_rows(BATCH, color=ColorJitterErase(IMG), rand=RandAugment(IMG))
    fit(m, (split, feed), None, epochs=2, lr=1e-3, seed=5, feed="resident", label_smoothing=0.1)
    eng = m._cara_engine
    assert torch.isfinite(eng._loss_buf[0]) and float(eng._loss_buf[0]) > 0 and eng.resident_bad_rows() == 0
    after = A._trainable(m)
    assert all(torch.isfinite(after[n]).all() for n in after) and any(not torch.equal(after[n], start[n]) for n in after)
