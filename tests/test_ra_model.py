"""Host side of the RandAugment feed: the statistic tables at their edges and against PIL, the fixed lookup ops against PIL, hand-made
matrices whose result is known exactly, the drawer (seed rule, level maps, 10 000 rows through check_ra), check_ra's strict rule, and
data.ra_reference (float64) against the fp32 restatement of tests/ra_model.py within the bound derived there.  No GPU."""
import functools
import math

import numpy as np
import pytest
import torch

from cara_amd import data as D
from tests import ra_model as R

OUT = 32


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def _hist(values):
    return np.bincount(np.asarray(values, dtype=np.int64).reshape(-1), minlength=256)


def test_table_edges():
    ident = list(range(256))
    for op in (R.AUTOCONTRAST, R.EQUALIZE):
        assert R.lut(_hist([7] * 100), op) == ident                       # a constant image: hi == lo
        assert R.lut(_hist([]), op) == ident                              # nothing counted (a refused source)
    # two levels: autocontrast spreads them to 0 and 255, everything between by integer division
    t = R.lut(_hist([10] * 5 + [20] * 7), R.AUTOCONTRAST)
    assert t[10] == 0 and t[20] == 255 and t[9] == 0 and t[21] == 255 and t[15] == (255 * 5) // 10 and t[255] == 255
    # two levels, 1024 pixels: step = (1024 - 500) // 255 = 2; fewer than 255 pixels below the last bin: step == 0, identity
    t = R.lut(_hist([10] * 524 + [20] * 500), R.EQUALIZE)
    assert t[:11] == [0] * 10 + [(2 // 2) // 2] and t[11] == min(255, (1 + 524) // 2) and t[20] == 255
    assert R.lut(_hist([10] * 254 + [20] * 5000), R.EQUALIZE) == ident
    assert R.lut(_hist([10] * 255 + [20] * 5000), R.EQUALIZE) != ident
    # the vectorised form of cara_amd.data is the same function
    g = np.random.default_rng(3)
    for _ in range(50):
        h = _hist(g.integers(0, 256, g.integers(1, 5000)) // g.integers(1, 9) * g.integers(1, 3) % 256)
        for op in (R.AUTOCONTRAST, R.EQUALIZE):
            assert list(D.ra_lut(h, op)) == R.lut(h, op)


def test_fixed_ops_at_their_edges():
    q = np.arange(256).reshape(1, 16, 16).repeat(3, 0)
    post = lambda bits: R.lookup(q, R.row([(R.POSTERIZE, bits)]))[0]   # noqa: E731
    assert not post(0).any() and (post(8) == q).all() and (post(1) == (q & 128)).all()
    sol = lambda thr: R.lookup(q, R.row([(R.SOLARIZE, thr)]))[0]   # noqa: E731
    assert (sol(0) == 255 - q).all() and (sol(256) == q).all() and (sol(128)[0, 8:] == 255 - q[0, 8:]).all() and (sol(128)[0, :8] == q[0, :8]).all()
    add = R.lookup(q, R.row([(R.SOLARIZE_ADD, 200)]))[0]
    assert add[0, 0, 0] == 200 and add[0, 7, 15] == 255 and (add[0, 8:] == q[0, 8:]).all()
    assert (R.lookup(q, R.row([(R.INVERT, 0)]))[0] == 255 - q).all()
    # slots apply in order 0, 1, 2; the statistic is taken of the image as it stands before its slot
    a = R.lookup(q, R.row([(R.INVERT, 0), (R.POSTERIZE, 2)]))[0]
    b = R.lookup(q, R.row([(R.POSTERIZE, 2), (R.INVERT, 0)]))[0]
    assert (a == ((255 - q) & 192)).all() and (b == 255 - (q & 192)).all()
    half = q // 2
    _, t = R.lookup(half, R.row([(R.INVERT, 0), (R.AUTOCONTRAST, 0)]))
    assert t[0][128] == 0 and t[0][255] == 255                                 # the histogram of 255 - q/2: bins 128..255
    for op, arg in ((R.POSTERIZE, 3), (R.SOLARIZE, 100), (R.SOLARIZE_ADD, 60), (R.INVERT, 0), (R.EQUALIZE, 0)):
        ours = D.ra_lookup_reference(half, R.row([(op, arg), (R.AUTOCONTRAST, 0) if op < 5 else (R.INVERT, 0)]))[0]
        assert (ours == R.lookup(half, R.row([(op, arg), (R.AUTOCONTRAST, 0) if op < 5 else (R.INVERT, 0)]))[0]).all(), op


def test_lookup_ops_equal_pil():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageOps
    g = np.random.default_rng(11)
    worst = 0
    for n in range(60):
        side = int(g.integers(16, 65))
        kind = n % 3
        img = g.integers(0, 256, (side, side)) if kind == 0 else (g.integers(40, 200, (side, side)) if kind == 1 else
                                                                 (g.normal(120, 25, (side, side)).clip(0, 255)))
        img = img.astype(np.uint8)
        pil = Image.fromarray(img, "L")
        q = img[None].repeat(3, 0)
        one = lambda op, arg=0: R.lookup(q, R.row([(op, arg)]))[0][0]   # noqa: E731
        assert (one(R.EQUALIZE) == np.asarray(ImageOps.equalize(pil))).all()
        assert (one(R.INVERT) == np.asarray(ImageOps.invert(pil))).all()
        for bits in range(1, 9):
            assert (one(R.POSTERIZE, bits) == np.asarray(ImageOps.posterize(pil, bits))).all()
        for thr in (0, 1, 77, 128, 255, 256):
            assert (one(R.SOLARIZE, thr) == np.asarray(ImageOps.solarize(pil, thr))).all()
        worst = max(worst, int(np.abs(one(R.AUTOCONTRAST).astype(int) - np.asarray(ImageOps.autocontrast(pil)).astype(int)).max()))
    print(f"autocontrast: largest difference from PIL {worst}")
    assert worst <= 1


# ---- hand-made matrices ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bytes_split():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 256, (3, 3, OUT, OUT), generator=g, dtype=torch.uint8)


def test_exact_matrices_on_a_box_of_the_outputs_size():
    px = _bytes_split()
    box = (0, 0, OUT, OUT, 0)
    src = px[1].numpy().astype(np.float32)
    assert (R.geometry_f32(px, 1, box, R.row(), OUT, OUT) == src).all()
    # (the identity as a general matrix, -0.0 in one word: the general path gives the bytes too)
    assert (R.geometry_f32(px, 1, box, R.row(matrix=(1, -0.0, 0, 0, 1, 0)), OUT, OUT) == src).all()
    fill = 0x0A141E
    got = R.geometry_f32(px, 1, box, R.row(matrix=(1, 0, 5, 0, 1, -3), fill=fill), OUT, OUT)       # u = x + 5, v = y - 3
    want = np.empty_like(src)
    want[:] = np.array([10, 20, 30], dtype=np.float32).reshape(3, 1, 1)
    want[:, 3:, :OUT - 5] = src[:, :OUT - 3, 5:]
    assert (got == want).all()
    got = R.geometry_f32(px, 1, box, R.row(matrix=(0, 1, 0, -1, 0, OUT)), OUT, OUT)                # u = y, v = Wi - x: a quarter turn
    assert (got == src[:, ::-1, :].transpose(0, 2, 1)).all()                                         # got[oy, ox] = src[Wi - 1 - ox, oy]
    # and a flipped box under the identity-valued general matrix is the flipped bytes
    got = R.geometry_f32(px, 1, (0, 0, OUT, OUT, 1), R.row(matrix=(1, -0.0, 0, 0, 1, 0)), OUT, OUT)
    assert (got == src[:, :, ::-1]).all()
    # the float64 reference agrees on all of them
    for m in ((1, 0, 5, 0, 1, -3), (0, 1, 0, -1, 0, OUT)):
        r = R.row(matrix=m, fill=fill)
        ref = D.ra_geometry_reference(px, 1, box, r, OUT, OUT).numpy()
        assert (ref == R.geometry_f32(px, 1, box, r, OUT, OUT)).all()


# ---- the drawer ---------------------------------------------------------------------------------------------------------------------
def test_seed_rule_and_level_maps():
    assert D.ra_seed(1, 2, 3) not in (D.box_seed(1, 2, 3), D.mix_seed(1, 2, 3), D.aug_seed(1, 2, 3), D.keep_seed(1, 2, 3))
    assert len({D.ra_seed(s, e, r) for s in range(4) for e in range(4) for r in range(4)}) == 64
    ra = D.RandAugment(OUT)
    a = ra.draw(4, 3, torch.Generator().manual_seed(9))
    b = ra.draw(4, 2, torch.Generator().manual_seed(9))
    assert torch.equal(a[0][:2], b[0]) and torch.equal(a[1][:2], b[1])               # batch k does not depend on steps
    arg = D.ra_level_arg
    assert [arg("Rotate", L) for L in (0, 5, 10)] == [0.0, 15.0, 30.0] and arg("Rotate", 10, -1) == -30.0
    assert [arg("ShearX", L) for L in (0, 5, 10)] == [0.0, 0.15, 0.3] and arg("ShearY", 5, -1) == -0.15
    assert [arg("TranslateXRel", L) for L in (0, 5, 10)] == [0.0, 0.225, 0.45] and arg("TranslateYRel", 10, -1) == -0.45
    assert [arg("Posterize", L) for L in (0, 5, 10)] == [4, 2, 0]
    assert [arg("Solarize", L) for L in (0, 5, 10)] == [256, 128, 0]
    assert [arg("SolarizeAdd", L) for L in (0, 5, 10)] == [0, 55, 110]
    for op in ("Color", "Contrast", "Brightness"):
        assert [arg(op, L) for L in (0, 5, 10)] == [1.0, 1.45, 1.9] and [arg(op, L, -1) for L in (0, 5, 10)] == [1.0, 0.55, 0.1]
    assert all(arg(op, 7) is None for op in ("AutoContrast", "Equalize", "Invert"))
    # rows: the geometric ops compose in drawn order into one matrix; rotation about the centre leaves the centre where it is
    r, s = ra.row([("Rotate", 10, 1)])
    m = np.array(r[6:12], dtype=np.int32).view(np.float32).astype(np.float64).reshape(2, 3)
    assert np.allclose(m @ np.array([OUT / 2, OUT / 2, 1.0]), [OUT / 2, OUT / 2], atol=1e-5) and s == [0] * 6
    c, sn = math.cos(math.radians(-30)), math.sin(math.radians(-30))
    assert np.allclose(m[:, :2], [[c, sn], [-sn, c]], atol=1e-6)
    r2, _ = ra.row([("TranslateXRel", 10, 1), ("ShearX", 10, 1)])          # translate first, then shear: out -> shear -> translate -> source
    m2 = np.array(r2[6:12], dtype=np.int32).view(np.float32).astype(np.float64)
    assert np.allclose(m2, [1, 0.3, 0.45 * OUT, 0, 1, 0], atol=1e-6)
    r3, _ = ra.row([("ShearX", 10, 1), ("TranslateYRel", 10, 1)])
    m3 = np.array(r3[6:12], dtype=np.int32).view(np.float32).astype(np.float64)
    assert np.allclose(m3, [1, 0.3, 0.3 * 0.45 * OUT, 0, 1, 0.45 * OUT], atol=1e-5)
    assert R.is_identity(ra.row([])[0]) and R.is_identity(ra.row([("Invert", 3, 1), ("Color", 3, 1)])[0])
    # lookup slots in drawn order, the second statistic op and a repeated jitter op dropped, jitter ops as the aug row's codes
    r, s = ra.row([("Equalize", 9, 1), ("Posterize", 5, 1), ("AutoContrast", 9, 1)])
    assert r[:6] == [6, 0, 1, 2, 0, 0]
    r, s = ra.row([("Color", 5, 1), ("Brightness", 5, -1), ("Color", 10, 1)])
    assert s == [3, R.fbits(1.45), 1, R.fbits(0.55), 0, 0] and r[:6] == [0] * 6
    assert r[12] == (124 << 16 | 116 << 8 | 104)


def test_ten_thousand_drawn_rows_pass_the_checks():
    ra = D.RandAugment(OUT, n=3, prob=0.9, mstd=3.0)
    t, s = ra.draw(100, 100, torch.Generator().manual_seed(D.ra_seed(0, 0, 0)))
    D.check_ra(t, 100)
    aug = D.identity_aug(100, 100)
    aug[..., :6] = s
    D.check_aug(aug, 100, OUT, OUT)
    ops = t[..., 0:6:2].reshape(-1)
    assert set(ops.tolist()) == set(range(7)) and set(s[..., 0::2].reshape(-1).tolist()) == {0, 1, 2, 3}
    assert int((t[..., 6:12].reshape(-1, 6) != D.identity_ra(1)[0, 6:12]).any(1).sum()) > 1000
    assert int(((t[..., 0:6:2] >= 5).sum(-1) > 1).sum()) == 0
    with pytest.raises(ValueError):
        D.RandAugment(OUT, n=4)
    with pytest.raises(ValueError):
        D.RandAugment(OUT, ops=("Sharpness",))


def test_check_ra_refuses_each_item_of_the_strict_rule():
    good = [R.row([(R.POSTERIZE, 8), (R.SOLARIZE, 256), (R.EQUALIZE, 0)], (1.5, -2, 32768, 0, -32768, 0.25), 0xFFFFFF), R.row()]
    D.check_ra(R.table(good), 2)
    D.check_ra(D.identity_ra(2, 3), 2)
    nan, inf = float("nan"), float("inf")
    bad = [R.row([(7, 0)]), R.row([(-1, 0)]), R.row([(0, 1)]), R.row([(R.POSTERIZE, 9)]), R.row([(R.POSTERIZE, -1)]), R.row([(R.SOLARIZE, 257)]),
           R.row([(R.SOLARIZE_ADD, 256)]), R.row([(R.INVERT, 1)]), R.row([(R.AUTOCONTRAST, 1)]), R.row([(R.EQUALIZE, -1)]),
           R.row([(R.EQUALIZE, 0), (R.AUTOCONTRAST, 0)]), R.row([(R.EQUALIZE, 0), (R.INVERT, 0), (R.EQUALIZE, 0)]),
           R.row(matrix=(nan, 0, 0, 0, 1, 0)), R.row(matrix=(1, 0, inf, 0, 1, 0)), R.row(matrix=(1, 0, 0, 0, 1, -inf)),
           R.row(matrix=(1, 0, 32769, 0, 1, 0)), R.row(matrix=(1, 0, 0, -4e4, 1, 0)), R.row(fill=0x1000000), R.row(fill=-1),
           R.row(pad=(1, 0, 0)), R.row(pad=(0, -1, 0)), R.row(pad=(0, 0, 2))]
    for entry in bad:
        with pytest.raises(ValueError):
            D.check_ra(R.table([good[0], entry]), 2)
    with pytest.raises(ValueError):
        D.check_ra(R.table(good), 3)
    with pytest.raises(ValueError):
        D.check_ra(R.table(good).to(torch.int64), 2)


# ---- the float64 reference against the restatement ----------------------------------------------------------------------------------
HS, WS = 37, 41


@functools.lru_cache(maxsize=None)
def _smooth_split():
    """three smooth images of 37 x 41: adjacent bytes differ by at most 4"""
    y, x = np.mgrid[0:HS, 0:WS].astype(np.float64)
    imgs = []
    for k in range(3):
        chans = [np.clip(129 + 60 * np.sin(0.012 * (k + 1) * x + c) + 60 * np.cos(0.012 * (c + 1) * y + k) + 1.0 * (x + y) * (c - 1) / 3, 0, 255)
                 for c in range(3)]
        imgs.append(np.rint(np.stack(chans)).astype(np.uint8))
    px = torch.from_numpy(np.stack(imgs))
    d = max(int(np.abs(np.diff(px.numpy().astype(int), axis=2)).max()), int(np.abs(np.diff(px.numpy().astype(int), axis=3)).max()))
    return px, d


REF_ROWS = [0, 2, 1, 2, 0]
REF_BOXES = [(0, 0, WS, HS, 0), (4, 2, 33, 31, 1), (3, 2, 35, 13, 0), (WS - 32, HS - 32, 32, 32, 1), (1, 1, 38, 35, 0)]


def _ref_table():
    ra = D.RandAugment(OUT, fill=(124, 116, 104))
    rows = [ra.row([("Rotate", 9, 1), ("Posterize", 5, 1)])[0], ra.row([("ShearX", 8, -1), ("Equalize", 0, 1), ("TranslateYRel", 4, 1)])[0],
            ra.row([("ShearY", 10, 1), ("Rotate", 3, -1)])[0], ra.row([("AutoContrast", 0, 1), ("Solarize", 6, 1), ("Invert", 0, 1)])[0],
            ra.row([("TranslateXRel", 9, -1), ("SolarizeAdd", 7, 1), ("Rotate", 10, 1)])[0]]
    return R.table(rows)


def test_ra_reference_against_the_restatement_within_the_derived_bound():
    px, Dmax = _smooth_split()
    assert Dmax <= 4
    ra = _ref_table()
    mix = torch.tensor([[3, 0, 0, 0, 0, R.fbits(0.25), R.fbits(0.25), 0], [4, 6, 3, 13, 11, 0, R.fbits(0.1), 0], [2, 0, 0, 0, 0, 0, 0, 0],
                        [0, 0, 0, 0, 0, R.fbits(0.5), R.fbits(0.5), 0], [1, 0, 5, OUT, 9, 0, R.fbits(0.2), 0]], dtype=torch.int32)
    out64, geo64, tab64 = D.ra_reference(px, REF_ROWS, torch.tensor(REF_BOXES, dtype=torch.int32), mix, None, ra, OUT, parts=True)
    mean, std = np.array(D.IMAGENET_MEAN, dtype=np.float32), np.array(D.IMAGENET_STD, dtype=np.float32)
    out32, tab32, _ = R.feed_f32(px, REF_ROWS, REF_BOXES, mix.tolist(), None, ra, OUT, OUT, mean, std)
    aside = total = 0
    ok = np.ones((5, 3, OUT, OUT), dtype=bool)
    for b in range(5):
        dp, e = R.geometry_bound(ra[b], REF_BOXES[b], OUT, OUT, Dmax)
        assert e < 2.0 ** -10, (b, e)                                        # (or a pixel not set aside could quantise differently)
        g32, g64 = R.geometry_f32(px, REF_ROWS[b], REF_BOXES[b], ra[b], OUT, OUT).astype(np.float64), geo64[b].numpy()
        m = np.array(ra[b, 6:12].tolist(), dtype=np.int32).view(np.float32).astype(np.float64)
        yy, xx = np.mgrid[0:OUT, 0:OUT] + 0.5
        u, v = m[0] * xx + m[1] * yy + m[2], m[3] * xx + m[4] * yy + m[5]
        edge = (np.minimum(np.abs(u), np.abs(u - OUT)) <= dp) | (np.minimum(np.abs(v), np.abs(v - OUT)) <= dp)
        half = np.abs(g64 - np.floor(g64) - 0.5) < 2.0 ** -10 if R.has_lookup(ra[b]) else np.zeros_like(g64, dtype=bool)
        away = edge[None] | half
        aside += int(away.sum())
        total += away.size
        err = np.abs(g32 - g64)
        print(f"sample {b}: geometry max |fp32 - fp64| {err[~away].max():.3e} (bound {e:.3e}), {int(away.sum())} pixels set aside")
        assert (err[~away] <= e).all(), b
        ok[b] = ~away
        if R.has_lookup(ra[b]):
            # not set aside: the same quantised value; and on these inputs the ones set aside agree too, so the histograms are equal
            assert (np.rint(g32) == np.rint(g64)).all(), b
        assert (tab32[b] is None) == (tab64[b] is None) and (tab32[b] is None or (tab32[b] == tab64[b]).all())
    share = aside / total
    print(f"set aside: {aside} of {total} values ({100 * share:.3f} %)")
    assert share < 0.01
    # the normalised, mixed output: an unquantised value carries e (both partners' through a blend: the blend is a convex
    # combination), a quantised one nothing; then the blend's fma and the normalisation's three roundings of a value below 2.7
    e_all = max(R.geometry_bound(ra[b], REF_BOXES[b], OUT, OUT, Dmax)[1] for b in range(5))
    bound = (e_all + 2 * R.U * 255) / (255 * float(std.min())) + 5e-7
    for b in range(5):
        p = int(mix[b, 0])
        both = ok[b] & ok[p]
        err = np.abs(out32[b].astype(np.float64) - out64[b].numpy())
        assert (err[both] <= bound).all(), (b, err[both].max(), bound)
