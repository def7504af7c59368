"""GPU side of the mixed resident feed.  cara_im2col_patches_u8_rows_mix: identity tables and rectangles bitwise against the
unmixed patch rows (cara_im2col_patches_u8_rows_crop / _rows), blends against data.mix_reference in float64 within the bound
derived in tests/mix_model.py, every guard.  cara_cross_entropy_mix: bitwise cara_cross_entropy_ex without smoothing and partner,
inside the derived bound with them, NaN rows for what it refuses.  Whole model: train_step_resident / forward_resident /
GraphedTrainStep / fit with a mix table against the unmixed calls (bitwise where pasting bytes is exact) and against fp32 autograd
of the oracle's as-written model on the float64 definition.  Shapes and helpers of tests/test_augmented_feed_gpu.py."""
import ctypes as C

import pytest
import torch

from tests import mix_model as M
from tests import small_kernels_common as S
from tests import test_augmented_feed_gpu as A
from tests.test_augmented_feed_gpu import DEV, HS, N_SPLIT, OUT, ROWS, SAME_SIZE, SCALED, SENTINEL, WS, L

pytestmark = pytest.mark.gpu
OPERANDS = ["bf16", "fp16"]
B6 = len(ROWS)


def bits(x):
    return int(torch.tensor(x, dtype=torch.float32).view(torch.int32))


def table(rows):
    """int32 [B, 8] on the host from rows (partner, cx0, cy0, cw, ch, m, t)"""
    return torch.tensor([[p, x, y, w, h, bits(m), bits(t), 0] for p, x, y, w, h, m, t in rows], dtype=torch.int32)


def _mix_patches(lib, dt, px, rows, boxes, mix, p, bad=None, out=OUT, n_split=N_SPLIT):
    """cara_im2col_patches_u8_rows_mix into a buffer between two sentinel guards (checked here); -> [B, patches, 3 p p] of dt"""
    B = len(rows)
    idx = torch.tensor(rows, device=DEV)
    bx = None if boxes is None else torch.tensor(boxes, dtype=torch.int32, device=DEV)
    mx = mix.to(DEV)
    mean, std = A._norm()
    nel = B * 3 * out * out
    buf = torch.full((nel + 128,), SENTINEL, dtype=torch.int16, device=DEV)
    got = buf[64:64 + nel]
    P = L().ptr
    L().check(lib.cara_im2col_patches_u8_rows_mix(P(px), n_split, px.shape[2], px.shape[3], P(idx), P(bx), P(mx), P(mean), P(std),
                                                  P(got), P(bad) if bad is not None else None, B, 3, out, out, p, L().stream()),
              "cara_im2col_patches_u8_rows_mix")
    torch.cuda.synchronize()
    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + nel:] == SENTINEL).all())
    return got.view(dt).view(B, (out // p) ** 2, 3 * p * p)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _identity(B=B6):
    from cara_amd.data import identity_mix
    return identity_mix(B)


# ---- patch rows, bitwise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("p", [16, 8])
def test_an_identity_table_gives_the_unmixed_patch_rows(p, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    _, px = A._split_px()
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for boxes in (SAME_SIZE, SCALED):
        assert _same(_mix_patches(lib, dt, px, ROWS, boxes, _identity(), p, bad), A._crop_patches(lib, dt, px, ROWS, boxes, p))
    # without boxes: a split of the output's size, against cara_im2col_patches_u8_rows
    sq = A._source_cpu()[:, :, 3:3 + OUT, 7:7 + OUT].contiguous().to(DEV)
    got = _mix_patches(lib, dt, sq[1:1 + N_SPLIT], ROWS, None, _identity(), p, bad)
    idx = torch.tensor(ROWS, device=DEV)
    mean, std = A._norm()
    want = torch.empty_like(got)
    P = L().ptr
    L().check(lib.cara_im2col_patches_u8_rows(P(sq[1:1 + N_SPLIT]), N_SPLIT, P(idx), P(mean), P(std), P(want), None, B6, 3, OUT, OUT, p,
                                              L().stream()), "cara_im2col_patches_u8_rows")
    assert _same(got, want) and int(bad) == 0


PARTNERS = [3, 5, 0, 3, 1, 2]     # with partner == i (sample 3); sample 0 unflipped <- 3 flipped, 1 flipped <- 5 unflipped (SCALED)


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("p", [16, 8])
def test_rectangles_give_the_own_or_the_partners_unmixed_element(p, operands):
    """a rectangle over the whole output: the partner's unmixed rows; partial ones -- touching each edge, 1 x 1, with both vertical
    edges inside a lane's four pixels (x 6 .. 18), an empty one -- element by element the own or the partner's"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    _, px = A._split_px()
    assert {SCALED[i][4] for i in range(B6)} == {0, 1} and SCALED[0][4] != SCALED[3][4] and SCALED[1][4] != SCALED[5][4]
    plain = A._crop_patches(lib, dt, px, ROWS, SCALED, p)
    full = _mix_patches(lib, dt, px, ROWS, SCALED, table([(q, 0, 0, OUT, OUT, 0.0, 1.0) for q in PARTNERS]), p)
    assert _same(full, plain[PARTNERS]) and not _same(full, plain)
    img = A._unpatch(plain, p)
    rect_sets = ([(0, 5, 7, 9), (OUT - 7, 5, 7, 9), (5, 0, 9, 7), (5, OUT - 7, 9, 7), (13, 17, 1, 1), (6, 3, 13, 11)],
                 [(0, 0, 1, OUT), (OUT - 1, 0, 1, OUT), (3, 3, 0, 9), (1, 1, OUT - 2, OUT - 2), (0, OUT - 1, OUT, 1), (17, 0, 5, 0)])
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for rects in rect_sets:
        got = A._unpatch(_mix_patches(lib, dt, px, ROWS, SCALED, table([(q, *r, 0.0, 0.5) for q, r in zip(PARTNERS, rects)]), p, bad), p)
        for i, (x0, y0, w, h) in enumerate(rects):
            want = img[i].clone()
            want[:, y0:y0 + h, x0:x0 + w] = img[PARTNERS[i]][:, y0:y0 + h, x0:x0 + w]
            assert _same(got[i], want), (i, rects[i])
    assert int(bad) == 0


# ---- patch rows, Mixup -----------------------------------------------------------------------------------------------------
BLENDS = [0.25, 0.5, 0.9, 0.9, 0.25, 0.5]
# ROWS = [2, 0, 3, 2, 1, 0] of the "apart" split: images 0, 1 hold bytes in [140, 255], images 2, 3 bytes in [0, 88]; every partner
# below reads an image of its sample's own range
APART_PARTNERS = [3, 5, 0, 2, 1, 4]


def _x64(kind, partners):
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD, mix_reference
    mix = table([(q, 0, 0, 0, 0, m, m) for q, m in zip(partners, BLENDS)])
    v = mix_reference(A._source_cpu(kind)[1:1 + N_SPLIT], ROWS, torch.tensor(SCALED, dtype=torch.int32), mix, OUT)
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).to(torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).to(torch.float64).view(1, 3, 1, 1)
    return mix, (v / 255.0 - mean) / std


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("p", [16, 8])
def test_blends_are_a_16_bit_neighbour_of_the_float64_reference(p, operands):
    """Every element is one of the two values of the 16-bit type that bracket normalize(mix_reference) in float64: the crop test's
    argument (its docstring) with the blend's roundings added -- for these bytes (neighbours at most 115 apart) an unmixed element
    is off by < 6e-5, a blend of two such by no more plus 3 u / std = 8e-7 (tests/mix_model.py), below half the 16-bit spacing at
    |x| >= 0.25 (fp16: 1.2e-4).  Both byte ranges are closed under convex combination, so |x| > 0.25 holds for the blends too."""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    _, px = A._split_px("apart")
    assert all((ROWS[i] < 2) == (ROWS[q] < 2) for i, q in enumerate(APART_PARTNERS))
    mix, x = _x64("apart", APART_PARTNERS)
    got = A._unpatch(_mix_patches(lib, dt, px, ROWS, SCALED, mix, p), p).cpu().to(torch.float64)
    assert float(x.abs().min()) > 0.25
    lo, hi = A._neighbours(x, dt)
    ok = (got == lo) | (got == hi)
    nearest = torch.where((x - lo) <= (hi - x), lo, hi)
    print(f"blends p {p} [{operands}]: {int((~ok).sum())} of {ok.numel()} elements are no neighbour of the float64 value, "
          f"{int((got != nearest).sum())} are not the nearer one; max |got - x| {float((got - x).abs().max()):.3e}")
    assert ok.all(), ok.logical_not().nonzero()[:20].tolist()


@pytest.mark.parametrize("operands", OPERANDS)
def test_blends_over_the_full_byte_range_within_the_derived_bound(operands):
    """|got - x| <= e + half a 16-bit spacing, e = tests.mix_model.E_MIX = 1.3e-4 + 3 u / 0.224 (derived there), the spacing taken
    at |x| + e as in the crop test.  Observed maxima: docs/findings/mixed_feed.md."""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    _, px = A._split_px()
    mix, x = _x64("bytes", PARTNERS)
    got = A._unpatch(_mix_patches(lib, dt, px, ROWS, SCALED, mix, 16), 16).cpu().to(torch.float64)
    err = (got - x).abs()
    fine = (err - A._spacing(x.abs() + M.E_MIX, dt) / 2).clamp(min=0)
    print(f"full byte range [{operands}]: derived e {M.E_MIX:.4e}; max |got - x| {float(err.max()):.3e} (at most half a 16-bit spacing of "
          f"it is the last rounding: largest {float(A._spacing(x.abs() + M.E_MIX, dt).max() / 2):.3e}), max of it beyond half a "
          f"16-bit spacing {float(fine.max()):.3e}")
    assert bool((err <= M.E_MIX + A._spacing(x.abs() + M.E_MIX, dt) / 2).all())


# ---- patch rows, guards ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
def test_what_the_mix_kernel_refuses_is_zeroed_counted_once_and_never_read(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    _, px = A._split_px()
    good = [(q, 4, 6, 9, 11, m, m) for q, m in zip(PARTNERS, [0.0, 0.5, 0.0, 0.25, 0.0, 0.9])]
    want = _mix_patches(lib, dt, px, ROWS, SCALED, table(good), 16)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    total = 0
    nan = float("nan")
    # sample 4 is nobody's partner but its own pair's (sample 1 reads sample 5): only it goes bad
    entries = [(-1, 4, 6, 9, 11, 0.0, 0.0), (B6, 4, 6, 9, 11, 0.0, 0.0), (2 ** 31 - 1, 4, 6, 9, 11, 0.0, 0.0),
               (1, -1, 6, 9, 11, 0.0, 0.0), (1, 4, -1, 9, 11, 0.0, 0.0), (1, OUT - 8, 6, 9, 11, 0.0, 0.0), (1, 4, OUT - 10, 9, 11, 0.0, 0.0),
               (1, 4, 6, -9, 11, 0.0, 0.0), (1, 4, 6, 9, -1, 0.0, 0.0), (1, 1, 6, 2 ** 31 - 1, 11, 0.0, 0.0),
               (1, 4, 6, 9, 11, -0.1, 0.0), (1, 4, 6, 9, 11, 1.5, 0.0), (1, 4, 6, 9, 11, nan, 0.0)]
    for entry in entries:
        rows_ = list(good)
        rows_[4] = entry
        got = _mix_patches(lib, dt, px, ROWS, SCALED, table(rows_), 16, bad)
        total += 1
        assert int(bad) == total, entry
        assert not got[4].view(torch.int16).any(), entry
        assert _same(got[[0, 1, 2, 3, 5]], want[[0, 1, 2, 3, 5]]), entry
    # a partner whose row is bad, a partner whose box is outside: the sample itself (5) and the one that reads it (1), once each
    for rows_, boxes_ in (([2, 0, 3, 2, 1, N_SPLIT], SCALED), ([2, 0, 3, 2, 1, -1], SCALED),
                          (ROWS, SCALED[:5] + [(20, 1, WS - 19, 33, 0)]), (ROWS, SCALED[:5] + [(20, -1, 31, 33, 0)])):
        got = _mix_patches(lib, dt, px, rows_, boxes_, table(good), 16, bad)
        total += 2
        assert int(bad) == total
        assert not got[1].view(torch.int16).any() and not got[5].view(torch.int16).any()
        assert _same(got[[0, 2, 3, 4]], want[[0, 2, 3, 4]])
    # a NULL counter is allowed
    rows_ = list(good)
    rows_[4] = entries[0]
    got = _mix_patches(lib, dt, px, ROWS, SCALED, table(rows_), 16, None)
    assert not got[4].view(torch.int16).any() and _same(got[:4], want[:4])
    # the refusals: status 1, nothing launched (the output and the counter stay as they are)
    P = L().ptr
    idx = torch.tensor(ROWS, device=DEV)
    bx = torch.tensor(SCALED, dtype=torch.int32, device=DEV)
    mx = table(good).to(DEV)
    mean, std = A._norm()
    out = torch.full((B6 * 3 * 40 * 40,), SENTINEL, dtype=torch.int16, device=DEV)
    a = dict(pixels=P(px), n=N_SPLIT, Hs=HS, Ws=WS, rows=P(idx), boxes=P(bx), mix=P(mx), mean=P(mean), std=P(std), out=P(out), Hi=OUT, Wi=OUT, p=16)

    def call(**kw):
        v = dict(a, **kw)
        return lib.cara_im2col_patches_u8_rows_mix(v["pixels"], v["n"], v["Hs"], v["Ws"], v["rows"], v["boxes"], v["mix"], v["mean"], v["std"],
                                                   v["out"], P(bad), B6, 3, v["Hi"], v["Wi"], v["p"], L().stream())
    for name in ("pixels", "rows", "mix", "mean", "std", "out"):
        assert call(**{name: None}) == 1, name
    assert call(boxes=None) == 1                                                        # no boxes: the split must have the output's size
    assert call(n=0) == 1 and call(Hs=0) == 1 and call(Ws=-4) == 1
    assert call(p=6, Hi=36, Wi=36) == 1 and call(p=2) == 1 and call(p=0) == 1 and call(Hi=40) == 1 and call(Wi=40) == 1
    torch.cuda.synchronize()
    assert int(bad) == total and bool((out == SENTINEL).all())


# ---- the loss --------------------------------------------------------------------------------------------------------------
def _xent_mix(lib, logits, labels, mix, eps, B, Cn, scaled=False, ex=False):
    """cara_cross_entropy_mix (ex: cara_cross_entropy_ex) between sentinels -> loss[0 .. B], dlogits"""
    from tests.test_small_kernels_gpu import is_sentinel, sentinel
    p, st = L().ptr, L().stream
    loss = sentinel((1 + B + 1,), torch.float32)
    d = sentinel((B + 1, Cn), torch.float32)
    amp, found = (torch.tensor([512.0, 0.0, 0.0, 0.0], device=DEV), torch.ones(1, device=DEV)) if scaled else (None, None)
    tail = (B, Cn, C.c_float(0.25 if scaled else 1.0), p(amp), p(found), st())
    if ex:
        L().check(lib.cara_cross_entropy_ex(p(logits), p(labels), p(loss), p(d), *tail), "cara_cross_entropy_ex")
    else:
        L().check(lib.cara_cross_entropy_mix(p(logits), p(labels), p(mix), C.c_float(eps), p(loss), p(d), *tail), "cara_cross_entropy_mix")
    torch.cuda.synchronize()
    assert is_sentinel(loss[1 + B:]) and is_sentinel(d[B:]) and (found is None or found.item() == 0.0)     # found_inf is cleared
    return loss[:1 + B], d[:B]


@pytest.mark.parametrize("operands", OPERANDS)
def test_loss_without_smoothing_and_partner_weight_is_bitwise_the_plain_one(operands):
    lib = L().lib(operands)
    for Cn in S.XENT_C:
        for B in S.XENT_B:
            lh, yh = S.xent_inputs(B, Cn)
            logits, labels = lh.to(DEV), yh.to(DEV)
            mix = table([(B - 1 - i, 3, 2, 5, 7, 0.5, 0.0) for i in range(B)]).to(DEV)      # t == 0: the partner carries no weight
            for scaled in (False, True):
                want = _xent_mix(lib, logits, labels, None, 0.0, B, Cn, scaled, ex=True)
                for m in (mix, None):
                    got = _xent_mix(lib, logits, labels, m, 0.0, B, Cn, scaled)
                    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (B, Cn, scaled, m is None)
                    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (B, Cn, scaled, m is None)


@pytest.mark.parametrize("operands", OPERANDS)
def test_loss_with_smoothing_and_partners_inside_the_derived_bound(operands):
    lib = L().lib(operands)
    worst = {"terms": 0.0, "loss": 0.0, "dlogits": 0.0}
    for Cn in S.XENT_C:
        for B in S.XENT_B:
            for eps in (0.0, 0.1):
                for t in (0.3, 1.0):
                    for same in (True, False):
                        lh, yh, mix = M.loss_case(B, Cn, t, same)
                        for scaled in (False, True):
                            loss, d = _xent_mix(lib, lh.to(DEV), yh.to(DEV), mix.to(DEV), eps, B, Cn, scaled)
                            model = M.xent_mix(lh, yh, mix, eps, *((0.25, 512.0) if scaled else (1.0, 1.0)))
                            for name, got in (("terms", loss[1:]), ("loss", loss[0]), ("dlogits", d)):
                                ok, ratio = S.K.hold_f32(got, *model[name])
                                assert ok.all(), (name, B, Cn, eps, t, same, scaled, ratio)
                                worst[name] = max(worst[name], ratio)
    print(f"cara_cross_entropy_mix [{operands}]: worst |device - model| / bound {worst}")


@pytest.mark.parametrize("Cn", [2, 65, 1000])
@pytest.mark.parametrize("operands", OPERANDS)
def test_loss_refuses_labels_partners_and_weights_outside(operands, Cn):
    lib, B = L().lib(operands), 5
    lh, yh, mix = M.loss_case(B, Cn, 0.3, False)
    big = torch.zeros(B + 2, Cn, device=DEV)
    big[1:B + 1] = lh.to(DEV)
    logits = big[1:B + 1]                       # (a whole row of margin on either side)
    loss, d = _xent_mix(lib, logits, yh.to(DEV), mix.to(DEV), 0.1, B, Cn)
    nan = float("nan")

    def check(labels, mix_, bad_at):
        lb, db = _xent_mix(lib, logits, labels.to(DEV), mix_.to(DEV), 0.1, B, Cn)
        good = [i for i in range(B) if i not in bad_at]
        assert torch.isnan(lb[0]) and torch.isnan(lb[1:][bad_at]).all() and torch.isnan(db[bad_at]).all(), bad_at
        assert torch.equal(lb[1:][good], loss[1:][good]) and torch.equal(db[good], d[good]), bad_at
    y = yh.clone()
    y[1] = Cn                                   # sample 1's own label, which is sample 3's partner label
    check(y, mix, [1, 3])
    y = yh.clone()
    y[4] = -1
    check(y, mix, [0, 4])
    for entry, at in (((-1, 0, 0, 0, 0, 0.0, 0.3), 2), ((B, 0, 0, 0, 0, 0.0, 0.3), 0), ((1, 0, 0, 0, 0, 0.0, 2.0), 3), ((1, 0, 0, 0, 0, 0.0, nan), 4),
                      ((1, 0, 0, 0, 0, 0.0, -0.5), 1)):
        m2 = mix.clone()
        m2[at] = table([entry])[0]
        check(yh, m2, [at])
    # the host refuses a smoothing outside [0, 1): status 1, nothing launched
    p = L().ptr
    out = torch.full((1 + B,), 7.0, device=DEV)
    yd, md = yh.to(DEV), mix.to(DEV)
    for eps in (1.0, 1.5, -0.1, nan):
        assert lib.cara_cross_entropy_mix(p(logits), p(yd), p(md), C.c_float(eps), p(out), None, B, Cn, C.c_float(1.0), None, None,
                                          L().stream()) == 1, eps
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- whole model: the crop test's shape ------------------------------------------------------------------------------------
DEPTH, N_MODEL, SRC, IMG, BATCH = A.DEPTH, A.N_MODEL, A.SRC, A.IMG, A.BATCH


def _dp(seed):
    return ((torch.rand(DEPTH, 2, BATCH, generator=torch.Generator().manual_seed(seed)) > 0.3).float() / 0.9).to(DEV)


def _one_step(precision, split, idx, dp, boxes=None, mix=None, eps=0.0, opt=True):
    """loss, flat gradient and the trainable tensors after one AdamW step, from a fresh model"""
    from cara_amd.optim import AdamW
    m = A._model(precision).train()
    eng = m._cara_engine
    o = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4) if opt else None
    kw = {k: v for k, v in (("boxes", boxes), ("mix", mix)) if v is not None}
    if eps:
        kw["label_smoothing"] = eps
    loss = eng.train_step_resident(split, idx, o, droppath=dp, **kw).clone()
    assert eng.resident_bad_rows() == 0
    return loss, eng._flat_grad.clone(), A._trainable(m), m


@pytest.mark.parametrize("precision", OPERANDS)
def test_step_with_an_identity_table_is_bitwise_the_step_without(precision):
    from cara_amd.data import identity_mix
    idx = torch.tensor([7, 0, 7, 11], device=DEV)
    boxes = A._same_size_boxes(BATCH, seed=1).to(DEV)
    dp = _dp(2)
    A._assert_same_step(_one_step(precision, A._split(), idx, dp, boxes, identity_mix(BATCH).to(DEV)), _one_step(precision, A._split(), idx, dp, boxes))


@pytest.mark.parametrize("precision", OPERANDS)
def test_cutmix_step_is_bitwise_the_step_on_the_host_composited_split(precision):
    """same-size boxes and pairs that share a label: pasting bytes is exact, and the soft target is the one-hot (the weights of a
    32-px rectangle are k / 1024: (1 - t) + t == 1 in fp32, and the loss's lerp is exact where ya == yb)"""
    from cara_amd.data import ResidentSplit
    rows = [7, 0, 0, 7]                                   # partner 3 - i: the pairs (0, 3) and (1, 2) share image and label
    boxes = A._same_size_boxes(BATCH, seed=1)
    rects = [(0, 0, 13, 32), (5, 9, 17, 6), (30, 31, 2, 1), (7, 0, 25, 32)]
    mix = table([(3 - i, *r, 0.0, r[2] * r[3] / IMG ** 2) for i, r in enumerate(rects)])
    px, labels = A._split_cpu()
    crops = A._precropped(px, rows, boxes.tolist()).cpu()
    comp = crops.clone()
    for i, (x0, y0, w, h) in enumerate(rects):
        comp[i, :, y0:y0 + h, x0:x0 + w] = crops[3 - i, :, y0:y0 + h, x0:x0 + w]
    assert not torch.equal(comp, crops)
    composited = ResidentSplit.from_tensors(comp.to(DEV), labels[rows].to(DEV))
    idx, dp, ar = torch.tensor(rows, device=DEV), _dp(2), torch.arange(BATCH, device=DEV)
    mixed = _one_step(precision, A._split(), idx, dp, boxes.to(DEV), mix.to(DEV))
    plain = _one_step(precision, composited, ar, dp)
    print(f"[{precision}] loss mixed {mixed[0].item()!r} composited {plain[0].item()!r}; gradient elements that differ: "
          f"{int((mixed[1] != plain[1]).sum())} of {plain[1].numel()}")
    A._assert_same_step(mixed, plain)
    got = mixed[3]._cara_engine.forward_resident(A._split(), idx, droppath=dp, boxes=boxes.to(DEV), mix=mix.to(DEV))
    want = plain[3]._cara_engine.forward_resident(composited, ar, droppath=dp)
    assert torch.equal(got, want) and torch.isfinite(got).all() and tuple(got.shape) == (BATCH, 100)
    # without boxes: a split of the model's size, the rectangle pasted between whole images
    small = ResidentSplit.from_tensors(crops.to(DEV), labels[rows].to(DEV))
    A._assert_same_step(_one_step(precision, small, ar, dp, None, mix.to(DEV)), plain)
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", OPERANDS)
def test_mixed_step_with_smoothing_against_the_loss_kernel_and_the_oracle(precision):
    """different labels, Mixup and CutMix rows in one table, eps = 0.1: the step's loss and dlogits are bitwise
    cara_cross_entropy_mix on forward_resident's logits; the loss and every CP / head gradient against fp32 autograd of the
    oracle's as-written model fed normalize(mix_reference) with soft_target, at the bars the train-step test holds
    (tests/test_model_gpu.py::test_train_step_against_oracle: tolerances.CP_GRAD, a fifth of it in fp16, loss 5e-3 / 5e-4)"""
    import torch.nn.functional as F
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD, mix_reference, soft_target
    from oracle import cara_oracle as O
    from tests.test_model_gpu import grad_bar, rel
    eps = 0.1
    rows = [7, 0, 3, 11]
    px, labels = A._split_cpu()
    assert len({int(labels[r]) for r in rows}) == 4
    boxes = torch.tensor([(0, 0, SRC, SRC, 0), (5, 9, 30, 37, 1), (16, 16, IMG, IMG, 0), (3, 2, 41, 20, 1)], dtype=torch.int32)
    mix = table([(3, 0, 0, 0, 0, 0.3, 0.3), (2, 4, 8, 20, 16, 0.0, 20 * 16 / IMG ** 2), (1, 0, 0, 0, 0, 0.75, 0.75), (0, 11, 0, 9, 32, 0.0, 9 / 32)])
    idx, dp = torch.tensor(rows, device=DEV), _dp(5)
    loss, flat, _, m = _one_step(precision, A._split(), idx, dp, boxes.to(DEV), mix.to(DEV), eps, opt=False)
    eng = m._cara_engine
    step_loss, step_dl = eng._loss_buf.clone(), eng._dlogits.clone()
    logits = eng.forward_resident(A._split(), idx, droppath=dp, boxes=boxes.to(DEV), mix=mix.to(DEV))
    lb, dl = torch.empty(1 + BATCH, device=DEV), torch.empty(BATCH, 100, device=DEV)
    fp16 = precision == "fp16"
    P = L().ptr
    yd, md = labels[rows].to(DEV), mix.to(DEV)            # (held: the call reads them after this line has run)
    L().check(eng._lib().cara_cross_entropy_mix(P(logits), P(yd), P(md), C.c_float(eps), P(lb), P(dl), BATCH, 100,
                                                C.c_float(1.0), P(eng._amp(torch.device(DEV, 0))) if fp16 else None, None, L().stream()),
              "cara_cross_entropy_mix")
    assert torch.equal(step_loss.view(torch.int32), lb.view(torch.int32)) and torch.equal(step_dl.view(torch.int32), dl.view(torch.int32))
    assert torch.equal(loss, lb[0])
    # the oracle: fp32 autograd of the as-written model on the float64 definition of the mixed batch
    mean, std = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1).double(), torch.tensor(IMAGENET_STD).view(1, 3, 1, 1).double()
    x = ((mix_reference(px, rows, boxes, mix, IMG) / 255.0 - mean) / std).float()
    q = soft_target(labels[rows], mix, 100, float(torch.tensor(eps, dtype=torch.float32))).float()
    w, cp = A._weights()
    cps = {k: v.clone().requires_grad_(True) for k, v in cp.items()}
    cps["CP_A1"], cps["CP_P1"] = cp["CP_A1"][:3 * DEPTH].clone().requires_grad_(True), cp["CP_P1"][:9 * DEPTH].clone().requires_grad_(True)
    ww = dict(w)
    ww["head.weight"], ww["head.bias"] = w["head.weight"].clone().requires_grad_(True), w["head.bias"].clone().requires_grad_(True)
    rlogits = O.vit_cara_forward(x, ww, cps, s=0.1, depth=DEPTH, drop_path_keep=dp.cpu())
    rloss = -(q * F.log_softmax(rlogits, 1)).sum(1).mean()
    rloss.backward()
    bar = M.LOSS_BAR[precision]
    worst = max(rel(getattr(m, n).grad, cps[n].grad) for n in O.CP_NAMES)
    rh = max(rel(m.head.weight.grad, ww["head.weight"].grad), rel(m.head.bias.grad, ww["head.bias"].grad))
    print(f"mixed step [{precision}]: loss {loss.item():.5f} vs oracle {rloss.item():.5f}; worst CP-gradient rel-L2 {worst:.2e}, head {rh:.2e}")
    assert abs(loss.item() - rloss.item()) < bar * max(1.0, abs(rloss.item())), (loss.item(), rloss.item())
    assert worst < grad_bar(precision) and rh < grad_bar(precision)
    assert bool(flat[:-1].any())


@pytest.mark.parametrize("precision", OPERANDS)
def test_graph_replay_rereads_the_mix_table(precision):
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    split = A._split()
    g = torch.Generator().manual_seed(8)
    rows = [torch.randint(0, N_MODEL, (BATCH,), generator=g).to(DEV) for _ in range(4)]
    boxes = [A._same_size_boxes(BATCH, seed=20 + i).to(DEV) for i in range(4)]
    mixes = [table([(3 - i, 2 * k, k, 9 + k, 20 - k, 0.0, (9 + k) * (20 - k) / IMG ** 2) if k % 2 else (3 - i, 0, 0, 0, 0, 0.2 * k + 0.1, 0.2 * k + 0.1)
                    for i in range(BATCH)]).to(DEV) for k in range(4)]
    rows[3], boxes[3] = rows[2], boxes[2]              # the last replay differs from the one before in its mix table alone
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
                loss = gstep(split, (rows[it], boxes[it], mixes[it]))
            else:
                opt.advance()
                loss = eng.train_step_resident(split, rows[it], opt, boxes=boxes[it], mix=mixes[it], label_smoothing=0.1)
            losses.append(loss.item())
        if gstep is not None:
            (ent,) = gstep._graphs.values()
            static = ent[2]
            assert ent[1] is split and sum(t.numel() * t.element_size() for t in static) == (8 + 20 + 32) * BATCH
        assert eng.resident_bad_rows() == 0 and eng.skipped_steps == 0
        out[mode] = (losses, A._trainable(m))
    print(f"[{precision}] losses eager {out['eager'][0]} graph {out['graph'][0]}")
    assert out["graph"][0] == out["eager"][0] and len(set(out["eager"][0])) == 4
    for n in out["eager"][1]:
        assert torch.equal(out["graph"][1][n], out["eager"][1][n]), n


@pytest.mark.parametrize("precision", OPERANDS)
def test_fit_over_rows_boxes_and_mix_tables(precision):
    from cara_amd.data import MixupCutmix, RandomResizedCropFlip
    from cara_amd.recipe import fit
    split = A._split()
    m = A._model(precision)
    start = A._trainable(m)
    feed = split.train_rows(BATCH, seed=5, rank=0, world=1, augment=RandomResizedCropFlip(IMG), mix=MixupCutmix(IMG))
    seen = [item for e in range(2) for item in feed(e)]
    assert len(seen) == 6 and all(len(item) == 3 for item in seen) and len({tuple(item[2].reshape(-1).tolist()) for item in seen}) > 1
    fit(m, (split, feed), None, epochs=2, lr=1e-3, seed=5, feed="resident", label_smoothing=0.1)
    eng = m._cara_engine
    assert torch.isfinite(eng._loss_buf[0]) and float(eng._loss_buf[0]) > 0 and eng.resident_bad_rows() == 0
    after = A._trainable(m)
    assert all(torch.isfinite(after[n]).all() for n in after) and any(not torch.equal(after[n], start[n]) for n in after)
