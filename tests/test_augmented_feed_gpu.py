"""GPU side of the augmented resident feed: cara_im2col_patches_u8_rows_crop against cara_im2col_patches_u8 on torch-sliced
bytes (bitwise, for boxes of the output's size and 1x1 boxes) and against data.resized_crop_reference in float64 (scaled
boxes), bad rows and boxes counted and never read, and train_step_resident / forward_resident / GraphedTrainStep / fit with
boxes against the same calls on pre-cropped splits (bitwise)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5a5a     # 16-bit pattern of the guard elements around a patches buffer (not a value the kernels write there)
HS, WS, N_SPLIT, OUT = 40, 52, 4, 32
ROWS = [2, 0, 3, 2, 1, 0]                      # B = 6, with duplicates


def L():
    from cara_amd import _lib
    return _lib


def _norm():
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD
    return torch.tensor(IMAGENET_MEAN, device=DEV), torch.tensor(IMAGENET_STD, device=DEV)


@functools.lru_cache(maxsize=None)
def _source_cpu(kind="bytes"):
    """six images of 40 x 52, of which the split is the middle four: a read before or behind the split lands in memory the
    test owns.  "bytes": every byte value in every channel of every image.  "apart": images 1, 2 of the allocation hold bytes
    in [140, 255] and images 3, 4 bytes in [0, 88] (see test_scaled_boxes...)"""
    g = torch.Generator().manual_seed(17)
    px = torch.randint(0, 256, (N_SPLIT + 2, 3, HS, WS), generator=g, dtype=torch.uint8)
    if kind == "bytes":
        px.view(N_SPLIT + 2, 3, -1)[:, :, :256] = torch.arange(256, dtype=torch.uint8)
    else:
        px[1:3] = (140 + px[1:3].to(torch.int32) * 116 // 256).to(torch.uint8)
        px[3:5] = (px[3:5].to(torch.int32) * 89 // 256).to(torch.uint8)
    return px


def _split_px(kind="bytes"):
    alloc = _source_cpu(kind).to(DEV)
    px = alloc[1:1 + N_SPLIT]
    assert px.is_contiguous()
    return alloc, px


def _u8_patches(lib, dt, batch_u8, p):
    """patch rows of a contiguous uint8 batch [B,3,H,W] by the existing cara_im2col_patches_u8"""
    B, _, H, W = batch_u8.shape
    mean, std = _norm()
    out = torch.empty(B * (H // p) * (W // p), 3 * p * p, dtype=dt, device=DEV)
    L().check(lib.cara_im2col_patches_u8(L().ptr(batch_u8), L().ptr(mean), L().ptr(std), L().ptr(out), B, 3, H, W, p, L().stream()),
              "cara_im2col_patches_u8")
    return out


def _crop_patches(lib, dt, px, rows, boxes, p, bad=None, out=OUT, n_split=N_SPLIT):
    """cara_im2col_patches_u8_rows_crop into a buffer between two sentinel guards; -> [B, patches per sample, 3 p p] of dt.
    The guards are checked here."""
    B = len(rows)
    idx = torch.tensor(rows, device=DEV)
    bx = torch.tensor(boxes, dtype=torch.int32, device=DEV)
    mean, std = _norm()
    nel = B * 3 * out * out
    buf = torch.full((nel + 128,), SENTINEL, dtype=torch.int16, device=DEV)
    got = buf[64:64 + nel]
    L().check(lib.cara_im2col_patches_u8_rows_crop(L().ptr(px), n_split, px.shape[2], px.shape[3], L().ptr(idx), L().ptr(bx), L().ptr(mean),
                                                   L().ptr(std), L().ptr(got), L().ptr(bad) if bad is not None else None, B, 3, out, out, p,
                                                   L().stream()), "cara_im2col_patches_u8_rows_crop")
    torch.cuda.synchronize()
    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + nel:] == SENTINEL).all())
    return got.view(dt).view(B, (out // p) ** 2, 3 * p * p)


def _precropped(px_cpu, rows, boxes):
    """the torch-sliced and torch.flip-ped bytes of same-size boxes: uint8 [B,3,h,w], contiguous, on the device"""
    out = []
    for r, (x0, y0, w, h, flip) in zip(rows, boxes):
        c = px_cpu[r, :, y0:y0 + h, x0:x0 + w]
        out.append(torch.flip(c, dims=[2]) if flip else c)
    return torch.stack(out).contiguous().to(DEV)


SAME_SIZE = [(0, 0, OUT, OUT, 0), (WS - OUT, HS - OUT, OUT, OUT, 1), (7, 3, OUT, OUT, 0), (0, HS - OUT, OUT, OUT, 5),
             (WS - OUT, 0, OUT, OUT, 0), (13, 5, OUT, OUT, -1)]


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
@pytest.mark.parametrize("p", [16, 8])
def test_boxes_of_the_outputs_size_are_bitwise_the_sliced_bytes(p, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    _, px = _split_px()
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = _crop_patches(lib, dt, px, ROWS, SAME_SIZE, p, bad)
    want = _u8_patches(lib, dt, _precropped(_source_cpu()[1:1 + N_SPLIT], ROWS, SAME_SIZE), p).view_as(got)
    differ = got.view(torch.int16) != want.view(torch.int16)
    print(f"same-size boxes p {p} [{operands}]: {int(differ.sum())} of {differ.numel()} elements differ")
    assert not differ.any(), differ.nonzero()[:20].tolist()
    assert int(bad) == 0


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_a_1x1_box_gives_the_constant_image_of_its_byte(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    _, px = _split_px()
    src = _source_cpu()[1:1 + N_SPLIT]
    boxes = [(0, 0, 1, 1, 0), (WS - 1, HS - 1, 1, 1, 1), (5, 0, 1, 1, 0), (0, 6, 1, 1, 1), (255 % WS, 255 // WS, 1, 1, 0), (30, 20, 1, 1, 0)]
    got = _crop_patches(lib, dt, px, ROWS, boxes, 16)
    const = torch.stack([src[r, :, y0, x0].view(3, 1, 1).expand(3, OUT, OUT) for r, (x0, y0, _, _, _) in zip(ROWS, boxes)])
    assert len({tuple(c[:, 0, 0].tolist()) for c in const}) == len(ROWS)
    want = _u8_patches(lib, dt, const.contiguous().to(DEV), 16).view_as(got)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def _unpatch(rows16, p, out=OUT):
    """[B, patches, 3 p p] -> [B, 3, out, out]"""
    B, g = rows16.shape[0], out // p
    return rows16.view(B, g, g, 3, p, p).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, out, out)


def _neighbours(x64, dt):
    """the two values of the 16-bit type dt that bracket each float64 x (equal where x is representable), as float64"""
    c = x64.to(torch.float32).to(dt)
    bits = c.view(torch.int16).to(torch.int32) & 0xffff
    sign, mag = bits & 0x8000, bits & 0x7fff

    def value(sign, mag):
        b = (sign | mag)
        b = torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16)
        return b.view(dt).to(torch.float64)
    away = value(sign, mag + 1)
    toward = torch.where(mag > 0, value(sign, (mag - 1).clamp(min=0)), value(sign ^ 0x8000, torch.ones_like(mag)))
    cand = torch.stack([toward, c.to(torch.float64), away])
    lo = torch.where(cand <= x64, cand, torch.full_like(cand, -float("inf"))).max(0).values
    hi = torch.where(cand >= x64, cand, torch.full_like(cand, float("inf"))).min(0).values
    return lo, hi


def _spacing(y64, dt):
    """distance from |y| rounded to dt to the next value of dt above it"""
    c = y64.abs().to(torch.float32).to(dt)
    return (c.view(torch.int16) + 1).view(dt).to(torch.float64) - c.to(torch.float64)


# up-sampling, down-sampling from the full source, w != h both ways, with and without flip
SCALED = [(0, 0, WS, HS, 0), (11, 9, 13, 13, 1), (3, 2, 45, 13, 0), (WS - 9, HS - 37, 9, 37, 1), (0, 0, WS, HS, 1), (20, 1, 31, 33, 0)]


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
@pytest.mark.parametrize("p", [16, 8])
def test_scaled_boxes_are_a_16_bit_neighbour_of_the_float64_reference(p, operands):
    """Every element is one of the two values of the 16-bit type that bracket x = normalize(resized_crop_reference) computed in
    float64.  Derived for these shapes, not measured: the kernel's x is off by less than half a 16-bit spacing where
    |x| >= 0.25.  The sample position s < 52 is two fp32 roundings off (< 1.3e-5), which moves v by at most 255 * (dfx + dfy)
    < 7e-3 of a byte step; the lerps' own roundings add < 1e-4; so |dx| < 7.1e-3 / 255 / 0.224 = 1.3e-4 in the worst case of
    neighbouring bytes 255 apart on both axes, and for this test's bytes (at most 115 apart) < 6e-5 -- below half the
    spacing at |x| >= 0.25, which is 2^-13 = 1.2e-4 in fp16 and 2^-10 in bf16.  Closer to the channel mean the 16-bit grid
    becomes finer than any fp32 evaluation of the position allows (it has no lower end: bf16 keeps fp32's exponent), so the
    images of this test keep away from it: bytes in [140, 255] or in [0, 88], hence |v - 255 mean[c]| > 15 and |x| > 0.25 for
    every convex combination.  The full byte range is held to the absolute form of the same bound in the test below.
    Measured (docs/findings/augmented_feed.md): how many elements are not the nearer of the two."""
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD, resized_crop_reference
    lib, dt = L().lib(operands), L().act_dtype(operands)
    _, px = _split_px("apart")
    got = _unpatch(_crop_patches(lib, dt, px, ROWS, SCALED, p), p).cpu().to(torch.float64)
    v = resized_crop_reference(_source_cpu("apart")[1:1 + N_SPLIT], ROWS, torch.tensor(SCALED, dtype=torch.int32), OUT)
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).to(torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).to(torch.float64).view(1, 3, 1, 1)
    x = (v / 255.0 - mean) / std
    assert float(x.abs().min()) > 0.25
    lo, hi = _neighbours(x, dt)
    assert bool((lo <= x).all()) and bool((x <= hi).all())
    nearest = torch.where((x - lo) <= (hi - x), lo, hi)
    ok = (got == lo) | (got == hi)
    print(f"scaled boxes p {p} [{operands}]: {int((~ok).sum())} of {ok.numel()} elements are no neighbour of the float64 value, "
          f"{int((got != nearest).sum())} are not the nearer one; max |got - x| {float((got - x).abs().max()):.3e}")
    assert ok.all(), ok.logical_not().nonzero()[:20].tolist()


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_scaled_boxes_over_the_full_byte_range_within_the_absolute_bound(operands):
    """|got - x| <= 1.3e-4 + half a 16-bit spacing: the worst-case bound of the docstring above (fp32 evaluation of the sample
    position, neighbouring bytes up to 255 apart) plus the one rounding to 16 bits (of a value of magnitude at most
    |x| + 1.3e-4: the spacing is taken there), for bytes of every value -- also where x is near 0 and the neighbour property
    cannot hold for an fp32 kernel"""
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD, resized_crop_reference
    lib, dt = L().lib(operands), L().act_dtype(operands)
    _, px = _split_px()
    got = _unpatch(_crop_patches(lib, dt, px, ROWS, SCALED, 16), 16).cpu().to(torch.float64)
    v = resized_crop_reference(_source_cpu()[1:1 + N_SPLIT], ROWS, torch.tensor(SCALED, dtype=torch.int32), OUT)
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).to(torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).to(torch.float64).view(1, 3, 1, 1)
    x = (v / 255.0 - mean) / std
    lo, hi = _neighbours(x, dt)
    ok = (got == lo) | (got == hi)
    err = (got - x).abs()
    print(f"full byte range [{operands}]: {int((~ok).sum())} of {ok.numel()} elements are no neighbour of the float64 value "
          f"(smallest |x| {float(x.abs().min()):.2e}); max |got - x| {float(err.max()):.3e}")
    assert bool((err <= 1.3e-4 + _spacing(x.abs() + 1.3e-4, dt) / 2).all())


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_bad_rows_and_boxes_are_counted_and_never_read(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    _, px = _split_px()
    src = _source_cpu()[1:1 + N_SPLIT]
    good = (7, 3, OUT, OUT, 1)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    # a row behind the split, one pixel outside on the left and above
    rows_a, boxes_a = [2, N_SPLIT, 0, 3, 1, 0], [good, good, (-1, 3, OUT, OUT, 0), (7, -1, OUT, OUT, 0), good, good]
    # one pixel outside on the right and below, w = 0, and a sample whose row and box are both bad (counted once)
    rows_b, boxes_b = [0, 1, 2, 3, 2, -1], [(WS - OUT + 1, 3, OUT, OUT, 0), good, (7, HS - OUT + 1, OUT, OUT, 0), (7, 3, 0, OUT, 0), good,
                                             (0, 0, WS + 1, 1, 0)]
    for rows, boxes, bad_at, total in ((rows_a, boxes_a, [1, 2, 3], 3), (rows_b, boxes_b, [0, 2, 3, 5], 7)):
        got = _crop_patches(lib, dt, px, rows, boxes, 16, bad)
        assert int(bad) == total
        ok_at = [i for i in range(6) if i not in bad_at]
        for i in bad_at:
            assert not got[i].view(torch.int16).any(), i
        want = _u8_patches(lib, dt, _precropped(src, [rows[i] for i in ok_at], [boxes[i] for i in ok_at]), 16).view(len(ok_at), 4, -1)
        for k, i in enumerate(ok_at):
            assert torch.equal(got[i].view(torch.int16), want[k].view(torch.int16)), i
    # a NULL counter is allowed
    got = _crop_patches(lib, dt, px, rows_a, boxes_a, 16, None)
    assert not got[1].view(torch.int16).any() and got[0].view(torch.int16).any()
    # the refusals: status 1, nothing launched (the output and the counter stay as they are)
    P = L().ptr
    idx = torch.tensor(rows_a, device=DEV)
    bx = torch.tensor(boxes_a, dtype=torch.int32, device=DEV)
    mean, std = _norm()
    out = torch.full((6 * 3 * 40 * 40,), SENTINEL, dtype=torch.int16, device=DEV)
    a = dict(pixels=P(px), n=N_SPLIT, Hs=HS, Ws=WS, rows=P(idx), boxes=P(bx), mean=P(mean), std=P(std), out=P(out), Hi=OUT, Wi=OUT, p=16)

    def call(**kw):
        v = dict(a, **kw)
        return lib.cara_im2col_patches_u8_rows_crop(v["pixels"], v["n"], v["Hs"], v["Ws"], v["rows"], v["boxes"], v["mean"], v["std"],
                                                    v["out"], P(bad), 6, 3, v["Hi"], v["Wi"], v["p"], L().stream())
    for name in ("pixels", "rows", "boxes", "mean", "std", "out"):
        assert call(**{name: None}) == 1, name
    assert call(n=0) == 1 and call(n=-3) == 1 and call(Hs=0) == 1 and call(Ws=0) == 1 and call(Hs=-1) == 1 and call(Ws=-4) == 1
    assert call(p=6, Hi=36, Wi=36) == 1 and call(p=2, Hi=32, Wi=32) == 1              # p % 4
    assert call(Hi=40) == 1 and call(Wi=40) == 1 and call(Hi=24, p=16) == 1             # not a multiple of p
    torch.cuda.synchronize()
    assert int(bad) == 7 and bool((out == SENTINEL).all())


# ---- whole model: depth 2, dim 768, 12 heads, rank 16, a 32-px model; the source split is 12 images of 48 x 48 -------------------
DEPTH, N_MODEL, SRC, IMG, BATCH = 2, 12, 48, 32, 4


@functools.lru_cache(maxsize=None)
def _weights():
    from oracle import cara_oracle as O
    return O.synthetic_backbone(depth=DEPTH, img=IMG), O.synthetic_cp(rank=16)     # CP_A2 / CP_P2 non-zero


def _model(precision="bf16", drop_path_rate=0.1):
    from tests.test_model_gpu import build
    w, cp = _weights()
    return build(w, cp, 16, 0.1, DEPTH, IMG, drop_path_rate=drop_path_rate, precision=precision)


@functools.lru_cache(maxsize=None)
def _split_cpu():
    """12 images of 48 px whose level and contrast vary per image, and their labels (host tensors: left unchanged)"""
    g = torch.Generator().manual_seed(41)
    level = torch.rand(N_MODEL, 3, 1, 1, generator=g) * 160 + 40
    contrast = torch.rand(N_MODEL, 1, 1, 1, generator=g) * 60 + 10
    px = (torch.randn(N_MODEL, 3, SRC, SRC, generator=g) * contrast + level).clamp_(0, 255).to(torch.uint8)
    return px, torch.randint(0, 100, (N_MODEL,), generator=g)


def _split():
    from cara_amd.data import ResidentSplit
    px, labels = _split_cpu()
    return ResidentSplit.from_tensors(px.to(DEV), labels.to(DEV))


def _same_size_boxes(n, seed):
    """n boxes of the model's size at random offsets (the corners included) with random flips"""
    g = torch.Generator().manual_seed(seed)
    xy = torch.randint(0, SRC - IMG + 1, (n, 2), generator=g)
    xy[0], xy[-1] = torch.tensor([0, 0]), torch.tensor([SRC - IMG, SRC - IMG])
    flip = torch.randint(0, 2, (n, 1), generator=g)
    flip[0], flip[-1] = 0, 1
    return torch.cat([xy, torch.full((n, 2), IMG), flip], 1).to(torch.int32)


def _precropped_split(rows, boxes):
    """ResidentSplit of the torch-sliced / flipped 32-px images of (rows, boxes), in that order, with their labels"""
    from cara_amd.data import ResidentSplit
    px, labels = _split_cpu()
    return ResidentSplit.from_tensors(_precropped(px, rows, boxes.tolist()), labels[rows].to(DEV))


def _trainable(m):
    return {n: p.detach().clone() for n, p in m.named_parameters() if "CP" in n or "head" in n}


def _one_step(precision, split, idx, dp, boxes):
    """loss, flat gradient and the trainable tensors after one AdamW step, from a fresh model"""
    from cara_amd.optim import AdamW
    m = _model(precision).train()
    eng = m._cara_engine
    opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    kw = {} if boxes is None else {"boxes": boxes}
    loss = eng.train_step_resident(split, idx, opt, droppath=dp, **kw).clone()
    assert eng.resident_bad_rows() == 0
    return loss, eng._flat_grad.clone(), _trainable(m), m


def _assert_same_step(a, b):
    assert torch.equal(a[0], b[0]) and torch.isfinite(a[0])
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and bool(a[1].any())
    assert a[2].keys() == b[2].keys() and len(a[2]) == 14
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_step_with_same_size_boxes_is_bitwise_the_step_on_the_precropped_split(precision):
    rows = [7, 0, 7, 11]
    boxes = _same_size_boxes(BATCH, seed=1)
    idx = torch.tensor(rows, device=DEV)
    dp = ((torch.rand(DEPTH, 2, BATCH, generator=torch.Generator().manual_seed(2)) > 0.3).float() / 0.9).to(DEV)
    start = _trainable(_model(precision))
    with_boxes = _one_step(precision, _split(), idx, dp, boxes.to(DEV))
    cropped = _precropped_split(rows, boxes)
    plain = _one_step(precision, cropped, torch.arange(BATCH, device=DEV), dp, None)
    print(f"[{precision}] loss with boxes {with_boxes[0].item()!r} on the pre-cropped split {plain[0].item()!r}; "
          f"gradient elements that differ: {int((with_boxes[1] != plain[1]).sum())} of {plain[1].numel()}")
    _assert_same_step(with_boxes, plain)
    assert any(not torch.equal(with_boxes[2][n], start[n]) for n in start)
    # the logits: forward_resident with boxes against forward_resident on the pre-cropped split (after the same step each)
    got = with_boxes[3]._cara_engine.forward_resident(_split(), idx, droppath=dp, boxes=boxes.to(DEV))
    want = plain[3]._cara_engine.forward_resident(cropped, torch.arange(BATCH, device=DEV), droppath=dp)
    assert torch.equal(got, want) and torch.isfinite(got).all() and tuple(got.shape) == (BATCH, 100)
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_identity_boxes_on_a_split_of_the_models_size_change_nothing(precision):
    from cara_amd._lib import CaraError
    from cara_amd.data import ResidentSplit
    px, labels = _split_cpu()
    split = ResidentSplit.from_tensors(px[:, :, 5:5 + IMG, 9:9 + IMG].contiguous().to(DEV), labels.to(DEV))
    idx = torch.tensor([3, 3, 10, 0], device=DEV)
    dp = ((torch.rand(DEPTH, 2, BATCH, generator=torch.Generator().manual_seed(3)) > 0.3).float() / 0.9).to(DEV)
    ident = torch.tensor([[0, 0, IMG, IMG, 0]] * BATCH, dtype=torch.int32, device=DEV)
    with_boxes = _one_step(precision, split, idx, dp, ident)
    plain = _one_step(precision, split, idx, dp, None)
    _assert_same_step(with_boxes, plain)
    eng = plain[3]._cara_engine
    assert torch.equal(eng.forward_resident(split, idx, droppath=dp, boxes=ident), eng.forward_resident(split, idx, droppath=dp))
    # without boxes a split of another size than square is still refused; with boxes on another device or of another batch too
    wide = ResidentSplit.from_tensors(px[:, :, :IMG, :].contiguous().to(DEV), labels.to(DEV))
    with pytest.raises(CaraError, match="split"):
        eng.train_step_resident(wide, idx, None)
    with pytest.raises(CaraError, match="boxes must be"):
        eng.train_step_resident(split, idx, None, boxes=ident.cpu())
    with pytest.raises(CaraError, match="boxes must be"):
        eng.train_step_resident(split, idx, None, boxes=ident[:3].contiguous())
    # a box outside its image reaches the device only from a hand-made table: not read, counted
    outside = ident.clone()
    outside[2, 0] = 1
    eng.train_step_resident(split, idx, None, droppath=dp, boxes=outside)
    assert eng.resident_bad_rows() == 1
    torch.cuda.synchronize()


def test_graph_replay_rereads_the_index_vector_and_the_box_table():
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    split = _split()
    g = torch.Generator().manual_seed(8)
    feed = [(torch.randint(0, N_MODEL, (BATCH,), generator=g).to(DEV), _same_size_boxes(BATCH, seed=20 + i).to(DEV)) for i in range(4)]
    assert len({tuple(r.tolist()) for r, _ in feed}) == 4 and len({tuple(b.reshape(-1).tolist()) for _, b in feed}) == 4
    feed[3] = (feed[2][0], feed[3][1])              # the last replay differs from the one before in its boxes alone
    out = {}
    for mode in ("eager", "graph"):
        m = _model(drop_path_rate=0.0).train()
        eng = m._cara_engine
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        gstep = GraphedTrainStep(eng, opt) if mode == "graph" else None
        losses = []
        for it, (r, b) in enumerate(feed):            # warm, capture + replay, replay, replay
            opt.param_groups[0]["lr"] = 1e-3 * (0.7 ** it)
            if gstep is not None:
                loss = gstep(split, (r, b))
            else:
                opt.advance()
                loss = eng.train_step_resident(split, r, opt, boxes=b)
            losses.append(loss.item())
        if gstep is not None:
            (ent,) = gstep._graphs.values()
            rs, bs = ent[2]
            assert ent[1] is split and rs.numel() * rs.element_size() + bs.numel() * bs.element_size() == 28 * BATCH
        assert eng.resident_bad_rows() == 0
        out[mode] = (losses, _trainable(m))
    print(f"losses eager {out['eager'][0]} graph {out['graph'][0]}")
    assert out["graph"][0] == out["eager"][0] and len(set(out["eager"][0])) == 4
    for n in out["eager"][1]:
        assert torch.equal(out["graph"][1][n], out["eager"][1][n]), n


def test_fit_over_rows_and_boxes_equals_fit_over_the_precropped_splits():
    from cara_amd import dist as D
    from cara_amd.recipe import fit
    split = _split()
    seed = 5
    epochs = [D.epoch_shard(N_MODEL, e, 0, 1, BATCH, seed) for e in range(2)]
    assert all(len(ep) == 3 for ep in epochs)
    boxes = [[_same_size_boxes(BATCH, seed=100 * e + s) for s in range(3)] for e in range(2)]
    # the pre-cropped feed: per epoch one split of the 12 cropped images in drawing order, read by rows 0..3, 4..7, 8..11
    cropped = [_precropped_split(torch.cat(epochs[e]).tolist(), torch.cat(boxes[e])) for e in range(2)]
    m_b, m_p = _model(), _model()
    start = _trainable(m_b)
    fit(m_b, (split, lambda e: ((epochs[e][s].to(DEV), boxes[e][s].to(DEV)) for s in range(3))), None, epochs=2, lr=1e-3, seed=seed,
        feed="resident")
    # (fit reads one (split, rows_of) pair and the pre-cropped images differ per epoch: the pixels are swapped in per epoch)
    holder = _precropped_split(torch.cat(epochs[0]).tolist(), torch.cat(boxes[0]))

    def rows_of(e):
        holder.pixels.copy_(cropped[e].pixels)
        holder.labels.copy_(cropped[e].labels)
        return (torch.arange(s * BATCH, (s + 1) * BATCH, device=DEV) for s in range(3))
    fit(m_p, (holder, rows_of), None, epochs=2, lr=1e-3, seed=seed, feed="resident")
    a, b = _trainable(m_b), _trainable(m_p)
    assert a.keys() == b.keys() and len(a) == 14
    for n in a:
        assert torch.equal(a[n], b[n]), n
    assert any(not torch.equal(a[n], start[n]) for n in a)
    assert m_b._cara_engine.resident_bad_rows() == 0
