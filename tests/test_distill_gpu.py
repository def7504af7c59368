"""GPU side of the distillation loss and the teacher pass, both operand builds.  cara_distill_loss through ctypes between sentinels:
every element of every output inside the bound derived in tests/distill_model.py (the shapes, modes and inputs are that module's), the
three bit-for-bit properties, the isolation of a bad label, partner or teacher row, the refusals.  Whole model (the small model of
tests/test_sam_gpu.py, fixed DropPath multipliers): train_step / train_step_resident / GraphedTrainStep with distill= against the same
forward, a direct call of the entry and the backward, by hand (bitwise); the teacher's logits against the teacher's own eval forward.
Figures are printed (-s) before they are asserted; docs/findings/distill.md holds them."""
import ctypes as C
import functools

import pytest
import torch

from oracle import small_kernels as K
from tests import distill_model as M
from tests import test_augmented_feed_gpu as A
from tests.test_augmented_feed_gpu import DEV, L
from tests.test_mix_gpu import _dp, table

pytestmark = pytest.mark.gpu
OPERANDS = ["bf16", "fp16"]
IMG, BATCH = A.IMG, A.BATCH
NAMES = ("terms", "loss", "dlogits")


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _kd(lib, logits, teacher, labels, mix, B, Cn, eps=0.0, alpha=0.5, temperature=1.0, hard=False, dscale=1.0, loss_scale=1.0, want_dlogits=True):
    """cara_distill_loss between sentinels -> loss[0 .. B], dlogits (None without).  logits / teacher / labels / mix: device tensors
    (teacher may be None)"""
    from tests.test_small_kernels_gpu import is_sentinel, sentinel
    p, st = L().ptr, L().stream
    loss = sentinel((64 + 1 + B + 64,), torch.float32)
    d = sentinel((1 + B + 1, Cn), torch.float32)            # (a whole row of guard on either side)
    scaled = loss_scale != 1.0
    amp, found = (torch.tensor([loss_scale, 0.0, 0.0, 0.0], device=DEV), torch.ones(1, device=DEV)) if scaled else (None, None)
    f = C.c_float
    L().check(lib.cara_distill_loss(p(logits), p(teacher), p(labels), p(mix), f(eps), f(alpha), f(temperature), int(hard), p(loss[64:65 + B]),
                                    p(d[1:1 + B]) if want_dlogits else None, B, Cn, f(dscale), p(amp), p(found), st()), "cara_distill_loss")
    torch.cuda.synchronize()
    assert is_sentinel(loss[:64]) and is_sentinel(loss[65 + B:]) and is_sentinel(d[:1]) and is_sentinel(d[1 + B:])
    assert want_dlogits or is_sentinel(d)
    assert found is None or found.item() == 0.0             # found_inf is cleared
    return loss[64:65 + B].clone(), d[1:1 + B].clone() if want_dlogits else None


def _mix(lib, logits, labels, mix, B, Cn, eps, dscale=1.0, loss_scale=1.0):
    """cara_cross_entropy_mix on the same buffers -> loss[0 .. B], dlogits"""
    p, f = L().ptr, C.c_float
    loss, d = torch.empty(1 + B, device=DEV), torch.empty(B, Cn, device=DEV)
    amp = torch.tensor([loss_scale, 0.0, 0.0, 0.0], device=DEV) if loss_scale != 1.0 else None
    L().check(lib.cara_cross_entropy_mix(p(logits), p(labels), p(mix), f(eps), p(loss), p(d), B, Cn, f(dscale), p(amp), None, L().stream()),
              "cara_cross_entropy_mix")
    torch.cuda.synchronize()
    return loss, d


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


# ---- the kernel against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", M.KD_C)
@pytest.mark.parametrize("operands", OPERANDS)
def test_every_element_inside_the_derived_bound(operands, Cn):
    lib = L().lib(operands)
    worst = dict.fromkeys(NAMES, 0.0)
    for B in M.KD_B:
        for v in range(len(M.VARIANTS)):
            z, t, y, mix, kw = M.variant_args(B, Cn, v)
            model = M.variant_model(B, Cn, v)                # (computed once, shared by the two builds)
            loss, d = _kd(lib, *_dev(z, t, y, mix), B, Cn, **kw)
            for name, got in (("terms", loss[1:]), ("loss", loss[0]), ("dlogits", d)):
                ok, ratio = K.hold_f32(got, *model[name])
                if not ok.all():
                    print(f"OUTSIDE {name} B {B} C {Cn} mode {M.VARIANTS[v]}: ratio {ratio}")
                assert ok.all(), (name, B, Cn, M.VARIANTS[v], ratio)
                worst[name] = max(worst[name], ratio)
    print(f"cara_distill_loss [{operands}] C {Cn}: worst |device - model| / bound {worst}")


# ---- the three properties, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
def test_the_three_properties_hold_bit_for_bit(operands):
    lib = L().lib(operands)
    for Cn in (1, 65, 397):
        for B in (3, 65):
            for peaked in (False, True):
                z, t, y, mix = M.kd_case(B, Cn, peaked)
                zd, td, yd, md = _dev(z, t, y, mix)
                for eps, table_, scale in ((0.1, md, M.SCALED), (0.0, None, (1.0, 1.0)), (0.0, md, (1.0, 1.0))):
                    kw = dict(eps=eps, dscale=scale[0], loss_scale=scale[1])
                    # alpha == 0: cara_cross_entropy_mix, with a teacher and with NULL, in either mode
                    base = _mix(lib, zd, yd, table_, B, Cn, **kw)
                    for teacher, hard in ((td, False), (None, False), (None, True), (td, True)):
                        got = _kd(lib, zd, teacher, yd, table_, B, Cn, alpha=0.0, temperature=4.0, hard=hard, **kw)
                        assert _bits_equal(got[0], base[0]) and _bits_equal(got[1], base[1]), ("alpha 0", B, Cn, kw, hard)
                    # dlogits NULL gives the same loss
                    for mode in (dict(alpha=0.5, temperature=4.0), dict(alpha=1.0, temperature=0.5), dict(alpha=0.5, hard=True), dict(alpha=0.0)):
                        with_d = _kd(lib, zd, td, yd, table_, B, Cn, **kw, **mode)
                        without = _kd(lib, zd, td, yd, table_, B, Cn, want_dlogits=False, **kw, **mode)
                        assert without[1] is None and _bits_equal(without[0], with_d[0]), ("no dlogits", B, Cn, kw, mode)
                    # teacher == logits (the same values, another buffer) and alpha == 1: every element of dlogits is exactly 0
                    for T in (0.5, 1.0, 4.0):
                        loss, d = _kd(lib, zd, zd.clone(), yd, table_, B, Cn, alpha=1.0, temperature=T, **kw)
                        assert bool((d == 0.0).all()) and bool((loss == 0.0).all()), ("self", B, Cn, T, kw)


@pytest.mark.parametrize("Cn", [2, 65, 397])
@pytest.mark.parametrize("operands", OPERANDS)
def test_a_bad_label_partner_or_teacher_row_is_isolated_and_bad_arguments_are_refused(operands, Cn):
    lib, B = L().lib(operands), 5
    z, t, _, _ = M.kd_case(B, Cn, False)
    yh = (torch.arange(B) * 7 + 1) % Cn                     # (labels that differ between partners wherever Cn allows)
    mix = table([(B - 1 - i, 0, 0, 0, 0, 0.0, 0.3) for i in range(B)])
    big = torch.zeros(2, B + 2, Cn, device=DEV)
    big[0, 1:B + 1], big[1, 1:B + 1] = z.to(DEV), t.to(DEV)
    logits, teacher = big[0, 1:B + 1], big[1, 1:B + 1]       # (a whole row of margin on either side)
    nan, inf = float("nan"), float("inf")
    for mode in (dict(alpha=0.5, temperature=4.0), dict(alpha=1.0, temperature=0.5), dict(alpha=0.5, hard=True), dict(alpha=1.0, hard=True)):
        loss, d = _kd(lib, logits, teacher, yh.to(DEV), mix.to(DEV), B, Cn, eps=0.1, **mode)
        assert torch.isfinite(loss).all() and torch.isfinite(d).all()

        def check(labels, mix_, bad_at, teacher_=teacher):
            lb, db = _kd(lib, logits, teacher_, labels.to(DEV), mix_.to(DEV), B, Cn, eps=0.1, **mode)
            good = [i for i in range(B) if i not in bad_at]
            assert torch.isnan(lb[0]) and torch.isnan(lb[1:][bad_at]).all() and torch.isnan(db[bad_at]).all(), bad_at
            assert _bits_equal(lb[1:][good], loss[1:][good]) and _bits_equal(db[good], d[good]), bad_at
        y = yh.clone()
        y[1] = Cn                                           # sample 1's own label, which is sample 3's partner label
        check(y, mix, [1, 3])
        y = yh.clone()
        y[4] = -1
        check(y, mix, [0, 4])
        y = yh.clone()
        y[2] = 2 ** 32 + 1                                  # (only its low 32 bits would be a class)
        check(y, mix, [2])
        for entry, at in (((-1, 0, 0, 0, 0, 0.0, 0.3), 2), ((B, 0, 0, 0, 0, 0.0, 0.3), 0), ((1, 0, 0, 0, 0, 0.0, 2.0), 3), ((1, 0, 0, 0, 0, 0.0, nan), 4)):
            m2 = mix.clone()
            m2[at] = table([entry])[0]
            check(yh, m2, [at])
        # a teacher row with a NaN, +inf or -inf: that row alone (the partner's TEACHER row is not read)
        for value, at, col in ((nan, 1, 0), (inf, 3, Cn - 1), (-inf, 0, Cn // 2), (inf, 4, 0)):
            tb = teacher.clone()
            tb[at, col] = value
            check(yh, mix, [at], tb)
    # the refusals: status 1, nothing launched, nothing written
    p, f = L().ptr, C.c_float
    out, dout = torch.full((1 + B,), 7.0, device=DEV), torch.full((B, Cn), 7.0, device=DEV)
    yd, md = yh.to(DEV), mix.to(DEV)

    def call(eps=0.1, alpha=0.5, T=1.0, hard=0, logits_=logits, teacher_=teacher, labels_=yd, loss_=out, B_=B, Cn_=Cn, dscale=1.0):
        return lib.cara_distill_loss(p(logits_), p(teacher_), p(labels_), p(md), f(eps), f(alpha), f(T), hard, p(loss_), p(dout), B_, Cn_,
                                     f(dscale), None, None, L().stream())
    for kw in ({"alpha": -0.1}, {"alpha": 1.5}, {"alpha": nan}, {"T": 0.0}, {"T": -1.0}, {"T": inf}, {"T": nan}, {"T": 1e-39}, {"hard": 2}, {"hard": -1},
               {"teacher_": None}, {"teacher_": None, "hard": 1}, {"eps": 1.0}, {"eps": -0.1}, {"eps": nan}, {"logits_": None}, {"labels_": None},
               {"loss_": None}, {"B_": 0}, {"Cn_": 0}, {"dscale": 0.0}, {"dscale": nan}, {"alpha": 0.0, "eps": 1.0}, {"alpha": 0.0, "hard": 3}):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dout == 7.0).all())


# ---- whole model -------------------------------------------------------------------------------------------------------------------
def _fresh(precision, drop_path_rate=0.1):
    m = A._model(precision, drop_path_rate=drop_path_rate).train()
    return m, m._cara_engine


@functools.lru_cache(maxsize=None)
def _teacher_weights():
    from oracle import cara_oracle as O
    return O.synthetic_cp(rank=8)


def _teacher_model(precision="bf16"):
    """a rank-8 cara() model on the same backbone, left in TRAIN mode with a DropPath rate: neither is consulted"""
    from tests.test_model_gpu import build
    w, _ = A._weights()
    return build(w, _teacher_weights(), 8, 0.1, A.DEPTH, IMG, drop_path_rate=0.2, precision=precision).train()


def _bare_teacher(precision, num_classes=100, img=IMG, patch=16):
    """a rank-8 cara() model as it is initialised (the refusals look at its shape, not at its weights)"""
    from cara_amd import cara, create_model
    m = create_model("vit_base_patch16_224_in21k", depth=A.DEPTH, img_size=img, num_classes=num_classes, patch_size=patch)
    return cara({"model": m, "rank": 8, "scale": 0.1, "l_mu": 1.5, "l_std": 0.1, "precision": precision}).to(DEV)


def _images():
    x = torch.randn(BATCH, 3, IMG, IMG, generator=torch.Generator().manual_seed(3)).to(DEV)
    return x, torch.tensor([5, 99, 0, 5], device=DEV)


def _tensor_teacher(seed=11):
    return (torch.randn(BATCH, 100, generator=torch.Generator().manual_seed(seed)) * 2.0).to(DEV)


def _ema_of(eng, capturable=False):
    """an average that is NOT the weights: every shadow moved by a fixed relative step"""
    ema = eng.make_ema(0.9, capturable=capturable)
    with torch.no_grad():
        for i, s in enumerate(ema.tensors):
            s.mul_(1.0 + 0.03 * ((i % 3) - 1)).add_(0.002)
    return ema


def _by_hand(eng, m, forward, labels, mix, eps, distill, tlogits, dscale, rho=None):
    """one micro-step without the step: forward on the given DropPath multipliers (inside ``forward``), a direct cara_distill_loss on
    its logits and ``tlogits`` with the engine's loss scale, _run_backward(prescaled=True) -- twice around the engine's own perturbation
    for a SAM step -> (loss [1 + B], dlogits, flat gradient, second loss), clones"""
    cp = [getattr(m, "CP_" + n) for n in eng.cp_fields]
    hw, hb = m.head.weight, m.head.bias
    fp16 = eng.precision == "fp16"
    P, f = L().ptr, C.c_float
    alpha, T, hard = distill.c_args()
    with torch.no_grad():
        gv = eng._grad_buffers(m, hw.device)
        eng._flat_grad.zero_()

        def one_pass(loss_buf, dl):
            logits, dp = forward(hw, hb, cp)
            B = logits.shape[0]
            L().check(eng._lib().cara_distill_loss(P(logits), P(tlogits), P(labels), P(mix), f(eps), f(alpha), f(T), hard, P(loss_buf), P(dl), B,
                                                   100, f(dscale), P(eng._amp(hw.device)) if fp16 else None,
                                                   P(gv["_found_inf"]) if fp16 else None, L().stream()), "cara_distill_loss")
            eng._run_backward(dl, dp, hw, cp, prescaled=True)
        B = labels.shape[0]
        lb, dl = torch.empty(1 + B, device=hw.device), torch.empty(B, 100, device=hw.device)
        one_pass(lb, dl)
        second = None
        if rho is not None:
            sam = eng._sam_perturb(m, hw.device, B, rho)
            second = torch.empty(1 + B, device=hw.device)
            one_pass(second, dl)
            eng._sam_restore(sam, hw.device)
        torch.cuda.synchronize()
        return lb.clone(), dl.clone(), eng._flat_grad.clone(), None if second is None else second.clone()


@pytest.mark.parametrize("precision", OPERANDS)
def test_step_with_distill_none_is_bitwise_the_step_without_the_argument(precision):
    from cara_amd.optim import AdamW
    idx = torch.tensor([7, 0, 7, 11], device=DEV)
    boxes = A._same_size_boxes(BATCH, seed=1).to(DEV)
    dp = _dp(2)
    x, y = _images()
    out = {}
    for kw in ({}, {"distill": None}):
        got = []
        for resident in (True, False):
            m, eng = _fresh(precision)
            opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
            if resident:
                loss = eng.train_step_resident(A._split(), idx, opt, droppath=dp, boxes=boxes, label_smoothing=0.1, **kw).clone()
            else:
                loss = eng.train_step(x, y, opt, droppath=dp, **kw).clone()
            assert eng.teacher_logits is None
            got.append((loss, eng._flat_grad.clone(), A._trainable(m), m))
        out[len(kw)] = got
    for a, b in zip(out[0], out[1]):
        A._assert_same_step(a, b)


@pytest.mark.parametrize("precision", OPERANDS)
@pytest.mark.parametrize("how", ["plain", "hard", "window", "sam", "clip"])
def test_step_with_a_tensor_teacher_is_forward_the_entry_and_backward_by_hand(precision, how):
    from cara_amd.loss import Distill
    x, y = _images()
    dp = _dp(2)
    tl = _tensor_teacher()
    d = Distill(tl, alpha=0.5, temperature=2.0, hard=how == "hard")
    m, eng = _fresh(precision)
    m2, eng2 = _fresh(precision)
    fwd = lambda hw, hb, cp: (eng2._run_forward(x, dp, hw, hb, cp), dp)   # noqa: E731
    if how == "window":
        x_b, tl_b, dp_b = torch.flip(x, (0,)).contiguous(), _tensor_teacher(12), _dp(7)
        d_b = Distill(tl_b, alpha=0.5, temperature=2.0)
        l0 = eng.train_step(x, y, None, droppath=dp, distill=d, accumulate=(0, 2)).clone()
        l1 = eng.train_step(x_b, y, None, droppath=dp_b, distill=d_b, accumulate=(1, 2)).clone()
        flat = eng._flat_grad.clone()
        assert eng.teacher_logits is tl_b
        h0 = _by_hand(eng2, m2, fwd, y, None, 0.0, d, tl, 0.5)
        h1 = _by_hand(eng2, m2, lambda hw, hb, cp: (eng2._run_forward(x_b, dp_b, hw, hb, cp), dp_b), y, None, 0.0, d_b, tl_b, 0.5)
        assert torch.equal(l0, h0[0][0]) and torch.equal(l1, h1[0][0]) and _bits_equal(eng._dlogits, h1[1])
        assert _bits_equal(flat, h0[2] + h1[2]) and bool(flat[:-1].any())
        return
    rho = 0.05 if how == "sam" else None
    kw = {"sam_rho": rho} if rho is not None else {"clip_grad": 0.01} if how == "clip" else {}
    got = eng.train_step(x, y, None, droppath=dp, label_smoothing=0.1, distill=d, **kw).clone()
    step = (eng._loss_buf.clone(), eng._dlogits.clone(), eng._flat_grad.clone())
    assert eng.teacher_logits is tl
    hand = _by_hand(eng2, m2, fwd, y, None, 0.1, d, tl, 1.0, rho=rho)
    if how == "clip":
        eng2._clip_flat(0.01)
        torch.cuda.synchronize()
        hand = (hand[0], hand[1], eng2._flat_grad.clone(), None)
        assert float(eng.grad_norm[1]) < 1.0                                   # the clip did scale
    assert torch.isfinite(got) and torch.equal(got, hand[0][0]) and bool(step[2][:-1].any())
    for a, b in zip(step, hand[:3]):
        assert _bits_equal(a, b)
    if rho is not None:
        assert torch.equal(eng.sam_loss, hand[3][0]) and float(eng.sam_loss) != float(got)
    # ... and it is not the plain loss
    m3, eng3 = _fresh(precision)
    plain = eng3.train_step(x, y, None, droppath=dp, label_smoothing=0.1)
    assert abs(float(plain) - float(got)) > 1e-2


def _resident_inputs():
    rows = [7, 0, 3, 11]
    boxes = torch.tensor([(0, 0, A.SRC, A.SRC, 0), (5, 9, 30, 37, 1), (16, 16, IMG, IMG, 0), (3, 2, 41, 20, 1)], dtype=torch.int32)
    mix = table([(3, 0, 0, 0, 0, 0.3, 0.3), (2, 4, 8, 20, 16, 0.0, 20 * 16 / IMG ** 2), (1, 0, 0, 0, 0, 0.75, 0.75), (0, 11, 0, 9, 32, 0.0, 9 / 32)])
    keep = torch.tensor([[0, 3, 1], [2, 2, 0], [3, 1, 2], [1, 0, 3]], dtype=torch.int32)      # 3 of the 4 patches of a 32-px image
    return torch.tensor(rows, device=DEV), boxes.to(DEV), mix.to(DEV), keep.to(DEV)


@pytest.mark.parametrize("precision", OPERANDS)
@pytest.mark.parametrize("feed", ["images", "images+keep", "resident"])
def test_ema_teacher_logits_are_the_engines_eval_forward_on_the_average(precision, feed):
    from cara_amd.loss import Distill
    m, eng = _fresh(precision)
    ema = _ema_of(eng)
    d = Distill(ema, alpha=0.5, temperature=2.0)
    dp = _dp(2)
    x, y = _images()
    idx, bd, md, kd = _resident_inputs()
    split = A._split()
    if feed == "resident":
        got = eng.train_step_resident(split, idx, None, droppath=dp, boxes=bd, mix=md, keep=kd, label_smoothing=0.1, distill=d).clone()
    else:
        got = eng.train_step(x, y, None, droppath=dp, distill=d, **({"keep": kd} if feed == "images+keep" else {})).clone()
    tl, flat, dl = eng.teacher_logits.clone(), eng._flat_grad.clone(), eng._dlogits.clone()
    assert torch.isfinite(got) and torch.isfinite(tl).all() and bool(flat[:-1].any())
    m.eval()                                                 # the engine's own eval-mode, no-grad forward on the average
    with torch.no_grad():
        if feed == "resident":
            want = eng.forward_resident(split, idx, boxes=bd, mix=md, keep=kd, weights=ema)
        else:
            cp, hw, hb = eng._forward_weights(m, x.device, ema)
            want = eng._run_forward(x, None, hw, hb, cp, need_backward=False, keep=kd if feed == "images+keep" else None)
        raw = eng.forward_resident(split, idx, boxes=bd, mix=md, keep=kd) if feed == "resident" else None
    torch.cuda.synchronize()
    assert _bits_equal(tl, want)
    assert raw is None or not _bits_equal(tl, raw)           # the average, not the weights
    assert eng.resident_bad_rows() == 0
    # the student's part is the hand-run sequence on that buffer
    m2, eng2 = _fresh(precision)
    if feed == "resident":
        from cara_amd.feed import Feed
        f = Feed(idx, bd, md, None, kd, None)
        model, dev = eng2._resident_args(split, f)
        labels = eng2._gather_labels(split, idx).clone()
        hand = _by_hand(eng2, m2, lambda hw, hb, cp: (eng2._run_forward_on(model, split, f, dp, hw, hb, cp, True, dev), dp), labels, md, 0.1, d, tl, 1.0)
    else:
        kw = {"keep": kd} if feed == "images+keep" else {}
        hand = _by_hand(eng2, m2, lambda hw, hb, cp: (eng2._run_forward(x, dp, hw, hb, cp, **kw), dp), y, None, 0.0, d, tl, 1.0)
    assert torch.equal(got, hand[0][0]) and _bits_equal(dl, hand[1]) and _bits_equal(flat, hand[2])


@pytest.mark.parametrize("precision", OPERANDS)
def test_alpha_zero_with_an_ema_teacher_leaves_the_plain_steps_gradient(precision):
    from cara_amd.loss import Distill
    from cara_amd.optim import AdamW
    x, y = _images()
    dp = _dp(2)
    out = []
    for distilled in (False, True):
        m, eng = _fresh(precision)
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
        kw = {"distill": Distill(_ema_of(eng), alpha=0.0, temperature=2.0)} if distilled else {}
        loss = eng.train_step(x, y, opt, droppath=dp, label_smoothing=0.1, **kw).clone()
        assert (eng.teacher_logits is not None) == distilled         # the pass did run
        out.append((loss, eng._flat_grad.clone(), A._trainable(m), m))
    A._assert_same_step(out[0], out[1])


@pytest.mark.parametrize("precision", OPERANDS)
@pytest.mark.parametrize("teacher_precision", OPERANDS)
def test_model_teacher_of_another_rank_runs_its_own_eval_forward_and_is_left_alone(precision, teacher_precision):
    from cara_amd.loss import Distill
    x, y = _images()
    dp = _dp(2)
    m, eng = _fresh(precision)
    tm = _teacher_model(teacher_precision)
    teng = tm._cara_engine
    assert teng.rank == 8 and eng.rank == 16 and tm.training
    before = {n: p.detach().clone() for n, p in tm.named_parameters()}
    d = Distill(tm, alpha=0.7, temperature=3.0)
    got = eng.train_step(x, y, None, droppath=dp, distill=d).clone()
    tl, flat, dl = eng.teacher_logits.clone(), eng._flat_grad.clone(), eng._dlogits.clone()
    assert tm.training and all(p.grad is None for p in tm.parameters()) and teng._flat_grad is None
    for n, p in tm.named_parameters():
        assert torch.equal(p, before[n]), n
    tm.eval()
    with torch.no_grad():
        want = tm(x)
    torch.cuda.synchronize()
    assert _bits_equal(tl, want) and torch.isfinite(got)
    m2, eng2 = _fresh(precision)
    hand = _by_hand(eng2, m2, lambda hw, hb, cp: (eng2._run_forward(x, dp, hw, hb, cp), dp), y, None, 0.0, d, tl, 1.0)
    assert torch.equal(got, hand[0][0]) and _bits_equal(dl, hand[1]) and _bits_equal(flat, hand[2])


def test_a_sam_step_runs_one_teacher_pass():
    """the attention-forward call sites of cara_vit_forward, counted by cara_profile_sites: a SAM step adds one student forward, a
    teacher adds one forward to either -- not two to the SAM step"""
    from cara_amd.loss import Distill
    x, y = _images()
    dp = _dp(2)
    m, eng = _fresh("bf16")
    d = Distill(_ema_of(eng), alpha=0.5)
    lib = eng._lib()
    site = 8                                                 # CARA_SITE_ATTN_FWD
    counts = {}
    try:
        for name, kw in (("plain", {}), ("sam", {"sam_rho": 0.05}), ("distill", {"distill": d}), ("sam+distill", {"sam_rho": 0.05, "distill": d})):
            eng.train_step(x, y, None, droppath=dp, **kw)    # (sizes what the leg needs, outside the count)
            torch.cuda.synchronize()
            L().check(lib.cara_profile_sites(C.c_ulonglong(1 << site), 1), "cara_profile_sites")
            eng.train_step(x, y, None, droppath=dp, **kw)
            torch.cuda.synchronize()
            avg, mark, cnt = C.c_float(), C.c_float(), C.c_int()
            L().check(lib.cara_profile_site_read(site, C.byref(avg), C.byref(mark), C.byref(cnt)), "cara_profile_site_read")
            counts[name] = cnt.value
            lib.cara_profile_sites(C.c_ulonglong(0), 1)
    finally:
        lib.cara_profile_sites(C.c_ulonglong(0), 1)
    print(f"attention-forward brackets per step: {counts}")
    per_forward = counts["plain"]
    assert per_forward > 0 and counts["sam"] == 2 * per_forward
    assert counts["distill"] == 2 * per_forward and counts["sam+distill"] == 3 * per_forward


def test_fp16_step_with_a_teacher_is_skipped_on_overflow_and_trains_after():
    from cara_amd.loss import Distill
    from cara_amd.optim import AdamW
    x, y = _images()
    dp = _dp(2)
    m, eng = _fresh("fp16")
    ema = _ema_of(eng)
    d = Distill(ema, alpha=0.5, temperature=2.0)
    opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    eng.train_step(x, y, opt, droppath=dp, distill=d)
    assert eng.skipped_steps == 0 and eng.loss_scale == eng.FP16_LOSS_SCALE
    clean_tl = eng.teacher_logits.clone()
    eng._amp(x.device)[0] = 2.0 ** 30
    before = A._trainable(m)
    loss = eng.train_step(x, y, opt, droppath=dp, distill=d)
    assert torch.isfinite(loss) and eng.skipped_steps == 1 and eng.loss_scale == 2.0 ** 29 and float(eng._flat_grad[-1]) != 0.0
    assert _bits_equal(eng.teacher_logits, clean_tl)         # the teacher pass knows no loss scale
    now = A._trainable(m)
    for n in now:
        assert torch.equal(now[n], before[n]), n
    eng._amp(x.device)[0] = eng.FP16_LOSS_SCALE
    eng.train_step(x, y, opt, droppath=dp, distill=d)
    now = A._trainable(m)
    assert eng.skipped_steps == 1 and float(eng._flat_grad[-1]) == 0.0 and any(not _bits_equal(now[n], before[n]) for n in now)


@pytest.mark.parametrize("precision", OPERANDS)
@pytest.mark.parametrize("teacher", ["tensor", "ema"])
def test_three_graph_replays_equal_three_eager_steps_and_reread_a_tensor_teacher(precision, teacher):
    from cara_amd.loss import Distill
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    split = A._split()
    g = torch.Generator().manual_seed(8)
    rows = [torch.randint(0, A.N_MODEL, (BATCH,), generator=g).to(DEV) for _ in range(4)]
    boxes = [A._same_size_boxes(BATCH, seed=20 + i).to(DEV) for i in range(4)]
    mixes = [table([(3 - i, 0, 0, 0, 0, 0.2 * k + 0.1, 0.2 * k + 0.1) for i in range(BATCH)]).to(DEV) for k in range(4)]
    out = {}
    for mode in ("eager", "graph", "eager, teacher left alone"):
        m, eng = _fresh(precision, drop_path_rate=0.0)
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        tl = _tensor_teacher()
        ema = _ema_of(eng, capturable=True) if teacher == "ema" else None
        d = Distill(tl if teacher == "tensor" else ema, alpha=0.5, temperature=2.0)
        kw = {"label_smoothing": 0.1, "distill": d, **({"ema": ema} if ema is not None else {})}
        gstep = GraphedTrainStep(eng, opt, **kw) if mode == "graph" else None
        losses = []
        for it in range(4):                                 # warm, capture + replay, replay, replay
            if it == 3 and teacher == "tensor" and mode != "eager, teacher left alone":
                tl.mul_(-1.5)                               # after the second replay, in place: the address the graph holds
            if gstep is not None:
                step_loss = gstep(split, (rows[it], boxes[it], mixes[it]))
            else:
                opt.advance()
                if ema is not None:
                    ema.advance()
                step_loss = eng.train_step_resident(split, rows[it], opt, boxes=boxes[it], mix=mixes[it], **kw)
            losses.append(step_loss.item())
        if gstep is not None:
            (key,), (ent,) = gstep._graphs.keys(), gstep._graphs.values()
            assert ent != "warm" and ent[1] is split and ("distill", id(d)) in key and ent[4][-1][0] is d
            assert GraphedTrainStep(eng, opt, label_smoothing=0.1).distill is None
        assert eng.resident_bad_rows() == 0 and eng.skipped_steps == 0
        out[mode] = (losses, A._trainable(m), eng.teacher_logits.clone())
    print(f"[{precision}, {teacher}] losses eager {out['eager'][0]} graph {out['graph'][0]} teacher left alone {out['eager, teacher left alone'][0]}")
    assert out["graph"][0] == out["eager"][0] and len(set(out["eager"][0])) == 4
    assert _bits_equal(out["graph"][2], out["eager"][2])
    for n in out["eager"][1]:
        assert torch.equal(out["graph"][1][n], out["eager"][1][n]), n
    if teacher == "tensor":
        alone = out["eager, teacher left alone"][0]
        assert alone[:3] == out["eager"][0][:3] and abs(alone[3] - out["eager"][0][3]) > 1e-3 * abs(alone[3])


@pytest.mark.parametrize("precision", OPERANDS)
def test_engine_refuses_a_bad_distill_before_a_launch(precision):
    from cara_amd._lib import CaraError
    from cara_amd.ema import ParamEma
    from cara_amd.loss import BCE, Distill
    m, eng = _fresh(precision)
    x, y = _images()
    dp = _dp(2)
    tl = _tensor_teacher()
    eng.train_step(x, y, None, droppath=dp, distill=Distill(tl))
    torch.cuda.synchronize()
    eng._loss_buf.fill_(-7.0)
    eng._dlogits.fill_(-7.0)
    flat = eng._flat_grad.clone()
    v = torch.ones(100, device=DEV)
    _, _, _, kd = _resident_inputs()
    cases = [({"distill": Distill(tl), "loss": BCE()}, "beside"), ({"distill": Distill(tl), "class_weight": v}, "beside"),
             ({"distill": Distill(tl), "logit_bias": v}, "beside"), ({"distill": "ema"}, "distill must be"),
             ({"distill": Distill("ema")}, "ParamEma itself"),
             ({"distill": Distill(tl[:, :99].contiguous())}, "tensor teacher"), ({"distill": Distill(tl[:3].contiguous())}, "tensor teacher"),
             ({"distill": Distill(tl.t().contiguous().t())}, "tensor teacher"), ({"distill": Distill(tl.double())}, "tensor teacher"),
             ({"distill": Distill(tl.cpu())}, "tensor teacher"),                                        # a teacher on another device
             ({"distill": Distill(_bare_teacher(precision).cpu())}, "step's device"),
             ({"distill": Distill(_bare_teacher(precision, num_classes=10))}, "classes"),
             ({"distill": Distill(_bare_teacher(precision, img=2 * IMG))}, "image size"),
             ({"distill": Distill(_bare_teacher(precision, patch=32)), "keep": kd}, "patch grid"),
             ({"distill": Distill(ParamEma([torch.zeros(3, device=DEV)], 0.9))}, "ParamEma")]
    for kw, match in cases:
        with pytest.raises(CaraError, match=match):
            eng.train_step(x, y, None, droppath=dp, **kw)
    torch.cuda.synchronize()
    assert bool((eng._loss_buf == -7.0).all()) and bool((eng._dlogits == -7.0).all()) and _bits_equal(eng._flat_grad, flat)


@pytest.mark.parametrize("precision", OPERANDS)
def test_resident_step_with_a_model_teacher_reads_the_same_rows_and_counts_into_the_students_counter(precision):
    """boxes, mix and keep tables through the teacher's own engine; an index outside the split is refused by the teacher pass too, and
    every refusal lands in the TRAINING engine's counter"""
    from cara_amd.loss import Distill
    idx, bd, md, kd = _resident_inputs()
    split = A._split()
    dp = _dp(5)
    m, eng = _fresh(precision)
    tm = _teacher_model(precision)
    teng = tm._cara_engine
    d = Distill(tm, alpha=0.5, temperature=2.0)
    got = eng.train_step_resident(split, idx, None, droppath=dp, boxes=bd, mix=md, keep=kd, label_smoothing=0.1, distill=d).clone()
    tl, flat, dl = eng.teacher_logits.clone(), eng._flat_grad.clone(), eng._dlogits.clone()
    assert eng.resident_bad_rows() == 0 and teng.resident_bad_rows() == 0 and tm.training
    tm.eval()
    with torch.no_grad():
        want = teng.forward_resident(split, idx, boxes=bd, mix=md, keep=kd)
    torch.cuda.synchronize()
    assert _bits_equal(tl, want) and torch.isfinite(got)
    from cara_amd.feed import Feed
    m2, eng2 = _fresh(precision)
    f = Feed(idx, bd, md, None, kd, None)
    model, dev = eng2._resident_args(split, f)
    labels = eng2._gather_labels(split, idx).clone()
    hand = _by_hand(eng2, m2, lambda hw, hb, cp: (eng2._run_forward_on(model, split, f, dp, hw, hb, cp, True, dev), dp), labels, md, 0.1, d, tl, 1.0)
    assert torch.equal(got, hand[0][0]) and _bits_equal(dl, hand[1]) and _bits_equal(flat, hand[2])
    # one index outside the split: the plain step counts it for the image row and the label row, the teacher pass once more
    bad_idx = idx.clone()
    bad_idx[2] = A.N_MODEL
    tm.train()
    eng.train_step_resident(split, bad_idx, None, droppath=dp, boxes=bd, mix=md, keep=kd)
    plain = eng.resident_bad_rows()
    eng.train_step_resident(split, bad_idx, None, droppath=dp, boxes=bd, mix=md, keep=kd, distill=d)
    distilled = eng.resident_bad_rows()
    print(f"[{precision}] refused indices counted: plain step {plain}, with a model teacher {distilled}")
    assert plain >= 1 and distilled > plain and teng.resident_bad_rows() == 0


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("precision", OPERANDS)
def test_fit_resolves_the_string_ema_to_the_average_it_trains_with(precision, graph):
    from cara_amd.loss import Distill
    from cara_amd.recipe import fit
    x, y = _images()
    m = A._model(precision, drop_path_rate=0.0)
    eng = m._cara_engine
    start, seen, losses = A._trainable(m), [], []
    real = eng.train_step

    def recording(*a, **kw):
        seen.append((kw.get("distill"), kw.get("ema")))
        return real(*a, **kw)
    eng.train_step = recording

    def batches(epoch):
        if epoch > 0:
            losses.append(float(eng._loss_buf[0]))
        return [(x, y)]
    try:
        fit(m, batches, None, epochs=6, lr=1e-2, seed=5, ema_decay=0.5, graph=graph, distill=Distill("ema", alpha=0.5, temperature=2.0))
    finally:
        del eng.train_step
    losses.append(float(eng._loss_buf[0]))
    print(f"[{precision}, graph {graph}] blended loss per epoch: {[round(v, 4) for v in losses]}")
    assert eng.ema is not None and eng.ema.num_updates == 6 and len(seen) >= 1
    for d, ema in seen:                                      # (graphed: the warm call and the capture; eager: every step)
        assert isinstance(d, Distill) and d.kind() == "ema" and d.teacher is eng.ema and ema is eng.ema
        assert (d.alpha, d.temperature, d.hard) == (0.5, 2.0, False)
    assert eng.teacher_logits is not None and eng.teacher_logits.shape == (BATCH, 100) and torch.isfinite(eng.teacher_logits).all()
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0]
    now = A._trainable(m)
    assert all(torch.isfinite(now[n]).all() for n in now) and any(not _bits_equal(now[n], start[n]) for n in now)
