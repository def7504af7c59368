"""GPU side of the sigmoid losses, both operand builds.  cara_sigmoid_loss through ctypes between sentinels: every element of every
output inside the bound derived in tests/sigmoid_loss_model.py (the shapes, modes and inputs are that module's), the three bit-for-bit
identities, the NaN isolation of a bad label, partner or weight, the refusals.  Whole model (the small model of
tests/test_balanced_loss_gpu.py): train_step / train_step_resident / GraphedTrainStep with loss= against the same forward, a direct
call of the entry and the backward, by hand (bitwise).  Figures are printed (-s) before they are asserted;
docs/findings/sigmoid_loss.md holds them.

Measured on an MI355X, worst |device - model| / bound over all cases: see docs/findings/sigmoid_loss.md."""
import ctypes as C

import pytest
import torch

from oracle import small_kernels as K
from tests import sigmoid_loss_model as M
from tests import test_augmented_feed_gpu as A
from tests.test_augmented_feed_gpu import DEV, L
from tests.test_mix_gpu import _dp, table

pytestmark = pytest.mark.gpu
OPERANDS = ["bf16", "fp16"]
DEPTH, N_MODEL, SRC, IMG, BATCH = A.DEPTH, A.N_MODEL, A.SRC, A.IMG, A.BATCH
NAMES = ("terms", "loss", "dlogits")


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _sig(lib, logits, labels, mix, B, Cn, eps=0.0, thr=None, fgamma=0.0, alpha=None, pw=None, sum_classes=False, dscale=1.0, loss_scale=1.0,
         want_dlogits=True):
    """cara_sigmoid_loss between sentinels -> loss[0 .. B], dlogits (None without).  logits / labels / mix: device tensors; pw: a host
    vector or None, handed over between sentinels of its own, which must stand afterwards like everything else"""
    from tests.test_small_kernels_gpu import is_sentinel, sentinel
    p, st = L().ptr, L().stream
    loss = sentinel((64 + 1 + B + 64,), torch.float32)
    d = sentinel((1 + B + 1, Cn), torch.float32)            # (a whole row of guard on either side)
    scaled = loss_scale != 1.0
    amp, found = (torch.tensor([loss_scale, 0.0, 0.0, 0.0], device=DEV), torch.ones(1, device=DEV)) if scaled else (None, None)
    wf = wv = None
    if pw is not None:
        wf = sentinel((64 + Cn + 64,), torch.float32)
        wf[64:64 + Cn] = pw.to(DEV)
        wv = wf[64:64 + Cn]
    f = C.c_float
    L().check(lib.cara_sigmoid_loss(p(logits), p(labels), p(mix), f(eps), f(-1.0 if thr is None else thr), f(fgamma),
                                    f(-1.0 if alpha is None else alpha), p(wv), int(sum_classes), p(loss[64:65 + B]),
                                    p(d[1:1 + B]) if want_dlogits else None, B, Cn, f(dscale), p(amp), p(found), st()), "cara_sigmoid_loss")
    torch.cuda.synchronize()
    assert is_sentinel(loss[:64]) and is_sentinel(loss[65 + B:]) and is_sentinel(d[:1]) and is_sentinel(d[1 + B:])
    assert want_dlogits or is_sentinel(d)
    assert found is None or found.item() == 0.0             # found_inf is cleared
    if wf is not None:
        assert is_sentinel(wf[:64]) and is_sentinel(wf[64 + Cn:]) and torch.equal(wv.cpu(), pw)
    return loss[64:65 + B].clone(), d[1:1 + B].clone() if want_dlogits else None


def _on_device(l, y, mix):
    return l.to(DEV), y.to(DEV), None if mix is None else mix.to(DEV)


# ---- the kernel against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", M.SIG_C)
@pytest.mark.parametrize("operands", OPERANDS)
def test_every_element_inside_the_derived_bound(operands, Cn):
    lib = L().lib(operands)
    worst = dict.fromkeys(NAMES, 0.0)
    for B in M.SIG_B:
        for v in range(len(M.VARIANTS)):
            l, y, mix, kw = M.variant_args(B, Cn, v)         # (asserts the threshold's margin on the float64 target)
            model = M.variant_model(B, Cn, v)                # (computed once, shared by the two builds)
            loss, d = _sig(lib, *_on_device(l, y, mix), B, Cn, **kw)
            for name, got in (("terms", loss[1:]), ("loss", loss[0]), ("dlogits", d)):
                ok, ratio = K.hold_f32(got, *model[name])
                if not ok.all():
                    print(f"OUTSIDE {name} B {B} C {Cn} mode {M.VARIANTS[v]}: ratio {ratio}")
                assert ok.all(), (name, B, Cn, M.VARIANTS[v], ratio)
                worst[name] = max(worst[name], ratio)
    print(f"cara_sigmoid_loss [{operands}] C {Cn}: worst |device - model| / bound {worst}")


# ---- identities, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
def test_the_three_identities_hold_bit_for_bit(operands):
    lib = L().lib(operands)
    for Cn in (1, 65, 397):
        ones = torch.ones(Cn)
        for B in (3, 65):
            l, y, mix = M.sig_case(B, Cn)
            ld, yd, md = _on_device(l, y, mix)
            for eps, thr, sumc, scale in ((0.1, None, False, M.SCALED), (0.1, M.THR, True, (1.0, 1.0)), (0.0, None, False, (1.0, 1.0))):
                kw = dict(eps=eps, thr=thr, sum_classes=sumc, dscale=scale[0], loss_scale=scale[1])
                base = _sig(lib, ld, yd, md, B, Cn, **kw)
                # pos_weight of all ones == pos_weight NULL
                got = _sig(lib, ld, yd, md, B, Cn, pw=ones, **kw)
                assert _bits_equal(got[0], base[0]) and _bits_equal(got[1], base[1]), ("ones", B, Cn, kw)
                # alpha < 0 (any negative number), gamma == 0 runs the BCE launches
                got = _sig(lib, ld, yd, md, B, Cn, alpha=-0.5, fgamma=0.0, **kw)
                assert _bits_equal(got[0], base[0]) and _bits_equal(got[1], base[1]), ("alpha < 0", B, Cn, kw)
                # dlogits NULL gives the same loss -- of either launch
                for extra in ({}, {"pw": M.pos_weight(Cn)}, {"fgamma": 2.0, "alpha": 0.25}, {"fgamma": 1.5}):
                    with_d = _sig(lib, ld, yd, md, B, Cn, **kw, **extra)
                    without = _sig(lib, ld, yd, md, B, Cn, want_dlogits=False, **kw, **extra)
                    assert without[1] is None and _bits_equal(without[0], with_d[0]), ("no dlogits", B, Cn, kw, extra)


@pytest.mark.parametrize("Cn", [2, 65, 397])
@pytest.mark.parametrize("operands", OPERANDS)
def test_a_bad_label_partner_or_weight_is_isolated_and_bad_arguments_are_refused(operands, Cn):
    lib, B = L().lib(operands), 5
    l, _, _ = M.sig_case(B, Cn)
    yh = (torch.arange(B) * 7 + 1) % Cn                     # (labels that differ between partners wherever Cn allows)
    mix = table([(B - 1 - i, 0, 0, 0, 0, 0.0, 0.3) for i in range(B)])
    big = torch.zeros(B + 2, Cn, device=DEV)
    big[1:B + 1] = l.to(DEV)
    logits = big[1:B + 1]                                   # (a whole row of margin on either side)
    nan = float("nan")
    for mode in (dict(pw=M.pos_weight(Cn)), dict(thr=M.THR), dict(fgamma=2.0, alpha=0.25, sum_classes=True)):
        loss, d = _sig(lib, logits, yh.to(DEV), mix.to(DEV), B, Cn, eps=0.1, **mode)
        assert torch.isfinite(loss).all() and torch.isfinite(d).all()

        def check(labels, mix_, bad_at):
            lb, db = _sig(lib, logits, labels.to(DEV), mix_.to(DEV), B, Cn, eps=0.1, **mode)
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
        for entry, at in (((-1, 0, 0, 0, 0, 0.0, 0.3), 2), ((B, 0, 0, 0, 0, 0.0, 0.3), 0), ((1, 0, 0, 0, 0, 0.0, 2.0), 3), ((1, 0, 0, 0, 0, 0.0, nan), 4),
                          ((1, 0, 0, 0, 0, 0.0, -0.5), 1)):
            m2 = mix.clone()
            m2[at] = table([entry])[0]
            check(yh, m2, [at])
    # the refusals: status 1, nothing launched, nothing written
    p, f = L().ptr, C.c_float
    out, dout = torch.full((1 + B,), 7.0, device=DEV), torch.full((B, Cn), 7.0, device=DEV)
    yd, md, wd = yh.to(DEV), mix.to(DEV), M.pos_weight(Cn).to(DEV)

    def call(eps=0.1, thr=-1.0, fgamma=0.0, alpha=-1.0, pw=None, sumc=0, logits_=logits, labels_=yd, loss_=out, B_=B, Cn_=Cn, dscale=1.0):
        return lib.cara_sigmoid_loss(p(logits_), p(labels_), p(md), f(eps), f(thr), f(fgamma), f(alpha), p(pw), sumc, p(loss_), p(dout), B_, Cn_,
                                     f(dscale), None, None, L().stream())
    inf = float("inf")
    for kw in ({"eps": 1.0}, {"eps": -0.1}, {"eps": nan}, {"thr": 1.0}, {"thr": nan}, {"fgamma": -1.0}, {"fgamma": 0.5}, {"fgamma": inf},
               {"fgamma": nan}, {"alpha": 1.5}, {"alpha": nan}, {"pw": wd, "fgamma": 2.0}, {"pw": wd, "alpha": 0.25}, {"sumc": 2}, {"sumc": -1},
               {"logits_": None}, {"labels_": None}, {"loss_": None}, {"B_": 0}, {"Cn_": 0}, {"dscale": 0.0}, {"dscale": nan}):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dout == 7.0).all())


# ---- whole model -------------------------------------------------------------------------------------------------------------------
def _fresh(precision, drop_path_rate=0.1):
    m = A._model(precision, drop_path_rate=drop_path_rate).train()
    return m, m._cara_engine


def _pw100():
    return M.pos_weight(100).to(DEV)


def _images():
    x = torch.randn(BATCH, 3, IMG, IMG, generator=torch.Generator().manual_seed(3)).to(DEV)
    return x, torch.tensor([5, 99, 0, 5], device=DEV)


def _by_hand(eng, m, forward, labels, mix, eps, loss, dscale, rho=None):
    """one micro-step without the step: forward on the given DropPath multipliers (inside ``forward``), a direct cara_sigmoid_loss on
    its logits with the engine's loss scale, _run_backward(prescaled=True) -- twice around the engine's own perturbation for a SAM
    step -> (loss [1 + B], dlogits, flat gradient), clones"""
    cp = [getattr(m, "CP_" + n) for n in eng.cp_fields]
    hw, hb = m.head.weight, m.head.bias
    fp16 = eng.precision == "fp16"
    P, f = L().ptr, C.c_float
    thr, fg, alpha = loss.c_args()
    with torch.no_grad():
        gv = eng._grad_buffers(m, hw.device)
        eng._flat_grad.zero_()

        def one_pass(loss_buf, dl):
            logits, dp = forward(hw, hb, cp)
            B = logits.shape[0]
            L().check(eng._lib().cara_sigmoid_loss(P(logits), P(labels), P(mix), f(eps), f(thr), f(fg), f(alpha), P(loss.pos_weight),
                                                   int(loss.sum_classes), P(loss_buf), P(dl), B, 100, f(dscale),
                                                   P(eng._amp(hw.device)) if fp16 else None, P(gv["_found_inf"]) if fp16 else None,
                                                   L().stream()), "cara_sigmoid_loss")
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
def test_train_step_with_a_bce_is_forward_the_entry_and_backward_by_hand(precision):
    x, y = _images()
    dp = _dp(2)
    loss = _bce(0.2)
    m, eng = _fresh(precision)
    got = eng.train_step(x, y, None, droppath=dp, label_smoothing=0.1, loss=loss).clone()
    step = (eng._loss_buf.clone(), eng._dlogits.clone(), eng._flat_grad.clone())
    m2, eng2 = _fresh(precision)
    hand = _by_hand(eng2, m2, lambda hw, hb, cp: (eng2._run_forward(x, dp, hw, hb, cp), dp), y, None, 0.1, loss, 1.0)
    assert torch.isfinite(got) and torch.equal(got, hand[0][0]) and bool(step[2][:-1].any())
    for a, b in zip(step, hand):
        assert _bits_equal(a, b)
    # ... and it is not the softmax loss
    m3, eng3 = _fresh(precision)
    plain = eng3.train_step(x, y, None, droppath=dp, label_smoothing=0.1)
    assert abs(float(plain) - float(got)) > 1e-2


def _bce(thr=None, sum_classes=False):
    from cara_amd.loss import BCE
    return BCE(target_threshold=thr, pos_weight=_pw100(), sum_classes=sum_classes)


def _resident_inputs():
    rows = [7, 0, 3, 11]
    boxes = torch.tensor([(0, 0, SRC, SRC, 0), (5, 9, 30, 37, 1), (16, 16, IMG, IMG, 0), (3, 2, 41, 20, 1)], dtype=torch.int32)
    mix = table([(3, 0, 0, 0, 0, 0.3, 0.3), (2, 4, 8, 20, 16, 0.0, 20 * 16 / IMG ** 2), (1, 0, 0, 0, 0, 0.75, 0.75), (0, 11, 0, 9, 32, 0.0, 9 / 32)])
    return torch.tensor(rows, device=DEV), boxes.to(DEV), mix.to(DEV)


def _resident_forward(eng, m, split, idx, bd, md, dp):
    from cara_amd.feed import Feed
    feed = Feed(idx, bd, md, None, None, None)
    model, dev = eng._resident_args(split, feed)
    return lambda hw, hb, cp: (eng._run_forward_on(model, split, feed, dp, hw, hb, cp, True, dev), dp)


@pytest.mark.parametrize("precision", OPERANDS)
@pytest.mark.parametrize("how", ["plain", "window", "sam"])
def test_resident_step_with_a_focal_loss_and_a_mix_is_the_sequence_by_hand(precision, how):
    from cara_amd.loss import Focal
    loss = Focal(gamma=2.0, alpha=0.25)
    split = A._split()
    idx, bd, md = _resident_inputs()
    dp = _dp(5)
    m, eng = _fresh(precision)
    m2, eng2 = _fresh(precision)
    labels = eng2._gather_labels(split, idx).clone()
    if how == "window":
        idx_b = torch.tensor([2, 9, 5, 1], device=DEV)
        dp_b = _dp(7)
        l0 = eng.train_step_resident(split, idx, None, droppath=dp, boxes=bd, mix=md, loss=loss, accumulate=(0, 2)).clone()
        l1 = eng.train_step_resident(split, idx_b, None, droppath=dp_b, boxes=bd, mix=md, loss=loss, accumulate=(1, 2)).clone()
        flat = eng._flat_grad.clone()
        h0 = _by_hand(eng2, m2, _resident_forward(eng2, m2, split, idx, bd, md, dp), labels, md, 0.0, loss, 0.5)
        labels_b = eng2._gather_labels(split, idx_b).clone()
        h1 = _by_hand(eng2, m2, _resident_forward(eng2, m2, split, idx_b, bd, md, dp_b), labels_b, md, 0.0, loss, 0.5)
        assert torch.equal(l0, h0[0][0]) and torch.equal(l1, h1[0][0]) and _bits_equal(eng._dlogits, h1[1])
        assert _bits_equal(flat, h0[2] + h1[2]) and bool(flat[:-1].any())
    else:
        rho = 0.05 if how == "sam" else None
        kw = {} if rho is None else {"sam_rho": rho}
        got = eng.train_step_resident(split, idx, None, droppath=dp, boxes=bd, mix=md, label_smoothing=0.1, loss=loss, **kw).clone()
        step = (eng._loss_buf.clone(), eng._dlogits.clone(), eng._flat_grad.clone())
        hand = _by_hand(eng2, m2, _resident_forward(eng2, m2, split, idx, bd, md, dp), labels, md, 0.1, loss, 1.0, rho=rho)
        assert torch.isfinite(got) and torch.equal(got, hand[0][0]) and bool(step[2][:-1].any())
        for a, b in zip(step, hand[:3]):
            assert _bits_equal(a, b)
        if rho is not None:
            assert torch.equal(eng.sam_loss, hand[3][0]) and float(eng.sam_loss) != float(got)
            for n, t in A._trainable(m).items():
                assert torch.equal(t, A._trainable(m2)[n]), n           # the weights are back
    assert eng.resident_bad_rows() == 0 and eng2.resident_bad_rows() == 0


@pytest.mark.parametrize("precision", OPERANDS)
def test_step_with_loss_none_is_bitwise_the_step_without_the_argument(precision):
    from cara_amd.optim import AdamW
    idx = torch.tensor([7, 0, 7, 11], device=DEV)
    boxes = A._same_size_boxes(BATCH, seed=1).to(DEV)
    dp = _dp(2)
    x, y = _images()
    out = {}
    for kw in ({}, {"loss": None}):
        got = []
        for resident in (True, False):
            m, eng = _fresh(precision)
            opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
            if resident:
                loss = eng.train_step_resident(A._split(), idx, opt, droppath=dp, boxes=boxes, label_smoothing=0.1, **kw).clone()
            else:
                loss = eng.train_step(x, y, opt, droppath=dp, **kw).clone()
            got.append((loss, eng._flat_grad.clone(), A._trainable(m), m))
        out[len(kw)] = got
    for a, b in zip(out[0], out[1]):
        A._assert_same_step(a, b)


@pytest.mark.parametrize("precision", OPERANDS)
def test_graph_replays_equal_the_eager_steps_and_reread_pos_weight(precision):
    from cara_amd.loss import BCE
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    split = A._split()
    g = torch.Generator().manual_seed(8)
    rows = [torch.randint(0, N_MODEL, (BATCH,), generator=g).to(DEV) for _ in range(4)]          # (different labels at every call)
    boxes = [A._same_size_boxes(BATCH, seed=20 + i).to(DEV) for i in range(4)]
    mixes = [table([(3 - i, 0, 0, 0, 0, 0.2 * k + 0.1, 0.2 * k + 0.1) for i in range(BATCH)]).to(DEV) for k in range(4)]
    out = {}
    for mode in ("eager", "graph", "eager, vector left alone"):
        pw = _pw100().clone()
        loss = BCE(target_threshold=None, pos_weight=pw, sum_classes=True)
        m, eng = _fresh(precision, drop_path_rate=0.0)
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        gstep = GraphedTrainStep(eng, opt, label_smoothing=0.1, loss=loss) if mode == "graph" else None
        losses = []
        for it in range(4):                                 # warm, capture + replay, replay, replay
            if it == 3 and mode != "eager, vector left alone":
                pw.mul_(torch.linspace(0.5, 2.0, 100, device=DEV))      # in place: the address the graph holds
            if gstep is not None:
                step_loss = gstep(split, (rows[it], boxes[it], mixes[it]))
            else:
                opt.advance()
                step_loss = eng.train_step_resident(split, rows[it], opt, boxes=boxes[it], mix=mixes[it], label_smoothing=0.1, loss=loss)
            losses.append(step_loss.item())
        if gstep is not None:
            (key,), (ent,) = gstep._graphs.keys(), gstep._graphs.values()
            assert ent[1] is split and any(t is pw for t in ent[4]) and any(t is loss for t in ent[4]) and ("loss", *loss.key()) in key
        assert eng.resident_bad_rows() == 0 and eng.skipped_steps == 0
        out[mode] = (losses, A._trainable(m))
    print(f"[{precision}] losses eager {out['eager'][0]} graph {out['graph'][0]} unchanged vector {out['eager, vector left alone'][0]}")
    assert out["graph"][0] == out["eager"][0] and len(set(out["eager"][0])) == 4
    for n in out["eager"][1]:
        assert torch.equal(out["graph"][1][n], out["eager"][1][n]), n
    alone = out["eager, vector left alone"][0]
    assert alone[:3] == out["eager"][0][:3] and abs(alone[3] - out["eager"][0][3]) > 1e-3 * abs(alone[3])


@pytest.mark.parametrize("precision", OPERANDS)
def test_engine_refuses_a_loss_beside_class_vectors_and_a_bad_pos_weight_before_a_launch(precision):
    from cara_amd._lib import CaraError
    from cara_amd.loss import BCE, Focal
    m, eng = _fresh(precision)
    x, y = _images()
    dp = _dp(2)
    pw = _pw100()
    eng.train_step(x, y, None, droppath=dp, loss=BCE(pos_weight=pw))
    torch.cuda.synchronize()
    eng._loss_buf.fill_(-7.0)
    eng._dlogits.fill_(-7.0)
    flat = eng._flat_grad.clone()
    bad = pw.clone()
    bad[3] = -1.0
    for kw, match in (({"loss": Focal(), "class_weight": pw}, "class_weight"), ({"loss": BCE(), "logit_bias": pw}, "class_weight"),
                      ({"loss": "bce"}, "loss must be"), ({"loss": BCE(pos_weight=bad)}, "pos_weight"), ({"loss": BCE(pos_weight=pw[:99].contiguous())}, "pos_weight"),
                      ({"loss": BCE(pos_weight=pw.cpu())}, "pos_weight")):
        with pytest.raises(CaraError, match=match):
            eng.train_step(x, y, None, droppath=dp, **kw)
    w2 = pw.clone()
    ok = BCE(pos_weight=w2)
    w2[7] = float("nan")                                    # (never seen good: refused at its first step)
    with pytest.raises(CaraError, match="pos_weight"):
        eng.train_step(x, y, None, droppath=dp, loss=ok)
    torch.cuda.synchronize()
    assert bool((eng._loss_buf == -7.0).all()) and bool((eng._dlogits == -7.0).all()) and _bits_equal(eng._flat_grad, flat)
