"""GPU side of the class-weighted, logit-adjusted loss, both operand builds.  cara_cross_entropy_bal through ctypes between sentinels:
bitwise cara_cross_entropy_mix without the two vectors, inside the bound derived in tests/balanced_loss_model.py with them (the
shapes, combinations and inputs are that module's), every guard.  Whole model (the small model of tests/test_mix_gpu.py):
train_step / train_step_resident / GraphedTrainStep / fit with class_weight and logit_bias against the step without them (bitwise),
against the kernel on forward_resident's logits (bitwise) and against fp32 autograd of the oracle's as-written model under torch's
cross_entropy(logits + bias, q, weight=w, reduction="sum") / B.  Figures are printed (-s) before they are asserted;
docs/findings/balanced_loss.md holds them."""
import ctypes as C
import functools

import pytest
import torch

from tests import balanced_loss_model as M
from tests import mix_model as X
from tests import small_kernels_common as S
from tests import test_augmented_feed_gpu as A
from tests.test_augmented_feed_gpu import DEV, L
from tests.test_mix_gpu import _dp, table

pytestmark = pytest.mark.gpu
OPERANDS = ["bf16", "fp16"]
DEPTH, N_MODEL, SRC, IMG, BATCH = A.DEPTH, A.N_MODEL, A.SRC, A.IMG, A.BATCH
SCALED = (0.25, 512.0)


def _between_sentinels(v):
    """a device copy of the host vector v with 64 sentinel words on either side -> (whole allocation, the vector's view)"""
    from tests.test_small_kernels_gpu import sentinel
    full = sentinel((64 + v.numel() + 64,), torch.float32)
    full[64:64 + v.numel()] = v.to(DEV)
    return full, full[64:64 + v.numel()]


def _xent_bal(lib, logits, labels, mix, eps, cw, cb, B, Cn, scale=(1.0, 1.0), mix_entry=False):
    """cara_cross_entropy_bal (mix_entry: cara_cross_entropy_mix) between sentinels -> loss[0 .. B], dlogits.  cw / cb: host vectors
    or None; they are handed over between sentinels of their own, which must stand afterwards like everything else"""
    from tests.test_small_kernels_gpu import is_sentinel, sentinel
    p, st = L().ptr, L().stream
    loss = sentinel((1 + B + 1,), torch.float32)
    d = sentinel((B + 1, Cn), torch.float32)
    scaled = scale != (1.0, 1.0)
    amp, found = (torch.tensor([scale[1], 0.0, 0.0, 0.0], device=DEV), torch.ones(1, device=DEV)) if scaled else (None, None)
    tail = (B, Cn, C.c_float(scale[0]), p(amp), p(found), st())
    wf, wv = _between_sentinels(cw) if cw is not None else (None, None)
    bf, bv = _between_sentinels(cb) if cb is not None else (None, None)
    if mix_entry:
        L().check(lib.cara_cross_entropy_mix(p(logits), p(labels), p(mix), C.c_float(eps), p(loss), p(d), *tail), "cara_cross_entropy_mix")
    else:
        L().check(lib.cara_cross_entropy_bal(p(logits), p(labels), p(mix), C.c_float(eps), p(wv), p(bv), p(loss), p(d), *tail),
                  "cara_cross_entropy_bal")
    torch.cuda.synchronize()
    assert is_sentinel(loss[1 + B:]) and is_sentinel(d[B:]) and (found is None or found.item() == 0.0)     # found_inf is cleared
    for full, v, host in ((wf, wv, cw), (bf, bv, cb)):
        if full is not None:
            assert is_sentinel(full[:64]) and is_sentinel(full[64 + v.numel():]) and torch.equal(v.cpu(), host)
    return loss[:1 + B], d[:B]


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
def test_without_weight_and_bias_it_is_bitwise_the_mixed_loss(operands):
    lib = L().lib(operands)
    for Cn in M.BAL_C:
        for B in M.BAL_B:
            for t, eps in ((0.3, 0.1), (0.3, 0.0), (None, 0.0), (None, 0.1)):     # a table with smoothing, one without, no table
                lh, yh, mix = M.bal_case(B, Cn, t)
                logits, labels, md = lh.to(DEV), yh.to(DEV), None if mix is None else mix.to(DEV)
                for scale in ((1.0, 1.0), SCALED):
                    want = _xent_bal(lib, logits, labels, md, eps, None, None, B, Cn, scale, mix_entry=True)
                    got = _xent_bal(lib, logits, labels, md, eps, None, None, B, Cn, scale)
                    assert _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1]), (B, Cn, t, eps, scale)


@pytest.mark.parametrize("operands", OPERANDS)
def test_with_weight_and_bias_inside_the_derived_bound(operands):
    lib = L().lib(operands)
    worst = {"terms": 0.0, "loss": 0.0, "dlogits": 0.0}
    for Cn in M.BAL_C:
        cw, cb = M.presets(Cn)
        for B in M.BAL_B:
            for use_w, use_b, t, eps, scale in M.variants():
                lh, yh, mix = M.bal_case(B, Cn, t)
                w_, b_ = (cw if use_w else None), (cb if use_b else None)
                loss, d = _xent_bal(lib, lh.to(DEV), yh.to(DEV), None if mix is None else mix.to(DEV), eps, w_, b_, B, Cn, scale)
                model = M.xent_bal(lh, yh, mix, eps, w_, b_, *scale)
                for name, got in (("terms", loss[1:]), ("loss", loss[0]), ("dlogits", d)):
                    ok, ratio = S.K.hold_f32(got, *model[name])
                    if not ok.all():
                        print(f"OUTSIDE {name} B {B} C {Cn} weight {use_w} bias {use_b} t {t} eps {eps} scale {scale}: ratio {ratio}")
                    assert ok.all(), (name, B, Cn, use_w, use_b, t, eps, scale, ratio)
                    worst[name] = max(worst[name], ratio)
    print(f"cara_cross_entropy_bal [{operands}]: worst |device - model| / bound {worst}")


@pytest.mark.parametrize("operands", OPERANDS)
def test_all_ones_and_all_zeros_stay_within_the_bounds_of_the_mixed_loss(operands):
    """not bitwise (W_b rounds): the two device results approximate ONE float64 value, each within its own derived bound of it, so
    they lie within the sum of the two bounds of each other"""
    lib = L().lib(operands)
    worst = 0.0
    for Cn in M.BAL_C:
        ones, zeros = torch.ones(Cn), torch.zeros(Cn)
        for B in M.BAL_B:
            for t, eps in ((0.3, 0.1), (None, 0.0)):
                lh, yh, mix = M.bal_case(B, Cn, t)
                args = (lh.to(DEV), yh.to(DEV), None if mix is None else mix.to(DEV), eps)
                want = _xent_bal(lib, *args, None, None, B, Cn, SCALED, mix_entry=True)
                got = _xent_bal(lib, *args, ones, zeros, B, Cn, SCALED)
                bal, mixed = M.xent_bal(lh, yh, mix, eps, ones, zeros, *SCALED), X.xent_mix(lh, yh, mix, eps, *SCALED)
                for name, g, w in (("terms", got[0][1:], want[0][1:]), ("loss", got[0][0], want[0][0]), ("dlogits", got[1], want[1])):
                    assert torch.allclose(bal[name][0], mixed[name][0], rtol=1e-13, atol=1e-15)
                    ok, ratio = S.K.hold_f32(g, w.double().cpu(), bal[name][1] + mixed[name][1])
                    assert ok.all(), (name, B, Cn, t, eps, ratio)
                    worst = max(worst, ratio)
    print(f"all-ones weight, all-zero bias vs cara_cross_entropy_mix [{operands}]: worst |difference| / (sum of the two bounds) {worst:.3f}")


@pytest.mark.parametrize("Cn", [2, 65, 397])
@pytest.mark.parametrize("operands", OPERANDS)
def test_it_refuses_labels_partners_and_weights_outside(operands, Cn):
    lib, B = L().lib(operands), 5
    lh, yh, mix = M.bal_case(B, Cn, 0.3)
    yh = (torch.arange(B) * 7 + 1) % Cn                     # (labels that differ between partners wherever Cn allows)
    cw, cb = M.presets(Cn)
    big = torch.zeros(B + 2, Cn, device=DEV)
    big[1:B + 1] = lh.to(DEV)
    logits = big[1:B + 1]                                   # (a whole row of margin on either side)
    loss, d = _xent_bal(lib, logits, yh.to(DEV), mix.to(DEV), 0.1, cw, cb, B, Cn)
    assert torch.isfinite(loss).all() and torch.isfinite(d).all()
    nan = float("nan")

    def check(labels, mix_, bad_at):
        lb, db = _xent_bal(lib, logits, labels.to(DEV), mix_.to(DEV), 0.1, cw, cb, B, Cn)
        good = [i for i in range(B) if i not in bad_at]
        assert torch.isnan(lb[0]) and torch.isnan(lb[1:][bad_at]).all() and torch.isnan(db[bad_at]).all(), bad_at
        assert _bits_equal(lb[1:][good], loss[1:][good]) and _bits_equal(db[good], d[good]), bad_at
    y = yh.clone()
    y[1] = Cn                                               # sample 1's own label, which is sample 3's partner label
    check(y, mix, [1, 3])
    y = yh.clone()
    y[4] = -1
    check(y, mix, [0, 4])
    y = yh.clone()
    y[2] = 2 ** 32 + 1                                      # (only its low 32 bits would be a class)
    check(y, mix, [2])
    for entry, at in (((-1, 0, 0, 0, 0, 0.0, 0.3), 2), ((B, 0, 0, 0, 0, 0.0, 0.3), 0), ((1, 0, 0, 0, 0, 0.0, 2.0), 3), ((1, 0, 0, 0, 0, 0.0, nan), 4),
                      ((1, 0, 0, 0, 0, 0.0, -0.5), 1)):
        m2 = mix.clone()
        m2[at] = table([entry])[0]
        check(yh, m2, [at])
    # the host refuses a smoothing outside [0, 1) and the other argument errors: status 1, nothing launched, nothing written
    p = L().ptr
    out, dout = torch.full((1 + B,), 7.0, device=DEV), torch.full((B, Cn), 7.0, device=DEV)
    yd, md, wd, bd = yh.to(DEV), mix.to(DEV), cw.to(DEV), cb.to(DEV)

    def call(eps=0.1, logits_=logits, labels_=yd, loss_=out, B_=B, Cn_=Cn, dscale=1.0, w_=wd, b_=bd):
        return lib.cara_cross_entropy_bal(p(logits_), p(labels_), p(md), C.c_float(eps), p(w_), p(b_), p(loss_), p(dout), B_, Cn_,
                                          C.c_float(dscale), None, None, L().stream())
    for eps in (1.0, 1.5, -0.1, nan):
        assert call(eps=eps) == 1 and call(eps=eps, b_=None) == 1 and call(eps=eps, w_=None) == 1 and call(eps=eps, w_=None, b_=None) == 1, eps
    assert call(logits_=None) == 1 and call(labels_=None) == 1 and call(loss_=None) == 1
    assert call(B_=0) == 1 and call(Cn_=0) == 1 and call(dscale=0.0) == 1 and call(dscale=nan) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dout == 7.0).all())


# ---- whole model -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vectors():
    """class weights and logit bias of the 100-class head, on the device (left unchanged)"""
    cw, cb = M.presets(100)
    return cw.to(DEV), cb.to(DEV)


def _fresh(precision, drop_path_rate=0.1):
    m = A._model(precision, drop_path_rate=drop_path_rate).train()
    return m, m._cara_engine


@pytest.mark.parametrize("precision", OPERANDS)
def test_step_with_none_for_both_is_bitwise_the_step_without_the_arguments(precision):
    from cara_amd.optim import AdamW
    idx = torch.tensor([7, 0, 7, 11], device=DEV)
    boxes = A._same_size_boxes(BATCH, seed=1).to(DEV)
    dp = _dp(2)
    x = torch.randn(BATCH, 3, IMG, IMG, generator=torch.Generator().manual_seed(3)).to(DEV)
    y = torch.tensor([5, 99, 0, 5], device=DEV)
    out = {}
    for kw in ({}, {"class_weight": None, "logit_bias": None}):
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
    for a, b in zip(out[0], out[2]):
        A._assert_same_step(a, b)


def _kernel_on(eng, logits, labels, mix, eps, cw, cb, dscale, precision):
    """cara_cross_entropy_bal on `logits` with the engine's loss scale -> loss [1 + B], dlogits"""
    B = logits.shape[0]
    lb, dl = torch.empty(1 + B, device=DEV), torch.empty(B, 100, device=DEV)
    P = L().ptr
    L().check(eng._lib().cara_cross_entropy_bal(P(logits), P(labels), P(mix), C.c_float(eps), P(cw), P(cb), P(lb), P(dl), B, 100,
                                                C.c_float(dscale), P(eng._amp(torch.device(DEV, 0))) if precision == "fp16" else None,
                                                None, L().stream()), "cara_cross_entropy_bal")
    torch.cuda.synchronize()
    return lb, dl


def _oracle(batches, cw, cb):
    """fp32 autograd of the oracle's as-written model: batches = [(x fp32, q float64, droppath)], loss = the mean over the batches of
    torch's cross_entropy(logits + bias, q, weight=w, reduction="sum") / B -> (losses, CP gradients, head gradients)"""
    import torch.nn.functional as F
    from oracle import cara_oracle as O
    w, cp = A._weights()
    cps = {k: v.clone().requires_grad_(True) for k, v in cp.items()}
    cps["CP_A1"], cps["CP_P1"] = cp["CP_A1"][:3 * DEPTH].clone().requires_grad_(True), cp["CP_P1"][:9 * DEPTH].clone().requires_grad_(True)
    ww = dict(w)
    ww["head.weight"], ww["head.bias"] = w["head.weight"].clone().requires_grad_(True), w["head.bias"].clone().requires_grad_(True)
    losses = []
    for x, q, dp in batches:
        rlogits = O.vit_cara_forward(x, ww, cps, s=0.1, depth=DEPTH, drop_path_keep=dp.cpu())
        losses.append(F.cross_entropy(rlogits + cb.cpu(), q.float(), weight=cw.cpu(), reduction="sum") / x.shape[0])
    (sum(losses) / len(losses)).backward()
    return [l_.item() for l_ in losses], cps, ww


def _normalized(v):
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD
    mean, std = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1).double(), torch.tensor(IMAGENET_STD).view(1, 3, 1, 1).double()
    return ((v / 255.0 - mean) / std).float()


def _check_against_oracle(what, precision, m, losses, rlosses, cps, ww, clip=None):
    from oracle import cara_oracle as O
    from tests.test_model_gpu import grad_bar, rel
    if clip is not None:
        torch.nn.utils.clip_grad_norm_([cps[n] for n in O.CP_NAMES] + [ww["head.weight"], ww["head.bias"]], clip)
    bar = X.LOSS_BAR[precision]
    worst = max(rel(getattr(m, n).grad, cps[n].grad) for n in O.CP_NAMES)
    rh = max(rel(m.head.weight.grad, ww["head.weight"].grad), rel(m.head.bias.grad, ww["head.bias"].grad))
    print(f"{what} [{precision}]: losses {[round(v, 5) for v in losses]} vs oracle {[round(v, 5) for v in rlosses]}; worst CP-gradient "
          f"rel-L2 {worst:.2e}, head {rh:.2e}")
    for got, want in zip(losses, rlosses):
        assert abs(got - want) < bar * max(1.0, abs(want)), (got, want)
    assert worst < grad_bar(precision) and rh < grad_bar(precision)


@pytest.mark.parametrize("precision", OPERANDS)
def test_weighted_step_with_mix_and_smoothing_against_the_kernel_and_the_oracle(precision):
    """the inputs of test_mix_gpu's mixed step (different labels, Mixup and CutMix rows in one table, eps = 0.1) with both vectors: the
    step's loss and dlogits are bitwise cara_cross_entropy_bal on forward_resident's logits; the loss and every CP / head gradient
    against fp32 autograd of the oracle under torch's weighted loss on data.soft_target, at the bars that test holds"""
    from cara_amd.data import mix_reference, soft_target
    eps = 0.1
    cw, cb = _vectors()
    rows = [7, 0, 3, 11]
    px, labels = A._split_cpu()
    boxes = torch.tensor([(0, 0, SRC, SRC, 0), (5, 9, 30, 37, 1), (16, 16, IMG, IMG, 0), (3, 2, 41, 20, 1)], dtype=torch.int32)
    mix = table([(3, 0, 0, 0, 0, 0.3, 0.3), (2, 4, 8, 20, 16, 0.0, 20 * 16 / IMG ** 2), (1, 0, 0, 0, 0, 0.75, 0.75), (0, 11, 0, 9, 32, 0.0, 9 / 32)])
    idx, dp, bd, md = torch.tensor(rows, device=DEV), _dp(5), boxes.to(DEV), mix.to(DEV)
    m, eng = _fresh(precision)
    loss = eng.train_step_resident(A._split(), idx, None, droppath=dp, boxes=bd, mix=md, label_smoothing=eps, class_weight=cw,
                                   logit_bias=cb).clone()
    assert eng.resident_bad_rows() == 0
    step_loss, step_dl, flat = eng._loss_buf.clone(), eng._dlogits.clone(), eng._flat_grad.clone()
    logits = eng.forward_resident(A._split(), idx, droppath=dp, boxes=bd, mix=md)
    lb, dl = _kernel_on(eng, logits, labels[rows].to(DEV), md, eps, cw, cb, 1.0, precision)
    assert _bits_equal(step_loss, lb) and _bits_equal(step_dl, dl) and torch.equal(loss, lb[0])
    # ... and it is not the unweighted loss
    plain = _kernel_on(eng, logits, labels[rows].to(DEV), md, eps, None, None, 1.0, precision)[0]
    assert abs(float(plain[0]) - float(lb[0])) > 1e-2
    x = _normalized(mix_reference(px, rows, boxes, mix, IMG))
    q = soft_target(labels[rows], mix, 100, float(torch.tensor(eps, dtype=torch.float32)))
    rlosses, cps, ww = _oracle([(x, q, dp)], cw, cb)
    _check_against_oracle("weighted mixed step", precision, m, [loss.item()], rlosses, cps, ww)
    assert bool(flat[:-1].any())


@pytest.mark.parametrize("precision", OPERANDS)
def test_weighted_window_of_two_with_a_clip_against_the_kernel_and_the_oracle(precision):
    """two micro-steps of one window (accumulate = (i, 2)) with clip_grad: each micro-step's loss is the kernel's on its own logits
    (the last one's dlogits too, at dscale = 1 / 2); the gradients left behind the clip against torch's clip_grad_norm_ of the
    oracle's gradient of the mean of the two losses"""
    from cara_amd.data import resized_crop_reference, soft_target
    cw, cb = _vectors()
    px, labels = A._split_cpu()
    clip = 0.01
    micro = [([7, 0, 3, 11], A._same_size_boxes(BATCH, seed=31), _dp(6)), ([2, 9, 5, 1], A._same_size_boxes(BATCH, seed=32), _dp(7))]
    m, eng = _fresh(precision)
    losses, batches = [], []
    for i, (rows, boxes, dp) in enumerate(micro):
        idx, bd = torch.tensor(rows, device=DEV), boxes.to(DEV)
        losses.append(eng.train_step_resident(A._split(), idx, None, droppath=dp, boxes=bd, accumulate=(i, 2), clip_grad=clip,
                                              class_weight=cw, logit_bias=cb).item())
        step_loss, step_dl = eng._loss_buf.clone(), eng._dlogits.clone()
        logits = eng.forward_resident(A._split(), idx, droppath=dp, boxes=bd)
        lb, dl = _kernel_on(eng, logits, labels[rows].to(DEV), None, 0.0, cw, cb, 0.5, precision)
        assert _bits_equal(step_loss, lb) and _bits_equal(step_dl, dl), i
        batches.append((_normalized(resized_crop_reference(px, rows, boxes, IMG)), soft_target(labels[rows], None, 100, 0.0), dp))
    assert eng.resident_bad_rows() == 0
    norm, coef = eng.grad_norm.tolist()
    rlosses, cps, ww = _oracle(batches, cw, cb)
    print(f"window [{precision}]: norm before the clip {norm:.4f}, coefficient {coef:.4f}")
    assert coef < 1.0                                       # the clip is active
    _check_against_oracle("weighted window of two, clipped", precision, m, losses, rlosses, cps, ww, clip=clip)


@pytest.mark.parametrize("precision", OPERANDS)
def test_graph_replay_rereads_the_class_vectors(precision):
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    split = A._split()
    g = torch.Generator().manual_seed(8)
    rows = [torch.randint(0, N_MODEL, (BATCH,), generator=g).to(DEV) for _ in range(4)]
    boxes = [A._same_size_boxes(BATCH, seed=20 + i).to(DEV) for i in range(4)]
    mixes = [table([(3 - i, 0, 0, 0, 0, 0.2 * k + 0.1, 0.2 * k + 0.1) for i in range(BATCH)]).to(DEV) for k in range(4)]
    out = {}
    for mode in ("eager", "graph", "eager, vector left alone"):
        cw, cb = (v.clone() for v in _vectors())
        m, eng = _fresh(precision, drop_path_rate=0.0)
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        gstep = GraphedTrainStep(eng, opt, label_smoothing=0.1, class_weight=cw, logit_bias=cb) if mode == "graph" else None
        losses = []
        for it in range(4):                                 # warm, capture + replay, replay, replay
            if it == 3 and mode != "eager, vector left alone":
                cw.mul_(torch.linspace(0.5, 2.0, 100, device=DEV))      # in place: the address the graph holds
            if gstep is not None:
                loss = gstep(split, (rows[it], boxes[it], mixes[it]))
            else:
                opt.advance()
                loss = eng.train_step_resident(split, rows[it], opt, boxes=boxes[it], mix=mixes[it], label_smoothing=0.1, class_weight=cw,
                                               logit_bias=cb)
            losses.append(loss.item())
        if gstep is not None:
            (key,), (ent,) = gstep._graphs.keys(), gstep._graphs.values()
            assert ent[1] is split and any(t is cw for t in ent[4]) and any(t is cb for t in ent[4]) and id(cw) in key and id(cb) in key
        assert eng.resident_bad_rows() == 0 and eng.skipped_steps == 0
        out[mode] = (losses, A._trainable(m))
    print(f"[{precision}] losses eager {out['eager'][0]} graph {out['graph'][0]} unchanged vector {out['eager, vector left alone'][0]}")
    assert out["graph"][0] == out["eager"][0]
    for n in out["eager"][1]:
        assert torch.equal(out["graph"][1][n], out["eager"][1][n]), n
    alone = out["eager, vector left alone"][0]
    assert alone[:3] == out["eager"][0][:3] and abs(alone[3] - out["eager"][0][3]) > 1e-3 * abs(alone[3])


@pytest.mark.parametrize("precision", OPERANDS)
def test_engine_refuses_vectors_that_are_no_class_vectors_before_a_launch(precision):
    from cara_amd._lib import CaraError
    from cara_amd.recipe import GraphedTrainStep
    from cara_amd.optim import AdamW
    cw, cb = _vectors()
    m, eng = _fresh(precision)
    idx, boxes, dp = torch.tensor([7, 0, 3, 11], device=DEV), A._same_size_boxes(BATCH, seed=1).to(DEV), _dp(2)
    x, y = torch.zeros(BATCH, 3, IMG, IMG, device=DEV), torch.tensor([5, 99, 0, 5], device=DEV)
    eng.train_step_resident(A._split(), idx, None, droppath=dp, boxes=boxes, class_weight=cw, logit_bias=cb)
    nan, inf = float("nan"), float("inf")

    def mark():
        torch.cuda.synchronize()
        eng._loss_buf.fill_(-7.0)
        eng._dlogits.fill_(-7.0)
        return eng._flat_grad.clone()

    def stands(flat):
        """nothing was launched: the loss buffer, dlogits and the gradients are what mark() left"""
        torch.cuda.synchronize()
        assert bool((eng._loss_buf == -7.0).all()) and bool((eng._dlogits == -7.0).all()) and _bits_equal(eng._flat_grad, flat)
    flat = mark()

    def changed(v, at, value):
        v = v.clone()
        v[at] = value
        return v
    bad = [("class_weight", cw[:99].contiguous()), ("class_weight", torch.cat([cw, cw[:1]])), ("class_weight", cw.double()),
           ("class_weight", cw.cpu()), ("class_weight", cw.reshape(1, 100)), ("class_weight", torch.stack([cw, cw], 1)[:, 0]),
           ("class_weight", cw.tolist()), ("class_weight", changed(cw, 99, -1e-3)), ("class_weight", changed(cw, 0, nan)),
           ("class_weight", changed(cw, 50, inf)),
           ("logit_bias", cb[:99].contiguous()), ("logit_bias", cb.half()), ("logit_bias", cb.cpu()), ("logit_bias", changed(cb, 3, inf)),
           ("logit_bias", changed(cb, 3, -inf)), ("logit_bias", changed(cb, 99, nan))]
    gstep = GraphedTrainStep(eng, AdamW(eng.trainable_parameters(), lr=1e-3, capturable=True), class_weight=changed(cw, 1, -1.0))
    for name, v in bad:
        kw = {"class_weight": cw, "logit_bias": cb, name: v}
        with pytest.raises(CaraError, match=name):
            eng.train_step_resident(A._split(), idx, None, droppath=dp, boxes=boxes, **kw)
        with pytest.raises(CaraError, match=name):
            eng.train_step(x, y, None, droppath=dp, **{name: v})
    with pytest.raises(CaraError, match="class_weight"):
        gstep(x, y)
    stands(flat)
    # a vector that turns bad in place is refused at the next step: the check is remembered per (address, version)
    w2 = cw.clone()
    eng.train_step(x, y, None, droppath=dp, class_weight=w2)
    flat = mark()
    w2[7] = -2.0
    with pytest.raises(CaraError, match="class_weight"):
        eng.train_step(x, y, None, droppath=dp, class_weight=w2)
    stands(flat)
    assert eng.resident_bad_rows() == 0


@pytest.mark.parametrize("precision", OPERANDS)
def test_fit_on_a_long_tailed_split_with_both_vectors(precision):
    from cara_amd.data import RandomResizedCropFlip, ResidentSplit, balanced_class_weight, class_counts, logit_prior
    from cara_amd.recipe import fit
    px, _ = A._split_cpu()
    labels = torch.tensor([0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 57])
    split = ResidentSplit.from_tensors(px.to(DEV), labels.to(DEV))
    test = ResidentSplit.from_tensors(px[:, :, :IMG, :IMG].contiguous().to(DEV), labels.to(DEV))
    counts = class_counts(split, 100)
    assert counts.tolist()[:3] == [6, 3, 2] and int(counts[57]) == 1 and int(counts.sum()) == N_MODEL
    w, a = balanced_class_weight(counts, power=0.5), logit_prior(counts)          # host tensors: fit moves them once
    m = A._model(precision)
    start = A._trainable(m)
    feed = split.train_rows(BATCH, seed=5, rank=0, world=1, augment=RandomResizedCropFlip(IMG))
    best, _ = fit(m, (split, feed), test, epochs=2, lr=1e-3, seed=5, feed="resident", class_weight=w, logit_bias=a, eval_mode="sharded",
                  eval_metric="mean_per_class")
    eng = m._cara_engine
    assert best == 0.0                                      # (no evaluation epoch among two)
    assert torch.isfinite(eng._loss_buf[0]) and float(eng._loss_buf[0]) > 0 and eng.resident_bad_rows() == 0
    after = A._trainable(m)
    assert all(torch.isfinite(after[n]).all() for n in after) and any(not torch.equal(after[n], start[n]) for n in after)
