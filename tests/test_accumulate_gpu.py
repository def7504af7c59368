"""Gradient accumulation in the fused step (train_step(..., accumulate=(i, k))) on the device: linearity -- the window's flat buffer is
bitwise the left-to-right fp32 sum of the micro-batches' stand-alone gradients, each scaled by the power of two 1 / k -- the window
against fp32 autograd of the as-written algorithm on the whole batch, what a window may and may not touch before its last
micro-step, the fp16 loss scale across a window, and recipe.fit(accum_steps=).  Depth 2, 224 px, rank 16, micro-batches of 2."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ["bf16", "fp16"]
DEPTH, MICRO = 2, 2


@functools.lru_cache(maxsize=None)
def _weights():
    from oracle import cara_oracle as O
    return O.synthetic_backbone(depth=DEPTH), O.synthetic_cp(rank=16, depth=DEPTH)


@functools.lru_cache(maxsize=None)
def _batch(n):
    """n samples (host tensors, left unchanged) and explicit DropPath multipliers [depth, 2, n]"""
    from oracle import cara_oracle as O
    from tests.test_model_gpu import _keep
    x, y = O.synthetic_batch(batch=n, seed_x=3, seed_y=4)
    return x, y, _keep(DEPTH, n, seed=13)


def _model(precision="bf16", drop_path_rate=0.1):
    from tests.test_model_gpu import build
    w, cp = _weights()
    return build(w, cp, 16, 0.1, DEPTH, 224, drop_path_rate=drop_path_rate, precision=precision).train()


def _micro(n, i, keep=True):
    x, y, dp = _batch(n)
    s = slice(i * MICRO, (i + 1) * MICRO)
    return x[s].to(DEV), y[s].to(DEV), (dp[:, :, s].contiguous().to(DEV) if keep else None)


def _run(eng, n, i, k, opt=None, **kw):
    """micro-step i of a window of k over the n-sample batch, with that micro-batch's DropPath multipliers"""
    x, y, dp = _micro(n, i)
    return eng.train_step(x, y, opt, droppath=dp, accumulate=(i, k), **kw)


def _trainable(m):
    return {n: p.detach().clone() for n, p in m.named_parameters() if "CP" in n or "head" in n}


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- linearity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 4])
def test_a_window_is_bitwise_the_sum_of_its_micro_batches_scaled_gradients(k):
    """bf16 build.  Scaling dlogits by 1 / k (a power of two) is exact in fp32 and commutes with every 16-bit rounding, and every
    backward kernel is linear in its incoming gradient: micro-step i's flat buffer is (1 / k) x the stand-alone step's, exactly,
    and cara_grad_accumulate adds them left to right with one rounding each."""
    n = k * MICRO
    win, alone = _model(), _model()
    ew, ea = win._cara_engine, alone._cara_engine
    parts, losses = [], []
    for i in range(k):
        x, y, dp = _micro(n, i)
        lw = ew.train_step(x, y, None, droppath=dp, accumulate=(i, k)).clone()
        la = ea.train_step(x, y, None, droppath=dp).clone()
        assert torch.equal(lw, la) and torch.isfinite(lw)              # the returned loss is the micro-batch's own mean, unscaled
        parts.append(ea._flat_grad.cpu().clone())
        losses.append(float(lw))
    want = parts[0] * (1.0 / k)
    for part in parts[1:]:
        want = want + part * (1.0 / k)
    got = ew._flat_grad.cpu()
    views = ew._grad_views
    off, differ = 0, {}
    for name, v in views.items():
        sz = v.numel()
        bad = int((got[off:off + sz].view(torch.int32) != want[off:off + sz].view(torch.int32)).sum())
        if bad:
            differ[name] = (bad, sz)
        off += sz
    print(f"k {k}: micro-batch losses {losses}; tensors whose bits differ from the scaled sum (elements, of): {differ}")
    assert off == got.numel() and bool(got[:-1].any()) and len(set(losses)) == k
    assert not differ, differ
    assert win.head.weight.grad.data_ptr() == views["head_w"].data_ptr()


# ---- against the reference algorithm -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [2, 3])
def test_a_window_against_the_as_written_algorithm_on_the_whole_batch(k, precision):
    """drop_path_rate = 0: the window's gradients are the full batch's (mean loss over k x 2 samples); the loss of every micro-step is
    its micro-batch's.  Bars of tests/tolerances.py as tests/test_model_gpu.py::test_train_step_against_oracle holds them."""
    import torch.nn.functional as F
    from oracle import cara_oracle as O
    from tests.mix_model import LOSS_BAR
    from tests.test_model_gpu import grad_bar, rel
    n = k * MICRO
    x, y, _ = _batch(n)
    w, cp = _weights()
    m = _model(precision, drop_path_rate=0.0)
    eng = m._cara_engine
    losses = [float(eng.train_step(*_micro(n, i, keep=False)[:2], None, accumulate=(i, k))) for i in range(k)]
    cps = dict(cp)
    cps["CP_A1"], cps["CP_P1"] = cp["CP_A1"][:3 * DEPTH], cp["CP_P1"][:9 * DEPTH]
    head = {"weight": w["head.weight"], "bias": w["head.bias"]}
    rloss, rlogits, gref = O.train_step_as_written(x, y, w, cps, head, s=0.1, depth=DEPTH)
    # (without DropPath a sample's logits do not depend on its batch: the micro-batches' losses come from the full batch's logits)
    want = [float(F.cross_entropy(rlogits[i * MICRO:(i + 1) * MICRO].detach(), y[i * MICRO:(i + 1) * MICRO])) for i in range(k)]
    assert abs(sum(want) / k - float(rloss)) < 1e-5
    for got, ref in zip(losses, want):
        assert abs(got - ref) < LOSS_BAR[precision] * max(1.0, abs(ref)), (losses, want)
    worst = max(rel(getattr(m, nm).grad, gref[nm]) for nm in O.CP_NAMES)
    rh = max(rel(m.head.weight.grad, gref["head.weight"]), rel(m.head.bias.grad, gref["head.bias"]))
    print(f"window {k} x {MICRO} [{precision}]: losses {losses} vs {want}; worst CP-gradient rel-L2 {worst:.2e}, head {rh:.2e}")
    assert worst < grad_bar(precision) and rh < grad_bar(precision)


# ---- window behaviour --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_nothing_moves_before_the_last_micro_step_and_then_one_adamw_step(precision, monkeypatch):
    from cara_amd import dist as cdist
    from cara_amd.optim import AdamW
    k, n = 3, 3 * MICRO
    assert not (torch.distributed.is_available() and torch.distributed.is_initialized())
    calls = []
    real = cdist.allreduce_sum_
    monkeypatch.setattr(cdist, "allreduce_sum_", lambda flat, group=None: (calls.append(flat.numel()), real(flat, group))[1])
    # the accumulated buffer of the window, from a model that never steps
    probe = _model(precision)
    for i in range(k):
        _run(probe._cara_engine, n, i, k)
    assert len(calls) == 1
    summed = {nm: p.grad.detach().clone() for nm, p in probe.named_parameters() if p.grad is not None}
    start = _trainable(probe)
    # the same window with AdamW: parameters stay as they are until the last micro-step ...
    m, clone = _model(precision), _model(precision)
    eng = m._cara_engine
    opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    copt = AdamW(clone._cara_engine.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    for i in range(k):
        if i == k - 1:
            assert len(calls) == 1 and len(opt.state) == 0
        _run(eng, n, i, k, opt)
        now = _trainable(m)
        assert all(torch.equal(now[nm], start[nm]) for nm in start) == (i < k - 1), i
    assert len(calls) == 2 and calls[0] == calls[1] == eng._flat_grad.numel()
    # ... and are then those of a clone stepped once on the accumulated buffer
    for nm, p in clone.named_parameters():
        if nm in summed:
            p.grad = summed[nm].clone()
    copt.step()
    a, b = _trainable(m), _trainable(clone)
    assert len(a) == 14 and all(torch.equal(a[nm], b[nm]) for nm in a)
    for p, q in zip(eng.trainable_parameters(), clone._cara_engine.trainable_parameters()):
        assert torch.equal(opt.state[p]["exp_avg"], copt.state[q]["exp_avg"]) and torch.equal(opt.state[p]["exp_avg_sq"], copt.state[q]["exp_avg_sq"])
        assert float(opt.state[p]["step"]) == 1.0
    # a second window: the moments too stay bitwise as they are before its last micro-step
    mom = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in eng.trainable_parameters()]
    for i in range(k):
        _run(eng, n, i, k, opt)
        same = all(torch.equal(opt.state[p]["exp_avg"], mv[0]) and torch.equal(opt.state[p]["exp_avg_sq"], mv[1])
                   for p, mv in zip(eng.trainable_parameters(), mom))
        now = _trainable(m)
        assert same == (i < k - 1) and all(torch.equal(now[nm], a[nm]) for nm in a) == (i < k - 1), i
    assert len(calls) == 3 and eng.skipped_steps == 0


def test_windows_come_in_order_with_one_batch_size():
    from cara_amd._lib import CaraError
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    m = _model()
    eng = m._cara_engine
    x0, y0, d0 = _micro(4, 0)
    x1, y1, d1 = _micro(4, 1)
    x4, y4, d4 = (t.to(DEV) for t in _batch(4))
    with pytest.raises(CaraError):
        eng.train_step(x1, y1, None, droppath=d1, accumulate=(1, 2))   # a window starts at 0
    eng.train_step(x0, y0, None, droppath=d0, accumulate=(0, 2))
    with pytest.raises(CaraError):
        eng.train_step(x0, y0, None, droppath=d0, accumulate=(0, 2))   # ... and goes on with 1
    eng.train_step(x0, y0, None, droppath=d0, accumulate=(0, 2))        # (a refused call closed the window)
    with pytest.raises(CaraError):
        eng.train_step(x4, y4, None, droppath=d4, accumulate=(1, 2))   # another batch size
    eng.train_step(x0, y0, None, droppath=d0, accumulate=(0, 3))
    with pytest.raises(CaraError):
        eng.train_step(x1, y1, None, droppath=d1, accumulate=(1, 2))   # another window length
    eng.train_step(x0, y0, None, droppath=d0, accumulate=(0, 2))
    with pytest.raises(CaraError):
        eng.train_step(x1, y1, None, droppath=d1)                      # a plain step inside a window
    for bad in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(CaraError):
            eng.train_step(x0, y0, None, droppath=d0, accumulate=bad)
    with pytest.raises(CaraError):
        eng.train_step(x0, y0, None, droppath=d0, clip_grad=0.0)
    # after all that a whole window and a plain step still run, and the window is the one a fresh model computes
    for i, (x, y, d) in enumerate(((x0, y0, d0), (x1, y1, d1))):
        eng.train_step(x, y, None, droppath=d, accumulate=(i, 2))
    fresh = _model()
    for i, (x, y, d) in enumerate(((x0, y0, d0), (x1, y1, d1))):
        fresh._cara_engine.train_step(x, y, None, droppath=d, accumulate=(i, 2))
    assert _same(eng._flat_grad, fresh._cara_engine._flat_grad)
    eng.train_step(x4, y4, None, droppath=d4)
    # under a graph a window is refused before anything is captured
    opt = AdamW(eng.trainable_parameters(), lr=1e-3, capturable=True)
    gstep = GraphedTrainStep(eng, opt)
    with pytest.raises(CaraError):
        gstep(x0, y0, accumulate=(0, 2))
    assert not gstep._graphs


# ---- fp16: one loss-scale decision per window --------------------------------------------------------------------------------
def test_fp16_overflow_in_a_window_skips_it_once():
    """the loss scale planted at 2^30, as tests/test_model_gpu.py::test_fp16_overflow_skips_the_step_and_backs_the_scale_off does:
    both micro-steps overflow, the summed found-inf word skips the window's ONE optimiser step, the clip leaves the gradients
    alone, and the scale halves once"""
    from cara_amd.optim import AdamW
    k, n = 2, 2 * MICRO
    m = _model("fp16")
    eng = m._cara_engine
    opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)

    def window():
        return [_run(eng, n, i, k, opt, clip_grad=1.0).clone() for i in range(k)]
    window()                                                            # a clean window at the default scale
    assert eng.skipped_steps == 0 and eng.loss_scale == eng.FP16_LOSS_SCALE and float(eng.grad_norm[1]) <= 1.0
    eng._amp(torch.device(DEV, torch.cuda.current_device()))[0] = 2.0 ** 30
    before = _trainable(m)
    mom = [opt.state[p]["exp_avg"].clone() for p in eng.trainable_parameters()]
    losses = window()
    assert all(torch.isfinite(l) for l in losses)                       # the loss itself is unscaled
    assert eng.skipped_steps == 1 and eng.loss_scale == 2.0 ** 29       # once, not twice
    assert float(eng._flat_grad[-1]) != 0.0 and float(eng.grad_norm[1]) == 1.0
    now = _trainable(m)
    assert all(torch.equal(now[nm], before[nm]) for nm in before)
    assert all(torch.equal(opt.state[p]["exp_avg"], mv) for p, mv in zip(eng.trainable_parameters(), mom))
    # the scale halves once per window until the pass is finite; later windows train
    for _ in range(24):
        window()
    assert eng.loss_scale < 2.0 ** 20 and eng.skipped_steps < 25
    skipped = eng.skipped_steps
    first = window()
    for _ in range(10):
        last = window()
    assert eng.skipped_steps == skipped
    now = _trainable(m)
    assert all(torch.isfinite(now[nm]).all() for nm in now) and any(not torch.equal(now[nm], before[nm]) for nm in now)
    print(f"fp16 window: scale {eng.loss_scale}, skipped {skipped}; losses {[float(l) for l in first]} -> {[float(l) for l in last]}")
    assert all(torch.isfinite(l) for l in first + last) and sum(float(l) for l in last) < sum(float(l) for l in first)


# ---- recipe ------------------------------------------------------------------------------------------------------------------
def test_fit_takes_one_optimiser_step_per_complete_window():
    from cara_amd._lib import CaraError
    from cara_amd.recipe import fit
    from tests import test_augmented_feed_gpu as A
    # the batches feed: 5 batches of 2 -> 2 windows, the fifth batch is dropped
    x, y, _ = _batch(4)
    batches = [(x[:2].to(DEV), y[:2].to(DEV)), (x[2:].to(DEV), y[2:].to(DEV))] * 2 + [(x[:2].to(DEV), y[:2].to(DEV))]
    m = _model(drop_path_rate=0.0)
    start = _trainable(m)
    _, opt = fit(m, lambda epoch: batches, None, epochs=1, lr=1e-3, accum_steps=2, clip_grad=1.0)
    eng = m._cara_engine
    steps = {float(opt.state[p]["step"]) for p in eng.trainable_parameters()}
    assert steps == {float(len(batches) // 2)} and eng.grad_norm is not None and float(eng.grad_norm[0]) > 0
    assert eng.__dict__.get("_win") is None
    now = _trainable(m)
    assert all(torch.isfinite(now[nm]).all() for nm in now) and any(not torch.equal(now[nm], start[nm]) for nm in now)
    # the resident feed: 3 index vectors per epoch -> 1 window
    split = A._split()
    r = A._model("bf16")
    feed = split.train_rows(A.BATCH, seed=5, rank=0, world=1)
    assert len(list(feed(0))) == 3
    _, ropt = fit(r, (split, feed), None, epochs=1, lr=1e-3, seed=5, feed="resident", accum_steps=2, clip_grad=1.0)
    reng = r._cara_engine
    assert {float(ropt.state[p]["step"]) for p in reng.trainable_parameters()} == {1.0} and reng.resident_bad_rows() == 0
    with pytest.raises(CaraError):
        fit(r, (split, feed), None, epochs=1, feed="resident", accum_steps=2, graph=True)
