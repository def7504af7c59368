"""Host side of the class-weighted, logit-adjusted loss: the float64 restatement of tests/balanced_loss_model.py against torch's
cross_entropy(logits + bias, q, weight=w, reduction="sum") / B and its autograd gradient, that the derived bound is neither vacuous
nor wrong (an fp32 emulation in the kernel's summation order on the GPU test's inputs; slips outside), and the presets of
cara_amd/data.py (class_counts, balanced_class_weight, logit_prior).  CPU only."""
import math

import pytest
import torch
import torch.nn.functional as F

from cara_amd.data import ResidentSplit, balanced_class_weight, class_counts, logit_prior, soft_target
from oracle import small_kernels as K
from tests import balanced_loss_model as M
from tests import mix_model as X


# ---- the definition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_w,use_b", [(True, False), (False, True), (True, True)])
def test_restatement_with_an_index_target_is_torchs_weighted_cross_entropy(use_w, use_b):
    B, Cn = 9, 23
    l, y, _ = M.bal_case(B, Cn, None)
    cw, cb = M.presets(Cn)
    cw, cb = (cw if use_w else None), (cb if use_b else None)
    model = M.xent_bal(l, y, None, 0.0, cw, cb)
    w64 = None if cw is None else cw.double()
    z = l.double() if cb is None else l.double() + cb.double()
    want = F.cross_entropy(z, y, weight=w64, reduction="sum") / B            # torch's index-target form
    assert abs(float(model["loss"][0] - want)) <= 1e-12 * max(1.0, abs(float(want)))
    loss, grad = M.torch_loss(l.double(), F.one_hot(y, Cn).double(), w64, None if cb is None else cb.double())
    assert abs(float(loss - want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert float((model["dlogits"][0] - grad).abs().max()) <= 1e-13
    per = F.cross_entropy(z, y, weight=w64, reduction="none") / B
    assert float((model["terms"][0] - per).abs().max()) <= 1e-12


@pytest.mark.parametrize("use_w,use_b", [(True, False), (False, True), (True, True)])
def test_restatement_with_a_mixed_smoothed_target_is_torchs_probability_target_form(use_w, use_b):
    B, Cn = 9, 23
    l, y, mix = M.bal_case(B, Cn, 0.3)
    cw, cb = M.presets(Cn)
    cw, cb = (cw if use_w else None), (cb if use_b else None)
    eps = float(torch.tensor(0.1, dtype=torch.float32))
    for scale in ((1.0, 1.0), (0.25, 512.0)):
        model = M.xent_bal(l, y, mix, 0.1, cw, cb, *scale)
        q = soft_target(y, mix, Cn, eps)
        assert float((model["q"] - q).abs().max()) <= 1e-15
        loss, grad = M.torch_loss(l.double(), q, None if cw is None else cw.double(), None if cb is None else cb.double())
        assert abs(float(model["loss"][0] - loss)) <= 1e-12 * max(1.0, abs(float(loss)))
        assert float((model["dlogits"][0] - grad * scale[0] * scale[1]).abs().max()) <= 1e-13 * scale[0] * scale[1]
        assert abs(float(model["terms"][0].sum() - loss)) <= 1e-12 * max(1.0, abs(float(loss)))


def test_restatement_without_weight_and_bias_is_the_mixed_loss_model():
    for B, Cn in ((1, 1), (5, 2), (65, 100)):
        l, y, mix = M.bal_case(B, Cn, 0.3)
        a, b = M.xent_bal(l, y, mix, 0.1, None, None, 0.25, 512.0), X.xent_mix(l, y, mix, 0.1, 0.25, 512.0)
        for name in ("terms", "loss", "dlogits"):
            assert torch.allclose(a[name][0], b[name][0], rtol=1e-13, atol=1e-15), name


# ---- the bound -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", M.BAL_C)
@pytest.mark.parametrize("B", M.BAL_B)
def test_bound_holds_the_fp32_emulation_on_the_gpu_tests_inputs_and_not_a_slip(B, Cn):
    cw, cb = M.presets(Cn)
    worst = 0.0
    for use_w, use_b, t, eps, scale in M.variants():
        l, y, mix = M.bal_case(B, Cn, t)
        w_, b_ = (cw if use_w else None), (cb if use_b else None)
        model = M.xent_bal(l, y, mix, eps, w_, b_, *scale)
        term, loss, dl = M.xent_bal_f32(l, y, mix, eps, w_, b_, *scale)
        for name, got in (("terms", term), ("loss", loss), ("dlogits", dl)):
            ok, ratio = K.hold_f32(got, *model[name])
            assert ok.all(), (name, use_w, use_b, t, eps, scale, ratio)
            worst = max(worst, ratio)
    print(f"B {B} C {Cn}: the fp32 emulation uses at most {worst:.3f} of the bound")
    assert worst > 1e-3                   # not vacuous: an emulation in fp32 does use the bound
    if Cn < 63:
        return
    # ... and not wrong: what a slip gives is outside it.  torch's "mean" divisor (the weight mass of the batch's targets) for B; the
    # bias forgotten; the weight left out of the gradient's target term
    l, y, mix = M.bal_case(B, Cn, 0.3)
    model = M.xent_bal(l, y, mix, 0.1, cw, cb)
    mass = float((model["q"] * cw.double()).sum())
    assert abs(mass / B - 1.0) > 1e-3
    by_mass = M.xent_bal_f32(l, y, mix, 0.1, cw, cb, dscale=B / mass)[2]
    assert not K.hold_f32(by_mass, *model["dlogits"])[0].all()
    no_bias = M.xent_bal_f32(l, y, mix, 0.1, cw, None)
    assert not K.hold_f32(no_bias[0], *model["terms"])[0].all() and not K.hold_f32(no_bias[2], *model["dlogits"])[0].all()
    unweighted_target = M.xent_bal_f32(l, y, mix, 0.1, cw, cb)[2] + (((cw.double() - 1.0) * model["q"]) / B).float()
    assert not K.hold_f32(unweighted_target, *model["dlogits"])[0].all()


def test_the_gpu_tests_presets_are_the_issues():
    """weights of a long-tailed 1 000-image count vector, about 0.05 to 20, with absent classes where the head is wide"""
    for Cn in M.BAL_C:
        n = M.long_tail_counts(Cn)
        assert int(n.sum()) == 1000 and bool((n[:-1] >= n[1:]).all())
        cw, cb = M.presets(Cn)
        assert cw.dtype == cb.dtype == torch.float32 and tuple(cw.shape) == tuple(cb.shape) == (Cn,)
        assert torch.isfinite(cw).all() and torch.isfinite(cb).all() and bool((cw > 0).all()) and bool((cb <= 0).all())
    n = M.long_tail_counts(100)
    cw, _ = M.presets(100)
    assert int(n.min()) == 0 and int(n.max()) > 300
    assert 0.02 < float(cw.min()) < 0.1 and 10.0 < float(cw.max()) < 40.0, (float(cw.min()), float(cw.max()))


# ---- the presets -----------------------------------------------------------------------------------------------------------
LONG_TAIL = [412, 0, 201, 97, 1, 44, 2, 0, 19, 1, 9, 5, 3, 0, 2, 1, 1, 0, 1, 1]


def test_class_counts_reads_a_split_or_labels():
    y = torch.tensor([3, 0, 3, 3, 5, 0])
    want = torch.tensor([2, 0, 0, 3, 0, 1, 0])
    got = class_counts(y, 7)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    split = ResidentSplit.from_tensors(torch.zeros(6, 3, 8, 8, dtype=torch.uint8), y)
    assert torch.equal(class_counts(split, 7), want)
    assert torch.equal(class_counts(torch.zeros(0, dtype=torch.int64), 3), torch.zeros(3, dtype=torch.int64))
    for bad_y, classes in ((y, 5), (torch.tensor([0, -1]), 4), (y, 0), (y, 2.0)):
        with pytest.raises(ValueError, match="class_counts"):
            class_counts(bad_y, classes)


@pytest.mark.parametrize("power", [1.0, 0.5, 0.0, 2])
def test_balanced_class_weight_meets_its_normalisation(power):
    n = torch.tensor(LONG_TAIL)
    N = float(n.sum())
    w64 = balanced_class_weight(n, power, dtype=torch.float64)
    # in float64: sum_c n_c w_c == sum_c n_c to the roundings of 20 products, their sum and the scale (a few 2^-53 of N)
    assert w64.dtype == torch.float64 and abs(float((n.double() * w64).sum()) - N) <= 64 * 2.0 ** -53 * N
    w = balanced_class_weight(n, power)
    assert w.dtype == torch.float32 and tuple(w.shape) == (len(LONG_TAIL),) and torch.equal(w, w64.float())
    # the fp32 weights: each is one rounding of its float64 value, |sum_c n_c (w_c - w64_c)| <= 2^-24 sum_c n_c w64_c = 2^-24 N
    assert abs(float((n.double() * w.double()).sum()) - N) <= 2.0 ** -24 * N + 64 * 2.0 ** -53 * N
    # proportional to max(n_c, 1) ** -power: an absent class weighs what a class of one image weighs
    raw = n.double().clamp_min(1.0) ** -float(power)
    assert float((w64 / w64[0] - raw / raw[0]).abs().max()) <= 1e-12 * float((raw / raw[0]).max())
    assert w64[1] == w64[4] and bool((w64 > 0).all())
    if power == 0.0:
        assert torch.equal(w, torch.ones(len(LONG_TAIL)))
    assert torch.equal(balanced_class_weight(LONG_TAIL, power), w)                       # (a list of counts is taken too)


def test_logit_prior_is_finite_for_an_absent_class():
    n = torch.tensor(LONG_TAIL)
    N, Cn = int(n.sum()), len(LONG_TAIL)
    a = logit_prior(n)
    assert a.dtype == torch.float32 and tuple(a.shape) == (Cn,) and torch.isfinite(a).all() and bool((a < 0).all())
    assert abs(float(a[1]) - math.log(1.0 / (N + Cn))) <= 1e-6 and abs(float(a[0]) - math.log(413.0 / (N + Cn))) <= 1e-6
    assert abs(float(torch.exp(a.double()).sum()) - 1.0) <= 1e-6                        # the smoothed prior sums to one
    assert torch.allclose(logit_prior(n, tau=0.5), 0.5 * a, rtol=1e-6, atol=0) and not logit_prior(n, tau=0.0).any()


def test_presets_refuse_negative_counts_and_an_empty_total():
    for fn in (balanced_class_weight, logit_prior):
        for bad in ([3, -1, 4], [0, 0, 0], [], [1.0, float("nan")], [float("inf"), 1.0]):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(torch.tensor(bad, dtype=torch.float64))
    for power in (-0.5, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="power"):
            balanced_class_weight([3, 1], power)
    for tau in (float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="tau"):
            logit_prior([3, 1], tau)
