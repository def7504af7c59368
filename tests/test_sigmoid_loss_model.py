"""Host side of the sigmoid losses (no GPU).  The float64 restatement of tests/sigmoid_loss_model.py IS torch's
binary_cross_entropy_with_logits (value and autograd gradient) and, for the focal loss, the formula as written under autograd; its
bound holds an fp32 restatement of the kernel on the GPU test's inputs and none of six slips; the library exports the entry and
refuses what the header says it refuses without a launch; cara_amd.loss refuses the same values."""
import ctypes as C
import math

import pytest
import torch

from oracle import small_kernels as K
from tests import sigmoid_loss_model as M


# ---- the restatement is the definition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_pw", [False, True])
@pytest.mark.parametrize("sum_classes", [False, True])
def test_restatement_is_torchs_bce_with_logits(use_pw, sum_classes):
    for B, Cn in ((3, 65), (5, 2), (1, 1)):
        l, y, mix = M.sig_case(B, Cn)
        pw = M.pos_weight(Cn) if use_pw else None
        for eps, table, thr in ((0.0, False, None), (0.1, True, None), (0.1, True, M.THR)):
            got = M.sigmoid_loss(l, y, mix if table else None, eps, thr=thr, pw=pw, sum_classes=sum_classes)
            q = got["q"] if thr is None else (got["q"] > M.THR).double()
            loss, g = M.torch_bce(l.double(), q, None if pw is None else pw.double(), sum_classes)
            assert torch.allclose(got["loss"][0], loss, rtol=1e-12, atol=1e-300)
            # (float64 on both sides, but torch forms sigmoid(z) - q, which cancels at a saturated logit: 2^-53 of a weight <= 4 there;
            # the restatement's (1 - q) s+ - q s- keeps its digits)
            assert torch.allclose(got["dlogits"][0], g, rtol=1e-12, atol=2e-15 / (B * (1 if sum_classes else Cn))), (B, Cn, eps, thr)


@pytest.mark.parametrize("fgamma,alpha", [(2.0, 0.25), (1.0, None), (0.0, 0.25), (1.5, 0.25), (2.0, None), (3.0, 0.75)])
def test_focal_restatements_analytic_gradient_is_autograd_of_the_written_formula(fgamma, alpha):
    for B, Cn in ((3, 65), (5, 2)):
        l, y, mix = M.sig_case(B, Cn)
        for eps, table, thr, sumc in ((0.0, False, None, True), (0.1, True, None, False), (0.1, True, M.THR, True)):
            got = M.sigmoid_loss(l, y, mix if table else None, eps, thr=thr, fgamma=fgamma, alpha=alpha, sum_classes=sumc)
            q = got["q"] if thr is None else (got["q"] > M.THR).double()
            loss, g = M.written_focal(l.double(), q, fgamma, alpha, sumc)
            assert torch.allclose(got["loss"][0], loss, rtol=1e-12, atol=1e-300)
            # (autograd differentiates sigmoid and the written m: absolute 2^-53 steps of values <= gamma + 1, as above)
            assert torch.allclose(got["dlogits"][0], g, rtol=1e-11, atol=4e-15 / (B * (1 if sumc else Cn))), (B, Cn, eps, thr, (got["dlogits"][0] - g).abs().max())


def test_focal_with_hard_targets_is_torchvisions_formula():
    """sigmoid_focal_loss of torchvision, restated from its documentation: p_t = p y + (1 - p)(1 - y), ce (1 - p_t)^gamma, alpha_t"""
    import torch.nn.functional as F
    B, Cn = 5, 65
    l, y, _ = M.sig_case(B, Cn)
    got = M.sigmoid_loss(l, y, None, 0.0, fgamma=2.0, alpha=0.25, sum_classes=True)
    x, t = l.double(), F.one_hot(y, Cn).double()
    p = torch.sigmoid(x)
    pt = p * t + (1 - p) * (1 - t)
    want = ((0.25 * t + 0.75 * (1 - t)) * F.binary_cross_entropy_with_logits(x, t, reduction="none") * (1 - pt) ** 2).sum() / B
    assert torch.allclose(got["loss"][0], want, rtol=1e-12)


# ---- the bound -------------------------------------------------------------------------------------------------------------------
SLIP_ON = {   # slip -> the variants (indices into M.VARIANTS) whose mode it touches
    "naive_softplus": (0, 6), "divisor_B": (0, 7), "pos_weight_on_negative": (1, 3), "no_1_minus_2q": (6, 8),
    "m_as_p_plus_q_minus_2pq": (6, 8), "threshold_before_smoothing": (2, 11),
}


def _held(got, model):
    return all(bool(K.hold_f32(g, *model[name])[0].all()) for name, g in zip(("terms", "loss", "dlogits"), got))


@pytest.mark.parametrize("Cn", M.SIG_C)
def test_bound_holds_the_fp32_restatement_on_the_gpu_tests_inputs_and_not_a_slip(Cn):
    worst = {"terms": 0.0, "loss": 0.0, "dlogits": 0.0}
    for B in M.SIG_B:
        for v in range(len(M.VARIANTS)):
            l, y, mix, kw = M.variant_args(B, Cn, v)
            model = M.variant_model(B, Cn, v)
            got = M.sigmoid_loss_f32(l, y, mix, **kw)
            for name, g in zip(("terms", "loss", "dlogits"), got):
                assert bool(torch.isfinite(model[name][1]).all() if torch.is_tensor(model[name][1]) else math.isfinite(model[name][1]))
                ok, ratio = K.hold_f32(g, *model[name])
                assert ok.all(), (name, B, Cn, M.VARIANTS[v], ratio)
                worst[name] = max(worst[name], ratio)
    print(f"C {Cn}: the fp32 restatement uses at most {worst} of the bound")
    assert min(worst.values()) > 1e-3          # not vacuous: a restatement in fp32 does use the bound
    if Cn < 63:
        return
    # ... and not wrong: each slip lands outside it, on these same inputs
    for slip, on in SLIP_ON.items():
        for B in (64, 65):                  # (batches whose labels sit on every planted value, the saturated ones included)
            for v in on:
                l, y, mix, kw = M.variant_args(B, Cn, v)
                assert not _held(M.sigmoid_loss_f32(l, y, mix, slip=slip, **kw), M.variant_model(B, Cn, v)), (slip, B, Cn, M.VARIANTS[v])


def test_the_inputs_are_the_issues():
    assert M.SIG_B == (1, 3, 64, 65) and M.SIG_C == (1, 2, 63, 64, 65, 100, 397, 1000)
    l, y, mix = M.sig_case(65, 100)
    for v in M.PLANTED:
        assert bool((l == v).any())
    assert bool((l.gather(1, y[:, None])[:, 0] == 200.0).any()) and bool((l.gather(1, y[:, None])[:, 0] == -88.8).any())
    assert not math.isfinite(float(torch.exp(torch.tensor(88.8))))                   # where a naive exp overflows in fp32
    assert float(torch.sigmoid(torch.tensor(17.0))) == 1.0                           # ... and sigma saturates
    assert int(mix[32, 0]) == 32                                                     # the self-partner
    ts = set(mix[:, 6].contiguous().view(torch.float32).tolist())
    assert ts == {0.0, float(torch.tensor(0.3)), 1.0}
    modes = M.VARIANTS
    assert {m[0] for m in modes} == {False, True} and {m[1] for m in modes} == {0.0, 0.1} and {m[2] for m in modes} == {None, 0.2}
    assert {m[3] for m in modes} == {None, "ones", "u"} and {m[4] for m in modes} >= {0.0, 1.0, 2.0} and {m[5] for m in modes} == {None, 0.25}
    assert {m[6] for m in modes} == {False, True} and {m[7][0] for m in modes} == {1.0, 0.125} and 1024.0 in {m[7][1] for m in modes}
    pw = M.pos_weight(100)
    assert 0.5 <= float(pw.min()) and float(pw.max()) <= 4.0


# ---- the library and the value objects, without a GPU ----------------------------------------------------------------------------
@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_library_exports_the_entry_and_refuses_bad_arguments_without_a_launch(operands):
    from cara_amd import _lib
    lib = _lib.lib(operands)
    assert hasattr(lib, "cara_sigmoid_loss") and "cara_sigmoid_loss" in _lib.SYMBOLS
    # host memory stands in for the device buffers: a refused call reads and launches nothing
    buf = (C.c_float * 64)()
    pbuf, nan, inf = C.cast(buf, C.c_void_p), float("nan"), float("inf")

    def call(logits=pbuf, labels=pbuf, eps=0.1, thr=-1.0, fgamma=0.0, alpha=-1.0, pw=None, sumc=0, loss=pbuf, B=2, Cn=3, dscale=1.0):
        f = C.c_float
        return lib.cara_sigmoid_loss(logits, labels, None, f(eps), f(thr), f(fgamma), f(alpha), pw, sumc, loss, pbuf, B, Cn, f(dscale),
                                     None, None, None)
    for kw in ({"eps": 1.0}, {"eps": -0.1}, {"eps": nan}, {"thr": 1.0}, {"thr": 1.5}, {"thr": nan}, {"fgamma": -1.0}, {"fgamma": 0.5},
               {"fgamma": 0.999}, {"fgamma": inf}, {"fgamma": nan}, {"alpha": 1.5}, {"alpha": nan}, {"pw": pbuf, "fgamma": 2.0},
               {"pw": pbuf, "alpha": 0.25}, {"pw": pbuf, "alpha": 0.0}, {"sumc": 2}, {"sumc": -1}, {"logits": None}, {"labels": None},
               {"loss": None}, {"B": 0}, {"B": -3}, {"Cn": 0}, {"dscale": 0.0}, {"dscale": nan}):
        assert call(**kw) == 1, kw
    assert all(v == 0.0 for v in buf)


def test_loss_objects_refuse_what_the_entry_refuses():
    from cara_amd._lib import CaraError
    from cara_amd.loss import BCE, Focal, check_loss
    nan, inf = float("nan"), float("inf")
    assert BCE().c_args() == (-1.0, 0.0, -1.0) and BCE(0.2, sum_classes=True).c_args() == (0.2, 0.0, -1.0) and BCE(0).target_threshold == 0.0
    f = Focal()
    assert f.c_args() == (-1.0, 2.0, 0.25) and f.sum_classes is True and f.pos_weight is None
    assert Focal(gamma=0, alpha=None).c_args() == BCE().c_args() and Focal(1, 0).c_args() == (-1.0, 1.0, 0.0) and Focal(3.5, 1).alpha == 1.0
    for bad in (1.0, 1.5, -0.1, nan, "0.2", True):
        with pytest.raises(CaraError, match="target_threshold"):
            BCE(target_threshold=bad)
    for bad in (-1.0, 0.5, 0.999, inf, nan, None, "2", True):
        with pytest.raises(CaraError, match="gamma"):
            Focal(gamma=bad)
    for bad in (1.5, -0.25, nan, inf, "a", False):
        with pytest.raises(CaraError, match="alpha"):
            Focal(alpha=bad)
    for bad in (2, -1, None, "yes", 0.5):
        with pytest.raises(CaraError, match="sum_classes"):
            BCE(sum_classes=bad)
        with pytest.raises(CaraError, match="sum_classes"):
            Focal(sum_classes=bad)
    with pytest.raises(CaraError, match="pos_weight"):
        BCE(pos_weight=[1.0, 2.0])
    with pytest.raises(TypeError):
        Focal(pos_weight=torch.ones(3))                     # the focal loss takes no pos_weight
    # the values of a pos_weight: shape, type, device, sign and finiteness, once per (address, version)
    seen, cpu = {}, torch.device("cpu")
    w = torch.tensor([0.5, 1.0, 4.0])
    BCE(pos_weight=w).check_pos_weight(3, cpu, seen)
    assert seen["pos_weight"] == (w.data_ptr(), w._version)
    for bad in (w[:2], w.double(), w.reshape(1, 3), torch.stack([w, w], 1)[:, 0], torch.tensor([1.0, -1e-3, 1.0]), torch.tensor([1.0, nan, 1.0]),
                torch.tensor([inf, 1.0, 1.0])):
        with pytest.raises(CaraError, match="pos_weight"):
            BCE(pos_weight=bad).check_pos_weight(3, cpu, {})
    w[1] = -2.0                                             # in place: another version, read again
    with pytest.raises(CaraError, match="pos_weight"):
        BCE(pos_weight=w).check_pos_weight(3, cpu, seen)
    # loss= beside the softmax loss's vectors, and something that is no loss
    v = torch.ones(3)
    assert check_loss(None, v, v) is None and check_loss(f) is f
    for kw in ({"class_weight": v}, {"logit_bias": v}, {"class_weight": v, "logit_bias": v}):
        with pytest.raises(CaraError, match="class_weight"):
            check_loss(BCE(), **kw)
    for bad in ("bce", 1.0, BCE, torch.nn.BCEWithLogitsLoss()):
        with pytest.raises(CaraError, match="loss must be"):
            check_loss(bad)
    # two objects with the same settings capture the same graph unless their weight vectors differ
    assert BCE(0.2).key() == BCE(0.2).key() != BCE(0.3).key() and BCE(pos_weight=v).key() != BCE(pos_weight=v.clone()).key()


def test_engine_and_recipe_refuse_a_loss_beside_class_weight_before_they_touch_a_device():
    from cara_amd._lib import CaraError
    from cara_amd.engine import CaraEngine
    from cara_amd.loss import BCE
    from cara_amd.recipe import GraphedTrainStep, fit
    import inspect
    for fn in (CaraEngine.train_step, CaraEngine.train_step_resident, CaraEngine._step, GraphedTrainStep.__init__, fit):
        assert inspect.signature(fn).parameters["loss"].default is None
    v = torch.ones(3)
    with pytest.raises(CaraError, match="class_weight"):
        fit(None, None, loss=BCE(), class_weight=v)
    with pytest.raises(CaraError, match="loss must be"):
        fit(None, None, loss="bce")
