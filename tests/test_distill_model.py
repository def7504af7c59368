"""Host side of the distillation loss (no GPU).  The float64 restatement of tests/distill_model.py IS the formula of the issue --
(1 - a) cross_entropy(z, q) + a T^2 kl_div(log_softmax(z / T), softmax(t / T), "batchmean"), DeiT's hard variant the cross-entropy on
q' -- in value and autograd gradient; its bound holds an fp32 restatement of the kernel on the GPU test's inputs and none of seven
slips; the library exports the entry and refuses what the header says it refuses without a launch; cara_amd.loss.Distill refuses the
same values."""
import ctypes as C
import math
import os

import pytest
import torch

from oracle import small_kernels as K
from tests import distill_model as M

NAMES = ("terms", "loss", "dlogits")


# ---- the restatement is the definition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", range(len(M.VARIANTS)))
def test_restatement_is_torchs_formula_and_its_autograd_gradient(v):
    for B, Cn in ((3, 65), (5, 2), (65, 100)):
        z, t, y, mix, kw = M.variant_args(B, Cn, v)
        got = M.distill_loss(z, t, y, mix, **kw)
        loss, g = M.torch_distill(z.double(), t.double(), got["q"], kw["alpha"], kw["temperature"], kw["hard"])
        assert torch.allclose(got["loss"][0], loss, rtol=1e-12, atol=1e-13), (B, Cn, M.VARIANTS[v])
        # (dlogits carries dscale and the loss scale; float64 on both sides, torch differentiating through softmax: 2^-53 steps of
        # values <= T + 1)
        assert torch.allclose(got["dlogits"][0], g * (kw["dscale"] * kw["loss_scale"]), rtol=1e-11, atol=1e-12), (B, Cn, M.VARIANTS[v])


def test_hard_mode_is_the_cross_entropy_on_the_blended_target():
    import torch.nn.functional as F
    B, Cn = 65, 100
    z, t, y, mix = M.kd_case(B, Cn, False)
    for alpha in (0.5, 1.0):
        got = M.distill_loss(z, t, y, mix, 0.1, alpha, hard=True)
        yt = got["yt"]
        # the lowest index of the row's maximum: the planted pairs are ties
        for b in range(B):
            assert int(yt[b]) == min(i for i in range(Cn) if float(t[b, i]) == float(t[b].max()))
        assert sum(int((t[b] == t[b].max()).sum()) > 1 for b in range(B)) >= B // 3
        qd = (1 - alpha) * got["q"] + alpha * F.one_hot(yt, Cn).double()
        x = z.double().requires_grad_(True)
        loss = F.cross_entropy(x, qd)
        (g,) = torch.autograd.grad(loss, x)
        assert torch.allclose(got["loss"][0], loss.detach(), rtol=1e-12) and torch.allclose(got["dlogits"][0], g, rtol=1e-11, atol=1e-15)
        # ... and temperature is not read
        other = M.distill_loss(z, t, y, mix, 0.1, alpha, temperature=7.0, hard=True)
        assert torch.equal(other["dlogits"][0], got["dlogits"][0]) and torch.equal(other["dlogits"][1], got["dlogits"][1])


# ---- the bound ---------------------------------------------------------------------------------------------------------------------
SLIP_ON = {   # slip -> the variants (indices into M.VARIANTS) whose mode it touches: T != 1, alpha != 0.5, hard
    "no_T2_in_loss": (0, 5, 7, 10), "no_T_in_grad": (0, 5, 7, 10), "kl_reversed": (0, 3, 9, 11), "teacher_at_T1": (1, 4, 6, 11),
    "alpha_on_wrong_term": (6, 9, 11, 14), "yt_from_student": (12, 13, 14, 15), "divisor_BC": (0, 3, 12, 15),
}


def _held(got, model):
    return all(bool(K.hold_f32(g, *model[name])[0].all()) for name, g in zip(NAMES, got))


@pytest.mark.parametrize("Cn", M.KD_C)
def test_bound_holds_the_fp32_restatement_on_the_gpu_tests_inputs_and_not_a_slip(Cn):
    worst = dict.fromkeys(NAMES, 0.0)
    for B in M.KD_B:
        for v in range(len(M.VARIANTS)):
            z, t, y, mix, kw = M.variant_args(B, Cn, v)
            model = M.variant_model(B, Cn, v)
            got = M.distill_loss_f32(z, t, y, mix, **kw)
            for name, g in zip(NAMES, got):
                assert bool(torch.isfinite(model[name][1]).all() if torch.is_tensor(model[name][1]) else math.isfinite(model[name][1]))
                ok, ratio = K.hold_f32(g, *model[name])
                assert ok.all(), (name, B, Cn, M.VARIANTS[v], ratio)
                worst[name] = max(worst[name], ratio)
    print(f"C {Cn}: the fp32 restatement uses at most {worst} of the bound")
    if Cn >= 2:
        assert min(worst.values()) > 1e-3          # not vacuous: a restatement in fp32 does use the bound
    if Cn < 63:
        return
    # ... and not wrong: each slip lands outside it, on these same inputs
    for slip, on in SLIP_ON.items():
        for B in (64, 65):
            for v in on:
                z, t, y, mix, kw = M.variant_args(B, Cn, v)
                assert not _held(M.distill_loss_f32(z, t, y, mix, slip=slip, **kw), M.variant_model(B, Cn, v)), (slip, B, Cn, M.VARIANTS[v])


def test_the_inputs_are_the_issues():
    assert M.KD_B == (1, 3, 64, 65) and M.KD_C == (1, 2, 63, 64, 65, 100, 397, 1000)
    modes = M.VARIANTS
    assert {(m[0], m[1]) for m in modes if not m[2]} == {(a, T) for a in (0.5, 1.0) for T in (0.5, 1.0, 4.0)}
    assert {m[0] for m in modes if m[2]} == {0.5, 1.0}
    for col in (3, 4, 5):                          # the table with eps = 0.1, peaked logits, the scales: on and off in every mode
        for mode in {(m[0], m[1], m[2]) for m in modes}:
            assert {m[col] for m in modes if (m[0], m[1], m[2]) == mode} == {False, True}
    assert M.SCALED == (0.5, 1024.0)
    z, t, y, mix = M.kd_case(65, 100, True)
    assert float(z.abs().max()) == 30.0 and float(t.abs().max()) <= 30.0 and bool((z.gather(1, y[:, None]) == 30.0).all())
    assert bool((mix[:, 0] != torch.arange(65)).all()) and set(mix[:, 6].contiguous().view(torch.float32).tolist()) == {float(torch.tensor(0.3))}
    zf, _, _, _ = M.kd_case(65, 100, False)
    assert float(zf.abs().max()) < 6.0


# ---- the library and the value object, without a GPU -------------------------------------------------------------------------------
def test_the_entry_is_declared_in_the_header_and_bound_in_the_loader():
    from cara_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "cara_hip.h")) as fh:
        header = fh.read()
    assert "int cara_distill_loss(const float* logits, const float* teacher, const int64_t* labels, const int* mix, float smoothing," in header
    assert "cara_distill_loss" in _lib.SYMBOLS


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_library_exports_the_entry_and_refuses_bad_arguments_without_a_launch(operands):
    from cara_amd import _lib
    lib = _lib.lib(operands)
    assert hasattr(lib, "cara_distill_loss")
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert lib.cara_distill_loss.argtypes == [P, P, P, P, F, F, F, I, P, P, I, I, F, P, P, P]
    assert lib.cara_abi_version() == 14
    # host memory stands in for the device buffers: a refused call reads and launches nothing
    buf = (C.c_float * 64)()
    pbuf, nan, inf = C.cast(buf, C.c_void_p), float("nan"), float("inf")

    def call(logits=pbuf, teacher=pbuf, labels=pbuf, eps=0.1, alpha=0.5, T=1.0, hard=0, loss=pbuf, B=2, Cn=3, dscale=1.0):
        f = C.c_float
        return lib.cara_distill_loss(logits, teacher, labels, None, f(eps), f(alpha), f(T), hard, loss, pbuf, B, Cn, f(dscale), None, None, None)
    for kw in ({"alpha": -0.1}, {"alpha": 1.5}, {"alpha": nan}, {"alpha": inf}, {"T": 0.0}, {"T": -1.0}, {"T": inf}, {"T": nan}, {"T": 1e-39}, {"T": 2.9e-39}, {"hard": 2},
               {"hard": -1}, {"teacher": None}, {"teacher": None, "hard": 1}, {"teacher": None, "alpha": 1.0}, {"eps": 1.0}, {"eps": -0.1},
               {"eps": nan}, {"logits": None}, {"labels": None}, {"loss": None}, {"B": 0}, {"B": -3}, {"Cn": 0}, {"dscale": 0.0}, {"dscale": nan},
               # what cara_cross_entropy_mix refuses is refused at alpha == 0 as well, where the call is its
               {"alpha": 0.0, "eps": 1.0}, {"alpha": 0.0, "logits": None}, {"alpha": 0.0, "B": 0}, {"alpha": 0.0, "hard": 2}):
        assert call(**kw) == 1, kw
    assert all(v == 0.0 for v in buf)


def test_distill_objects_refuse_what_the_entry_refuses():
    from cara_amd._lib import CaraError
    from cara_amd.ema import ParamEma
    from cara_amd.loss import BCE, Distill, check_distill
    nan, inf = float("nan"), float("inf")
    t = torch.zeros(4, 3)
    d = Distill(t)
    assert d.c_args() == (0.5, 1.0, 0) and d.kind() == "tensor" and d.teacher is t
    assert Distill(t, 1, 4, True).c_args() == (1.0, 4.0, 1) and Distill(t, alpha=0).alpha == 0.0
    assert Distill("ema", 0.3, 2.0).kind() == "fit"
    assert Distill(object.__new__(ParamEma)).kind() == "ema"     # (an average lives on the GPU: only its type is looked at here)
    for bad in (-0.1, 1.5, nan, inf, "0.5", True, None):
        with pytest.raises(CaraError, match="alpha"):
            Distill(t, alpha=bad)
    for bad in (0.0, -1.0, inf, nan, "1", False, None, 1e-39, 1e-46, 1e39):    # (the last three: 1 / T or T itself is infinite in fp32)
        with pytest.raises(CaraError, match="temperature"):
            Distill(t, temperature=bad)
    assert Distill(t, temperature=3e-39).temperature == 3e-39 and Distill(t, temperature=3e38).c_args()[1] == 3e38
    Distill(t, temperature=0.0, hard=True)                       # hard mode does not read it (a number all the same)
    for bad in (2, -1, None, "yes", 0.5):
        with pytest.raises(CaraError, match="hard"):
            Distill(t, hard=bad)
    for bad in (None, "teacher", [[0.0]], torch.nn.Linear(3, 3), 1.0):
        with pytest.raises(CaraError, match="teacher"):
            Distill(bad)
    # distill= beside the other losses, and something that is no Distill
    v = torch.ones(3)
    assert check_distill(None, BCE(), v, v) is None and check_distill(d) is d
    for kw in ({"loss": BCE()}, {"class_weight": v}, {"logit_bias": v}):
        with pytest.raises(CaraError, match="beside"):
            check_distill(d, **kw)
    for bad in ("ema", 0.5, Distill, t):
        with pytest.raises(CaraError, match="distill must be"):
            check_distill(bad)


def test_engine_and_recipe_take_distill_and_refuse_it_before_they_touch_a_device():
    from cara_amd._lib import CaraError
    from cara_amd.engine import CaraEngine
    from cara_amd.loss import BCE, Distill
    from cara_amd.recipe import GraphedTrainStep, fit
    import inspect
    for fn in (CaraEngine.train_step, CaraEngine.train_step_resident, CaraEngine._step, GraphedTrainStep.__init__, fit):
        assert inspect.signature(fn).parameters["distill"].default is None
    assert CaraEngine.teacher_logits is None
    d, v = Distill(torch.zeros(4, 3)), torch.ones(3)
    for kw in ({"loss": BCE()}, {"class_weight": v}, {"logit_bias": v}):
        with pytest.raises(CaraError, match="beside"):
            fit(None, None, distill=d, **kw)
    with pytest.raises(CaraError, match="distill must be"):
        fit(None, None, distill="ema")
    with pytest.raises(CaraError, match="ema_decay"):
        fit(None, None, distill=Distill("ema"))
