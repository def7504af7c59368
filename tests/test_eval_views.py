"""CPU side of the multi-view evaluation (CaraEngine.evaluate(views=)): the host model ``evalcount.combine_views``, the view tables
of ``data.EvalViews``, how ``ResidentSplit.eval_view_shard`` cuts a split into whole samples per rank, the refusals that need no
GPU, and that the derived bound of tests/views_model.py holds for an fp32 evaluation in another order."""
import math

import pytest
import torch

from cara_amd import CaraError
from cara_amd import evalcount as EC
from cara_amd.data import EVAL_MAX_VIEWS, EvalViews, ResidentSplit
from tests import views_model as VM


def _logits(S, V, C, seed, sigma=3.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(S * V, C, generator=g) * sigma


# ---- combine_views ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 5, 100])
def test_one_view_prob_is_log_softmax_and_logit_is_a_copy(C):
    lg = _logits(7, 1, C, seed=C)
    assert torch.allclose(EC.combine_views(lg, 1, "prob"), torch.log_softmax(lg.double(), 1), rtol=0, atol=1e-14)
    assert torch.equal(EC.combine_views(lg, 1, "logit"), lg.double())


@pytest.mark.parametrize("V", [2, 5, 16])
def test_prob_is_permutation_invariant_sums_to_one_and_logit_is_the_mean(V):
    S, C = 6, 37
    lg = _logits(S, V, C, seed=V, sigma=8.0)
    out = EC.combine_views(lg, V, "prob")
    assert out.dtype == torch.float64 and tuple(out.shape) == (S, C)
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(1))
    shuffled = lg.view(S, V, C)[:, perm].reshape(S * V, C)
    assert torch.allclose(EC.combine_views(shuffled, V, "prob"), out, rtol=0, atol=1e-13)
    assert torch.allclose(torch.exp(out).sum(1), torch.ones(S, dtype=torch.float64), rtol=0, atol=1e-13)
    # against the literal definition
    want = torch.log(torch.softmax(lg.double().view(S, V, C), 2).mean(1))
    assert torch.allclose(out, want, rtol=0, atol=1e-12)
    assert torch.allclose(EC.combine_views(lg, V, "logit"), lg.double().view(S, V, C).mean(1), rtol=0, atol=1e-14)


def test_minus_infinity_rule_and_argument_checks():
    S, V, C = 3, 4, 9
    lg = _logits(S, V, C, seed=2)
    lg.view(S, V, C)[:, :, 2] = -float("inf")        # probability zero in every view
    lg.view(S, V, C)[:, :2, 5] = -float("inf")       # ... and in two of the four views only
    out = EC.combine_views(lg, V, "prob")
    assert bool(torch.isinf(out[:, 2]).all()) and bool((out[:, 2] < 0).all()) and not bool(torch.isnan(out).any())
    assert bool(torch.isfinite(out[:, 5]).all())
    p = torch.softmax(lg.double().view(S, V, C), 2).mean(1)
    assert torch.allclose(torch.exp(out), p, rtol=0, atol=1e-14)
    # and the rows are scored without a NaN by the counting model
    st = EC.accumulate(EC.new_state(), out, torch.tensor([0, 1, 3]))
    assert math.isfinite(float(st[EC.LOSS])) and int(st[EC.N]) == 3
    with pytest.raises(ValueError):
        EC.combine_views(lg, V, "mean")
    with pytest.raises(ValueError):
        EC.combine_views(lg, 5, "prob")              # 12 rows are no whole samples of five views


# ---- the derived bound, on the host ------------------------------------------------------------------------------------------------
def _fp32_other_order(lg, V, mode):
    """the kernel's op sequence in fp32 torch ops (torch's own summation order and libm): a second fp32 evaluation"""
    S, C = lg.shape[0] // V, lg.shape[1]
    l = lg.view(S, V, C)
    if mode == "logit":
        acc = l[:, 0].clone()
        for v in range(1, V):
            acc = acc + l[:, v]
        return acc / torch.tensor(float(V))
    m = l.max(2, keepdim=True).values
    lse = m + torch.log(torch.exp(l - m).sum(2, keepdim=True))
    a = l - lse
    M = a.max(1, keepdim=True).values
    t = torch.zeros(S, 1, C)
    for v in range(V):
        t = t + torch.exp(a[:, v:v + 1] - M)
    out = (M + torch.log(t)) - torch.log(torch.tensor(float(V)))
    return torch.where(torch.isinf(M), M, out).squeeze(1)


@pytest.mark.parametrize("mode", ["prob", "logit"])
@pytest.mark.parametrize("sigma", [0.02, 3.0, 30.0])
def test_an_fp32_evaluation_holds_the_derived_bound_and_a_slip_does_not(mode, sigma):
    worst = 0.0
    for V, C in [(1, 5), (2, 100), (5, 397), (16, 1000)]:
        lg = _logits(4, V, C, seed=V + C, sigma=sigma)
        v, d = VM.combine_bound(lg, V, mode)
        assert torch.allclose(v, EC.combine_views(lg, V, mode), rtol=0, atol=1e-11)     # the two fp64 statements agree
        ok, ratio = VM.hold(_fp32_other_order(lg, V, mode), v, d)
        assert bool(ok.all()), (V, C, ratio)
        worst = max(worst, ratio)
        if V > 1:
            # a plausible slip -- the mean divided by V - 1, or log(V) left out -- is far outside
            slip = v * V / (V - 1) if mode == "logit" else v + math.log(V)
            assert not bool(VM.hold(slip.float(), v, d)[0].all())
    print(f"{mode} sigma {sigma}: worst fp32 error / bound {worst:.3f}")


def test_bound_model_keeps_the_minus_infinity_rule():
    lg = _logits(2, 3, 7, seed=4)
    lg.view(2, 3, 7)[:, :, 1] = -float("inf")
    lg.view(2, 3, 7)[:, 0, 4] = -float("inf")
    v, d = VM.combine_bound(lg, 3, "prob")
    assert bool(torch.isinf(v[:, 1]).all()) and bool((d[:, 1] == 0).all()) and bool(torch.isfinite(v[:, 4]).all())
    assert not bool(torch.isnan(v).any()) and not bool(torch.isnan(d).any())
    ok, _ = VM.hold(_fp32_other_order(lg, 3, "prob"), v, d)
    assert bool(ok.all())
    bad = _fp32_other_order(lg, 3, "prob")
    bad[:, 1] = float("nan")
    assert not bool(VM.hold(bad, v, d)[0].all())


# ---- EvalViews ---------------------------------------------------------------------------------------------------------------------
def test_view_tables():
    assert EvalViews.center(224).table(256, 256).tolist() == [[16, 16, 224, 224, 0]]
    assert EvalViews.center(224, flip=True).table(256, 256).tolist() == [[16, 16, 224, 224, 0], [16, 16, 224, 224, 1]]
    assert EvalViews.resize(224).table(224, 224).tolist() == [[0, 0, 224, 224, 0]]
    assert EvalViews.resize(224, flip=True).table(256, 320).tolist() == [[0, 0, 320, 256, 0], [0, 0, 320, 256, 1]]
    five = [[0, 0, 224, 224, 0], [32, 0, 224, 224, 0], [0, 32, 224, 224, 0], [32, 32, 224, 224, 0], [16, 16, 224, 224, 0]]
    assert EvalViews.five_crop(224).table(256, 256).tolist() == five
    ten = EvalViews.ten_crop(224)
    assert ten.V == 10 and ten.table(256, 256).tolist() == five + [b[:4] + [1] for b in five]
    # a source that is not square: the side follows the shorter edge, the corners both
    t = EvalViews.five_crop(224, crop_pct=0.5).table(100, 200)
    assert t.tolist() == [[0, 0, 50, 50, 0], [150, 0, 50, 50, 0], [0, 50, 50, 50, 0], [150, 50, 50, 50, 0], [75, 25, 50, 50, 0]]
    assert t.dtype == torch.int32 and not t.is_cuda
    hand = EvalViews([[1, 2, 3, 4, 1]])
    assert hand.V == 1 and hand.size is None and hand.table(8, 8).tolist() == [[1, 2, 3, 4, 1]]
    assert [EvalViews.resize(224).V, EvalViews.center(224, flip=True).V, EvalViews.five_crop(224).V] == [1, 2, 5]


def test_view_table_refusals():
    with pytest.raises(ValueError, match="outside"):
        EvalViews([[0, 0, 225, 224, 0]]).table(224, 224)
    with pytest.raises(ValueError, match="outside"):
        EvalViews([[-1, 0, 10, 10, 0]]).table(224, 224)
    with pytest.raises(ValueError, match="at most"):
        EvalViews([[0, 0, 8, 8, 0]] * (EVAL_MAX_VIEWS + 1)).table(8, 8)
    assert EvalViews([[0, 0, 8, 8, 0]] * EVAL_MAX_VIEWS).table(8, 8).shape == (EVAL_MAX_VIEWS, 5)
    with pytest.raises(ValueError):
        EvalViews(torch.zeros(3, 4, dtype=torch.int32))
    with pytest.raises(ValueError):
        EvalViews.center(224, crop_pct=1.5)


# ---- eval_view_shard ---------------------------------------------------------------------------------------------------------------
def _split(n, size=12):
    px = torch.arange(n, dtype=torch.uint8).view(n, 1, 1, 1).expand(n, 3, size, size).contiguous()
    return ResidentSplit.from_tensors(px, torch.arange(n, dtype=torch.int64) * 3)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n,batch,V", [(23, 8, 2), (23, 11, 5), (7, 10, 10), (16, 8, 2)])
def test_eval_view_shard_covers_every_sample_once_in_constant_shapes(world, n, batch, V):
    split = _split(n)
    table = EvalViews([[v, 0, 3, 4, v % 2] for v in range(V)]).table(12, 12)
    S = batch // V
    seen = []
    for rank in range(world):
        first_boxes = None
        for rows, boxes, labels, n_valid in split.eval_view_shard(table, batch, rank, world):
            assert tuple(rows.shape) == (S * V,) and rows.dtype == torch.int64
            assert tuple(boxes.shape) == (S * V, 5) and boxes.dtype == torch.int32 and boxes.is_contiguous()
            assert tuple(labels.shape) == (S,) and labels.dtype == torch.int64 and 1 <= n_valid <= S
            first_boxes = boxes if first_boxes is None else first_boxes
            assert boxes is first_boxes                                   # one tensor per pass
            assert torch.equal(boxes.view(S, V, 5), table.view(1, V, 5).expand(S, V, 5))   # row s*V + v holds view v
            per_sample = rows.view(S, V)
            assert bool((per_sample == per_sample[:, :1]).all())          # ... of sample s
            idx = per_sample[:, 0]
            assert torch.equal(labels, idx * 3)
            assert torch.equal(idx[n_valid:], idx[:1].expand(S - n_valid))    # the padding: copies of the batch's first sample
            seen += idx[:n_valid].tolist()
    assert seen == list(range(n))


def test_eval_view_shard_refuses_before_the_first_batch():
    split = _split(5)
    table = EvalViews.five_crop(8, crop_pct=0.5).table(12, 12)
    with pytest.raises(ValueError, match="no whole sample"):
        split.eval_view_shard(table, 4, 0, 1)                               # raised by the call, not by the first next()
    with pytest.raises(ValueError, match="outside"):
        split.eval_view_shard(torch.tensor([[0, 0, 13, 12, 0]], dtype=torch.int32), 4, 0, 1)


# ---- refusals of the engine and the recipe ----------------------------------------------------------------------------------------
def _cpu_model():
    from cara_amd import cara, create_model
    torch.manual_seed(0)
    return cara({"model": create_model("vit_base_patch16_224_in21k", depth=1, num_classes=4, drop_path_rate=0.1), "rank": 8,
                 "scale": 1.0, "l_mu": 1.0, "l_std": 0.0})


def test_evaluate_refuses_views_on_another_source_and_an_unknown_combine():
    eng = _cpu_model()._cara_engine
    x, y = torch.zeros(2, 3, 224, 224), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(CaraError, match="ResidentSplit"):
        eng.evaluate([(x, y)], views=EvalViews.resize(224))
    with pytest.raises(CaraError, match="ResidentSplit"):
        eng.evaluate(lambda: [(x, y)], views=EvalViews.resize(224))
    with pytest.raises(CaraError, match="EvalViews"):
        eng.evaluate(_split(4), views=[[0, 0, 12, 12, 0]])
    with pytest.raises(CaraError, match="combine"):
        eng.evaluate(_split(4), views=EvalViews.resize(224), combine="mean")


def test_fit_refuses_eval_views_with_the_reference_mode():
    from cara_amd.recipe import fit
    m = _cpu_model()
    with pytest.raises(CaraError, match="sharded"):
        fit(m, lambda epoch: [], _split(4), epochs=1, eval_mode="reference", eval_views=EvalViews.resize(224))
    with pytest.raises(CaraError, match="sharded"):
        fit(m, lambda epoch: [], _split(4), epochs=1, eval_views=EvalViews.resize(224))
