"""Host side of the per-sample predictions (no GPU): evalcount.predict_rows against a brute-force stable ordering and against the
host model of the accumulate / report launches; the bounds of tests/predict_model.py against an fp32 emulation of the arithmetic
they are derived for; the helpers of evalcount.Predictions on CPU tensors; the header and the exports."""
import os
import re

import numpy as np
import pytest
import torch

from cara_amd import evalcount as EC
from tests import predict_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -float("inf")


def tied_logits(B, C, seed):
    """multiples of 0.5 in a narrow range (so that most rows hold ties), a -inf column, a row of nothing but -inf"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, generator=g) * 1.5 * 2).round() / 2
    if C > 2:
        x[:, C // 2] = NEG
        x[::3, 0] = NEG
    if B > 2:
        x[B - 2] = NEG
    return x


def labels_for(B, C, seed):
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed))
    if B > 3:
        y[1], y[3] = -1, C          # both sides of [0, classes)
    return y


@pytest.mark.parametrize("classes", [1, 2, 5, 7, 64, 101])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_host_model_is_the_stable_descending_sort(classes, k):
    B = 12
    x, y = tied_logits(B, classes, seed=classes * 31 + k), labels_for(B, classes, seed=k)
    idx, prob, loss, rank = EC.predict_rows(x, y, k)
    assert idx.dtype == torch.int32 and rank.dtype == torch.int32 and idx.shape == prob.shape == (B, k)
    xn = x.numpy().astype(np.float64)
    order = np.argsort(-xn, axis=1, kind="stable")
    kk = min(k, classes)
    for b in range(B):
        if not np.isfinite(xn[b]).any():                      # no finite maximum: class 0, then nothing; NaN everywhere
            assert idx[b].tolist() == [0] + [-1] * (k - 1)
            assert bool(torch.isnan(prob[b]).all()) and bool(torch.isnan(loss[b]))
        else:
            assert idx[b, :kk].tolist() == order[b, :kk].tolist(), (b, xn[b])
            assert idx[b, kk:].tolist() == [-1] * (k - kk) and prob[b, kk:].tolist() == [0.0] * (k - kk)
            p = np.exp(xn[b] - xn[b].max())
            p /= p.sum()
            np.testing.assert_allclose(prob[b, :kk].numpy(), p[order[b, :kk]], rtol=1e-12, atol=0)
            assert bool((prob[b, :kk][torch.from_numpy(xn[b][order[b, :kk]]) == NEG] == 0).all())
        yb = int(y[b])
        if not 0 <= yb < classes:
            assert int(rank[b]) == -1 and bool(torch.isnan(loss[b]))
        else:
            assert int(rank[b]) == order[b].tolist().index(yb)                 # the label's position in that sort
            assert (int(rank[b]) < kk) == (yb in idx[b].tolist()) or not np.isfinite(xn[b]).any()
    if classes >= 7:
        assert any(len(set(r)) < len(r) for r in x.tolist()), "the quantised rows were meant to hold ties"
    i2, p2, l2, r2 = EC.predict_rows(x, None, k)
    assert torch.equal(i2, idx) and l2 is None and r2 is None


@pytest.mark.parametrize("classes", [3, 10, 100])
def test_host_model_agrees_with_the_models_of_the_existing_launches(classes):
    B, bins = 40, 15
    g = torch.Generator().manual_seed(classes)
    x = (torch.randn(B, classes, generator=g) * 2).round() / 2
    y = torch.randint(0, classes, (B,), generator=g)
    idx, prob, loss, rank = EC.predict_rows(x, y, 5)
    state, report = EC.accumulate_report(EC.new_state(), EC.new_report(classes, bins), x, y)
    assert int(state[EC.N]) == B and int(state[EC.TOP1]) == int((rank == 0).sum()) and int(state[EC.TOP5]) == int((rank < 5).sum())
    assert abs(float(state[EC.LOSS]) - float(loss.sum())) <= 1e-12 * float(loss.sum())
    conf = torch.zeros(classes, classes, dtype=torch.float64)
    conf.view(-1).index_add_(0, y * classes + idx[:, 0].long(), torch.ones(B, dtype=torch.float64))
    assert torch.equal(conf, report["confusion"])                              # pred = topk[:, 0]
    which = torch.clamp(torch.floor(prob[:, 0] * bins).long(), max=bins - 1)   # conf = prob[:, 0]
    assert torch.equal(torch.bincount(which, minlength=bins).double(), report["bin_count"])
    assert torch.allclose(torch.zeros(bins, dtype=torch.float64).index_add_(0, which, prob[:, 0]), report["bin_conf"], rtol=1e-12, atol=0)
    assert torch.equal((rank == 0), idx[:, 0].long() == y)
    # a label outside the classes: the accumulate model counts it in word 4, the predictions mark it
    y[5] = classes
    assert int(EC.accumulate(EC.new_state(), x, y)[EC.BAD]) == 1 and int(EC.predict_rows(x, y, 1)[3][5]) == -1


@pytest.mark.parametrize("kind", ["flat", "peaked", "tied", "neg_inf"])
def test_derived_bounds_hold_an_fp32_emulation_and_are_not_vacuous(kind):
    worst_p = worst_l = 0.0
    for C, vec in [(3, True), (5, False), (65, True), (100, True), (397, False)]:
        g = torch.Generator().manual_seed(C)
        x = torch.randn(3, C, generator=g) * {"flat": 0.02, "peaked": 30.0, "tied": 3.0, "neg_inf": 3.0}[kind]
        if kind == "tied":
            x = (x * 2).round() / 2
        if kind == "neg_inf":
            x[:, 1::3] = NEG
            x[:, 0] = 0.5                                     # (every row keeps a finite class, and the label's)
        y = torch.zeros(3, dtype=torch.int64)
        k = 5
        _, want_p, want_l, _ = EC.predict_rows(x, y, k)
        d_p, d_l = PM.bounds(x, y, k)
        got_p, got_l = PM.emulate(x, y, k, vec)
        ok, rp = PM.hold(got_p, want_p, d_p)
        assert bool(ok.all()), (kind, C, rp)
        ok, rl = PM.hold(got_l, want_l, d_l)
        assert bool(ok.all()), (kind, C, rl)
        # the bound scales with the value: a relative bound of at most 2^-9 (not vacuous)
        live = want_p > 2.0 ** -100
        assert float((d_p[live] / want_p[live]).max()) < 2.0 ** -9
        assert float((d_l / (want_l.abs() + (x.double().abs().max(1).values + 1))).max()) < 2.0 ** -9
        worst_p, worst_l = max(worst_p, rp), max(worst_l, rl)
    print(f"{kind}: worst emulated error / bound: prob {worst_p:.3f}, loss {worst_l:.3f}")
    assert worst_p > 0.01          # ... and within two orders of magnitude of what fp32 really does (not too loose to see a bug)


def table():
    """a hand-made table of six samples, three classes, k = 2"""
    topk = torch.tensor([[0, 1], [2, 0], [1, 2], [1, 0], [0, 2], [2, 1]], dtype=torch.int32)
    prob = torch.tensor([[.9, .1], [.5, .3], [.6, .3], [.4, .35], [.99, .01], [.7, .2]])
    labels = torch.tensor([0, 0, 1, 2, 0, 1])
    rank = torch.tensor([0, 1, 0, 2, 0, 1], dtype=torch.int32)
    loss = torch.tensor([.1, 1.2, .5, 1.4, .01, 1.6])
    return EC.Predictions(topk, prob, loss, rank, labels)


def test_predictions_helpers_on_cpu_tensors(tmp_path):
    from cara_amd._lib import CaraError
    p = table()
    assert len(p) == 6 and p.k == 2
    c = p.counts()
    assert c["n"] == 6 and c["top1"] == 3 / 6 and c["top5"] == 1.0
    assert abs(c["loss"] - float(p.loss.double().sum()) / 6) < 1e-15
    assert p.confusion(3).tolist() == [[2, 0, 1], [0, 1, 1], [0, 1, 0]]
    assert p.errors().tolist() == [1, 3, 5]
    idx, cls = p.confident(0.6)
    assert idx.tolist() == [0, 2, 4, 5] and cls.tolist() == [0, 1, 0, 2] and cls.dtype == torch.int64
    path = p.save(str(tmp_path / "pred"), names=[(f"img{i}.jpg", 0) for i in range(6)])
    assert path.endswith("pred.npz")
    z = np.load(path)
    assert sorted(z.files) == ["labels", "loss", "names", "prob", "rank", "topk"] and z["prob"].dtype == np.float32
    q, names = EC.Predictions.load(path)
    assert names == [f"img{i}.jpg" for i in range(6)]
    for a in ("topk", "prob", "loss", "rank", "labels"):
        assert torch.equal(getattr(q, a), getattr(p, a)) and getattr(q, a).dtype == getattr(p, a).dtype, a
    assert q.counts() == c
    with pytest.raises(ValueError):
        p.save(str(tmp_path / "short"), names=["a"])
    # a label outside the classes: counts raises as evaluate does; the per-sample views still answer
    bad = table()
    bad.rank[2], bad.loss[2] = -1, float("nan")
    with pytest.raises(CaraError, match="1 label"):
        bad.counts()
    assert bad.errors().tolist() == [1, 2, 3, 5]
    # a pass without labels
    bare = EC.Predictions(p.topk, p.prob)
    assert bare.confident(0.95)[0].tolist() == [4]
    for call in (bare.counts, bare.errors, lambda: bare.confusion(3)):
        with pytest.raises(CaraError, match="no labels"):
            call()
    q, names = EC.Predictions.load(bare.save(str(tmp_path / "bare.npz")))
    assert names is None and q.loss is None and q.rank is None and q.labels is None and torch.equal(q.topk, p.topk)


def test_header_declares_and_the_binding_exports_the_entry():
    from cara_amd import _lib
    text = open(os.path.join(ROOT, "include", "cara_hip.h")).read()
    assert re.search(r"\bint\s+cara_eval_predict\s*\(", text)
    assert re.search(r"#define\s+CARA_EVAL_PREDICT_MAX_K\s+16\b", text) and _lib.PREDICT_MAX_K == 16
    assert "cara_eval_predict" in _lib.SYMBOLS
    path = _lib.LIB_PATHS["bf16"]
    if os.path.exists(path):        # (a built tree: the library exports it and still reports ABI 14)
        import ctypes
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "cara_eval_predict") and lib.cara_abi_version() == 14
