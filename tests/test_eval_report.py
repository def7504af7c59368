"""CPU side of the evaluation report (CaraEngine.evaluate(report=True)): the host model of cara_eval_accumulate_report
(cara_amd/evalcount.py: confusion matrix and confidence bins) on tables worked by hand, its invariants, the arithmetic of
report_result, the one all-reduce of state + report under gloo, and what fit(eval_metric=) refuses and calls."""
import math

import pytest
import torch
import torch.multiprocessing as mp

from cara_amd import evalcount as EC
from tests.test_eval_shard import _free_port, _run_fit, table


def _hand_table():
    """four classes, five rows, n_valid = 4: two rows of one exact tie (labels 0 and 1), a confident hit, a bad label and a row
    behind n_valid.  Class 3 is never a label and never predicted."""
    logits = torch.tensor([[1.0, 1.0, 0.0, 0.0],     # y = 0: tie of classes 0 and 1 -> pred 0, a hit
                           [1.0, 1.0, 0.0, 0.0],     # y = 1: the same tie -> pred 0, a miss
                           [0.0, 0.0, 5.0, 0.0],     # y = 2: pred 2, a hit, confidence 0.98
                           [2.0, 0.0, 0.0, 0.0],     # y = 7: outside [0, 4)
                           [0.0, 3.0, 0.0, 0.0]])    # behind n_valid
    labels = torch.tensor([0, 1, 2, 7, 1])
    conf_tie = 1.0 / (2.0 + 2.0 * math.exp(-1.0))    # 0.3655 -> bin 1 of 4
    conf_hit = 1.0 / (1.0 + 3.0 * math.exp(-5.0))    # 0.9802 -> bin 3 of 4
    return logits, labels, conf_tie, conf_hit


def test_accumulate_report_on_a_table_worked_by_hand():
    logits, labels, conf_tie, conf_hit = _hand_table()
    st, rep = EC.accumulate_report(EC.new_state(), EC.new_report(4, 4), logits, labels, n_valid=4)
    assert [int(v) for v in st[[EC.N, EC.TOP1, EC.TOP5, EC.BAD]]] == [3, 2, 3, 1]
    want = torch.zeros(4, 4, dtype=torch.float64)
    want[0, 0] = want[1, 0] = want[2, 2] = 1.0
    assert torch.equal(rep["confusion"], want)
    assert rep["bin_count"].tolist() == [0.0, 2.0, 0.0, 1.0] and rep["bin_hits"].tolist() == [0.0, 1.0, 0.0, 1.0]
    assert rep["bin_conf"][[0, 2]].tolist() == [0.0, 0.0]
    assert abs(float(rep["bin_conf"][1]) - 2 * conf_tie) <= 1e-15 and abs(float(rep["bin_conf"][3]) - conf_hit) <= 1e-15
    # the state is what accumulate alone leaves, and a second batch adds to both
    assert torch.equal(st, EC.accumulate(EC.new_state(), logits, labels, 4))
    EC.accumulate_report(st, rep, logits[4:], labels[4:])
    assert int(st[EC.N]) == 4 and rep["confusion"][1, 1] == 1.0 and rep["confusion"].sum() == 4.0
    with pytest.raises(ValueError):
        EC.accumulate_report(EC.new_state(), EC.new_report(5, 4), logits, labels)      # a report of another class count


def test_confidence_on_a_bin_edge_goes_to_the_upper_bin_and_one_is_clamped():
    for classes in (2, 4):
        st, rep = EC.accumulate_report(EC.new_state(), EC.new_report(classes, classes), torch.zeros(3, classes),
                                       torch.tensor([0, classes - 1, 0]))
        count = [0.0] * classes
        count[1] = 3.0                                     # conf = 1 / classes exactly: the edge between bins 0 and 1
        assert rep["bin_count"].tolist() == count and float(rep["bin_conf"][1]) == 3.0 / classes
        assert rep["confusion"][:, 0].sum() == 3.0 and float(rep["bin_hits"][1]) == 2.0    # every tie goes to class 0
    lg = torch.zeros(2, 5)
    lg[:, 3] = 80.0
    _, rep = EC.accumulate_report(EC.new_state(), EC.new_report(5, 15), lg, torch.tensor([3, 0]))
    assert float(rep["bin_count"][14]) == 2.0 and float(rep["bin_conf"][14]) == 2.0 and float(rep["bin_hits"][14]) == 1.0


@pytest.mark.parametrize("classes,bins", [(2, 1), (5, 15), (37, 64), (397, 15)])
def test_report_invariants(classes, bins):
    logits, labels = table(classes, 96, seed=classes)
    labels[11] = classes                                    # one bad label: in no count of the report
    st, rep = EC.accumulate_report(EC.new_state(), EC.new_report(classes, bins), logits, labels, n_valid=77)
    n, hits = int(st[EC.N]), int(st[EC.TOP1])
    assert n == 76 and int(st[EC.BAD]) == 1
    assert int(rep["confusion"].sum()) == n and int(rep["confusion"].diagonal().sum()) == hits
    assert int(rep["bin_count"].sum()) == n and int(rep["bin_hits"].sum()) == hits
    assert bool((rep["bin_hits"] <= rep["bin_count"]).all()) and bool((rep["bin_conf"] <= rep["bin_count"]).all())
    # the predicted class is numpy.argmax's: the first index of the maximum
    keep = torch.ones(77, dtype=torch.bool)
    keep[11] = False
    pred = torch.from_numpy(logits[:77][keep].numpy().argmax(axis=1))
    want = torch.zeros(classes, classes, dtype=torch.float64)
    want.view(-1).index_add_(0, labels[:77][keep] * classes + pred, torch.ones(76, dtype=torch.float64))
    assert torch.equal(rep["confusion"], want)
    # the vector form is the kernel's layout, and it is undone without a copy
    vec = EC.report_vector(rep)
    assert vec.shape[0] == EC.report_words(classes, bins) == classes * classes + 3 * bins
    back = EC.report_from_vector(vec, classes, bins)
    assert all(torch.equal(back[k], rep[k]) for k in EC.REPORT_KEYS)


def test_report_result_arithmetic():
    logits, labels, conf_tie, conf_hit = _hand_table()
    st, rep = EC.accumulate_report(EC.new_state(), EC.new_report(4, 4), logits, labels, n_valid=4)
    with pytest.raises(ValueError):
        EC.report_result(st, rep)                           # the bad label, as result() reports it
    st[EC.BAD] = 0.0
    r = EC.report_result(st, rep)
    assert r["n"] == 3 and r["top1"] == 2 / 3 and r["top5"] == 1.0 and set(r) >= {"top1", "top5", "loss", "n"}
    assert r["confusion"].dtype == torch.int64 and r["confusion"].tolist() == [[1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert r["support"].tolist() == [1, 1, 1, 0] and r["support"].dtype == torch.int64
    assert r["per_class"][:3].tolist() == [1.0, 0.0, 1.0] and math.isnan(float(r["per_class"][3]))
    assert r["precision"][[0, 2]].tolist() == [0.5, 1.0] and bool(torch.isnan(r["precision"][[1, 3]]).all())
    assert r["mean_per_class"] == 2 / 3                      # over the three classes with support, not over four
    assert r["calibration"]["count"].tolist() == [0, 2, 0, 1] and r["calibration"]["hits"].tolist() == [0, 1, 0, 1]
    want_ece = (2 / 3) * abs(0.5 - conf_tie) + (1 / 3) * abs(1.0 - conf_hit)
    assert abs(r["ece"] - want_ece) <= 1e-15
    # two bins worked by hand: 4 rows at mean confidence 0.4 with 1 hit (gap 0.15), 6 rows at 0.9 with 5 hits (gap 1/15)
    state = torch.tensor([10.0, 6.0, 10.0, 3.0, 0.0], dtype=torch.float64)
    rep2 = EC.new_report(2, 2)
    rep2["confusion"] += torch.tensor([[4.0, 1.0], [3.0, 2.0]], dtype=torch.float64)
    rep2["bin_count"] += torch.tensor([4.0, 6.0], dtype=torch.float64)
    rep2["bin_hits"] += torch.tensor([1.0, 5.0], dtype=torch.float64)
    rep2["bin_conf"] += torch.tensor([1.6, 5.4], dtype=torch.float64)
    r2 = EC.report_result(state, rep2)
    assert abs(r2["ece"] - 0.1) <= 1e-15                     # 0.4 * 0.15 + 0.6 / 15
    assert r2["per_class"].tolist() == [0.8, 0.4] and abs(r2["mean_per_class"] - 0.6) <= 1e-15
    assert r2["precision"].tolist() == [4 / 7, 2 / 3] and r2["calibration"]["confidence"].tolist() == [1.6, 5.4]
    # nothing scored: no NaN in the scalars that need none, NaN where there is no class to average
    r0 = EC.report_result(EC.new_state(), EC.new_report(3, 5))
    assert r0["n"] == 0 and r0["ece"] == 0.0 and math.isnan(r0["mean_per_class"]) and bool(torch.isnan(r0["per_class"]).all())


def test_two_gloo_ranks_hold_the_single_process_report(tmp_path):
    from tests import _eval_report_worker as W
    out = str(tmp_path / "rep.pt")
    mp.spawn(W.worker, args=(2, _free_port(), out), nprocs=2, join=True)
    logits, labels = table(W.CLASSES, W.ROWS, seed=W.SEED)
    st, rep = EC.accumulate_report(EC.new_state(), EC.new_report(W.CLASSES, W.BINS), logits, labels)
    one = torch.cat([st, EC.report_vector(rep)])
    exact = torch.ones(one.shape[0], dtype=torch.bool)
    exact[EC.LOSS] = False
    exact[-W.BINS:] = False                                  # the loss word and bin_conf: two fp64 partial sums instead of one
    for rank in range(2):
        got = torch.load(out + f".{rank}")
        assert got.shape == one.shape and torch.equal(got[exact], one[exact]) and int(got[0]) == W.ROWS
        assert bool(((got[~exact] - one[~exact]).abs() <= 1e-12 * one[~exact].abs()).all())
        r = EC.report_result(got[:5], EC.report_from_vector(got[5:], W.CLASSES, W.BINS))
        assert int(r["confusion"].sum()) == W.ROWS and int(r["support"].sum()) == W.ROWS


class _ReportEngine:
    """CaraEngine's evaluate as fit sees it: records its keywords, returns a dict whose two metrics differ"""

    def __init__(self, log):
        self.log = log

    def seed_rank_streams(self, seed, rank):
        pass

    def train_step(self, x, y, opt, group=None):
        pass

    def evaluate(self, split, batch_size=256, group=None, **kw):
        self.log.append(("engine.evaluate", kw))
        out = {"top1": 0.5, "top5": 1.0, "loss": 0.0, "n": 2}
        if kw.get("report"):
            out["mean_per_class"] = 0.25
        return out


def test_fit_eval_metric_refusals_and_calls(monkeypatch):
    from cara_amd._lib import CaraError
    for kw in ({"eval_metric": "mean_per_class"}, {"eval_metric": "mean_per_class", "eval_mode": "reference"},
               {"eval_metric": "recall", "eval_mode": "sharded"}):
        with pytest.raises(CaraError, match="eval_metric"):
            _run_fit(monkeypatch, test=lambda x, y, log: "a-split", **kw)

    def swap_engine(x, y, log):
        return "a-split"
    import cara_amd.recipe as recipe
    real_fit = recipe.fit

    def fit_with_report_engine(m, *a, **kw):
        m._cara_engine = _ReportEngine(m.log)
        return real_fit(m, *a, **kw)
    monkeypatch.setattr(recipe, "fit", fit_with_report_engine)
    best, log, _ = _run_fit(monkeypatch, test=swap_engine, eval_mode="sharded", eval_metric="mean_per_class")
    assert log == [("engine.evaluate", {"report": True}), ("on_eval", 10, 0.25),
                   ("engine.evaluate", {"report": True}), ("on_eval", 20, 0.25)] and best == 0.25
    best, log, _ = _run_fit(monkeypatch, test=swap_engine, eval_mode="sharded")
    assert log == [("engine.evaluate", {}), ("on_eval", 10, 0.5), ("engine.evaluate", {}), ("on_eval", 20, 0.5)] and best == 0.5
