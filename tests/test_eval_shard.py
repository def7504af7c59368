"""CPU side of the sharded, device-resident evaluation (CaraEngine.evaluate): how a split is cut over the ranks, the counting
that cara_eval_accumulate performs (cara_amd/evalcount.py, its plain-torch restatement) against a literal numpy one, the one
all-reduce of the counters under gloo, and that fit()'s default evaluation path is the one it always was."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cara_amd import evalcount as EC
from cara_amd.dist import allreduce_sum_, eval_shard

CLASSES = [2, 4, 5, 6, 37, 397, 1000, 21843]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 711, 10_000, 73_728])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_eval_shard_covers_every_index_once_in_order(n, world):
    batch = 256
    parts = [eval_shard(n, r, world, batch) for r in range(world)]
    assert [i for p in parts for i in p] == list(range(n))          # disjoint, in file order, nothing left out
    cap = -(-(-(-n // world)) // batch) * batch                       # ceil(n / world) rounded up to whole batches
    assert all(len(p) <= cap for p in parts)
    short = [r for r, p in enumerate(parts) if len(p) % batch]
    assert len(short) <= 1                                           # only the range that holds the end has a short batch
    if short:
        assert all(len(p) == 0 for p in parts[short[0] + 1:])


def table(classes, B, seed):
    """random logits with planted EXACT ties: in a third of the rows the label's value is copied to other columns (before
    and behind it), in some rows to five or more of them, so that every branch of the tie rule is taken"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, classes, generator=g) * 3.0
    labels = torch.randint(0, classes, (B,), generator=g)
    for b in range(0, B, 3):
        k = int(torch.randint(1, min(classes, 8) + 1, (1,), generator=g))
        cols = torch.randperm(classes, generator=g)[:k]
        top = bool(torch.rand(1, generator=g) < 0.5)
        v = float(logits[b].max() + 1.0 if top else logits[b, labels[b]])
        logits[b, cols] = v
        logits[b, labels[b]] = v
    return logits, labels


def numpy_counts(logits, labels, n_valid):
    """the literal restatement: numpy.argmax, a stable argsort for the top five, log-sum-exp in fp64"""
    l = logits[:n_valid].numpy().astype(np.float64)
    y = labels[:n_valid].numpy()
    top1 = int((np.argmax(l, axis=1) == y).sum())
    order = np.argsort(-l, axis=1, kind="stable")[:, :5]
    top5 = int((order == y[:, None]).any(axis=1).sum())
    m = l.max(axis=1)
    loss = float((m + np.log(np.exp(l - m[:, None]).sum(axis=1)) - l[np.arange(len(y)), y]).sum())
    return len(y), top1, top5, loss


@pytest.mark.parametrize("classes", CLASSES)
def test_counting_fallback_equals_numpy(classes):
    B, n_valid = 96, 77
    logits, labels = table(classes, B, seed=classes)
    st = EC.accumulate(EC.new_state(), logits, labels, n_valid)
    n, top1, top5, loss = numpy_counts(logits, labels, n_valid)
    assert [int(st[EC.N]), int(st[EC.TOP1]), int(st[EC.TOP5]), int(st[EC.BAD])] == [n, top1, top5, 0]
    assert abs(float(st[EC.LOSS]) - loss) <= 1e-12 * abs(loss)
    if classes < 5:
        assert top5 == n_valid
    assert 0 < top1 < n_valid or classes == 2                       # the planted ties make hits and misses both


def test_counting_fallback_accumulates_and_flags_bad_labels():
    logits, labels = table(37, 64, seed=3)
    st = EC.new_state()
    for lo in (0, 20, 40):
        EC.accumulate(st, logits[lo:lo + 24], labels[lo:lo + 24], 20 if lo < 40 else 24)
    n, top1, top5, loss = numpy_counts(logits, labels, 64)
    assert [int(st[EC.N]), int(st[EC.TOP1]), int(st[EC.TOP5])] == [n, top1, top5]
    assert abs(float(st[EC.LOSS]) - loss) <= 1e-12 * abs(loss)
    bad = labels.clone()
    bad[5], bad[9] = 37, -1
    st2 = EC.accumulate(EC.new_state(), logits, bad)
    keep = torch.ones(64, dtype=torch.bool)
    keep[5] = keep[9] = False
    n, top1, top5, loss = numpy_counts(logits[keep], labels[keep], 62)
    assert [int(st2[EC.N]), int(st2[EC.TOP1]), int(st2[EC.TOP5]), int(st2[EC.BAD])] == [n, top1, top5, 2]
    with pytest.raises(ValueError):
        EC.result(st2)
    assert EC.result(st)["n"] == 64


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    logits, labels = table(100, 711, seed=8)
    st = EC.new_state()
    mine = eval_shard(711, rank, world, 256)
    for i in range(mine.start, mine.stop, 256):
        j = min(i + 256, mine.stop)
        # (the padded form of ResidentSplit.eval_shard: 256 rows, n_valid of them real)
        pad = 256 - (j - i)
        lg = torch.cat([logits[i:j], logits[i:i + 1].expand(pad, -1)])
        lb = torch.cat([labels[i:j], labels[i:i + 1].expand(pad)])
        EC.accumulate(st, lg, lb, j - i)
    allreduce_sum_(st)
    torch.save(st.clone(), out + f".{rank}")
    dist.destroy_process_group()


def test_two_gloo_ranks_hold_the_single_process_counts(tmp_path):
    out = str(tmp_path / "ev.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    logits, labels = table(100, 711, seed=8)
    one = EC.accumulate(EC.new_state(), logits, labels)
    for rank in range(2):
        got = torch.load(out + f".{rank}")
        assert [int(v) for v in got[[0, 1, 2, 4]]] == [int(v) for v in one[[0, 1, 2, 4]]] and int(got[0]) == 711
        assert abs(float(got[3]) - float(one[3])) <= 1e-12 * abs(float(one[3]))   # (two fp64 partial sums instead of one)


class _StubEngine:
    def __init__(self, log):
        self.log = log

    def seed_rank_streams(self, seed, rank):
        self.log.append(("seed_rank_streams",))

    def train_step(self, x, y, opt, group=None):
        self.log.append(("train_step",))

    def evaluate(self, split, batch_size=256, group=None):
        self.log.append(("engine.evaluate",))
        return {"top1": 0.5, "top5": 1.0, "loss": 0.0, "n": 2}


class _StubModel(torch.nn.Module):
    def __init__(self, log):
        super().__init__()
        self.CP_x = torch.nn.Parameter(torch.zeros(4))
        self.head = torch.nn.Linear(4, 2)
        self._cara_engine = _StubEngine(log)
        self.log = log

    def forward(self, x):
        self.log.append(("model.forward", self.training))
        return self.head(x)


def _run_fit(monkeypatch, **kw):
    from cara_amd import recipe

    class _Opt(torch.optim.SGD):   # (the real AdamW launches a HIP kernel; the loop only needs param_groups and step())
        def __init__(self, params, lr, weight_decay, capturable=False):
            super().__init__(params, lr=lr)

    import cara_amd.optim
    monkeypatch.setattr(cara_amd.optim, "AdamW", _Opt)
    log = []
    m = _StubModel(log)
    x, y = torch.zeros(2, 4), torch.tensor([0, 1])
    test = kw.pop("test")
    best, _ = recipe.fit(m, lambda epoch: [(x, y)], test(x, y, log), epochs=21,
                         on_eval=lambda e, a: log.append(("on_eval", e, a)), **kw)
    return best, log, m


def test_fit_reference_eval_mode_is_the_unchanged_call_sequence(monkeypatch):
    def test(x, y, log):
        def batches():
            log.append(("test_batches()",))
            return [(x, y)]
        return batches
    want = ([("train_step",)] * 11 + [("test_batches()",), ("model.forward", False), ("on_eval", 10, 0.5)]
            + [("train_step",)] * 10 + [("test_batches()",), ("model.forward", False), ("on_eval", 20, 0.5)])
    for kw in ({}, {"eval_mode": "reference"}):
        best, log, m = _run_fit(monkeypatch, test=test, **kw)
        assert log == want and best == 0.5 and not m.training       # recipe.evaluate over test_batches(), never engine.evaluate
    best, log, m = _run_fit(monkeypatch, test=lambda x, y, log: "a-split", eval_mode="sharded")
    assert log == ([("train_step",)] * 11 + [("engine.evaluate",), ("on_eval", 10, 0.5)]
                   + [("train_step",)] * 10 + [("engine.evaluate",), ("on_eval", 20, 0.5)]) and best == 0.5
    from cara_amd._lib import CaraError
    with pytest.raises(CaraError):
        _run_fit(monkeypatch, test=lambda x, y, log: None, eval_mode="fast")
