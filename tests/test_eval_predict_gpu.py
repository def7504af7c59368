"""GPU side of the per-sample predictions: cara_eval_predict against its host model (evalcount.predict_rows, fp64 on the same fp32
logits) -- indices and ranks EXACTLY, probabilities and losses inside the bound DERIVED in tests/predict_model.py, element by
element --, its guard words, its agreement with cara_eval_accumulate_report on the same device logits (bit-equal confidence), its
determinism and its refusals; and CaraEngine.predict / fit(save_predictions=) on the depth-2 model.

Measured on an MI355X, worst device error / derived bound over every case of the first test: docs/findings/eval_predict.md."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from cara_amd import evalcount as EC
from tests import predict_model as PM
from tests.test_eval_gpu import _model
from tests.test_eval_views_gpu import BATCH, N_SPLIT, layouts, model_and_split, pixels_at, same_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = [1, 3, 4, 5, 63, 64, 65, 100, 397, 1000]   # below the vector width, its tail, both sides of the lane stride, unaligned rows
KS = [1, 5, 16]
ROWS = [1, 4, 5, 9]                                  # 5 crosses a workgroup of four waves
KINDS = ["flat", "peaked", "tied", "neg_inf"]
GUARD = 8
SENTINEL = 0x7FC12345                                # a NaN pattern no kernel writes
NEG = -float("inf")


def L():
    from cara_amd import _lib
    return _lib


def make_logits(B, C, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g) * {"flat": 0.02, "peaked": 30.0, "tied": 1.5, "neg_inf": 3.0}[kind]
    if kind == "tied":
        x = (x * 2).round() / 2
    if kind == "neg_inf" and C > 1:
        x[:, 1::3] = NEG                                           # (class 0 stays finite in every row)
    return x, torch.randint(0, C, (B,), generator=g)


class Table:
    """the four output tables of ``n_rows`` rows in ONE int32 buffer, guard words in front of, between and behind them"""

    def __init__(self, n_rows, k):
        self.n_rows, self.k = n_rows, k
        sizes = [n_rows * k, n_rows * k, n_rows, n_rows]
        self.buf = torch.full((GUARD * 5 + sum(sizes),), SENTINEL, dtype=torch.int32, device=DEV)
        self.at, o = [], GUARD
        for s in sizes:
            self.at.append((o, o + s))
            o += s + GUARD
        self.topk, self.prob, self.loss, self.rank = (self.buf[a:b] for a, b in self.at)

    def pointers(self, labelled=True):
        p = [t.data_ptr() for t in (self.topk, self.prob, self.loss, self.rank)]
        return p if labelled else p[:2] + [None, None]

    def rows(self, first, n):
        """rows [first, first + n) on the CPU: (idx int32 [n, k], prob fp32, loss fp32 [n], rank int32)"""
        k = self.k
        return (self.topk.view(-1, k)[first:first + n].cpu(), self.prob.view(torch.float32).view(-1, k)[first:first + n].cpu(),
                self.loss.view(torch.float32)[first:first + n].cpu(), self.rank[first:first + n].cpu())

    def untouched_outside(self, first, n, labelled=True):
        """every word but the rows [first, first + n) (of the label tables too, when ``labelled``) is as it was filled"""
        seen = self.buf.clone()
        for (a, b), width, used in zip(self.at, (self.k, self.k, 1, 1), (True, True, labelled, labelled)):
            if used:
                seen[a:b].view(-1, width)[first:first + n] = SENTINEL
        return bool((seen == SENTINEL).all())


def launch(lib, src, ldl, labels, B, n_valid, C, k, first, table, labelled=True):
    status = lib.cara_eval_predict(src.data_ptr(), ldl, labels.data_ptr() if labelled else None, B, n_valid, C, k, first, table.n_rows,
                                   *table.pointers(labelled), L().stream())
    torch.cuda.synchronize()
    return status


def on_device(x, ldl):
    """the rows of ``x`` with stride ``ldl``; what lies between them would wreck a sum or a maximum that read it"""
    src = torch.full((x.shape[0], ldl), 7.0e37, device=DEV)
    src[:, :x.shape[1]] = x.to(DEV)
    return src


def compare(got, x, y, k, what):
    """device rows against the host model: indices and ranks exactly, probabilities and loss within the derived bound
    -> (worst prob error / bound, worst loss error / bound)"""
    idx, prob, loss, rank = EC.predict_rows(x, y, k)
    d_p, d_l = PM.bounds(x, y, k)
    assert torch.equal(got[0], idx), (what, "topk_idx", got[0].tolist(), idx.tolist())
    ok, rp = PM.hold(got[1], prob, d_p)
    assert bool(ok.all()), (what, "topk_prob", rp, (~ok).nonzero()[:5].tolist())
    if y is None:
        return rp, 0.0
    assert torch.equal(got[3], rank), (what, "rank", got[3].tolist(), rank.tolist())
    ok, rl = PM.hold(got[2], loss, d_l)
    assert bool(ok.all()), (what, "loss", rl, (~ok).nonzero()[:5].tolist())
    return rp, rl


@pytest.mark.parametrize("classes", CLASSES)
@pytest.mark.parametrize("k", KS)
def test_predict_against_the_host_model(k, classes):
    lib = L().lib()
    worst_p = worst_l = 0.0
    for B in ROWS:
        for n, kind in enumerate(KINDS):
            x, y = make_logits(B, classes, kind, seed=1000 * classes + 10 * B + n)
            for ldl, _, _ in layouts(classes):
                t = Table(B, k)
                assert launch(lib, on_device(x, ldl), ldl, y.to(DEV), B, B, classes, k, 0, t) == 0
                assert t.untouched_outside(0, B)
                rp, rl = compare(t.rows(0, B), x, y, k, (classes, k, B, kind, ldl))
                worst_p, worst_l = max(worst_p, rp), max(worst_l, rl)
    print(f"predict {classes} classes, k = {k}: worst device error / derived bound: prob {worst_p:.3f}, loss {worst_l:.3f}")


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_predict_special_rows_in_both_libraries(operands):
    """no labels; labels outside the classes; a row of nothing but -inf; a label on a -inf class"""
    lib = L().lib(operands)
    B, C, k = 6, 37, 5
    x, y = make_logits(B, C, "neg_inf", seed=7)
    x[2] = NEG
    y[0], y[3], y[4] = -1, C, 1                      # (class 1 is -inf: its loss is +inf, its rank that of the first -inf)
    for ldl, _, _ in layouts(C):
        t = Table(B, k)
        assert launch(lib, on_device(x, ldl), ldl, y.to(DEV), B, B, C, k, 0, t) == 0
        got = t.rows(0, B)
        compare(got, x, y, k, (operands, ldl))
        assert got[3].tolist()[0] == -1 and got[3].tolist()[3] == -1 and bool(torch.isnan(got[2][[0, 3]]).all())
        assert got[0][2].tolist() == [0, -1, -1, -1, -1] and bool(torch.isnan(got[1][2]).all()) and bool(torch.isnan(got[2][2]))
        assert float(got[2][4]) == float("inf") and int(got[3][4]) == int((x[4] > NEG).sum())
        t = Table(B, k)
        assert launch(lib, on_device(x, ldl), ldl, y, B, B, C, k, 0, t, labelled=False) == 0
        assert t.untouched_outside(0, B, labelled=False)
        compare(t.rows(0, B), x, None, k, (operands, ldl, "no labels"))


def test_predict_writes_its_own_rows_only():
    lib = L().lib()
    for C, k, B, n_valid, first, n_rows in [(100, 5, 9, 6, 3, 11), (5, 16, 5, 1, 7, 8), (397, 1, 4, 4, 2, 6), (64, 5, 9, 9, 1, 10)]:
        x, y = make_logits(B, C, "tied", seed=C + first)
        for ldl, _, _ in layouts(C):
            t = Table(n_rows, k)
            assert launch(lib, on_device(x, ldl), ldl, y.to(DEV), B, n_valid, C, k, first, t) == 0
            assert t.untouched_outside(first, n_valid), (C, k, first, n_valid)
            compare(t.rows(first, n_valid), x[:n_valid], y[:n_valid], k, (C, k, first))
    t = Table(4, 5)                                   # no valid row: nothing is launched, nothing is written
    x, y = make_logits(4, 10, "flat", seed=1)
    assert launch(lib, on_device(x, 10), 10, y.to(DEV), 4, 0, 10, 5, 4, t) == 0 and t.untouched_outside(0, 0)


def half_ulp32(v):
    """half an fp32 unit in the last place of |v|"""
    _, e = torch.frexp(torch.tensor(abs(float(v)), dtype=torch.float64))
    return 2.0 ** (int(e) - 1 - 24)


@pytest.mark.parametrize("classes,kind", [(100, "flat"), (100, "peaked"), (5, "tied"), (397, "tied"), (1000, "neg_inf"), (3, "tied")])
def test_predict_agrees_with_the_accumulate_and_report_launches(classes, kind):
    lib = L().lib()
    B, bins, k = 203, 15, 5
    x, y = make_logits(B, classes, kind, seed=classes)
    ldl = classes + 1
    src, yd = on_device(x, ldl), y.to(DEV)
    state = torch.zeros(5, dtype=torch.int64, device=DEV)
    rep = torch.zeros(classes * classes + 3 * bins, dtype=torch.int64, device=DEV)
    assert lib.cara_eval_accumulate_report(src.data_ptr(), ldl, yd.data_ptr(), B, B, classes, state.data_ptr(), rep.data_ptr(), bins,
                                           L().stream()) == 0
    t = Table(B, k)
    assert launch(lib, src, ldl, yd, B, B, classes, k, 0, t) == 0
    idx, prob, loss, rank = t.rows(0, B)
    words = state.cpu()
    assert int(words[0]) == B and int(words[4]) == 0
    assert int((rank == 0).sum()) == int(words[1]) and int((rank < 5).sum()) == int(words[2])
    confusion = torch.bincount(y * classes + idx[:, 0].long(), minlength=classes * classes).view(classes, classes)
    assert torch.equal(confusion, rep[:classes * classes].view(classes, classes).cpu())
    # the header's rule on the fp32 confidence: bin = min(bins - 1, (int)(conf * bins)) in fp32
    fb = prob[:, 0] * torch.tensor(float(bins), dtype=torch.float32)
    which = torch.where(fb >= float(bins - 1), torch.full_like(fb, bins - 1), fb.floor()).long()
    assert torch.equal(torch.bincount(which, minlength=bins), rep[classes * classes:classes * classes + bins].cpu())
    hits = torch.bincount(which[rank == 0], minlength=bins)
    assert torch.equal(hits, rep[classes * classes + bins:classes * classes + 2 * bins].cpu())
    finite = torch.isfinite(loss)
    if bool(finite.all()):
        total = float(words.view(torch.float64)[3])
        slack = B * half_ulp32(loss.abs().max()) + 1e-12 * abs(total)
        print(f"{classes} classes [{kind}]: |sum of loss - state word 3| {abs(float(loss.double().sum()) - total):.3e}, allowed {slack:.3e}")
        assert abs(float(loss.double().sum()) - total) <= slack
    else:                                            # a label on a -inf class: both say +inf
        assert float(loss.double().sum()) == float(words.view(torch.float64)[3]) == float("inf")


def test_predict_is_deterministic():
    lib = L().lib()
    B, C, k = 300, 1000, 16                          # more rows than one round of the grid's waves would need at 64
    x, y = make_logits(B, C, "flat", seed=2)
    src, yd = on_device(x, C), y.to(DEV)
    a, b = Table(B, k), Table(B, k)
    assert launch(lib, src, C, yd, B, B, C, k, 0, a) == 0 and launch(lib, src, C, yd, B, B, C, k, 0, b) == 0
    assert torch.equal(a.buf, b.buf)
    compare(a.rows(0, B), x, y, k, "300 rows")


def test_predict_refusals_launch_nothing():
    lib = L().lib()
    B, C, k, n_rows = 4, 10, 5, 6
    x, y = make_logits(B, C, "flat", seed=3)
    src, yd, t = on_device(x, C), y.to(DEV), Table(n_rows, k)
    p, q, st = src.data_ptr(), yd.data_ptr(), L().stream()
    ti, tp, tl, tr = t.pointers()
    ok = dict(logits=p, ldl=C, labels=q, B=B, n_valid=B, classes=C, k=k, first=0, n_rows=n_rows, topk=ti, prob=tp, loss=tl, rank=tr)
    refused = {
        "logits NULL": dict(logits=None), "topk_idx NULL": dict(topk=None), "topk_prob NULL": dict(prob=None),
        "labels without loss": dict(loss=None), "labels without rank": dict(rank=None), "loss without labels": dict(labels=None, rank=None),
        "rank without labels": dict(labels=None, loss=None), "loss and rank without labels": dict(labels=None),
        "k = 0": dict(k=0), "k = 17": dict(k=17), "k < 0": dict(k=-1), "first < 0": dict(first=-1),
        "first + n_valid > n_rows": dict(first=3), "n_rows < 0": dict(n_rows=-1, first=0, n_valid=0),
        "first past the table": dict(first=n_rows + 1, n_valid=0),
        "logits off by 2 bytes": dict(logits=p + 2), "topk_idx off by 2 bytes": dict(topk=ti + 2), "topk_prob off by 1 byte": dict(prob=tp + 1),
        "loss off by 2 bytes": dict(loss=tl + 2), "rank off by 2 bytes": dict(rank=tr + 2), "labels off by 4 bytes": dict(labels=q + 4),
        "B = 0": dict(B=0, n_valid=0), "n_valid < 0": dict(n_valid=-1), "n_valid > B": dict(n_valid=B + 1, n_rows=64),
        "classes < 1": dict(classes=0), "ldl < classes": dict(ldl=C - 1),
    }
    for what, change in refused.items():
        a = dict(ok, **change)
        assert lib.cara_eval_predict(a["logits"], a["ldl"], a["labels"], a["B"], a["n_valid"], a["classes"], a["k"], a["first"], a["n_rows"],
                                     a["topk"], a["prob"], a["loss"], a["rank"], st) == 1, what
    torch.cuda.synchronize()
    assert t.untouched_outside(0, 0)
    # the neighbours of the refused values are legal
    for change in (dict(first=2), dict(k=16, n_rows=1, n_valid=1), dict(k=1), dict(labels=None, loss=None, rank=None)):
        a = dict(ok, **change)
        assert lib.cara_eval_predict(a["logits"], a["ldl"], a["labels"], a["B"], a["n_valid"], a["classes"], a["k"], a["first"], a["n_rows"],
                                     a["topk"], a["prob"], a["loss"], a["rank"], st) == 0, change
    torch.cuda.synchronize()


# ---- the whole model ---------------------------------------------------------------------------------------------------------------
def table_of(p):
    return (p.topk.cpu(), p.prob.cpu(), p.loss.cpu(), p.rank.cpu())


def check_pass(eng, split, k=5, **kw):
    """predict(**kw) against the host model on the logits evaluate(**kw)'s debug_hook shows, and its counts against evaluate's"""
    seen = []
    hook = (lambda lg, lb, nv: seen.append((lg[:nv].cpu(), lb[:nv].cpu()))) if kw.get("views") is None else \
        (lambda lg, lb, nv, comb: seen.append((comb[:nv].cpu(), lb[:nv].cpu())))
    before = eng.evaluate(split, BATCH, debug_hook=hook, **kw)
    assert [lg.shape[0] for lg, _ in seen][-1] < seen[0][0].shape[0], "the last batch was meant to be a padded one"
    x, y = torch.cat([lg for lg, _ in seen]), torch.cat([lb for _, lb in seen])
    assert x.shape[0] == len(split) and torch.equal(y, split.labels.cpu())
    pred = eng.predict(split, k, BATCH, **kw)
    assert len(pred) == len(split) and pred.topk.dtype == torch.int32 and pred.prob.shape == (len(split), k)
    rp, rl = compare(table_of(pred), x, y, k, kw)
    got = pred.counts()
    n = before["n"]
    assert (got["n"], round(got["top1"] * n), round(got["top5"] * n)) == (n, round(before["top1"] * n), round(before["top5"] * n))
    # evaluate adds the unrounded fp64 terms, the table holds them rounded to fp32: half a unit in the last place each
    slack = half_ulp32(pred.loss.abs().max()) + 1e-12 * abs(before["loss"])
    print(f"{sorted(kw)}: error / bound prob {rp:.3f} loss {rl:.3f}; mean loss {got['loss']!r} against {before['loss']!r}, allowed {slack:.3e}")
    assert abs(got["loss"] - before["loss"]) <= slack
    assert torch.equal(pred.confusion(100), eng.evaluate(split, BATCH, report=True, **kw)["confusion"])
    same_dict(eng.evaluate(split, BATCH, **kw), before)                           # predict left the pass's outputs alone
    return pred


def test_predict_whole_model_rows_and_counts():
    m, split = model_and_split(N_SPLIT, size=224)
    eng = m._cara_engine
    pred = check_pass(eng, split)
    assert pred.errors().tolist() == (pred.rank != 0).nonzero()[:, 0].tolist()
    again = eng.predict(split, 5, BATCH)
    assert all(torch.equal(a, b) for a, b in zip(table_of(pred), table_of(again)))
    # the same images as batches: this rank's rows in arrival order; without labels no loss and no rank
    batches = list(split.eval_shard(BATCH, 0, 1))
    listed = eng.predict(batches, 5)
    assert all(torch.equal(a, b) for a, b in zip(table_of(pred), table_of(listed))) and torch.equal(listed.labels, split.labels)
    bare = eng.predict([(px, None, nv) for px, _, nv in batches], 3)
    assert bare.loss is None and bare.rank is None and bare.labels is None and torch.equal(bare.topk, pred.topk[:, :3])
    assert torch.equal(bare.prob, pred.prob[:, :3])
    from cara_amd._lib import CaraError
    for k in (0, 17, True, 2.0):
        with pytest.raises(CaraError, match="k must be"):
            eng.predict(split, k)


def test_predict_through_two_views():
    from cara_amd.data import EvalViews
    m, split = model_and_split(N_SPLIT)                                           # 256-pixel images, S = 4 samples of two views
    check_pass(m._cara_engine, split, views=EvalViews.center(224, flip=True))
    check_pass(m._cara_engine, split, views=EvalViews.center(224, flip=True), combine="logit")


def test_predict_on_the_averaged_weights():
    m, split = model_and_split(N_SPLIT, size=224)
    eng = m._cara_engine
    ema = eng.make_ema(0.5)
    with torch.no_grad():
        for i, s in enumerate(ema.tensors):                                       # shadows that are not the parameters
            s.mul_(1.0 + 0.05 * ((i % 3) - 1)).add_(1e-3)
    avg = check_pass(eng, split, weights=ema)
    raw = eng.predict(split, 5, BATCH)
    assert not torch.equal(avg.prob, raw.prob)
    with ema.swapped_in():
        want = eng.predict(split, 5, BATCH)
    assert all(torch.equal(a, b) for a, b in zip(table_of(avg), table_of(want)))


@functools.lru_cache(maxsize=None)
def fp16_model():
    m = _model(2, "fp16").eval()
    with torch.no_grad():
        m.head.weight.mul_(8.0)
    return m


def test_predict_in_fp16_precision():
    from cara_amd.data import ResidentSplit
    px, labels = pixels_at(N_SPLIT, 224, seed=31)
    check_pass(fp16_model()._cara_engine, ResidentSplit.from_tensors(px.to(DEV), labels.to(DEV)))


def test_predict_two_ranks_on_one_gpu_assemble_the_one_rank_table(tmp_path):
    from tests.test_eval_shard import _free_port
    out = str(tmp_path / "pr")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_eval_predict_two_ranks.py"), str(r), "2", out], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), logs
    a, b = (torch.load(f"{out}.{r}.pt") for r in range(2))
    assert a["filled"] + b["filled"] == N_SPLIT and a["filled"] == BATCH          # the shards: 8 and 3 rows
    from cara_amd.data import EvalViews
    m, split = model_and_split(N_SPLIT)
    for key, kw in (("plain", {}), ("views", {"views": EvalViews.center(224, flip=True)})):
        if key == "plain":
            _, split224 = model_and_split(N_SPLIT, size=224)
            one = m._cara_engine.predict(split224, 5, BATCH)
        else:
            one = m._cara_engine.predict(split, 5, BATCH, **kw)
        words = [t.view(torch.int32) if t.dtype == torch.float32 else t for t in table_of(one)]
        for r, got in enumerate((a, b)):
            for name, w in zip(("topk", "prob", "loss", "rank"), words):
                assert torch.equal(got[key][name], w), (key, r, name)                # bit for bit, on both ranks


def test_fit_writes_the_predictions_of_its_best_pass(tmp_path):
    from cara_amd import cara, create_model
    from cara_amd._lib import CaraError
    from cara_amd.data import EvalViews, ResidentSplit, normalize_u8
    from cara_amd.recipe import fit
    g = torch.Generator().manual_seed(1)
    y = torch.arange(16) % 4
    px = (torch.randn(16, 3, 256, 256, generator=g) * 20 + 40 + 50 * y.float().reshape(-1, 1, 1, 1)).clamp_(0, 255).to(torch.uint8)
    x = normalize_u8(px[:, :, 16:240, 16:240].contiguous()).to(DEV)
    split = ResidentSplit.from_tensors(px.to(DEV), y.to(DEV))
    torch.manual_seed(0)
    m = cara({"model": create_model("vit_base_patch16_224_in21k", depth=2, num_classes=4, drop_path_rate=0.1), "rank": 8,
              "scale": 1.0, "l_mu": 1.0, "l_std": 0.0}).to(DEV)
    views = EvalViews.center(224, flip=True)
    path = str(tmp_path / "best.npz")
    # (the schedule evaluates every tenth epoch: eleven epochs are the shortest run that does)
    best, _ = fit(m, lambda epoch: [(x, y.to(DEV))], split, epochs=11, lr=1e-2, seed=3, eval_mode="sharded", eval_views=views,
                  ema_decay=0.9, save_predictions=path)
    table, names = EC.Predictions.load(path)
    got = table.counts()
    print(best, got)
    assert got["n"] == 16 and got["top1"] == best and best > 0 and len(names) == 16
    direct = m._cara_engine.predict(split, 5, views=views, weights=m._cara_engine.ema)
    assert all(torch.equal(a, b) for a, b in zip(table_of(direct), (table.topk, table.prob, table.loss, table.rank)))
    with pytest.raises(CaraError, match="sharded"):
        fit(m, lambda epoch: [(x, y.to(DEV))], split, epochs=1, save_predictions=path)
