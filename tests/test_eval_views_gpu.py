"""GPU side of the multi-view evaluation: cara_eval_combine_views against its host model (evalcount.combine_views, fp64 on the
same fp32 logits) inside the bound DERIVED in tests/views_model.py, element by element; its guard words, its -inf rule and its
refusals; and CaraEngine.evaluate(views=) / fit(eval_views=) on the depth-2 model: bit for bit the plain pass where the views
are the identity, the per-view logits against forward_resident, the counts against the host model, padding, ten crops, the
averaged weights, two ranks on one GPU.  Measured error / bound ratios: docs/findings/eval_views.md."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from cara_amd import evalcount as EC
from tests import views_model as VM
from tests.test_eval_gpu import LOSS_REL, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = [1, 3, 4, 5, 100, 397, 1000]      # below one lane stride, the vector tail, unaligned rows
VIEWS = [1, 2, 3, 5, 10, 16]
SAMPLES = [1, 4, 5, 9]                      # 5 crosses a workgroup of four waves
KINDS = ["flat", "peaked", "disagree"]
MODES = {"prob": 0, "logit": 1}
GUARD = 8                                   # words in front of and behind the output buffer
SENTINEL = 0x7FC12345                       # a NaN pattern no kernel writes
BATCH, N_SPLIT, N_TWO_RANKS = 8, 11, 11     # whole-model tests: 8 rows per forward, 11 samples (S = 4 of two views: 4 + 4 + 3)
RANKS = [0, 0, 1, 4, 5, 0, 3, 6, 0, 2, 9]   # where the label of sample i stands in its combined row: 4 top-1 hits, 8 top-5 hits


def L():
    from cara_amd import _lib
    return _lib


def make_logits(S, V, C, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "flat":
        return torch.randn(S * V, C, generator=g) * 0.02
    if kind == "peaked":
        return torch.randn(S * V, C, generator=g) * 30.0
    lg = torch.randn(S, V, C, generator=g)                         # every view of a sample puts its weight on another class
    for v in range(V):
        lg[:, v, (3 * v + 1) % C] += 20.0
    return lg.reshape(S * V, C).contiguous()


def run_combine(lib, lg, V, mode, ldl, ldo, out_offset=0):
    """the kernel on ``lg`` [S*V, C] laid out with row stride ``ldl`` into rows of stride ``ldo`` that start ``out_offset`` floats
    behind a 16-byte boundary -> out [S, C] on the CPU; every word the kernel must not write is checked to be as it was filled"""
    rows, C = lg.shape
    S = rows // V
    src = torch.full((rows, ldl), 7.0e37, device=DEV)              # (what lies between the rows would wreck a sum that read it)
    src[:, :C] = lg.to(DEV)
    words = GUARD + out_offset + S * ldo + GUARD
    buf = torch.full((words,), SENTINEL, dtype=torch.int32, device=DEV)
    out = buf[GUARD + out_offset:GUARD + out_offset + S * ldo].view(S, ldo)
    status = lib.cara_eval_combine_views(L().ptr(src), ldl, S, V, C, MODES[mode], out.data_ptr(), ldo, L().stream())
    torch.cuda.synchronize()
    assert status == 0, status
    got = out[:, :C].clone().view(torch.float32).cpu()
    untouched = buf.clone()
    untouched[GUARD + out_offset:GUARD + out_offset + S * ldo].view(S, ldo)[:, :C] = SENTINEL
    assert bool((untouched == SENTINEL).all()), "a word outside the [S, classes] block was written"
    return got


def layouts(C):
    """(ldl, ldo, out_offset): packed rows; classes + 1 (every second row misaligned: the scalar path); rows padded to 16 bytes
    (the 16-byte loads with a scalar tail where classes % 4 != 0) into 16-byte aligned output rows"""
    up4 = (C + 3) // 4 * 4
    return [(C, C + 3, 0), (C + 1, C + 3, 1), (up4 + 4, up4 + 4, 0)]


@pytest.mark.parametrize("classes", CLASSES)
@pytest.mark.parametrize("mode", list(MODES))
def test_combine_views_holds_the_derived_bound_element_by_element(mode, classes):
    lib = L().lib()
    worst = 0.0
    for V in VIEWS:
        for S in SAMPLES:
            for k, kind in enumerate(KINDS):
                lg = make_logits(S, V, classes, kind, seed=1000 * classes + 10 * V + S + k)
                v, d = VM.combine_bound(lg, V, mode)
                want = EC.combine_views(lg, V, mode)
                assert torch.allclose(v, want, rtol=0, atol=1e-9 * max(1.0, float(want.abs().max())))
                for ldl, ldo, off in layouts(classes):
                    got = run_combine(lib, lg, V, mode, ldl, ldo, off)
                    ok, ratio = VM.hold(got, want, d)
                    assert bool(ok.all()), (mode, classes, V, S, kind, ldl, ldo, ratio, (~ok).nonzero()[:5].tolist())
                    worst = max(worst, ratio)
    print(f"combine_views [{mode}] {classes} classes: worst device error / derived bound {worst:.3f}")


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_combine_views_in_both_libraries_and_one_view(operands):
    lib = L().lib(operands)
    for mode in MODES:
        for C in (5, 397):
            lg = make_logits(5, 3, C, "disagree", seed=C)
            ok, ratio = VM.hold(run_combine(lib, lg, 3, mode, C, C + 3), *VM.combine_bound(lg, 3, mode))
            assert bool(ok.all()), (operands, mode, C, ratio)
    lg = make_logits(6, 1, 100, "peaked", seed=3)
    assert torch.equal(run_combine(lib, lg, 1, "logit", 100, 104), lg)              # one view: a copy, bit for bit
    ok, _ = VM.hold(run_combine(lib, lg, 1, "prob", 100, 104), *VM.combine_bound(lg, 1, "prob"))   # ... and log_softmax
    assert bool(ok.all())


def test_combine_views_minus_infinity_rule():
    lib = L().lib()
    S, V, C = 5, 4, 37
    lg = make_logits(S, V, C, "disagree", seed=11)
    lg.view(S, V, C)[:, :, 6] = -float("inf")          # probability zero in every view
    lg.view(S, V, C)[:, 1:3, 20] = -float("inf")       # ... and in two views only
    want, d = VM.combine_bound(lg, V, "prob")
    for ldl, ldo, off in layouts(C):
        got = run_combine(lib, lg, V, "prob", ldl, ldo, off)
        assert not bool(torch.isnan(got).any())
        assert bool((got[:, 6] == -float("inf")).all()) and bool(torch.isfinite(got[:, 20]).all())
        ok, ratio = VM.hold(got, want, d)
        assert bool(ok.all()), (ldl, ldo, ratio)


def test_combine_views_refusals_launch_nothing():
    lib = L().lib()
    S, V, C = 3, 4, 10
    src = torch.randn(S * V + 8, C, device=DEV)
    out = torch.full((S + 4, C), 3.5, device=DEV)
    p, q, st = src.data_ptr(), out.data_ptr(), L().stream()
    refused = {
        "logits NULL": (None, C, S, V, C, 0, q, C), "out NULL": (p, C, S, V, C, 0, None, C),
        "S < 1": (p, C, 0, V, C, 0, q, C), "V < 1": (p, C, S, 0, C, 0, q, C), "V > 16": (p, C, 1, 17, C, 0, q, C),
        "classes < 1": (p, C, S, V, 0, 0, q, C), "ldl < classes": (p, C - 1, S, V, C, 0, q, C),
        "ldo < classes": (p, C, S, V, C, 0, q, C - 1), "mode 2": (p, C, S, V, C, 2, q, C), "mode -1": (p, C, S, V, C, -1, q, C),
        "logits off by 2 bytes": (p + 2, C, S, V, C, 0, q, C), "out off by 2 bytes": (p, C, S, V, C, 0, q + 2, C),
        "out inside logits": (p, C, S, V, C, 0, p + 4 * C, C), "out == logits": (p, C, S, V, C, 1, p, C),
        "logits' last row ends inside out": (q - 4 * ((S * V - 1) * C + 1), C, S, V, C, 0, q, C),
    }
    before_out, before_src = out.clone(), src.clone()
    for what, (a, ldl, s, v, c, mode, o, ldo) in refused.items():
        assert lib.cara_eval_combine_views(a, ldl, s, v, c, mode, o, ldo, st) == 1, what
    torch.cuda.synchronize()
    assert torch.equal(out, before_out) and torch.equal(src, before_src)
    # the neighbours of the refused ranges are legal: out directly behind the last logit that is read
    legal = torch.full((S * V * C + S * C,), 3.5, device=DEV)
    assert lib.cara_eval_combine_views(legal.data_ptr(), C, S, V, C, 1, legal.data_ptr() + 4 * S * V * C, C, st) == 0
    assert lib.cara_eval_combine_views(p, C, 1, 16, C, 0, q, C, st) == 0
    torch.cuda.synchronize()


# ---- the whole model ---------------------------------------------------------------------------------------------------------------
def pixels_at(n, size, seed, classes=100):
    """uint8 images whose level and contrast vary per image and whose left half is brighter (a flip is another image), and labels"""
    g = torch.Generator().manual_seed(seed)
    level = torch.rand(n, 3, 1, 1, generator=g) * 140 + 40
    contrast = torch.rand(n, 1, 1, 1, generator=g) * 60 + 10
    px = torch.randn(n, 3, size, size, generator=g) * contrast + level
    px[..., :size // 2] += 25.0
    return px.clamp_(0, 255).to(torch.uint8), torch.randint(0, classes, (n,), generator=g)


@functools.lru_cache(maxsize=None)
def the_model():
    m = _model(2).eval()
    with torch.no_grad():
        m.head.weight.mul_(8.0)    # (a trained head is far from its std-0.02 initialisation: wider logits and margins)
    return m


def model_and_split(n, size=256, seed=31):
    from cara_amd.data import ResidentSplit
    px, labels = pixels_at(n, size, seed)
    return the_model(), ResidentSplit.from_tensors(px.to(DEV), labels.to(DEV))


def same_dict(a, b):
    """two returned dicts hold the same keys and, bit for bit, the same values (a NaN equals a NaN: per_class without support)"""
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            same_dict(a[k], b[k])
        elif torch.is_tensor(a[k]):
            x, y = (torch.nan_to_num(t.double(), nan=-1.0) for t in (a[k], b[k]))
            assert torch.equal(x, y), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (k, a[k], b[k])


@pytest.mark.parametrize("report", [False, True])
def test_identity_views_are_the_plain_pass_bit_for_bit(report):
    from cara_amd.data import EvalViews, ResidentSplit
    m, split = model_and_split(N_SPLIT, size=224)
    eng = m._cara_engine
    plain = eng.evaluate(split, BATCH, report=report)
    assert plain["n"] == N_SPLIT
    same_dict(eng.evaluate(split, BATCH, report=report, views=EvalViews.resize(224)), plain)
    same_dict(eng.evaluate(split, BATCH, report=report, views=EvalViews.resize(224), combine="logit"), plain)
    # the flipped view of resize(flip=True) alone, as a one-row hand table, is the plain pass over the mirrored pixels
    flipped = EvalViews(EvalViews.resize(224, flip=True).table(224, 224)[1:])
    mirrored = ResidentSplit.from_tensors(split.pixels.flip(-1).contiguous(), split.labels)
    want = eng.evaluate(mirrored, BATCH, report=report)
    same_dict(eng.evaluate(split, BATCH, report=report, views=flipped), want)
    assert want["loss"] != plain["loss"]                     # (the mirror image is another image to this model)


def collect(eng, split, views, **kw):
    seen = []
    out = eng.evaluate(split, BATCH, views=views, **kw,
                       debug_hook=lambda lg, lb, nv, comb: seen.append((lg.clone(), lb.clone(), nv, comb.clone())))
    return out, seen


@pytest.mark.parametrize("combine", ["prob", "logit"])
def test_centre_crop_and_flip_against_forward_resident_and_the_host_model(combine):
    from cara_amd.data import EvalViews, ResidentSplit
    m, split = model_and_split(N_SPLIT)
    eng = m._cara_engine
    views = EvalViews.center(224, flip=True)
    # labels that make hits and misses on both sides of both boundaries: sample i is labelled with the class the host model ranks
    # RANKS[i]-th on its combined row (the logits do not depend on the labels: a first pass gives them)
    _, first = collect(eng, split, views, combine=combine)
    rows_of = torch.cat([EC.combine_views(lg.cpu(), 2, combine)[:nv] for lg, _, nv, _ in first])
    order = rows_of.argsort(dim=1, descending=True, stable=True)
    split = ResidentSplit.from_tensors(split.pixels, order[torch.arange(N_SPLIT), torch.tensor(RANKS)].to(DEV))
    out, seen = collect(eng, split, views, combine=combine)
    assert out["n"] == N_SPLIT and [nv for _, _, nv, _ in seen] == [4, 4, 3] and all(lg.shape[0] == BATCH for lg, _, _, _ in seen)
    assert round(out["top1"] * N_SPLIT) == sum(r == 0 for r in RANKS) and round(out["top5"] * N_SPLIT) == sum(r < 5 for r in RANKS)
    batches = list(split.eval_view_shard(views.table(256, 256), BATCH, 0, 1))
    assert batches[0][1].tolist() == [[16, 16, 224, 224, 0], [16, 16, 224, 224, 1]] * 4
    want, bound, margin, ratio = EC.new_state(), 0.0, float("inf"), 0.0
    for (lg, lb, nv, comb), (rows, boxes, labels, n_valid) in zip(seen, batches):
        assert nv == n_valid and torch.equal(lb, labels)
        assert torch.equal(lg, eng.forward_resident(split, rows, boxes=boxes)), "per-view logits differ from forward_resident"
        v, d = VM.combine_bound(lg, 2, combine)
        host = EC.combine_views(lg.cpu(), 2, combine)
        ok, r = VM.hold(comb, host, d)
        assert bool(ok.all()), r
        ratio = max(ratio, r)
        EC.accumulate(want, host, lb.cpu(), nv)
        m1, m5 = VM.boundary_margins(host[:nv], lb.cpu()[:nv])
        margin = min(margin, float(torch.minimum(m1, m5).min()) / (2.0 * float(d[:nv].max())))
        bound += VM.loss_bound(host[:nv], d[:nv], lb.cpu()[:nv]) * nv
    # the precondition of exact counts: every sample's top-1 and top-5 boundary margins exceed twice the kernel bound
    print(f"[{combine}] smallest boundary margin / (2 x bound) {margin:.3e}; combine error / bound {ratio:.3f}")
    assert margin > 1.0, "choose another seed for the split: a sample sits on a top-1 / top-5 boundary"
    r = EC.result(want)
    bound /= N_SPLIT
    print(f"[{combine}] evaluate {out}; host model {r}; |loss difference| {abs(out['loss'] - r['loss']):.3e}, bound {bound:.3e}")
    assert round(out["top1"] * N_SPLIT) == int(want[EC.TOP1]) and round(out["top5"] * N_SPLIT) == int(want[EC.TOP5])
    assert abs(out["loss"] - r["loss"]) <= bound


def test_padded_samples_change_nothing():
    """11 samples in batches of four: the last batch holds one copy of its first sample, which no counter sees"""
    from cara_amd.data import EvalViews
    m, split = model_and_split(N_SPLIT)
    out, seen = collect(m._cara_engine, split, EvalViews.center(224, flip=True))
    assert out["n"] == len(split) == N_SPLIT
    want = EC.new_state()
    for lg, lb, nv, comb in seen:
        EC.accumulate(want, comb.cpu(), lb.cpu(), nv)            # the device's combined rows: the counts are then exact
    assert torch.equal(seen[2][0][6:8], seen[2][0][0:2])         # the padding is the batch's first sample
    r = EC.result(want)
    assert [round(out["top1"] * N_SPLIT), round(out["top5"] * N_SPLIT)] == [int(want[EC.TOP1]), int(want[EC.TOP5])]
    assert abs(out["loss"] - r["loss"]) <= LOSS_REL * abs(r["loss"])
    # the same eight first samples as a split whose length the batch divides: the first two batches above, bit for bit
    from cara_amd.data import ResidentSplit
    split8 = ResidentSplit.from_tensors(split.pixels[:8].contiguous(), split.labels[:8].contiguous())
    out8, seen8 = collect(m._cara_engine, split8, EvalViews.center(224, flip=True))
    assert out8["n"] == 8 and [nv for _, _, nv, _ in seen8] == [4, 4]
    assert all(torch.equal(a[3], b[3]) and torch.equal(a[0], b[0]) for a, b in zip(seen[:2], seen8))


def test_ten_crop_one_sample_per_batch_and_too_many_views():
    from cara_amd._lib import CaraError
    from cara_amd.data import EvalViews
    m, split = model_and_split(3)
    eng = m._cara_engine
    seen = []
    out = eng.evaluate(split, 10, views=EvalViews.ten_crop(224),
                       debug_hook=lambda lg, lb, nv, comb: seen.append((lg.clone(), lb.clone(), nv, comb.clone())))
    assert out["n"] == 3 and len(seen) == 3 and all(lg.shape[0] == 10 and comb.shape[0] == 1 and nv == 1 for lg, _, nv, comb in seen)
    for lg, lb, nv, comb in seen:
        ok, ratio = VM.hold(comb, EC.combine_views(lg.cpu(), 10, "prob"), VM.combine_bound(lg, 10, "prob")[1])
        assert bool(ok.all()), ratio
    with pytest.raises(CaraError, match="no whole sample"):
        eng.evaluate(split, 9, views=EvalViews.ten_crop(224))
    with pytest.raises(CaraError, match="outside"):
        eng.evaluate(split, 10, views=EvalViews([[40, 0, 224, 224, 0]]))


def test_views_on_the_averaged_weights():
    """weights=ema with views == the model evaluated with the shadows swapped in, with views"""
    from cara_amd.data import EvalViews
    m, split = model_and_split(N_SPLIT)
    eng = m._cara_engine
    ema = eng.make_ema(0.5)
    with torch.no_grad():
        for i, s in enumerate(ema.tensors):                      # shadows that are not the parameters
            s.mul_(1.0 + 0.05 * ((i % 3) - 1)).add_(1e-3)
    views = EvalViews.center(224, flip=True)
    raw = eng.evaluate(split, BATCH, views=views)
    avg = eng.evaluate(split, BATCH, views=views, weights=ema)
    with ema.swapped_in():
        want = eng.evaluate(split, BATCH, views=views)
    assert avg == want and avg["loss"] != raw["loss"]
    assert eng.evaluate(split, BATCH, views=views) == raw         # the parameters were not touched


def test_views_two_ranks_on_one_gpu_return_the_same_dict(tmp_path):
    from cara_amd.data import EvalViews
    from tests.test_eval_shard import _free_port
    out = str(tmp_path / "ev")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_eval_views_two_ranks.py"), str(r), "2", out], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), logs
    a, b = (json.load(open(f"{out}.{r}.json")) for r in range(2))
    assert a == b and a["n"] == N_TWO_RANKS and a["samples"] == [8, 3]
    m, split = model_and_split(N_TWO_RANKS)
    one = m._cara_engine.evaluate(split, BATCH, views=EvalViews.center(224, flip=True))
    print(f"two ranks {a}; one rank {one}")
    assert (a["n"], a["top1"], a["top5"]) == (one["n"], one["top1"], one["top5"])
    assert abs(a["loss"] - one["loss"]) <= 1e-12 * abs(one["loss"])   # (two fp64 partial sums instead of one)


def test_fit_scores_the_evaluation_epochs_through_the_views():
    from cara_amd import cara, create_model
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
    evals = []

    def on_eval(epoch, acc):
        direct = m._cara_engine.evaluate(split, 256, views=views)
        evals.append((epoch, acc, direct["top1"], direct["n"]))
    # (the schedule evaluates every tenth epoch: eleven epochs are the shortest run that does)
    best, _ = fit(m, lambda epoch: [(x, y.to(DEV))], split, epochs=11, lr=1e-2, seed=3, on_eval=on_eval, eval_mode="sharded",
                  eval_views=views)
    print(evals)
    assert [e for e, _, _, _ in evals] == [10] and evals[0][1] == evals[0][2] == best and evals[0][3] == 16
    mpc, _ = fit(m, lambda epoch: [(x, y.to(DEV))], split, epochs=11, lr=1e-3, seed=3, eval_mode="sharded", eval_views=views,
                 eval_combine="logit", eval_metric="mean_per_class")
    assert 0.0 <= mpc <= 1.0
