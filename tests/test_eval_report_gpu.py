"""GPU side of the evaluation report: cara_eval_accumulate_report against its host model (cara_amd/evalcount.py) -- integers
exactly, the fp64 confidence sums inside the guard band of docs/findings/eval_report.md --, the exact bin edges, the argument
checks, the plain entry beside it, CaraEngine.evaluate(report=True) in both precisions and on an EMA, two ranks on one GPU, and
fit(eval_metric="mean_per_class")."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from cara_amd import evalcount as EC
from tests.test_eval_gpu import LOSS_REL, _model, _pixels

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = [2, 5, 37, 100, 397, 1000]
SHAPES = [(1, 1), (64, 64), (96, 77), (300, 211)]          # (B, n_valid)
BINS = [1, 15, 64]
SEED = 2                                                      # of report_table: chosen so that no confidence sits in a guard band
INTS = [EC.N, EC.TOP1, EC.TOP5, EC.BAD]


def guard(classes):
    """|conf_kernel - conf_fp64| of one row, from the kernel's own summation order (docs/findings/eval_report.md): C/64 sequential
    fp32 adds per lane, six shuffle levels, the ulps of expf, of the subtraction in front of it and of the reciprocal -- doubled."""
    return (classes / 64 + 16) * 2.0 ** -23


def L():
    from cara_amd import _lib
    return _lib


def report_table(classes, B, seed):
    """random logits (sigma 3) with planted EXACT ties in every third row, at the row maximum or at the label's value, over at most
    classes - 1 columns: a tie over ALL columns makes the confidence exactly 1 / classes, which can be a bin edge (the exact edges
    have their own test).  Two classes: no planted tie for that reason."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * classes + B)
    logits = torch.randn(B, classes, generator=g) * 3.0
    labels = torch.randint(0, classes, (B,), generator=g)
    if classes > 2:
        for b in range(0, B, 3):
            k = int(torch.randint(1, min(classes - 2, 7) + 1, (1,), generator=g))
            others = [c for c in torch.randperm(classes, generator=g).tolist() if c != int(labels[b])][:k]
            top = bool(torch.rand(1, generator=g) < 0.5)
            v = float(logits[b].max() + 1.0 if top else logits[b, labels[b]])
            logits[b, others] = v
            logits[b, labels[b]] = v
    return logits, labels


def edge_distance(logits, labels, n_valid, bins):
    """smallest distance of a scored row's fp64 confidence to an interior bin edge k / bins (inf with one bin)"""
    l = logits[:n_valid].double()
    ok = (labels[:n_valid] >= 0) & (labels[:n_valid] < l.shape[1])
    conf = torch.exp(l[ok].max(1).values - torch.logsumexp(l[ok], 1))
    if bins == 1 or conf.numel() == 0:
        return math.inf
    edges = torch.arange(1, bins, dtype=torch.float64) / bins
    return float((conf.view(-1, 1) - edges.view(1, -1)).abs().min())


def kernel_report(launches, classes, bins, lib=None, ldl=None):
    """state and report after cara_eval_accumulate_report over [(logits, labels, n_valid)] -> (float64 [5], evalcount report)"""
    lib = lib or L().lib()
    words = int(lib.cara_eval_report_bytes(classes, bins)) // 8
    assert words == EC.report_words(classes, bins)
    st = torch.zeros(5, dtype=torch.int64, device=DEV)
    rep = torch.zeros(words, dtype=torch.int64, device=DEV)
    for lg, lb, nv in launches:
        lg, lb = lg.to(DEV).contiguous(), lb.to(DEV)
        L().check(lib.cara_eval_accumulate_report(L().ptr(lg), ldl or lg.shape[1], L().ptr(lb), lg.shape[0], nv, classes, L().ptr(st),
                                                  L().ptr(rep), bins, L().stream()), "cara_eval_accumulate_report")
    torch.cuda.synchronize()
    return _host_state(st), _host_report(rep, classes, bins)


def _host_state(st):
    out = st.cpu().to(torch.float64)
    out[EC.LOSS] = st.cpu().view(torch.float64)[EC.LOSS]
    return out


def _host_report(rep, classes, bins):
    vec = rep.cpu().to(torch.float64)
    vec[-bins:] = rep.cpu().view(torch.float64)[-bins:]
    return EC.report_from_vector(vec, classes, bins)


def model_report(launches, classes, bins):
    st, rep = EC.new_state(), EC.new_report(classes, bins)
    for lg, lb, nv in launches:
        EC.accumulate_report(st, rep, lg, lb, nv)
    return st, rep


def same_report(got, want, classes, what):
    (gs, gr), (ws, wr) = got, want
    print(f"{what}: state kernel {gs.tolist()} model {ws.tolist()}; bin_count {gr['bin_count'].tolist()}")
    assert [int(v) for v in gs[INTS]] == [int(v) for v in ws[INTS]], what
    assert abs(float(gs[EC.LOSS]) - float(ws[EC.LOSS])) <= LOSS_REL * abs(float(ws[EC.LOSS])), (what, float(gs[EC.LOSS]), float(ws[EC.LOSS]))
    for k in ("confusion", "bin_count", "bin_hits"):
        assert torch.equal(gr[k], wr[k]), (what, k, (gr[k] != wr[k]).nonzero()[:10].tolist())
    err = (gr["bin_conf"] - wr["bin_conf"]).abs()
    bound = wr["bin_count"] * guard(classes)
    print(f"{what}: bin_conf error / (n_b g) at worst {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), (what, err.tolist(), bound.tolist())


def checked(launches, classes, bins, what):
    """the launches, after the CPU check that no scored row's fp64 confidence lies within the guard band of a bin edge"""
    for lg, lb, nv in launches:
        d = edge_distance(lg, lb, nv, bins)
        assert d > guard(classes), f"{what}: a confidence lies {d:.3e} from a bin edge (guard band {guard(classes):.3e}): pick another SEED"
    return launches


# ---- 1. the kernel against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", CLASSES)
def test_report_kernel_against_the_model(classes):
    for B, nv in SHAPES:
        lg, lb = report_table(classes, B, SEED)
        for bins in BINS:
            what = f"{classes} classes, B {B}, n_valid {nv}, {bins} bins"
            launches = checked([(lg, lb, nv)], classes, bins, what)
            same_report(kernel_report(launches, classes, bins), model_report(launches, classes, bins), classes, what)


# ---- 2. exact edges ----------------------------------------------------------------------------------------------------------
def test_report_exact_edges_clamp_and_contention():
    for classes in (2, 4):
        lg, lb = torch.zeros(8, classes), torch.arange(8) % classes
        want = model_report([(lg, lb, 8)], classes, classes)
        assert float(want[1]["bin_count"][1]) == 8.0 and float(want[1]["bin_conf"][1]) == 8.0 / classes   # 1 / C: the edge, upper bin
        gs, gr = kernel_report([(lg, lb, 8)], classes, classes)
        assert all(torch.equal(gr[k], want[1][k]) for k in EC.REPORT_KEYS), (classes, gr)          # (bin_conf too: sums of 1 / C)
        assert [int(v) for v in gs[INTS]] == [int(v) for v in want[0][INTS]]
    for classes, bins in ((5, 15), (100, 64), (37, 1)):
        lg = torch.zeros(6, classes)
        lg[:, 3] = 80.0                                                      # conf rounds to 1 in fp32: (int)(1 * bins) is clamped
        lb = torch.tensor([3, 0, 3, 3, 1, 3])
        want = model_report([(lg, lb, 6)], classes, bins)
        assert float(want[1]["bin_count"][bins - 1]) == 6.0 and float(want[1]["bin_conf"][bins - 1]) == 6.0
        gs, gr = kernel_report([(lg, lb, 6)], classes, bins)
        assert all(torch.equal(gr[k], want[1][k]) for k in EC.REPORT_KEYS), (classes, bins, gr)
    # 300 rows on one (label, pred) cell and one bin: 75 waves' worth of adds to three LDS words and one confusion cell
    row = torch.tensor([0.5, -1.0, 2.0, 0.0, 2.0])                            # pred 2 (tie with 4), conf = 0.41: bin 6 of 15
    lg, lb = row.repeat(300, 1), torch.full((300,), 4)
    launches = checked([(lg, lb, 300)], 5, 15, "contention")
    got, want = kernel_report(launches, 5, 15), model_report(launches, 5, 15)
    same_report(got, want, 5, "300 rows on one cell")
    assert float(got[1]["confusion"][4, 2]) == 300.0 and float(got[1]["bin_count"][6]) == 300.0 and float(got[1]["bin_hits"].sum()) == 0.0


# ---- 3. state and arguments --------------------------------------------------------------------------------------------------
def test_report_over_launches_bad_labels_and_strided_rows():
    lg, lb = report_table(37, 300, SEED)
    parts = checked([(lg[:100], lb[:100], 100), (lg[100:200], lb[100:200], 60), (lg[200:], lb[200:], 100)], 37, 15, "three launches")
    same_report(kernel_report(parts, 37, 15), model_report(parts, 37, 15), 37, "three launches into one report")
    bad = lb.clone()
    bad[3], bad[150], bad[299] = 37, -1, 1 << 40
    launches = checked([(lg, bad, 300)], 37, 15, "bad labels")
    got, want = kernel_report(launches, 37, 15), model_report(launches, 37, 15)
    assert int(got[0][EC.BAD]) == 3 and int(got[1]["confusion"].sum()) == 297
    same_report(got, want, 37, "three labels out of range")
    # rows 41 floats apart: not 16-byte aligned
    g = torch.Generator().manual_seed(41)
    wide = torch.randn(64, 41, generator=g) * 3.0
    launches = checked([(wide[:, :37].contiguous(), lb[:64], 64)], 37, 15, "row stride 41")
    same_report(kernel_report([(wide, lb[:64], 64)], 37, 15, ldl=41), model_report(launches, 37, 15), 37, "row stride 41")


def test_report_refusals_leave_the_report_untouched_and_byte_counts():
    lib = L().lib()
    rb = lib.cara_eval_report_bytes
    assert int(rb(1, 1)) == 8 * 4 and int(rb(100, 15)) == 8 * (100 * 100 + 45) and int(rb(4096, 64)) == 8 * (4096 * 4096 + 192)
    assert [int(rb(c, b)) for c, b in ((4097, 15), (0, 15), (-1, 15), (10, 0), (10, 65), (10, -1))] == [0] * 6
    assert int(L().lib("fp16").cara_eval_report_bytes(37, 15)) == int(rb(37, 15)) == 8 * (37 * 37 + 45)
    SENT = 0x5A5A5A5A5A5A5A5A
    lg = torch.randn(64, 41).to(DEV)
    y = (torch.arange(64) % 37).to(DEV)
    st = torch.full((5,), SENT, dtype=torch.int64, device=DEV)
    rep = torch.full((37 * 37 + 3 * 64 + 1,), SENT, dtype=torch.int64, device=DEV)
    big = torch.zeros(2, 4097, device=DEV)
    P, S = L().ptr, L().stream()
    odd = P(rep).value + 4
    call = lib.cara_eval_accumulate_report
    refused = {
        "classes above the cap": call(P(big), 4097, P(y), 2, 2, 4097, P(st), P(rep), 15, S),
        "bins 0": call(P(lg), 41, P(y), 64, 64, 37, P(st), P(rep), 0, S),
        "bins -3": call(P(lg), 41, P(y), 64, 64, 37, P(st), P(rep), -3, S),
        "bins 65": call(P(lg), 41, P(y), 64, 64, 37, P(st), P(rep), 65, S),
        "report NULL": call(P(lg), 41, P(y), 64, 64, 37, P(st), None, 15, S),
        "report not 8-byte aligned": call(P(lg), 41, P(y), 64, 64, 37, P(st), odd, 15, S),
        "n_valid > B": call(P(lg), 41, P(y), 64, 65, 37, P(st), P(rep), 15, S),
        "ldl < classes": call(P(lg), 36, P(y), 64, 64, 37, P(st), P(rep), 15, S),
        "state NULL": call(P(lg), 41, P(y), 64, 64, 37, None, P(rep), 15, S),
        "logits NULL": call(None, 41, P(y), 64, 64, 37, P(st), P(rep), 15, S),
        "labels NULL": call(P(lg), 41, None, 64, 64, 37, P(st), P(rep), 15, S),
        "B 0": call(P(lg), 41, P(y), 0, 0, 37, P(st), P(rep), 15, S),
        "classes 0": call(P(lg), 41, P(y), 64, 64, 0, P(st), P(rep), 15, S),
    }
    torch.cuda.synchronize()
    assert all(v == 1 for v in refused.values()), refused
    assert bool((rep == SENT).all()) and bool((st == SENT).all())
    assert call(P(lg), 41, P(y), 64, 0, 37, P(st), P(rep), 15, S) == 0          # n_valid 0: accepted, nothing to add
    torch.cuda.synchronize()
    assert bool((rep == SENT).all()) and bool((st == SENT).all())


# ---- 4. the plain entry beside it --------------------------------------------------------------------------------------------
def test_plain_entry_and_report_entry_count_the_same():
    from tests.test_eval_gpu import kernel_counts
    for operands in ("bf16", "fp16"):
        lib = L().lib(operands)
        for classes in (5, 397):
            lg, lb = report_table(classes, 300, SEED + 1)
            lb[7] = classes
            launches = [(lg[:100], lb[:100], 77), (lg[100:], lb[100:], 200)]
            plain = kernel_counts(launches, classes, lib)
            with_report, _ = kernel_report(launches, classes, 15, lib)
            assert [int(v) for v in plain[INTS]] == [int(v) for v in with_report[INTS]] and int(plain[EC.N]) == 276
            assert abs(float(plain[EC.LOSS]) - float(with_report[EC.LOSS])) <= 1e-12 * abs(float(plain[EC.LOSS]))   # (the fp64 sum's order)


# ---- 5. the engine -----------------------------------------------------------------------------------------------------------
def _engine_case(precision, with_ema):
    m = _model(2, precision, num_classes=7).eval()
    with torch.no_grad():
        m.head.weight.mul_(10.0)       # (the synthetic head's logits are narrow: spread the confidences over the bins)
    eng = m._cara_engine
    px, labels = _pixels(150, seed=33, classes=7)
    from cara_amd.data import ResidentSplit
    split = ResidentSplit.from_tensors(px.to(DEV), labels.to(DEV))
    ema = None
    if with_ema:
        ema = eng.make_ema(0.9)
        g = torch.Generator().manual_seed(2)
        with torch.no_grad():
            for t in ema.tensors:          # an average that is not the model: another set of logits
                t.add_((torch.randn(t.shape, generator=g) * 0.05).to(DEV) * t.abs().mean())
    return m, eng, split, ema


def _check_engine(eng, split, ema, bins):
    seen = []
    out = eng.evaluate(split, 64, weights=ema, report=True, bins=bins,
                       debug_hook=lambda lg, lb, nv: seen.append((lg.cpu().clone(), lb.cpu().clone(), nv)))
    assert [nv for _, _, nv in seen] == [64, 64, 22]
    launches = checked(seen, 7, bins, "engine")
    st, rep = model_report(launches, 7, bins)
    want = EC.report_result(st, rep)
    print(f"evaluate(report=True): top1 {out['top1']:.4f} mean_per_class {out['mean_per_class']:.4f} ece {out['ece']:.4f} "
          f"count {out['calibration']['count'].tolist()}")
    assert out["n"] == want["n"] == 150 and out["top1"] == want["top1"] and out["top5"] == want["top5"]
    assert abs(out["loss"] - want["loss"]) <= LOSS_REL * abs(want["loss"])
    for k in ("confusion", "support"):
        assert out[k].dtype == torch.int64 and out[k].device.type == "cpu" and torch.equal(out[k], want[k]), k
    for k in ("per_class", "precision"):
        assert out[k].dtype == torch.float64 and torch.equal(out[k].nan_to_num(-1.0), want[k].nan_to_num(-1.0)), k
    assert out["mean_per_class"] == want["mean_per_class"]
    cal, wcal = out["calibration"], want["calibration"]
    assert torch.equal(cal["count"], wcal["count"]) and torch.equal(cal["hits"], wcal["hits"]) and len(cal["confidence"]) == bins
    assert bool(((cal["confidence"] - wcal["confidence"]).abs() <= wcal["count"] * guard(7)).all())
    assert abs(out["ece"] - want["ece"]) <= guard(7)          # sum_b n_b / n * (an error of at most n_b g / n_b)
    return out


def test_evaluate_report_against_the_model_on_the_hooked_logits():
    from cara_amd._lib import CaraError
    m, eng, split, _ = _engine_case("bf16", False)
    out = _check_engine(eng, split, None, 15)
    assert int((out["calibration"]["count"] > 0).sum()) >= 3, "the confidences should spread over several bins"
    plain = eng.evaluate(split, 64)
    assert set(plain) == {"top1", "top5", "loss", "n"}
    assert (plain["top1"], plain["top5"], plain["n"]) == (out["top1"], out["top5"], out["n"])
    assert abs(plain["loss"] - out["loss"]) <= 1e-12 * abs(plain["loss"])
    assert set(out) == {"top1", "top5", "loss", "n", "confusion", "support", "per_class", "precision", "mean_per_class", "ece", "calibration"}
    _check_engine(eng, split, None, 64)
    for bins in (0, 65, 2.5):
        with pytest.raises(CaraError):
            eng.evaluate(split, 64, report=True, bins=bins)


def test_evaluate_report_in_fp16():
    _, eng, split, _ = _engine_case("fp16", False)
    _check_engine(eng, split, None, 15)


def test_evaluate_report_on_an_ema():
    _, eng, split, ema = _engine_case("bf16", True)
    averaged = _check_engine(eng, split, ema, 15)
    raw = eng.evaluate(split, 64, report=True)
    assert not torch.equal(raw["calibration"]["confidence"], averaged["calibration"]["confidence"])   # the shadows were scored


def test_evaluate_report_refuses_a_head_wider_than_the_cap():
    from cara_amd._lib import CaraError
    m = _model(2, num_classes=4097).eval()
    forwards = []

    def batches():
        forwards.append(1)
        return iter(())
    with pytest.raises(CaraError, match="4097 classes"):
        m._cara_engine.evaluate(batches, report=True)
    assert not forwards and not m._cara_engine.__dict__.get("_eval_ws")      # refused before any batch was asked for


# ---- 6. two ranks on one GPU -------------------------------------------------------------------------------------------------
def test_two_ranks_on_one_gpu_return_the_one_rank_report(tmp_path):
    """both ranks on cuda:0 over gloo, fresh child processes, each under its own time limit; the one-rank dict is this process's"""
    from tests import _eval_report_two_ranks as H
    from tests.test_eval_shard import _free_port
    out = str(tmp_path / "rep")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_eval_report_two_ranks.py"), str(r), "2", out], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), logs
    a, b = (json.load(open(f"{out}.{r}.json")) for r in range(2))
    assert a == b and a["batches"] == [3, 2]                                  # 300 images at batch 64: 192 + 108
    one = H.as_json(H.score(None))
    print({k: one[k] for k in ("top1", "top5", "loss", "n", "mean_per_class", "ece")})
    assert a["n"] == one["n"] == 300
    for k in ("top1", "top5", "confusion", "support", "per_class", "precision", "mean_per_class"):
        assert a[k] == one[k], k
    assert a["calibration"]["count"] == one["calibration"]["count"] and a["calibration"]["hits"] == one["calibration"]["hits"]
    # the fp64 sums arrive in another order: the loss, the bins' confidence sums and what is formed from them
    assert abs(a["loss"] - one["loss"]) <= 1e-12 * abs(one["loss"]) and abs(a["ece"] - one["ece"]) <= 1e-12
    assert all(abs(x - y) <= 1e-12 * max(abs(y), 1.0) for x, y in zip(a["calibration"]["confidence"], one["calibration"]["confidence"]))


# ---- 7. fit ------------------------------------------------------------------------------------------------------------------
def test_fit_with_mean_per_class_as_the_metric(tmp_path):
    from cara_amd import cara, create_model
    from cara_amd._lib import CaraError
    from cara_amd.data import ResidentSplit, normalize_u8
    from cara_amd.recipe import checkpoint_name, fit
    g = torch.Generator().manual_seed(1)
    y = torch.arange(16) % 4
    px = (torch.randn(16, 3, 224, 224, generator=g) * 20 + 40 + 50 * y.float().reshape(-1, 1, 1, 1)).clamp_(0, 255).to(torch.uint8)
    x, px, y = normalize_u8(px).to(DEV), px.to(DEV), y.to(DEV)
    # the test split is imbalanced (4 + 3 + 2 + 2 images of the four classes) and its last image is one of class 0 filed under
    # class 3, which a model that has learnt the levels misses: the two metrics weigh that miss differently (7 / 8 against 10 / 11)
    pick = torch.tensor([0, 4, 8, 12, 1, 5, 9, 2, 6, 3, 0], device=DEV)
    filed = y[pick].clone()
    filed[-1] = 3
    split = ResidentSplit.from_tensors(px[pick].contiguous(), filed)
    torch.manual_seed(0)
    m = cara({"model": create_model("vit_base_patch16_224_in21k", depth=2, num_classes=4, drop_path_rate=0.1), "rank": 8,
              "scale": 1.0, "l_mu": 1.0, "l_std": 0.0}).to(DEV)
    with pytest.raises(CaraError, match="eval_metric"):
        fit(m, lambda epoch: [(x, y)], lambda: [(x, y)], epochs=1, eval_metric="mean_per_class", eval_mode="reference")
    evals = []

    def on_eval(epoch, acc):
        r = m._cara_engine.evaluate(split, 256, report=True)                 # the model as it was scored
        evals.append((epoch, acc, r["mean_per_class"], r["top1"]))
    save_best = {"dataset": "imbalanced", "seed": 3, "dir": str(tmp_path)}
    best, _ = fit(m, lambda epoch: [(x, y)], split, epochs=21, lr=1e-2, seed=3, on_eval=on_eval, eval_mode="sharded",
                  eval_metric="mean_per_class", save_best=save_best)
    print(f"(epoch, on_eval value, mean_per_class, top1): {evals}")
    assert [e for e, _, _, _ in evals] == [10, 20] and all(acc == mpc for _, acc, mpc, _ in evals)
    assert best == max(acc for _, acc, _, _ in evals) and best > 0.0
    assert any(mpc != top1 for _, _, mpc, top1 in evals), "the split should tell the two metrics apart"
    assert save_best["path"] == checkpoint_name("imbalanced", best, 3, str(tmp_path)) and os.path.exists(save_best["path"])
    assert os.listdir(str(tmp_path)) == [os.path.basename(save_best["path"])]
