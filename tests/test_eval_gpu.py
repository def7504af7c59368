"""GPU side of the device-resident, rank-sharded evaluation: the counting kernel against cara_amd/evalcount.py, the uint8 patch
kernel against cara_im2col_patches on the CPU-normalised image (bitwise), the inference-sized workspace, and
CaraEngine.evaluate / fit(eval_mode="sharded") against the existing path (model(x), recipe.evaluate)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from cara_amd import evalcount as EC
from tests import tolerances as T
from tests.test_eval_shard import CLASSES, table

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# cara_vit_workspace_bytes of the commit before the inference-sized layout, ViT-B/16 batch 64, 100 classes (bench.py's shapes)
PARENT_WS_BYTES = {16: 4918791680, 64: 5255920128}
LOSS_REL = 1.0e-6   # the kernel sums rows in fp64: what is left is the fp32 log-sum-exp of a row (a few 2^-24 of |lse|)


def L():
    from cara_amd import _lib
    return _lib


def kernel_counts(launches, classes, lib=None):
    """state after cara_eval_accumulate over [(logits, labels, n_valid)] -> float64 [5] like evalcount's"""
    lib = lib or L().lib()
    assert int(lib.cara_eval_state_bytes()) == 40
    st = torch.zeros(5, dtype=torch.int64, device=DEV)
    for lg, lb, nv in launches:
        lg, lb = lg.to(DEV).contiguous(), lb.to(DEV)
        L().check(lib.cara_eval_accumulate(L().ptr(lg), lg.shape[1], L().ptr(lb), lg.shape[0], nv, classes, L().ptr(st),
                                           L().stream()), "cara_eval_accumulate")
    torch.cuda.synchronize()
    out = st.cpu().to(torch.float64)
    out[3] = st.cpu().view(torch.float64)[3]
    return out


def same_counts(got, want, what):
    print(f"{what}: kernel {got.tolist()} fallback {want.tolist()}")
    assert [int(v) for v in got[[0, 1, 2, 4]]] == [int(v) for v in want[[0, 1, 2, 4]]], what
    assert abs(float(got[3]) - float(want[3])) <= LOSS_REL * abs(float(want[3])), (what, float(got[3]), float(want[3]))


@pytest.mark.parametrize("classes", CLASSES)
def test_eval_accumulate_against_the_fallback(classes):
    for B, nv in [(1, 1), (64, 64), (96, 77), (256, 256), (300, 211)]:
        if classes == 21843 and B > 96:
            continue   # (26 MB of logits per launch is enough for the widest head)
        lg, lb = table(classes, B, seed=classes + B)
        same_counts(kernel_counts([(lg, lb, nv)], classes), EC.accumulate(EC.new_state(), lg, lb, nv), f"{classes} classes, B {B}, n_valid {nv}")


def test_eval_accumulate_over_launches_bad_labels_and_strided_rows():
    lg, lb = table(37, 300, seed=5)
    parts = [(lg[:100], lb[:100], 100), (lg[100:200], lb[100:200], 60), (lg[200:], lb[200:], 100)]
    want = EC.new_state()
    for p in parts:
        EC.accumulate(want, *p)
    same_counts(kernel_counts(parts, 37), want, "three launches into one state")
    bad = lb.clone()
    bad[3], bad[150], bad[299] = 37, -1, 1 << 40
    got = kernel_counts([(lg, bad, 300)], 37)
    assert int(got[4]) == 3
    same_counts(got, EC.accumulate(EC.new_state(), lg, bad), "three labels out of range")
    # rows 41 floats apart (ldl > classes: rows not 16-byte aligned), and the argument checks
    lib = L().lib()
    wide = torch.randn(64, 41).to(DEV)
    st = torch.zeros(5, dtype=torch.int64, device=DEV)
    y = lb[:64].to(DEV)
    L().check(lib.cara_eval_accumulate(L().ptr(wide), 41, L().ptr(y), 64, 64, 37, L().ptr(st), L().stream()), "cara_eval_accumulate")
    torch.cuda.synchronize()
    got = st.cpu().to(torch.float64)
    got[3] = st.cpu().view(torch.float64)[3]
    same_counts(got, EC.accumulate(EC.new_state(), wide[:, :37].cpu(), lb[:64]), "row stride 41")
    assert lib.cara_eval_accumulate(L().ptr(wide), 41, L().ptr(y), 64, 65, 37, L().ptr(st), L().stream()) == 1   # n_valid > B
    assert lib.cara_eval_accumulate(L().ptr(wide), 36, L().ptr(y), 64, 64, 37, L().ptr(st), L().stream()) == 1   # ldl < classes
    assert lib.cara_eval_accumulate(L().ptr(wide), 41, L().ptr(y), 64, 64, 37, None, L().stream()) == 1


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
@pytest.mark.parametrize("size", [224, 384, 208])
def test_im2col_u8_is_bitwise_the_fp32_route(size, operands):
    """cara_im2col_patches_u8(pixels) == cara_im2col_patches(normalize_u8(pixels) computed on the CPU: correctly rounded fp32)"""
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD, normalize_u8
    lib, dt = L().lib(operands), L().act_dtype(operands)
    g = torch.Generator().manual_seed(size)
    px = torch.randint(0, 256, (2, 3, size, size), generator=g, dtype=torch.uint8)
    for c in range(3):
        px[0, c].view(-1)[:256] = torch.arange(256, dtype=torch.uint8)    # every pixel value in every channel
    img = normalize_u8(px).to(DEV)
    rows, cols = 2 * (size // 16) ** 2, 3 * 256
    want = torch.empty(rows, cols, dtype=dt, device=DEV)
    got = torch.zeros(rows, cols, dtype=dt, device=DEV)
    mean, std = torch.tensor(IMAGENET_MEAN, device=DEV), torch.tensor(IMAGENET_STD, device=DEV)
    L().check(lib.cara_im2col_patches(L().ptr(img), L().ptr(want), 2, 3, size, size, 16, L().stream()), "cara_im2col_patches")
    L().check(lib.cara_im2col_patches_u8(L().ptr(px.to(DEV)), L().ptr(mean), L().ptr(std), L().ptr(got), 2, 3, size, size, 16,
                                         L().stream()), "cara_im2col_patches_u8")
    torch.cuda.synchronize()
    differ = (got.view(torch.int16) != want.view(torch.int16))
    print(f"im2col_u8 {size} [{operands}]: {int(differ.sum())} of {differ.numel()} patch-row elements differ")
    assert not differ.any(), differ.nonzero()[:20].tolist()


def _ws_bytes(lib, depth, dim, heads, img, B, rank, inference, ncls=100):
    g = L().Geom(depth, dim, heads, rank, 32 if rank <= 32 else 64, 0.1, 4)
    s = L().VitShape(B, img, 16, 3, (img // 16) ** 2 + 1, ncls, 1e-6, 0, 0.1, 0, inference)
    return int(lib.cara_vit_workspace_bytes(C.byref(g), C.byref(s)))


def test_inference_workspace_sizes():
    for operands in ("bf16", "fp16"):
        lib = L().lib(operands)
        for rank, want in PARENT_WS_BYTES.items():
            assert _ws_bytes(lib, 12, 768, 12, 224, 64, rank, 0) == want           # training size: unchanged
        b_tr, b_inf = _ws_bytes(lib, 12, 768, 12, 224, 256, 16, 0), _ws_bytes(lib, 12, 768, 12, 224, 256, 16, 1)
        l_tr, l_inf = _ws_bytes(lib, 24, 1024, 16, 384, 32, 16, 0), _ws_bytes(lib, 24, 1024, 16, 384, 32, 16, 1)
        print(f"[{operands}] ViT-B/16 b256: {b_inf} / {b_tr} = {b_inf / b_tr:.4f}; ViT-L/16@384 b32: {l_inf} / {l_tr} = {l_inf / l_tr:.4f}")
        assert 0 < b_inf <= b_tr / 3 and 0 < l_inf <= l_tr / 5


def _model(depth, precision="bf16", num_classes=100, cp_length=4):
    from oracle import cara_oracle as O
    from tests.test_model_gpu import build
    w = O.synthetic_backbone(depth=depth, num_classes=num_classes)
    cp = O.synthetic_cp(rank=16, cp_length=cp_length)       # CP_A2 / CP_P2 non-zero: a trained-like adapter
    return build(w, cp, 16, 0.1, depth, 224, num_classes=num_classes, precision=precision, cp_length=cp_length)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("depth", [2, 3, 12])
def test_inference_sized_workspace_gives_the_same_logits_and_refuses_a_backward(depth, precision):
    from oracle import cara_oracle as O
    from cara_amd._lib import CaraError
    m = _model(depth, precision).eval()
    eng = m._cara_engine
    x, y = O.synthetic_batch(batch=4)
    x, y = x.to(DEV), y.to(DEV)
    with torch.no_grad():
        want = m(x)                      # inference = 1 on the training-sized workspace of _ws
    seen = []
    out = eng.evaluate([(x, y)], debug_hook=lambda lg, lb, nv: seen.append(lg.clone()))
    assert out["n"] == 4 and torch.equal(seen[0], want)
    (tr,), (ev,) = eng._ws.values(), eng._eval_ws.values()
    assert ev["shape"].inference == 1 and ev["ws"].numel() < tr["ws"].numel()
    cp = [getattr(m, "CP_" + n) for n in eng.cp_fields]
    with pytest.raises(CaraError, match="CARA_E_ARG"):
        eng._run_backward_on(m, ev, torch.zeros_like(want), None, m.head.weight, cp, x.device)
    torch.cuda.synchronize()


def _pixels(n, seed, classes=100):
    """uint8 images whose level and contrast vary per image (so that the logits do), and labels"""
    g = torch.Generator().manual_seed(seed)
    level = torch.rand(n, 3, 1, 1, generator=g) * 160 + 40
    contrast = torch.rand(n, 1, 1, 1, generator=g) * 60 + 10
    px = (torch.randn(n, 3, 224, 224, generator=g) * contrast + level).clamp_(0, 255).to(torch.uint8)
    return px, torch.randint(0, classes, (n,), generator=g)


def _tie_rule(ref_logits, got_logits, labels):
    """rows whose predicted class may differ between two logit tables of one batch: top-2 margin of the yardstick not above the
    measured logit difference.  -> (ambiguous rows, rows that differ without that excuse)"""
    diff = float((ref_logits - got_logits).abs().max())
    top2 = ref_logits.topk(2, dim=1).values
    ambiguous = (top2[:, 0] - top2[:, 1]) <= diff
    differ = ref_logits.argmax(1) != got_logits.argmax(1)
    return int(ambiguous.sum()), int((differ & ~ambiguous).sum()), diff


def test_evaluate_whole_model_against_the_existing_path():
    from cara_amd import recipe
    from cara_amd.data import ResidentSplit, normalize_u8
    m = _model(12).eval()
    with torch.no_grad():
        m.head.weight.mul_(8.0)    # (a trained head is far from its std-0.02 initialisation: logits, and their margins, 8x wider)
    eng = m._cara_engine
    px, labels = _pixels(600, seed=21)
    split = ResidentSplit.from_tensors(px.to(DEV), labels.to(DEV))
    seen = []
    out = eng.evaluate(split, 256, debug_hook=lambda lg, lb, nv: seen.append((lg.clone(), lb.clone(), nv)))
    assert out["n"] == 600 and [nv for _, _, nv in seen] == [256, 256, 88] and all(lg.shape[0] == 256 for lg, _, _ in seen)
    # the counters are the fallback's on the logits of the same forwards; the 168 padded rows reach nothing
    want = EC.new_state()
    for lg, lb, nv in seen:
        EC.accumulate(want, lg.cpu(), lb.cpu(), nv)
    r = EC.result(want)
    print(f"engine.evaluate {out}; fallback on the same logits {r}")
    assert out["top1"] * 600 == r["top1"] * 600 and out["top5"] * 600 == r["top5"] * 600
    assert round(out["top1"] * 600) == int(want[EC.TOP1]) and round(out["top5"] * 600) == int(want[EC.TOP5])
    assert abs(out["loss"] - r["loss"]) <= LOSS_REL * abs(r["loss"])
    # the existing path on the CPU-normalised (correctly rounded) images
    xs = [normalize_u8(px[i:i + 256]).to(DEV) for i in (0, 256, 512)]
    ys = [labels[i:i + 256].to(DEV) for i in (0, 256, 512)]
    with torch.no_grad():
        ref = [m(x).clone() for x in xs]
    for b in (0, 1):
        assert torch.equal(seen[b][0], ref[b]), f"full batch {b}: {(seen[b][0] - ref[b]).abs().max().item():.3e}"
        top2 = ref[b].topk(2, dim=1).values
        margin = float((top2[:, 0] - top2[:, 1]).min())
        assert margin >= 1e-3, f"redraw the split: batch {b} of the reference path has a top-2 margin of {margin:.3e}"
    last = seen[2][0][:88]
    rel = float((last.double() - ref[2].double()).norm() / ref[2].double().norm())
    print(f"padded last batch (88 rows of a 256-row launch vs an 88-row launch): logits rel-L2 {rel:.3e}")
    assert T.logits_ok(rel, 0.0)
    acc = recipe.evaluate(m, zip(xs, ys))
    hits_ref = sum(int((r_.argmax(1) == y_).sum()) for r_, y_ in zip(ref, ys))
    assert acc == hits_ref / 600
    ambiguous, unexplained, diff = _tie_rule(ref[2], last, ys[2])
    print(f"top-1: recipe.evaluate {acc:.6f}, engine.evaluate {out['top1']:.6f}; last batch: max logit difference {diff:.3e}, "
          f"{ambiguous} row(s) inside it, {unexplained} differ outside it")
    assert unexplained == 0 and abs(round(out["top1"] * 600) - hits_ref) <= ambiguous


def test_evaluate_leaves_the_training_workspace_alive():
    from oracle import cara_oracle as O
    from cara_amd.data import ResidentSplit
    x, y = O.synthetic_batch(batch=64)
    x, y = x.to(DEV), y.to(DEV)
    px, labels = _pixels(300, seed=4)
    split = ResidentSplit.from_tensors(px.to(DEV), labels.to(DEV))

    def run(with_eval):
        m = _model(2).train()
        eng = m._cara_engine
        eng.seed_rank_streams(5, 0)
        opt = torch.optim.SGD(eng.trainable_parameters(), lr=1e-2)
        eng.train_step(x, y, opt)
        first = next(iter(eng._ws.values()))
        if with_eval:
            assert eng.evaluate(split, 256)["n"] == 300
            m.train()
            assert len(eng._ws) == 1 and next(iter(eng._ws.values())) is first and len(eng._eval_ws) == 1
        loss = float(eng.train_step(x, y, opt))
        assert next(iter(eng._ws.values())) is first
        return loss
    a, b = run(False), run(True)
    print(f"loss of the second step: {a!r} without, {b!r} with an evaluation in between")
    assert a == b


def test_fit_sharded_eval_mode_matches_the_reference_mode():
    from cara_amd import cara, create_model
    from cara_amd.data import ResidentSplit, normalize_u8
    from cara_amd.recipe import fit
    g = torch.Generator().manual_seed(1)
    y = torch.arange(16) % 4
    px = (torch.randn(16, 3, 224, 224, generator=g) * 20 + 40 + 50 * y.float().reshape(-1, 1, 1, 1)).clamp_(0, 255).to(torch.uint8)
    x, px, y = normalize_u8(px).to(DEV), px.to(DEV), y.to(DEV)   # (class = mean level, as in test_recipe_fit_learns_...)
    split = ResidentSplit.from_tensors(px, y)

    def run(mode):
        torch.manual_seed(0)
        m = cara({"model": create_model("vit_base_patch16_224_in21k", depth=2, num_classes=4, drop_path_rate=0.1), "rank": 8,
                  "scale": 1.0, "l_mu": 1.0, "l_std": 0.0}).to(DEV)
        evals, ref_accs = [], []

        def on_eval(epoch, acc):
            evals.append((epoch, acc))
            if mode != "sharded":
                return
            # the model as it was scored: the existing path (a 16-row launch) against the 256-row launch of evaluate
            with torch.no_grad():
                lg_ref = m(x)
            got = []
            m._cara_engine.evaluate(split, 256, debug_hook=lambda lg, lb, nv: got.append(lg[:nv].clone()))
            ambiguous, unexplained, diff = _tie_rule(lg_ref, got[0], y)
            hits_ref = int((lg_ref.argmax(1) == y).sum())
            print(f"epoch {epoch}: sharded {acc}, existing path {hits_ref / 16}; logit difference {diff:.3e}, {ambiguous} row(s) inside it")
            assert unexplained == 0 and abs(round(acc * 16) - hits_ref) <= ambiguous
            ref_accs.append(hits_ref / 16)
        test = split if mode == "sharded" else (lambda: [(x, y)])
        best, _ = fit(m, lambda epoch: [(x, y)], test, epochs=21, lr=1e-2, seed=3, on_eval=on_eval, eval_mode=mode)
        return m, evals, best, ref_accs
    m_ref, ev_ref, best_ref, _ = run("reference")
    m_sh, ev_sh, best_sh, ref_accs = run("sharded")
    print(f"reference {ev_ref}, sharded {ev_sh}")
    assert not m_sh.training and not m_ref.training and [e for e, _ in ev_sh] == [e for e, _ in ev_ref] == [10, 20]
    assert ref_accs == [a for _, a in ev_ref]     # the same training run in both modes: evaluation does not disturb it
    assert best_sh >= 0.75


def test_two_ranks_on_one_gpu_return_the_same_dict(tmp_path):
    """both ranks on cuda:0 over gloo, fresh child processes (the rehearsal pattern of bench.py --gpus)"""
    out = str(tmp_path / "ev")
    from tests.test_eval_shard import _free_port
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_eval_two_ranks.py"), str(r), "2", out], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), logs
    a, b = (json.load(open(f"{out}.{r}.json")) for r in range(2))
    print(a)
    assert a == b and a["n"] == 700 and a["batches"] == [2, 1]     # 512 + 188 images: the split, divided
