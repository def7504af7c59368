"""The mean-pooled readout on the device, in both operand builds: cara_token_mean and cara_token_mean_bwd against float64 within the
bounds tests/pool_model.py derives (and tests/test_pool_model.py shows attainable by another summation order on the host), with guard
bands, refusals and run-to-run bits; the whole pooled model against the fp32 restatement and its rounding twin; and one short case
per composition: train_step, keep, evaluate, predict, graph replay.  Figures are printed (-s) before they are asserted.

Measured figures: docs/findings/pooled_readout.md."""
import ctypes as C
import functools

import pytest
import torch

from tests import pool_model as PM
from tests import tolerances as T
from tests.test_kernels_gpu import DEV, L
from tests.test_model_gpu import check_logits, grad_bar, rel

pytestmark = pytest.mark.gpu

OPERANDS = ["bf16", "fp16"]
GUARD = 64          # elements in front of and behind every output (a multiple of 16 bytes in both widths)
SENT = {2: (torch.int16, 0x5A5A), 4: (torch.int32, 0x5A5A5A5A)}   # finite in bf16, fp16 and fp32


def guarded(n, dtype):
    """-> (whole allocation, its middle n elements): GUARD sentinel elements on either side"""
    it, val = SENT[torch.empty(0, dtype=dtype).element_size()]
    full = torch.full((n + 2 * GUARD,), val, dtype=it, device=DEV).view(dtype)
    return full, full[GUARD:GUARD + n]


def guards_intact(full, n):
    it, val = SENT[full.element_size()]
    raw = full.view(it)
    return bool((raw[:GUARD] == val).all()) and bool((raw[GUARD + n:] == val).all())


def all_sentinel(full):
    it, val = SENT[full.element_size()]
    return bool((full.view(it) == val).all())


def dt16(operands):
    return torch.float16 if operands == "fp16" else torch.bfloat16


def mean_call(lib, x, first, out, B=None, tokens=None, D=None):
    p = L().ptr
    return lib.cara_token_mean(p(x), x.shape[0] if B is None else B, x.shape[1] if tokens is None else tokens, first,
                               x.shape[2] if D is None else D, p(out), L().stream())


# ---- 1. cara_token_mean ----------------------------------------------------------------------------------------------------------------
MEAN_SHAPES = [(b, n, d) for b in (1, 3) for n in (1, 2, 49, 196, 576) for d in (256, 768, 1024, 260)]


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("kind", PM.FAMILIES)
def test_token_mean_against_float64(operands, kind):
    lib = L().lib(operands)
    worst = 0.0
    for (b, n, d) in MEAN_SHAPES:
        x = PM.family(kind, b, n + 1, d, seed=n + d)
        x[:, 0] = float("nan")                                   # the cls rows are never read into the sum
        xd = x.to(DEV)
        full, out = guarded(b * d, torch.float32)
        L().check(mean_call(lib, xd, 1, out), "cara_token_mean")
        full2, out2 = guarded(b * d, torch.float32)
        L().check(mean_call(lib, xd, 1, out2), "cara_token_mean")
        torch.cuda.synchronize()
        got = out.reshape(b, d).cpu()
        assert guards_intact(full, b * d) and bool(torch.isfinite(got).all()), (kind, b, n, d)
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), (kind, b, n, d)         # the same bits on every run
        err, bound = (got.double() - PM.mean64(x, 1)).abs(), PM.mean_bound(x, 1)
        ratio = float((err / bound.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), (kind, b, n, d, ratio)
        if n == 1:
            assert torch.equal(got.view(torch.int32), x[:, 1].contiguous().view(torch.int32)), (kind, b, d)   # one token: the row itself
    print(f"cara_token_mean [{operands}, {kind}]: worst error / bound {worst:.3f} over {len(MEAN_SHAPES)} shapes")


@pytest.mark.parametrize("operands", OPERANDS)
def test_token_mean_first_and_sample_isolation(operands):
    """first = 0 and first = 3 (the kernel is told the first row, it does not assume the cls row), and a sample's row does not depend
    on the other samples"""
    lib = L().lib(operands)
    x = PM.family("gauss", 3, 50, 768, seed=1)
    for first in (0, 3):
        xx = x.clone()
        xx[:, :first] = float("nan")
        out = torch.empty(3, 768, device=DEV)
        L().check(mean_call(lib, xx.to(DEV), first, out), "cara_token_mean")
        err = (out.cpu().double() - PM.mean64(x, first)).abs()
        assert bool((err <= PM.mean_bound(x, first)).all()), first
        one = torch.empty(1, 768, device=DEV)
        L().check(mean_call(lib, xx[1:2].contiguous().to(DEV), first, one), "cara_token_mean")
        assert torch.equal(one[0], out[1])


@pytest.mark.parametrize("operands", OPERANDS)
def test_token_mean_refusals_launch_nothing(operands):
    lib = L().lib(operands)
    p, st = L().ptr, L().stream
    x = torch.randn(2, 5, 256, device=DEV)
    full, out = guarded(2 * 256, torch.float32)
    refused = {"x NULL": (None, 2, 5, 1, 256, p(out)), "out NULL": (p(x), 2, 5, 1, 256, None), "B = 0": (p(x), 0, 5, 1, 256, p(out)),
               "B < 0": (p(x), -1, 5, 1, 256, p(out)), "first < 0": (p(x), 2, 5, -1, 256, p(out)),
               "tokens == first": (p(x), 2, 5, 5, 256, p(out)), "tokens < first": (p(x), 2, 3, 4, 256, p(out)),
               "D = 0": (p(x), 2, 5, 1, 0, p(out)), "D < 0": (p(x), 2, 5, 1, -4, p(out)), "D % 4": (p(x), 2, 5, 1, 254, p(out))}
    for what, a in refused.items():
        assert lib.cara_token_mean(*a, st()) == 1, what
    torch.cuda.synchronize()
    assert all_sentinel(full)
    assert lib.cara_token_mean(p(x), 2, 5, 4, 256, p(out), st()) == 0      # the neighbour of a refused value is legal
    torch.cuda.synchronize()
    assert torch.equal(out.reshape(2, 256), x[:, 4])


# ---- 2. cara_token_mean_bwd ------------------------------------------------------------------------------------------------------------
BWD_SHAPES = [(b, n, d) for b in (1, 3) for n in (1, 2, 49, 196, 576) for d in (256, 768, 1024)] + [(3, 49, 260), (1, 2, 260)]


def bwd_call(lib, dpool, rs, B, tokens, first, D, dx, dyb, panels):
    p = L().ptr
    return lib.cara_token_mean_bwd(p(dpool), p(rs), B, tokens, first, D, p(dx), p(dyb), panels, L().stream())


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("kind", PM.FAMILIES)
def test_token_mean_bwd_against_float64(operands, kind):
    lib, dt = L().lib(operands), dt16(operands)
    cases = 0
    for (b, n, d) in BWD_SHAPES:
        tokens, rows = n + 1, b * (n + 1)
        dpool = PM.family(kind, b, 2, d, seed=3 * n + d)[:, 1].contiguous()
        scales = torch.tensor([1.0 / 0.9, 0.0, 1.0 / 0.7])[:b].contiguous()
        for rs in (None, scales):
            dx64, v64 = PM.bwd64(dpool, rs, tokens, 1)
            for panels in ((0,) if d % 32 else (0, rows + 5)):
                n16 = (d // 32) * panels * 32 if panels else rows * d
                fx, dx = guarded(rows * d, torch.float32)
                fy, dyb = guarded(n16, dt)
                L().check(bwd_call(lib, dpool.to(DEV), None if rs is None else rs.to(DEV), b, tokens, 1, d, dx, dyb, panels), "cara_token_mean_bwd")
                torch.cuda.synchronize()
                assert guards_intact(fx, rows * d) and guards_intact(fy, n16), (kind, b, n, d, panels)
                gx = dx.reshape(b, tokens, d).cpu()
                if panels:
                    img = dyb.reshape(d // 32, panels, 32).cpu()
                    it, val = SENT[2]
                    assert bool((img[:, rows:].contiguous().view(it) == val).all())       # the panels' spare rows are not written
                    gy = PM.from_panels(img, rows).reshape(b, tokens, d)
                else:
                    gy = dyb.reshape(b, tokens, d).cpu()
                # every element is written: the cls rows exactly zero (sentinels are not), the others within the bounds
                assert not gx[:, 0].view(torch.int32).any() and not gy[:, 0].contiguous().view(torch.int16).any(), (kind, b, n, d, panels)
                assert PM.dx_ok(gx, dx64), (kind, b, n, d, float(((gx.double() - dx64).abs() / dx64.abs().clamp_min(1e-300)).max()) / PM.U32)
                assert PM.dyb_ok(gy, v64, dt), (kind, b, n, d, panels, rs is not None)
                cases += 1
    print(f"cara_token_mean_bwd [{operands}, {kind}]: {cases} launches inside dx <= 2 u |v|, dyb in the 3 u interval")


@pytest.mark.parametrize("operands", OPERANDS)
def test_token_mean_bwd_refusals_launch_nothing(operands):
    lib, dt = L().lib(operands), dt16(operands)
    p, st = L().ptr, L().stream
    B, tokens, D = 2, 5, 256
    dpool = torch.randn(B, D, device=DEV)
    fx, dx = guarded(B * tokens * D, torch.float32)
    fy, dyb = guarded(B * tokens * D, dt)
    ok = dict(dpool=p(dpool), rs=None, B=B, tokens=tokens, first=1, D=D, dx=p(dx), dyb=p(dyb), panels=0)
    refused = {"dpool NULL": dict(dpool=None), "dx NULL": dict(dx=None), "dyb NULL": dict(dyb=None), "B = 0": dict(B=0), "B < 0": dict(B=-2),
               "first < 0": dict(first=-1), "tokens == first": dict(first=5), "tokens < first": dict(first=6), "D = 0": dict(D=0),
               "D % 4": dict(D=254), "panels < 0": dict(panels=-1), "panels < rows": dict(panels=B * tokens - 1),
               "panels, D % 32": dict(panels=B * tokens, D=252)}
    for what, change in refused.items():
        a = dict(ok, **change)
        assert lib.cara_token_mean_bwd(a["dpool"], a["rs"], a["B"], a["tokens"], a["first"], a["D"], a["dx"], a["dyb"], a["panels"], st()) == 1, what
    torch.cuda.synchronize()
    assert all_sentinel(fx) and all_sentinel(fy)
    a = dict(ok, panels=B * tokens)
    assert lib.cara_token_mean_bwd(a["dpool"], a["rs"], a["B"], a["tokens"], a["first"], a["D"], a["dx"], a["dyb"], a["panels"], st()) == 0
    torch.cuda.synchronize()
    assert guards_intact(fx, B * tokens * D) and guards_intact(fy, B * tokens * D)


# ---- 3. the whole model ----------------------------------------------------------------------------------------------------------------
DEPTH, IMG, NCLS, BATCH, RANK, SCALE = 2, 96, 5, 3, 8, 0.1


@functools.lru_cache(maxsize=None)
def _weights():
    """(token-readout state dict, the pooled one, CP tensors): computed once, never written to"""
    from oracle import cara_oracle as O
    w = O.synthetic_backbone(depth=DEPTH, img=IMG, num_classes=NCLS)
    cp = dict(O.synthetic_cp(rank=RANK, depth=DEPTH))
    cp["CP_A1"], cp["CP_P1"] = cp["CP_A1"][:3 * DEPTH], cp["CP_P1"][:9 * DEPTH]
    pw = PM.pooled_weights(w)
    tok = dict(w)
    tok["norm.weight"], tok["norm.bias"] = pw["fc_norm.weight"], pw["fc_norm.bias"]      # the same numbers in the other role
    return tok, pw, cp


def _model(precision="bf16", pooled=True, drop_path_rate=0.1):
    from cara_amd import cara, create_model
    tok, pw, cp = _weights()
    m = create_model("vit_base_patch16_224_in21k", depth=DEPTH, img_size=IMG, num_classes=NCLS, drop_path_rate=drop_path_rate,
                     global_pool="avg" if pooled else "token")
    m = cara({"model": m, "rank": RANK, "scale": SCALE, "l_mu": 1.5, "l_std": 0.1, "precision": precision})
    sd = dict(pw if pooled else tok)
    sd.update(cp)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train()


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(BATCH, 3, IMG, IMG, generator=g), torch.randint(0, NCLS, (BATCH,), generator=g)


def _droppath():
    """[depth, 2, B]: the last block's MLP multiplier is 1 / 0.9, 0 and 1 / 0.9 -- the row scale of the pooled backward's dyb"""
    dp = torch.ones(DEPTH, 2, BATCH)
    dp[0, 0] = torch.tensor([0.0, 1 / 0.95, 1 / 0.95])
    dp[1, 0] = torch.tensor([1 / 0.9, 1 / 0.9, 0.0])
    dp[1, 1] = torch.tensor([1 / 0.9, 0.0, 1 / 0.9])
    return dp


@functools.lru_cache(maxsize=None)
def _reference():
    """fp32 restatement (logits, loss, gradients by autograd), its bf16 and fp16 rounding twins, the token readout's logits: once"""
    tok, pw, cp = _weights()
    x, y = _batch()
    dp = _droppath()
    leaves = {k: v.clone().requires_grad_(True) for k, v in cp.items()}
    ww = dict(pw)
    ww["head.weight"], ww["head.bias"] = pw["head.weight"].clone().requires_grad_(True), pw["head.bias"].clone().requires_grad_(True)
    logits = PM.forward(x, ww, leaves, s=SCALE, depth=DEPTH, drop_path_keep=dp, readout="avg")
    loss = torch.nn.functional.cross_entropy(logits, y)
    loss.backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["head.weight"], grads["head.bias"] = ww["head.weight"].grad, ww["head.bias"].grad
    with torch.no_grad():
        sims = {p: PM.forward(x, pw, cp, s=SCALE, depth=DEPTH, drop_path_keep=dp, factored=True, bf16_sim=True,
                              sim_dtype=dt16(p), readout="avg") for p in OPERANDS}
        token = PM.forward(x, tok, cp, s=SCALE, depth=DEPTH, drop_path_keep=dp, readout="token")
    return logits.detach(), loss.detach(), grads, sims, token


@pytest.mark.parametrize("precision", OPERANDS)
def test_pooled_model_logits_and_gradients_against_the_restatement(precision):
    from oracle import cara_oracle as O
    x, y = _batch()
    dp = _droppath().to(DEV)
    ref, rloss, gref, sims, token = _reference()
    m = _model(precision)
    eng = m._cara_engine
    logits = eng.forward(x.to(DEV), droppath=dp)
    check_logits(logits.detach(), ref, sims[precision], precision, "pooled readout, depth 2, 37 tokens")
    loss = torch.nn.functional.cross_entropy(logits, y.to(DEV))
    loss.backward()
    parts = {n: rel(getattr(m, n).grad, gref[n]) for n in O.CP_NAMES}
    parts["head.weight"], parts["head.bias"] = rel(m.head.weight.grad, gref["head.weight"]), rel(m.head.bias.grad, gref["head.bias"])
    print(f"pooled readout [{precision}]: loss {loss.item():.5f} vs {rloss.item():.5f}; gradient rel-L2 per part: "
          + ", ".join(f"{k} {v:.2e}" for k, v in parts.items()))
    assert all(v < T.CP_GRAD for v in parts.values()), parts
    if precision == "fp16":
        assert all(v < grad_bar(precision) for v in parts.values()), parts
    # the order of pool and norm: the token readout with the SAME numbers as its norm is another function
    t = _model(precision, pooled=False)
    with torch.no_grad():
        tl = t._cara_engine.forward(x.to(DEV), droppath=dp)
    noise = max(rel(tl, token), rel(logits.detach(), ref))
    assert rel(tl, token) < 1e-2 and rel(tl, ref) > 10 * noise and rel(logits.detach(), token) > 10 * noise, (noise, rel(tl, ref))


# ---- 4. composition ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", OPERANDS)
def test_train_step_is_forward_loss_backward_and_adamw_through_autograd(precision):
    from oracle import cara_oracle as O
    x, y = _batch()
    xd, yd, dp = x.to(DEV), y.to(DEV), _droppath().to(DEV)
    _, rloss, gref, _, _ = _reference()
    a, b = _model(precision), _model(precision)
    names = O.CP_NAMES + ("head.weight", "head.bias")
    before = {n: a.get_parameter(n).detach().clone() for n in names}
    oa = torch.optim.AdamW(a._cara_engine.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    ob = torch.optim.AdamW(b._cara_engine.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    la = a._cara_engine.train_step(xd, yd, oa, droppath=dp)
    lb = torch.nn.functional.cross_entropy(b._cara_engine.forward(xd, droppath=dp), yd)
    ob.zero_grad()
    lb.backward()
    ob.step()
    bar = 5e-4 if precision == "fp16" else 5e-3                    # (the loss bar of test_train_step_against_oracle)
    print(f"train_step [{precision}]: loss {la.item():.6f}, autograd path {lb.item():.6f}, fp32 restatement {rloss.item():.6f}")
    assert abs(la.item() - rloss.item()) < bar * max(1.0, abs(rloss.item())) and abs(la.item() - lb.item()) < 1e-5 * max(1.0, abs(lb.item()))
    worst = max(rel(getattr(a, n).grad, gref[n]) for n in O.CP_NAMES)
    assert worst < grad_bar(precision), worst
    worst_b = max(rel(getattr(b, n).grad, gref[n]) for n in O.CP_NAMES)
    assert worst_b < grad_bar(precision), worst_b
    # one AdamW step on either path: the UPDATE (after - before), not the parameter -- a step moves a value by ~1e-3 of itself, so a
    # bar on the parameter would pass a skipped update.  Adam's first step is lr * sign(g) per element; elements whose gradient is
    # below the rounding noise may step either way, so the updates are held by direction (the bar of
    # test_three_adamw_steps_follow_the_oracle_trajectory) and both must have moved every tensor.
    for n in names:
        ua = (a.get_parameter(n).detach() - before[n]).double().flatten()
        ub = (b.get_parameter(n).detach() - before[n]).double().flatten()
        assert float(ua.norm()) > 0 and float(ub.norm()) > 0, n
        cos = float(ua @ ub / (ua.norm() * ub.norm()))
        assert cos > 0.9, (n, cos)


@pytest.mark.parametrize("precision", OPERANDS)
def test_identity_keep_table_is_bitwise_the_step_without_it(precision):
    from cara_amd.data import identity_keep
    from cara_amd.optim import AdamW
    x, y = _batch()
    xd, yd, dp = x.to(DEV), y.to(DEV), _droppath().to(DEV)
    ident = identity_keep(BATCH, (IMG // 16) ** 2).to(DEV)
    out = []
    for keep in (ident, None):
        m = _model(precision)
        eng = m._cara_engine
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
        loss = eng.train_step(xd, yd, opt, droppath=dp, keep=keep).clone()
        out.append((loss, eng._flat_grad.clone(), [p.detach().clone() for p in eng.trainable_parameters()]))
    (l0, g0, p0), (l1, g1, p1) = out
    assert torch.equal(l0, l1) and torch.isfinite(l0) and torch.equal(g0.view(torch.int32), g1.view(torch.int32)) and bool(g0.any())
    assert all(torch.equal(u, v) for u, v in zip(p0, p1))
    # a real subset: the mean is over the kept rows (the restatement on the same rows would need its own feed; here: it runs and differs)
    sub = torch.stack([torch.randperm(36, generator=torch.Generator().manual_seed(b))[:9] for b in range(BATCH)]).to(torch.int32).to(DEV)
    m = _model(precision)
    l2 = m._cara_engine.train_step(xd, yd, None, droppath=dp, keep=sub)
    assert torch.isfinite(l2) and float(l2) != float(l0) and bool(torch.isfinite(m._cara_engine._flat_grad).all())


def _split(n=7):
    from cara_amd.data import ResidentSplit
    g = torch.Generator().manual_seed(9)
    px = torch.randint(0, 256, (n, 3, IMG, IMG), dtype=torch.uint8, generator=g)
    return px, torch.randint(0, NCLS, (n,), generator=g), ResidentSplit


@pytest.mark.parametrize("precision", OPERANDS)
def test_evaluate_and_predict_agree_with_the_python_loop(precision):
    from cara_amd import recipe
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD
    px, labels, ResidentSplit = _split()
    m = _model(precision)
    eng = m._cara_engine
    split = ResidentSplit.from_tensors(px.to(DEV), labels.to(DEV))
    got = eng.evaluate(split, 4)                                    # two batches, the second a padded one
    mean, std = torch.tensor(IMAGENET_MEAN).reshape(1, 3, 1, 1), torch.tensor(IMAGENET_STD).reshape(1, 3, 1, 1)
    x = ((px.float() / 255 - mean) / std).to(DEV)
    acc = recipe.evaluate(m, [(x[:4], labels[:4].to(DEV)), (x[4:], labels[4:].to(DEV))])
    print(f"evaluate [{precision}]: top-1 {got['top1']:.4f} on the device, {acc:.4f} by the loop; loss {got['loss']:.5f}")
    assert got["n"] == 7 and round(got["top1"] * 7) == round(acc * 7)
    pred = eng.predict(split, 3, 4)
    with torch.no_grad():
        top1 = m(x).argmax(1)
    assert torch.equal(pred.topk[:, 0].long().cpu(), top1.cpu()) and pred.counts()["top1"] == got["top1"]
    assert round(pred.counts()["top1"] * 7) == int((top1.cpu() == labels).sum())


def test_graphed_train_step_replays_equal_the_eager_steps():
    from oracle import cara_oracle as O
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    xa, ya = _batch(0)
    xb, yb = _batch(4)
    batches = [(xa.to(DEV), ya.to(DEV)), (xb.to(DEV), yb.to(DEV))]
    for precision in OPERANDS:
        out = {}
        for mode in ("capturable", "graph"):
            m = _model(precision, drop_path_rate=0.0)
            eng = m._cara_engine
            opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
            gstep = GraphedTrainStep(eng, opt) if mode == "graph" else None
            losses = []
            for it in range(4):                                     # the first call of a graph runs eagerly: three replays behind it
                x, y = batches[it % 2]
                if mode == "graph":
                    losses.append(gstep(x, y).item())
                else:
                    opt.advance()
                    losses.append(eng.train_step(x, y, opt).item())
            out[mode] = (losses, {n: getattr(m, n).detach().clone() for n in O.CP_NAMES}, m.head.weight.detach().clone())
        assert out["graph"][0] == out["capturable"][0], (precision, out["graph"][0], out["capturable"][0])
        assert all(torch.equal(out["graph"][1][n], out["capturable"][1][n]) for n in O.CP_NAMES) and torch.equal(out["graph"][2], out["capturable"][2])
        assert all(map(lambda v: v == v, out["graph"][0])) and out["graph"][0][2] < out["graph"][0][0]


def test_exact_weight_dropout_is_refused_before_a_launch():
    from cara_amd._lib import CaraError
    m = _model()
    m._cara_engine.weight_dropout = "exact"
    x, _ = _batch()
    with pytest.raises(CaraError, match="pooled"):
        m(x.to(DEV))
    lib = L().lib()
    geom = L().Geom(DEPTH, 768, 12, RANK, 32, SCALE, 4)
    for kw in (dict(pool=1, wd_exact=1), dict(pool=2), dict(pool=-1)):
        s = L().VitShape(BATCH, IMG, 16, 3, 37, NCLS, 1e-6, wd_p=0.1, **kw)
        assert int(lib.cara_vit_workspace_bytes(C.byref(geom), C.byref(s))) == 0, kw
