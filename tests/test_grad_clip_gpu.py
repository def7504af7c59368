"""GPU side of the global-norm clip and the accumulation kernel.  cara_grad_clip through ctypes at the sizes of
tests/optim_model.py: norm, coefficient and every element inside the bound DERIVED there against float64, the partial sums bitwise
the numpy-fp32 restatement of the kernel's tree, two runs bitwise equal, nothing written when nothing is clipped or when the
found-inf word is set, guards untouched, bad arguments refused.  cara_grad_accumulate bitwise against torch's fp32 sum on the host
in every aliasing form and alignment.  Whole step: train_step(clip_grad=) against the unclipped step's gradients clipped in
float64, the AdamW step behind it, the autograd path's clip_grad_norm_, and GraphedTrainStep with the clip captured."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import optim_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ["bf16", "fp16"]
GUARD_BITS = 0x7b5a5a5a     # guard elements: a float no kernel here writes (1.13e36)


def L():
    from cara_amd import _lib
    return _lib


def _guarded(n, lead):
    """-> (whole buffer, the n elements `lead` floats in): guards of `lead` floats in front and 4 behind, holding GUARD_BITS"""
    buf = torch.full((lead + n + 4,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[lead:lead + n]


def _guards_ok(buf, n, lead):
    w = buf.view(torch.int32)
    return bool((w[:lead] == GUARD_BITS).all()) and bool((w[lead + n:] == GUARD_BITS).all())


def _clip(lib, g_host, max_norm, lead=4, found=None):
    """cara_grad_clip on a copy of g_host that starts `lead` floats into its allocation (4: 16-byte aligned, the float4 path; 1: the
    dword path) -> (g afterwards, partial sums, out) on the host; the guards around g, the scratch and out are checked here"""
    n = g_host.numel()
    chunks = int(lib.cara_grad_clip_scratch_bytes(n)) // 4
    assert chunks == M.chunks(n)
    gb, g = _guarded(n, lead)
    sb, scratch = _guarded(chunks, 4)
    ob, out = _guarded(2, 4)
    g.copy_(g_host)
    fw = None if found is None else torch.tensor([float(found)], device=DEV)
    p = L().ptr
    L().check(lib.cara_grad_clip(p(g), n, max_norm, p(scratch), p(fw), p(out), L().stream()), "cara_grad_clip")
    torch.cuda.synchronize()
    assert _guards_ok(gb, n, lead) and _guards_ok(sb, chunks, 4) and _guards_ok(ob, 2, 4)
    assert fw is None or float(fw) == float(found)
    return g.cpu(), scratch.cpu(), out.cpu()


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _case(n):
    """the seeded buffer of a size, its float64 norm and the restatement's partial sums (computed once, left unchanged)"""
    g = M.buffer(n, 7)
    return torch.from_numpy(g), M.clip64(g, math.inf)[0], torch.from_numpy(M.partials_f32(g))


@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("n", M.SIZES)
def test_clip_against_float64_within_the_derived_bound(n, side):
    lib = L().lib()
    g, norm64, partials = _case(n)
    max_norm = (0.5 if side == "below" else 2.0) * norm64
    _, coef64, want = M.clip64(g.numpy(), max_norm)
    runs = [_clip(lib, g, max_norm, lead) for lead in (4, 4, 1)]
    for got, scratch, out in runs:
        assert _same(scratch, partials)                              # launch 1 is the documented tree, bit for bit
        e_norm = abs(float(out[0]) - norm64) / norm64
        e_coef = abs(float(out[1]) - coef64) / coef64
        err = (got.double() - torch.from_numpy(want)).abs() / g.double().abs()
        print(f"n {n} {side}: |norm - norm64| / norm64 {e_norm:.3e} (bound {M.norm_bound(n):.3e}), coef {e_coef:.3e}, worst element "
              f"{float(err.max()):.3e} (bound {M.elem_bound(n):.3e})")
        assert e_norm <= M.norm_bound(n) and e_coef <= M.elem_bound(n)
        assert bool((err <= M.elem_bound(n)).all())
        if side == "above":
            assert float(out[1]) == 1.0 and _same(got, g)            # not clipped: bitwise unchanged
        else:
            assert float(out[1]) < 1.0 and not _same(got, g)
    # two runs on the same input, and the float4 and the dword path: the same bits
    for other in runs[1:]:
        assert all(_same(a, b) for a, b in zip(runs[0], other))


@pytest.mark.parametrize("n", M.SIZES)
def test_clip_leaves_an_overflowed_step_alone_and_only_measures_at_infinity(n):
    lib = L().lib()
    g, norm64, _ = _case(n)
    bad = g.clone()
    bad[n // 2] = float("inf")
    got, _, out = _clip(lib, bad, 0.5 * norm64, found=1.0)
    assert _same(got, bad) and float(out[1]) == 1.0                   # no Inf x 0 = NaN, no scaling at all
    got, _, out = _clip(lib, g, 0.5 * norm64, found=1.0)
    assert _same(got, g) and float(out[1]) == 1.0 and abs(float(out[0]) - norm64) <= M.norm_bound(n) * norm64
    # a clear word changes nothing about the clip
    assert all(_same(a, b) for a, b in zip(_clip(lib, g, 0.5 * norm64, found=0.0), _clip(lib, g, 0.5 * norm64)))
    got, _, out = _clip(lib, g, math.inf)
    assert _same(got, g) and float(out[1]) == 1.0 and abs(float(out[0]) - norm64) <= M.norm_bound(n) * norm64


def test_clip_refuses_bad_arguments_and_launches_nothing():
    lib = L().lib()
    p, st = L().ptr, L().stream
    gb, g = _guarded(100, 4)
    g.fill_(3.0)
    scratch, out = torch.full((1,), 7.0, device=DEV), torch.full((2,), 7.0, device=DEV)
    for max_norm in (0.0, -1.0, float("nan"), -math.inf):
        assert lib.cara_grad_clip(p(g), 100, max_norm, p(scratch), None, p(out), st()) == 1, max_norm
    assert lib.cara_grad_clip(None, 100, 1.0, p(scratch), None, p(out), st()) == 1
    assert lib.cara_grad_clip(p(g), 100, 1.0, None, None, p(out), st()) == 1
    assert lib.cara_grad_clip(p(g), 100, 1.0, p(scratch), None, None, st()) == 1
    assert lib.cara_grad_clip(p(g), 0, 1.0, p(scratch), None, p(out), st()) == 1
    assert lib.cara_grad_clip(p(g), 2 ** 31 + 1, 1.0, p(scratch), None, p(out), st()) == 1
    assert lib.cara_grad_clip(C.c_void_p(g.data_ptr() + 2), 50, 1.0, p(scratch), None, p(out), st()) == 1
    assert lib.cara_grad_accumulate(None, p(g), None, 100, st()) == 1 and lib.cara_grad_accumulate(p(g), None, None, 100, st()) == 1
    assert lib.cara_grad_accumulate(p(g), p(g), None, 0, st()) == 1
    assert lib.cara_grad_accumulate(p(g), C.c_void_p(g.data_ptr() + 2), None, 50, st()) == 1
    assert [int(lib.cara_grad_clip_scratch_bytes(n)) for n in (0, 1, 8192, 8193, 2 ** 31, 2 ** 31 + 1)] == [0, 4, 4, 8, 4 * 2 ** 18, 0]
    torch.cuda.synchronize()
    assert bool((g == 3.0).all()) and _guards_ok(gb, 100, 4) and bool((scratch == 7.0).all()) and bool((out == 7.0).all())


# ---- cara_grad_accumulate ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 1027, M.FLAT_R16_C100])
def test_accumulate_is_bitwise_the_fp32_sum_in_every_aliasing_form_and_alignment(n):
    """dst distinct, dst == a, dst == b, b == NULL; all pointers 16-byte aligned, all 4 bytes off (a scalar head, then float4),
    and one pointer alone 4 bytes off (dword accesses)"""
    lib = L().lib()
    p, st = L().ptr, L().stream
    a_h, b_h = torch.from_numpy(M.buffer(n, 11)), torch.from_numpy(M.buffer(n, 12))
    want = a_h + b_h                                                   # torch on the host: one fp32 rounding per element
    for la, lb, ld in ((4, 4, 4), (5, 5, 5), (4, 5, 4), (5, 4, 4), (4, 4, 7), (3, 3, 3)):
        for form in ("distinct", "dst==a", "dst==b", "copy", "copy in place"):
            ab, a = _guarded(n, la)
            bb, b = _guarded(n, lb)
            db, d = _guarded(n, ld)
            a.copy_(a_h)
            b.copy_(b_h)
            if form == "distinct":
                rc, got, exp, (gbuf, lead) = lib.cara_grad_accumulate(p(d), p(a), p(b), n, st()), d, want, (db, ld)
            elif form == "dst==a":
                rc, got, exp, (gbuf, lead) = lib.cara_grad_accumulate(p(a), p(a), p(b), n, st()), a, want, (ab, la)
            elif form == "dst==b":
                rc, got, exp, (gbuf, lead) = lib.cara_grad_accumulate(p(b), p(a), p(b), n, st()), b, want, (bb, lb)
            elif form == "copy":
                rc, got, exp, (gbuf, lead) = lib.cara_grad_accumulate(p(d), p(a), None, n, st()), d, a_h, (db, ld)
            else:
                rc, got, exp, (gbuf, lead) = lib.cara_grad_accumulate(p(a), p(a), None, n, st()), a, a_h, (ab, la)
            torch.cuda.synchronize()
            assert rc == 0 and _same(got.cpu(), exp), (form, la, lb, ld)
            assert _guards_ok(gbuf, n, lead), (form, la, lb, ld)
            if form in ("distinct", "copy"):                           # the sources are only read
                assert _same(a.cpu(), a_h) and _same(b.cpu(), b_h)


# ---- whole step: depth 2, 224 px, rank 16 ------------------------------------------------------------------------------------
DEPTH, BATCH = 2, 4


@functools.lru_cache(maxsize=None)
def _inputs():
    from oracle import cara_oracle as O
    from tests.test_model_gpu import _keep
    w = O.synthetic_backbone(depth=DEPTH)
    cp = O.synthetic_cp(rank=16, depth=DEPTH)
    x, y = O.synthetic_batch(batch=BATCH)
    return w, cp, x, y, _keep(DEPTH, BATCH)


def _model(precision, drop_path_rate=0.1):
    from tests.test_model_gpu import build
    w, cp = _inputs()[:2]
    return build(w, cp, 16, 0.1, DEPTH, 224, drop_path_rate=drop_path_rate, precision=precision).train()


def _trainable(m):
    return {n: p.detach().clone() for n, p in m.named_parameters() if "CP" in n or "head" in n}


def _hold_clipped(eng, flat_before, max_norm):
    """engine.grad_norm and the flat buffer against flat_before clipped in float64"""
    n = flat_before.numel() - 1
    g = flat_before[:-1].cpu().numpy()
    norm64, coef64, want = M.clip64(g, max_norm)
    out = eng.grad_norm.cpu()
    assert eng.grad_norm.is_cuda and tuple(out.shape) == (2,)
    assert abs(float(out[0]) - norm64) <= M.norm_bound(n) * norm64 and abs(float(out[1]) - coef64) <= M.elem_bound(n) * coef64
    err = (eng._flat_grad[:-1].cpu().double() - torch.from_numpy(want)).abs()
    assert bool((err <= torch.from_numpy(np.abs(g.astype(np.float64))) * M.elem_bound(n)).all())
    assert _same(eng._flat_grad[-1:].cpu(), flat_before[-1:].cpu())    # the found-inf word is no gradient
    return norm64, coef64, float(out[0]), float(out[1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_step_with_clip_grad_clips_the_unclipped_steps_gradients(precision):
    from cara_amd.optim import AdamW
    _, _, x, y, keep = _inputs()
    xd, yd, kd = x.to(DEV), y.to(DEV), keep.to(DEV)
    plain = _model(precision)
    plain._cara_engine.train_step(xd, yd, None, droppath=kd)
    before = plain._cara_engine._flat_grad.clone()
    assert plain._cara_engine.grad_norm is None and bool(before[:-1].any()) and float(before[-1]) == 0.0
    c = 0.5 * M.clip64(before[:-1].cpu().numpy(), math.inf)[0]
    clipped = _model(precision)
    eng = clipped._cara_engine
    eng.train_step(xd, yd, None, droppath=kd, clip_grad=c)
    norm64, coef64, norm, coef = _hold_clipped(eng, before, c)
    print(f"[{precision}] norm {norm!r} (float64 {norm64!r}), coef {coef!r} (float64 {coef64!r})")
    assert coef < 1.0
    for n, p in zip(list(eng.cp_fields) + ["head_w", "head_b"], eng.trainable_parameters()):
        assert p.grad.data_ptr() == eng._grad_views[n].data_ptr()      # p.grad are the views that were clipped
    # a norm above the bound: the step is the unclipped one, bit for bit
    loose = _model(precision)
    loose._cara_engine.train_step(xd, yd, None, droppath=kd, clip_grad=4 * c)
    assert _same(loose._cara_engine._flat_grad, before) and float(loose._cara_engine.grad_norm[1]) == 1.0
    # with AdamW: the parameters are those of a clone stepped on the clipped gradients
    stepped, clone = _model(precision), _model(precision)
    so = AdamW(stepped._cara_engine.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    co = AdamW(clone._cara_engine.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    stepped._cara_engine.train_step(xd, yd, so, droppath=kd, clip_grad=c)
    for p, q in zip(clone._cara_engine.trainable_parameters(), eng.trainable_parameters()):
        p.grad = q.grad.detach().clone()
    co.step()
    a, b = _trainable(stepped), _trainable(clone)
    start = _trainable(plain)
    assert len(a) == 14 and all(torch.equal(a[n], b[n]) for n in a) and any(not torch.equal(a[n], start[n]) for n in a)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_clip_grad_norm_on_the_autograd_path(precision):
    _, _, x, y, keep = _inputs()
    m = _model(precision)
    eng = m._cara_engine
    loss = torch.nn.functional.cross_entropy(eng.forward(x.to(DEV), droppath=keep.to(DEV)), y.to(DEV))
    loss.backward()
    params = eng.trainable_parameters()
    before = torch.cat([p.grad.detach().reshape(-1) for p in params] + [eng._grad_views["_found_inf"].reshape(-1)])
    c = 0.5 * M.clip64(before[:-1].cpu().numpy(), math.inf)[0]
    out = eng.clip_grad_norm_(c)
    assert out is eng.grad_norm
    _hold_clipped(eng, before, c)
    for n, p in zip(list(eng.cp_fields) + ["head_w", "head_b"], params):
        assert p.grad.data_ptr() == eng._grad_views[n].data_ptr()
    from cara_amd._lib import CaraError
    with pytest.raises(CaraError):
        eng.clip_grad_norm_(0.0)
    fresh = _model(precision)
    with pytest.raises(CaraError):
        fresh._cara_engine.clip_grad_norm_(1.0)                        # no backward yet


@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_replays_with_clip_grad_are_bitwise_the_eager_steps(precision):
    from cara_amd._lib import CaraError
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    from oracle import cara_oracle as O
    _, _, xa, ya, _ = _inputs()
    xb, yb = O.synthetic_batch(batch=BATCH, seed_x=5, seed_y=6)
    batches = [(xa.to(DEV), ya.to(DEV)), (xb.to(DEV), yb.to(DEV))]
    out = {}
    for mode in ("eager", "graph"):
        m = _model(precision, drop_path_rate=0.0)
        eng = m._cara_engine
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        gstep = GraphedTrainStep(eng, opt, clip_grad=1e-3) if mode == "graph" else None
        losses, norms = [], []
        for it in range(4):                                            # warm, capture + replay, replay, replay
            opt.param_groups[0]["lr"] = 1e-3 * (0.7 ** it)
            x, y = batches[it % 2]
            if gstep is not None:
                loss = gstep(x, y)
            else:
                opt.advance()
                loss = eng.train_step(x, y, opt, clip_grad=1e-3)
            losses.append(loss.item())
            norms.append(eng.grad_norm.cpu().clone())
        if gstep is not None:
            assert len(gstep._graphs) == 1 and all(ent != "warm" for ent in gstep._graphs.values())
            with pytest.raises(CaraError):
                gstep(x, y, accumulate=(0, 2))
            gstep(x, y, accumulate=(0, 1))                             # k == 1 is the plain step: one more replay
        else:
            opt.advance()
            eng.train_step(x, y, opt, clip_grad=1e-3, accumulate=(0, 1))
        out[mode] = (losses, norms, _trainable(m))
    print(f"[{precision}] losses {out['eager'][0]}; (norm, coef) per step {[t.tolist() for t in out['eager'][1]]}")
    assert out["graph"][0] == out["eager"][0] and len(set(out["eager"][0])) == 4
    assert all(_same(a, b) for a, b in zip(out["graph"][1], out["eager"][1]))
    assert all(float(t[1]) < 1.0 for t in out["eager"][1])             # every step was clipped
    for n in out["eager"][2]:
        assert torch.equal(out["graph"][2][n], out["eager"][2][n]), n
