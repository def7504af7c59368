"""The weight EMA on the device.  cara_ema_update through ctypes bitwise against the numpy-fp32 restatement of tests/ema_model.py
(one 32-tensor call, both access paths, every weight by value and from device memory, guards, refusals), ParamEma over more than
32 tensors, and the whole-model paths on the depth-2 ViT-B/16 rank-16 model of tests/test_accumulate_gpu.py at batch 4: the fused
step with ema=, an accumulation window, evaluation on the averaged weights, graph replay with a warming-up decay, checkpoints, fit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import ema_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ["bf16", "fp16"]
GUARD_BITS = 0x7b5a5a5a     # guard elements: a float no kernel here writes (1.13e36)
BATCH = 4


def L():
    from cara_amd import _lib
    return _lib


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _guarded(host, lead):
    """-> (whole buffer, the view holding `host`, `lead` floats in): guards of `lead` floats in front and 4 behind"""
    n = host.size
    buf = torch.full((lead + n + 4,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    buf[lead:lead + n].copy_(torch.from_numpy(host))
    return buf, buf[lead:lead + n]


def _guards_ok(buf, n, lead):
    w = buf.view(torch.int32)
    return bool((w[:lead] == GUARD_BITS).all()) and bool((w[lead + n:] == GUARD_BITS).all())


def _arrays(es, ps):
    k = len(es)
    return ((C.c_void_p * k)(*[t.data_ptr() for t in es]), (C.c_void_p * k)(*[t.data_ptr() for t in ps]),
            (C.c_size_t * k)(*[t.numel() for t in es]))


def _leads(i):
    """(shadow, parameter) offsets into their allocations: both 16-byte aligned -> the float4 path; any one float in -> dwords"""
    return ((4, 4), (1, 1), (4, 1), (1, 4))[i % 4]


@functools.lru_cache(maxsize=None)
def _case():
    return M.kernel_case()


# ---- 1. the kernel, bitwise -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", M.WEIGHTS + M.EXTRA_WEIGHTS, ids=lambda w: repr(float(w)))
def test_kernel_is_bitwise_the_restatement_by_value_and_from_device_memory(w):
    lib = L().lib()
    case = _case()
    assert len(case) == M.MAX_TENSORS
    results = []
    for form in ("value", "device"):
        eb = [_guarded(e, _leads(i)[0]) for i, (e, _) in enumerate(case)]
        pb = [_guarded(p, _leads(i)[1]) for i, (_, p) in enumerate(case)]
        assert sum(1 for _, v in eb if v.data_ptr() % 16) == 16 and all(v.data_ptr() % 4 == 0 for _, v in eb + pb)
        earr, parr, narr = _arrays([v for _, v in eb], [v for _, v in pb])
        wdev = torch.tensor([float(w)], device=DEV) if form == "device" else None
        # (the by-value weight is ignored when a device weight is given: a value that would be refused proves it)
        rc = lib.cara_ema_update(len(case), earr, parr, narr, float(w) if wdev is None else -1.0, L().ptr(wdev), L().stream())
        torch.cuda.synchronize()
        assert rc == 0
        got = []
        for i, (e, p) in enumerate(case):
            (ebuf, ev), (pbuf, pv) = eb[i], pb[i]
            assert _guards_ok(ebuf, e.size, _leads(i)[0]) and _guards_ok(pbuf, p.size, _leads(i)[1]), i
            assert np.array_equal(M.bits(pv.cpu().numpy()), M.bits(p)), i          # param is never written
            want = M.update_f32(e, p, w)
            g = ev.cpu().numpy()
            assert np.array_equal(M.bits(g), M.bits(want)), (form, i, e.size, int(np.count_nonzero(M.bits(g) != M.bits(want))))
            got.append(g)
        assert wdev is None or float(wdev) == float(w)
        results.append(got)
    assert all(np.array_equal(M.bits(a), M.bits(b)) for a, b in zip(*results))


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_bad_device_weights_write_nothing():
    lib = L().lib()
    st = L().stream
    host = [M.random_pairs(n, 40 + n) for n in (5, 1024, 1027)]
    eb = [_guarded(e, 4) for e, _ in host]
    pb = [_guarded(p, 4) for _, p in host]
    es, ps = [v for _, v in eb], [v for _, v in pb]
    earr, parr, narr = _arrays(es, ps)
    k = len(es)

    def patched(arr, i, value, kind=C.c_void_p):
        vals = [arr[j] for j in range(k)]
        vals[i] = value
        return (kind * k)(*vals)
    E_ARG = 1
    assert lib.cara_ema_update(k, None, parr, narr, 0.5, None, st()) == E_ARG
    assert lib.cara_ema_update(k, earr, None, narr, 0.5, None, st()) == E_ARG
    assert lib.cara_ema_update(k, earr, parr, None, 0.5, None, st()) == E_ARG
    assert lib.cara_ema_update(k, patched(earr, 1, None), parr, narr, 0.5, None, st()) == E_ARG             # a null entry
    assert lib.cara_ema_update(k, earr, patched(parr, 2, None), narr, 0.5, None, st()) == E_ARG
    assert lib.cara_ema_update(k, earr, parr, patched(narr, 0, 0, C.c_size_t), 0.5, None, st()) == E_ARG    # n[i] == 0
    assert lib.cara_ema_update(k, patched(earr, 1, es[1].data_ptr() + 2), parr, narr, 0.5, None, st()) == E_ARG   # not 4-byte aligned
    assert lib.cara_ema_update(k, earr, patched(parr, 1, ps[1].data_ptr() + 2), narr, 0.5, None, st()) == E_ARG
    assert lib.cara_ema_update(k, earr, patched(parr, 2, es[2].data_ptr()), narr, 0.5, None, st()) == E_ARG   # ema[i] == param[i]
    big = M.MAX_TENSORS + 1
    many = ((C.c_void_p * big)(*[es[0].data_ptr()] * big), (C.c_void_p * big)(*[ps[0].data_ptr()] * big), (C.c_size_t * big)(*[5] * big))
    for nt in (0, -1, big):
        assert lib.cara_ema_update(nt, *many, 0.5, None, st()) == E_ARG, nt
    for w in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        assert lib.cara_ema_update(k, earr, parr, narr, w, None, st()) == E_ARG, w
    wdev = torch.tensor([0.5, 0.5], device=DEV)
    assert lib.cara_ema_update(k, earr, parr, narr, 0.5, C.c_void_p(wdev.data_ptr() + 2), st()) == E_ARG
    # a device weight outside [0, 1], or a NaN: the launch runs and writes nothing
    for bad in (1.5, -0.25, float("nan")):
        wdev = torch.tensor([bad], device=DEV)
        assert lib.cara_ema_update(k, earr, parr, narr, 0.5, L().ptr(wdev), st()) == 0
    torch.cuda.synchronize()
    for (ebuf, ev), (pbuf, pv), (e, p) in zip(eb, pb, host):
        assert np.array_equal(M.bits(ev.cpu().numpy()), M.bits(e)) and np.array_equal(M.bits(pv.cpu().numpy()), M.bits(p))
        assert _guards_ok(ebuf, e.size, 4) and _guards_ok(pbuf, p.size, 4)
    # ... and the same arrays are taken once nothing is wrong with them
    assert lib.cara_ema_update(k, earr, parr, narr, 0.5, None, st()) == 0
    torch.cuda.synchronize()
    assert all(np.array_equal(M.bits(ev.cpu().numpy()), M.bits(M.update_f32(e, p, 0.5))) for (_, ev), (e, p) in zip(eb, host))


# ---- 3. ParamEma: more tensors than one launch carries ---------------------------------------------------------------------------
def test_param_ema_over_40_tensors_updates_each_exactly_once():
    from cara_amd._lib import CaraError
    from cara_amd.ema import ParamEma
    host = [M.random_pairs(3 + 37 * i, 200 + i)[1] for i in range(40)]
    params = [torch.from_numpy(p).to(DEV) for p in host]
    ema = ParamEma(params, decay=0.9)
    assert len(ema.tensors) == 40 and all(_same(s, p) and s.data_ptr() != p.data_ptr() for s, p in zip(ema.tensors, params))
    moved = [M.random_pairs(p.size, 300 + i)[0] for i, p in enumerate(host)]
    for p, new in zip(params, moved):
        p.copy_(torch.from_numpy(new))
    ema.update()
    torch.cuda.synchronize()
    w = M.weight_at(0.9, False, 0)
    assert ema.num_updates == 1 and float(w) == ema.weight_at(0)
    for i, (s, old, new) in enumerate(zip(ema.tensors, host, moved)):
        assert np.array_equal(M.bits(s.cpu().numpy()), M.bits(M.update_f32(old, new, w))), i    # (twice would be another value)
        assert np.array_equal(M.bits(params[i].cpu().numpy()), M.bits(new))
    # the state dict round trip, and copy_to
    other = ParamEma([torch.zeros_like(p) for p in params], decay=0.5, warmup=True)
    other.load_state_dict(ema.state_dict())
    assert (other.num_updates, other.decay, other.warmup) == (1, 0.9, False) and all(_same(a, b) for a, b in zip(other.tensors, ema.tensors))
    ema.copy_to()
    assert all(_same(s, p) for s, p in zip(ema.tensors, params))
    # what it refuses, as optim.AdamW does
    for bad in ([torch.zeros(4)], [torch.zeros(4, device=DEV, dtype=torch.float16)], [torch.zeros(4, 4, device=DEV).t()], []):
        with pytest.raises(CaraError):
            ParamEma(bad)
    with pytest.raises(CaraError):
        ParamEma(params, decay=1.5)
    with pytest.raises(CaraError):
        ParamEma(params, capturable=True).update()             # advance() first
    with pytest.raises(CaraError):
        ema.advance()


# ---- the whole model: tests/test_accumulate_gpu.py's, batch 4 -------------------------------------------------------------------
def _model(precision="bf16", drop_path_rate=0.1):
    from tests.test_accumulate_gpu import _model as build
    return build(precision, drop_path_rate)


def _batch():
    from tests.test_accumulate_gpu import _batch as batch
    x, y, dp = batch(BATCH)
    return x.to(DEV), y.to(DEV), dp.to(DEV)


def _np(params):
    return [p.detach().cpu().numpy().copy() for p in params]


# ---- 4. the fused step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_three_steps_with_ema_average_the_parameters_and_change_nothing_else(precision):
    from cara_amd.optim import AdamW
    x, y, dp = _batch()
    runs = {}
    for with_ema in (False, True):
        m = _model(precision)
        eng = m._cara_engine
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
        ema = eng.make_ema(0.9) if with_ema else None
        shadow = _np(ema.tensors) if with_ema else None
        losses = []
        for it in range(3):
            losses.append(eng.train_step(x, y, opt, droppath=dp, **({"ema": ema} if with_ema else {})).item())
            if with_ema:
                now = _np(eng.trainable_parameters())
                shadow = [M.update_f32(s, p, M.weight_at(0.9, False, it)) for s, p in zip(shadow, now)]
                assert ema.num_updates == it + 1
                for i, (s, want) in enumerate(zip(ema.tensors, shadow)):
                    assert np.array_equal(M.bits(s.cpu().numpy()), M.bits(want)), (it, i)
        params = eng.trainable_parameters()
        runs[with_ema] = (losses, _np(params), [(opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()) for p in params])
        if with_ema:
            assert len(ema.tensors) == 14 and any(not np.array_equal(s.cpu().numpy(), p) for s, p in zip(ema.tensors, runs[True][1]))
    (la, pa, ma), (lb, pb, mb) = runs[False], runs[True]
    assert la == lb and len(set(la)) == 3
    assert all(np.array_equal(M.bits(a), M.bits(b)) for a, b in zip(pa, pb))
    assert all(_same(a[0], b[0]) and _same(a[1], b[1]) for a, b in zip(ma, mb))


# ---- 5. an accumulation window --------------------------------------------------------------------------------------------------
def test_a_window_updates_the_average_once_after_its_last_micro_step():
    from cara_amd.optim import AdamW
    from tests.test_accumulate_gpu import _run
    m = _model()
    eng = m._cara_engine
    opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    ema = eng.make_ema(0.9)
    start = _np(ema.tensors)
    _run(eng, BATCH, 0, 2, opt, ema=ema)
    assert ema.num_updates == 0 and all(np.array_equal(M.bits(s.cpu().numpy()), M.bits(a)) for s, a in zip(ema.tensors, start))
    _run(eng, BATCH, 1, 2, opt, ema=ema)
    now = _np(eng.trainable_parameters())
    assert ema.num_updates == 1 and any(not np.array_equal(a, b) for a, b in zip(now, start))
    for s, a, p in zip(ema.tensors, start, now):
        assert np.array_equal(M.bits(s.cpu().numpy()), M.bits(M.update_f32(a, p, M.weight_at(0.9, False, 0))))


# ---- 6. evaluation on the averaged weights ---------------------------------------------------------------------------------------
def _trained(precision="bf16"):
    """a model two steps into training and its average (decay 0.5: the shadows are neither the start nor the parameters)"""
    from cara_amd.optim import AdamW
    x, y, dp = _batch()
    m = _model(precision)
    eng = m._cara_engine
    opt = AdamW(eng.trainable_parameters(), lr=1e-2, weight_decay=1e-4)
    ema = eng.make_ema(0.5)
    for _ in range(2):
        eng.train_step(x, y, opt, droppath=dp, ema=ema)
    assert all(not _same(s, p) for s, p in zip(ema.tensors[:1], eng.trainable_parameters()[:1]))
    return m, ema


def _split5():
    from cara_amd.data import ResidentSplit
    from tests.test_resident_feed_gpu import _split_cpu
    px, labels = _split_cpu()
    return ResidentSplit.from_tensors(px[:5].to(DEV), labels[:5].to(DEV))


def _logits_of(eng, split, **kw):
    seen = []
    out = eng.evaluate(split, BATCH, debug_hook=lambda lg, lb, nv: seen.append((lg.clone(), nv)), **kw)
    return out, seen


@pytest.mark.parametrize("precision", PRECISIONS)
def test_evaluate_and_forward_resident_on_the_averaged_weights(precision):
    from cara_amd._lib import CaraError
    from cara_amd.ema import ParamEma
    m, ema = _trained(precision)
    eng = m._cara_engine
    split = _split5()
    own_out, own = _logits_of(eng, split)
    before = _np(eng.trainable_parameters())
    shadows = _np(ema.tensors)
    ws_before = eng.eval_workspace_bytes()
    # the yardstick: a second model whose trainable tensors were overwritten with the shadows
    other = _model(precision)
    ema.copy_to(other._cara_engine.trainable_parameters())
    want_out, want = _logits_of(other._cara_engine, split)
    got_out, got = _logits_of(eng, split, weights=ema)
    assert [nv for _, nv in got] == [4, 1] and len(want) == 2
    assert all(_same(a[0], b[0]) for a, b in zip(got, want)) and got_out == want_out and got_out["n"] == 5
    assert not all(_same(a[0], b[0]) for a, b in zip(got, own))                     # (the average is not the iterate)
    assert eng.eval_workspace_bytes() == ws_before                                   # the same workspace
    # nothing of the model moved, the shadows neither
    assert all(np.array_equal(M.bits(p), M.bits(q)) for p, q in zip(_np(eng.trainable_parameters()), before))
    assert all(np.array_equal(M.bits(p), M.bits(q)) for p, q in zip(_np(ema.tensors), shadows))
    again_out, again = _logits_of(eng, split)
    assert again_out == own_out and all(_same(a[0], b[0]) for a, b in zip(again, own))
    # forward_resident (the model is in eval mode now: no DropPath)
    rows = torch.tensor([4, 0, 2, 2], device=DEV)
    a = eng.forward_resident(split, rows, weights=ema)
    b = other._cara_engine.forward_resident(split, rows)
    c = eng.forward_resident(split, rows)
    assert _same(a, b) and not _same(a, c)
    assert all(np.array_equal(M.bits(p), M.bits(q)) for p, q in zip(_np(eng.trainable_parameters()), before))
    # weights that do not match the model
    with pytest.raises(CaraError):
        eng.evaluate(split, BATCH, weights=ParamEma(eng.trainable_parameters()[:3]))
    with pytest.raises(CaraError):
        eng.forward_resident(split, rows, weights=[t for t in ema.tensors])
    wrong = ParamEma([torch.zeros(p.shape[::-1], device=DEV) if p.ndim == 2 and p.shape[0] != p.shape[1] else torch.zeros_like(p)
                      for p in eng.trainable_parameters()])
    with pytest.raises(CaraError):
        eng.evaluate(split, BATCH, weights=wrong)


# ---- 7. graph replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_replays_follow_the_warming_up_decay_bitwise(precision):
    from cara_amd._lib import CaraError
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    x, y, _ = _batch()
    out = {}
    for mode in ("eager", "graph"):
        m = _model(precision, drop_path_rate=0.0)
        eng = m._cara_engine
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        ema = eng.make_ema(0.9998, warmup=True, capturable=(mode == "graph"))
        if mode == "graph":
            with pytest.raises(CaraError):
                GraphedTrainStep(eng, opt, ema=eng.make_ema(0.9998))           # not capturable
            gstep = GraphedTrainStep(eng, opt, ema=ema)
        shadows = []
        for it in range(4):                                                    # warm, capture + replay, replay, replay
            if mode == "graph":
                gstep(x, y)
            else:
                opt.advance()
                eng.train_step(x, y, opt, ema=ema)
            shadows.append([s.clone() for s in ema.tensors])
        if mode == "graph":
            assert len(gstep._graphs) == 1 and all(ent != "warm" for ent in gstep._graphs.values())
        assert ema.num_updates == 4
        out[mode] = (shadows, [p.detach().clone() for p in eng.trainable_parameters()])
    weights = [float(M.weight_at(0.9998, True, t)) for t in range(4)]
    assert len(set(weights)) == 4                                              # a capture that froze the weight fails below
    for it in range(4):
        assert all(_same(a, b) for a, b in zip(out["graph"][0][it], out["eager"][0][it])), it
    assert all(_same(a, b) for a, b in zip(out["graph"][1], out["eager"][1]))
    assert not all(_same(a, b) for a, b in zip(out["eager"][0][2], out["eager"][0][3]))


# ---- 8. checkpoints -------------------------------------------------------------------------------------------------------------
def test_checkpoint_of_the_averaged_weights(tmp_path):
    from cara_amd.recipe import load_checkpoint, save_checkpoint
    m, ema = _trained()
    eng = m._cara_engine
    plain, avg = str(tmp_path / "plain.pt"), str(tmp_path / "avg.pt")
    save_checkpoint(m, plain)
    save_checkpoint(m, avg, weights=ema)
    sd_plain, sd_avg = torch.load(plain, map_location="cpu"), torch.load(avg, map_location="cpu")
    assert list(sd_plain) == list(sd_avg)
    fresh = _model()
    load_checkpoint(fresh, avg)
    assert all(_same(p, s) for p, s in zip(fresh._cara_engine.trainable_parameters(), ema.tensors))
    names = {id(p): n for n, p in m.named_parameters()}
    shadow_of = {names[id(p)]: s.cpu() for p, s in zip(eng.trainable_parameters(), ema.tensors)}
    assert set(shadow_of) == {n for n, _ in m.named_parameters() if "CP" in n or "head" in n} and len(shadow_of) == 14
    own = m.state_dict()
    for k in sd_plain:
        assert torch.equal(sd_plain[k], own[k].cpu()), k
        assert torch.equal(sd_avg[k], shadow_of.get(k, sd_plain[k])), k         # frozen entries are the model's, the rest the shadows
    assert any(not torch.equal(sd_avg[k], sd_plain[k]) for k in shadow_of)
    # evaluate on the loaded model reproduces the scores of the averaged weights
    split = _split5()
    got_out, got = _logits_of(fresh._cara_engine, split)
    want_out, want = _logits_of(eng, split, weights=ema)
    assert got_out == want_out and all(_same(a[0], b[0]) for a, b in zip(got, want))
    # ParamEma.state_dict round trip
    other = fresh._cara_engine.make_ema(0.1, warmup=True)
    other.load_state_dict(ema.state_dict())
    assert (other.num_updates, other.decay, other.warmup) == (2, 0.5, False)
    assert all(_same(a, b) for a, b in zip(other.tensors, ema.tensors))


# ---- fit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eval_mode", ["reference", "sharded"])
def test_fit_scores_and_saves_the_averaged_weights(eval_mode, tmp_path):
    from cara_amd import cara, create_model
    from cara_amd.data import ResidentSplit, normalize_u8
    from cara_amd.recipe import fit, load_checkpoint
    g = torch.Generator().manual_seed(1)
    y = torch.arange(8) % 4
    px = (torch.randn(8, 3, 224, 224, generator=g) * 20 + 40 + 50 * y.float().reshape(-1, 1, 1, 1)).clamp_(0, 255).to(torch.uint8)
    x, px, y = normalize_u8(px).to(DEV), px.to(DEV), y.to(DEV)
    split = ResidentSplit.from_tensors(px, y)

    def make():
        torch.manual_seed(0)
        return cara({"model": create_model("vit_base_patch16_224_in21k", depth=2, num_classes=4, drop_path_rate=0.1), "rank": 8,
                     "scale": 1.0, "l_mu": 1.0, "l_std": 0.0}).to(DEV)
    m = make()
    eng = m._cara_engine
    evals = []

    def score(weights=None):
        return eng.evaluate(split, 256, weights=weights)["top1"]

    def on_eval(epoch, raw, avg):
        params = _np(eng.trainable_parameters())
        if eval_mode == "sharded":
            assert raw == score() and avg == score(eng.ema)
        else:
            with torch.no_grad():
                assert raw == float((m(x).argmax(1) == y).sum()) / 8
                with eng.ema.swapped_in():
                    assert all(p.data_ptr() == s.data_ptr() for p, s in zip(eng.trainable_parameters(), eng.ema.tensors))
                    assert avg == float((m(x).argmax(1) == y).sum()) / 8
        assert all(np.array_equal(M.bits(a), M.bits(b)) for a, b in zip(params, _np(eng.trainable_parameters())))
        assert all(p.data_ptr() != s.data_ptr() for p, s in zip(eng.trainable_parameters(), eng.ema.tensors))
        evals.append((epoch, raw, avg))
    save = {"dataset": "toy", "seed": 3, "dir": str(tmp_path)}
    test = split if eval_mode == "sharded" else (lambda: [(x, y)])
    best, opt = fit(m, lambda epoch: [(x, y)], test, epochs=11, lr=1e-2, seed=3, on_eval=on_eval, eval_mode=eval_mode,
                    save_best=save, ema_decay=0.5, ema_warmup=True)
    assert [e for e, _, _ in evals] == [10] and best == evals[0][2] and eng.ema.num_updates == 11
    assert {float(opt.state[p]["step"]) for p in eng.trainable_parameters()} == {11.0}
    print(f"[{eval_mode}] epoch 10: raw {evals[0][1]}, averaged {evals[0][2]}")
    if best > 0:
        fresh = make()
        load_checkpoint(fresh, save["path"])
        assert all(_same(p, s) for p, s in zip(fresh._cara_engine.trainable_parameters(), eng.ema.tensors))
        assert fresh._cara_engine.evaluate(split, 256)["top1"] == score(eng.ema)
