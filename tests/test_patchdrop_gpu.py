"""GPU side of the patch dropout.  The keep kernels against the existing calls (a kept row is bit for bit the row of the same patch),
guards and bad entries; cara_assemble_tokens_keep against the torch expression; the identity table against the step without one;
one subset for all samples against the smaller model (bit for bit); different subsets against the oracle's restatement
(tests/patchdrop_model.py); sample isolation; refusals.  ViT-B geometry, depth 2, rank 16, patch 16, 64 / 96 px, batch 3."""
import ctypes as C
import functools

import pytest
import torch

from tests import aug_model as G
from tests import patchdrop_model as PM
from tests import test_mix_gpu as T
from tests import tolerances as TOL
from tests.test_augmented_feed_gpu import DEV, SENTINEL, L, _norm

pytestmark = pytest.mark.gpu
OPERANDS = ["bf16", "fp16"]
B, P16, KCOLS = 3, 16, 768
ROWS = [3, 0, 3]
BOXES = [(0, 0, 72, 80, 0), (5, 7, 40, 33, 1), (8, 16, 64, 64, 0)]              # in an 80 x 72 source (Hs = 80, Ws = 72)
MIX = T.table([(2, 0, 0, 0, 0, 0.25, 0.25), (0, 6, 3, 29, 11, 0.0, 0.1), (2, 0, 0, 0, 0, 0.0, 0.0)])
AUG = G.table([G.row([(2, 1.3), (3, 0.7), (1, 1.1)], erase=(3, 5, 40, 30), emode=1, eseed=99), G.row([(1, 0.8)]),
               G.row([(3, 1.4), (2, 0.6)], erase=(20, 0, 12, 64), emode=1, eseed=3)])
SOURCES = ["fp32", "rows", "crop", "mix", "crop+mix+aug"]


@functools.lru_cache(maxsize=None)
def _pixels(Hs, Ws):
    return torch.randint(0, 256, (5, 3, Hs, Ws), generator=torch.Generator().manual_seed(31), dtype=torch.uint8)


def _keep_table(K, P=P16, seed=0):
    """unordered, different per sample"""
    return torch.stack([torch.randperm(P, generator=torch.Generator().manual_seed(seed + b))[:K] for b in range(B)]).to(torch.int32)


def _guarded(nel):
    buf = torch.full((nel + 128,), SENTINEL, dtype=torch.int16, device=DEV)
    return buf, buf[64:64 + nel]


def _guards_ok(buf, nel):
    return bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + nel:] == SENTINEL).all())


def _rows_of(lib, dt, source, keep, bad=None, rows=ROWS, img=64):
    """patch rows [B, K or P, 768] of `source`, by the keep entry (keep given) or the existing one, between checked guards"""
    ptr, st = L().ptr, L().stream
    K = (img // 16) ** 2 if keep is None else keep.shape[1]
    nel = B * K * KCOLS
    buf, got = _guarded(nel)
    kd = None if keep is None else keep.to(DEV)
    if source == "fp32":
        x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(4)).to(DEV)
        if keep is None:
            L().check(lib.cara_im2col_patches(ptr(x), ptr(got), B, 3, img, img, 16, st()), "cara_im2col_patches")
        else:
            L().check(lib.cara_im2col_patches_keep(ptr(x), ptr(kd), K, ptr(got), ptr(bad), B, 3, img, img, 16, st()), "cara_im2col_patches_keep")
    else:
        crop = "crop" in source
        px = _pixels(80, 72).to(DEV) if crop else _pixels(img, img).to(DEV)
        idx = torch.tensor(rows, device=DEV)
        bx = torch.tensor(BOXES, dtype=torch.int32, device=DEV) if crop else None
        mx = MIX.to(DEV) if "mix" in source else None
        ag = AUG.to(DEV) if "aug" in source else None
        stat = torch.empty(int(lib.cara_aug_stat_bytes(B)) // 4, device=DEV)
        mean, std = _norm()
        if keep is None:
            L().check(lib.cara_im2col_patches_u8_rows_aug(ptr(px), 5, px.shape[2], px.shape[3], ptr(idx), ptr(bx), ptr(mx), ptr(ag), ptr(stat), ptr(mean),
                                                          ptr(std), ptr(got), ptr(bad), B, 3, img, img, 16, st()), "cara_im2col_patches_u8_rows_aug")
        else:
            L().check(lib.cara_im2col_patches_u8_rows_keep(ptr(px), 5, px.shape[2], px.shape[3], ptr(idx), ptr(bx), ptr(mx), ptr(ag), ptr(stat), ptr(kd), K,
                                                           ptr(mean), ptr(std), ptr(got), ptr(bad), B, 3, img, img, 16, st()),
                      "cara_im2col_patches_u8_rows_keep")
    torch.cuda.synchronize()
    assert _guards_ok(buf, nel), source
    return got.view(dt).view(B, K, KCOLS)


# ---- 1. patch rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("source", SOURCES)
def test_a_kept_row_is_bitwise_the_row_of_the_call_without_keep(source, operands):
    from cara_amd.data import keep_reference
    lib, dt = L().lib(operands), L().act_dtype(operands)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    full = _rows_of(lib, dt, source, None, bad)
    assert len({tuple(r.tolist()) for r in full.view(torch.int16)[0, :, :8]}) == P16          # the rows differ: a gather is visible
    for K in (1, 5, 16):
        keep = _keep_table(K)
        got = _rows_of(lib, dt, source, keep, bad)
        assert T._same(got, keep_reference(full, keep)), (source, K)
    assert int(bad) == 0
    # entries -1 and P: zero rows, one count each; the other rows as they were
    keep = _keep_table(5)
    keep[0, 2], keep[2, 0], keep[2, 4] = -1, P16, 2 ** 31 - 1
    ok = torch.ones(B, 5, dtype=torch.bool)
    ok[0, 2] = ok[2, 0] = ok[2, 4] = False
    got = _rows_of(lib, dt, source, keep, bad)
    want = keep_reference(full, keep.clamp(0, P16 - 1))
    assert int(bad) == 3 and not got[~ok].view(torch.int16).any() and T._same(got[ok], want[ok])
    got = _rows_of(lib, dt, source, keep, None)                                              # a NULL counter is allowed
    assert not got[~ok].view(torch.int16).any() and T._same(got[ok], want[ok])
    if source != "fp32":
        # a bad `rows` index: K zero rows, counted once, whatever its keep entries are; with a partner (mix) the partner's too
        bad.zero_()
        got = _rows_of(lib, dt, source, keep, bad, rows=[3, 5, 3])
        assert not got[1].view(torch.int16).any()
        hit = [1] + ([b for b in range(B) if int(MIX[b, 0]) == 1 and b != 1] if "mix" in source else [])
        assert int(bad) == len(hit) + sum(int((~ok[b]).sum()) for b in range(B) if b not in hit)


# ---- 2. assembly -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5, 16])
def test_assembly_adds_the_kept_patchs_own_position(K):
    lib = L().lib("bf16")
    g = torch.Generator().manual_seed(9)
    D = 768
    emb, cls, pos = torch.randn(B * K, D, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV), torch.randn(1 + P16, D, generator=g).to(DEV)
    keep = _keep_table(K)
    if K > 1:
        keep[1, 0], keep[2, K - 1] = -1, P16
    kd = keep.to(DEV)
    nel = B * (1 + K) * D
    buf = torch.full((nel + 64,), 12345.0, device=DEV)
    x = buf[32:32 + nel]
    ptr = L().ptr
    L().check(lib.cara_assemble_tokens_keep(ptr(emb), ptr(cls), ptr(pos), ptr(kd), ptr(x), B, K, P16, D, L().stream()), "cara_assemble_tokens_keep")
    torch.cuda.synchronize()
    assert bool((buf[:32] == 12345.0).all()) and bool((buf[32 + nel:] == 12345.0).all())
    inside = ((kd >= 0) & (kd < P16))[..., None]
    rows = emb.view(B, K, D) + torch.where(inside, pos[(1 + kd.clamp(0, P16 - 1)).long()], torch.zeros((), device=DEV))
    want = torch.cat([(cls + pos[0]).expand(B, 1, D), rows], dim=1)
    assert torch.equal(x.view(B, 1 + K, D), want)
    # the identity table is cara_assemble_tokens
    if K == P16:
        from cara_amd.data import identity_keep
        y = torch.empty_like(x)
        L().check(lib.cara_assemble_tokens_keep(ptr(emb), ptr(cls), ptr(pos), ptr(identity_keep(B, P16).to(DEV)), ptr(x), B, K, P16, D, L().stream()), "keep")
        L().check(lib.cara_assemble_tokens(ptr(emb), ptr(cls), ptr(pos), ptr(y), B, P16, D, L().stream()), "cara_assemble_tokens")
        assert torch.equal(x, y)
    assert lib.cara_assemble_tokens_keep(ptr(emb), ptr(cls), ptr(pos), ptr(kd), ptr(x), B, P16 + 1, P16, D, L().stream()) == 1
    assert lib.cara_assemble_tokens_keep(ptr(emb), ptr(cls), ptr(pos), None, ptr(x), B, K, P16, D, L().stream()) == 1


# ---- whole model -----------------------------------------------------------------------------------------------------------------
DEPTH = 2


@functools.lru_cache(maxsize=None)
def _weights(img, cp_length=4):
    from oracle import cara_oracle as O
    return O.synthetic_backbone(depth=DEPTH, img=img), O.synthetic_cp(rank=16, depth=DEPTH, cp_length=cp_length)


def _model(img, precision="bf16", pos=None, cp_length=4, **eng_kw):
    """the depth-2 model at `img` px; `pos`: another pos_embed (the smaller model's rows of the larger one's)"""
    from tests.test_model_gpu import build
    w, cp = _weights(96, cp_length)
    w = dict(w)
    if pos is not None:
        w["pos_embed"] = pos
    elif img != 96:
        w["pos_embed"] = _weights(img)[0]["pos_embed"]
    m = build(w, cp, 16, 0.1, DEPTH, img, drop_path_rate=0.0, cp_length=cp_length, precision=precision).train()
    for k, v in eng_kw.items():
        setattr(m._cara_engine, k, v)
    return m


def _batch(img, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, img, img, generator=g), torch.randint(0, 100, (B,), generator=g)


def _trainable(m):
    return {n: p.detach().clone() for n, p in m.named_parameters() if "CP" in n or "head" in n}


def _step(m, run, opt=True):
    """-> (loss, flat gradient, trainable tensors after one AdamW step) of run(engine, optimizer)"""
    from cara_amd.optim import AdamW
    eng = m._cara_engine
    o = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4) if opt else None
    loss = run(eng, o).clone()
    assert eng.resident_bad_rows() == 0
    return loss, eng._flat_grad.clone(), _trainable(m)


def _assert_same_step(a, b, tensors=14):
    assert torch.equal(a[0], b[0]) and torch.isfinite(a[0])
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and bool(a[1].any())
    assert a[2].keys() == b[2].keys() and len(a[2]) == tensors     # 12 CP tensors (11 at cp_length 3) and the head's two
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def _split(Hs, Ws):
    from cara_amd.data import ResidentSplit
    return ResidentSplit.from_tensors(_pixels(Hs, Ws).to(DEV), torch.tensor([7, 1, 99, 42, 0], device=DEV))


# ---- 3. the identity table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", OPERANDS)
def test_the_identity_table_is_bitwise_the_step_without_one(precision):
    from cara_amd.data import identity_keep
    ident = identity_keep(B, P16).to(DEV)
    x, y = _batch(64)
    x, y = x.to(DEV), y.to(DEV)
    a = _step(_model(64, precision), lambda e, o: e.train_step(x, y, o, keep=ident))
    b = _step(_model(64, precision), lambda e, o: e.train_step(x, y, o))
    _assert_same_step(a, b)
    m1, m2 = _model(64, precision), _model(64, precision)
    with torch.no_grad():
        l1 = m1._cara_engine._run_forward(x, None, m1.head.weight, m1.head.bias, m1._cara_engine.trainable_parameters()[:-2], False, keep=ident)
        l2 = m2._cara_engine._run_forward(x, None, m2.head.weight, m2.head.bias, m2._cara_engine.trainable_parameters()[:-2], False)
    assert torch.equal(l1, l2)
    # the resident feed with boxes, mix and aug present
    idx = torch.tensor(ROWS, device=DEV)
    tables = dict(boxes=torch.tensor(BOXES, dtype=torch.int32, device=DEV), mix=MIX.to(DEV), aug=AUG.to(DEV), label_smoothing=0.1)
    a = _step(_model(64, precision), lambda e, o: e.train_step_resident(_split(80, 72), idx, o, keep=ident, **tables))
    b = _step(_model(64, precision), lambda e, o: e.train_step_resident(_split(80, 72), idx, o, **tables))
    _assert_same_step(a, b)


# ---- 4. one subset for all samples = the smaller model ---------------------------------------------------------------------------
CASES4 = [("bf16", {}, 4), ("fp16", {}, 4), ("bf16", dict(weight_dropout="exact", weight_dropout_seed=1234), 4), ("bf16", {}, 3)]


@pytest.mark.parametrize("precision,eng_kw,cp_length", CASES4)
def test_one_subset_for_all_samples_is_bitwise_the_smaller_model(precision, eng_kw, cp_length):
    """img 96, K = 16, one unordered index row for the whole batch, against a model at 64 px whose pos_embed is rows [0] + (1 + keep)
    of the first and whose input is the image built from the kept patches: behind the embedding the launches are the same ones on
    the same numbers."""
    row = torch.randperm(36, generator=torch.Generator().manual_seed(3))[:16].to(torch.int32)
    assert not torch.equal(row, row.sort().values)
    keep = row.expand(B, 16).contiguous()
    pos_small = PM.kept_pos(_weights(96)[0]["pos_embed"], row)
    # fp32 feed: rearranged pixels
    x, y = _batch(96)
    xs = torch.stack([PM.kept_image(x[b], row) for b in range(B)])
    big = _step(_model(96, precision, cp_length=cp_length, **eng_kw), lambda e, o: e.train_step(x.to(DEV), y.to(DEV), o, keep=keep.to(DEV)))
    small = _step(_model(64, precision, pos=pos_small, cp_length=cp_length, **eng_kw), lambda e, o: e.train_step(xs.to(DEV), y.to(DEV), o))
    _assert_same_step(big, small, 13 if cp_length == 3 else 14)
    lb, ls = _model(96, precision, cp_length=cp_length, **eng_kw), _model(64, precision, pos=pos_small, cp_length=cp_length, **eng_kw)
    with torch.no_grad():
        a = lb._cara_engine._run_forward(x.to(DEV), None, lb.head.weight, lb.head.bias, lb._cara_engine.trainable_parameters()[:-2], False, keep=keep.to(DEV))
        b = ls._cara_engine._run_forward(xs.to(DEV), None, ls.head.weight, ls.head.bias, ls._cara_engine.trainable_parameters()[:-2], False)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # resident feed: rearranged uint8 pixels
    from cara_amd.data import ResidentSplit
    px = _pixels(96, 96)
    labels = torch.tensor([7, 1, 99, 42, 0], device=DEV)
    sp_big = ResidentSplit.from_tensors(px.to(DEV), labels)
    sp_small = ResidentSplit.from_tensors(torch.stack([PM.kept_image(px[i], row) for i in range(5)]).to(DEV), labels)
    idx = torch.tensor(ROWS, device=DEV)
    big = _step(_model(96, precision, cp_length=cp_length, **eng_kw), lambda e, o: e.train_step_resident(sp_big, idx, o, keep=keep.to(DEV)))
    small = _step(_model(64, precision, pos=pos_small, cp_length=cp_length, **eng_kw), lambda e, o: e.train_step_resident(sp_small, idx, o))
    _assert_same_step(big, small, 13 if cp_length == 3 else 14)
    assert torch.equal(lb._cara_engine.forward_resident(sp_big, idx, keep=keep.to(DEV)), ls._cara_engine.forward_resident(sp_small, idx))


# ---- 5. different subsets against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [9, 16])
def test_different_subsets_per_sample_against_the_oracle(K):
    """bf16 build, img 96.  Logits through tolerances.logits_ok (the fp32 restatement and the same restatement with the build's rounding
    points give r_ref and r_model), every CP and head gradient within CP_GRAD; the full-token step of the same model printed beside
    them as a control."""
    from oracle import cara_oracle as O
    from tests.test_model_gpu import rel
    w, cp = _weights(96)
    head = {"weight": w["head.weight"], "bias": w["head.bias"]}
    x, y, keep = PM.case5_inputs(K)          # (tests/test_patchdrop_model.py holds the rounding model to the bounds on these, on the host)
    m = _model(96)
    eng = m._cara_engine
    with torch.no_grad():
        logits = eng._run_forward(x.to(DEV), None, m.head.weight, m.head.bias, eng.trainable_parameters()[:-2], False, keep=keep.to(DEV))
        sim = PM.dropped_forward(x, w, cp, keep, s=0.1, depth=DEPTH, factored=True, bf16_sim=True)
    loss = eng.train_step(x.to(DEV), y.to(DEV), None, keep=keep.to(DEV))
    rloss, ref, gref = PM.dropped_train_step(x, y, w, cp, head, keep, s=0.1, depth=DEPTH)
    r_ref, r_model = rel(logits, ref), rel(sim, ref)
    worst = max(rel(getattr(m, n).grad, gref[n][:getattr(m, n).shape[0]]) for n in O.CP_NAMES)
    rh = max(rel(m.head.weight.grad, gref["head.weight"]), rel(m.head.bias.grad, gref["head.bias"]))
    # the control: the full-token step of the same model
    m2 = _model(96)
    e2 = m2._cara_engine
    with torch.no_grad():
        full = e2._run_forward(x.to(DEV), None, m2.head.weight, m2.head.bias, e2.trainable_parameters()[:-2], False)
        fsim = O.vit_cara_forward(x, w, cp, s=0.1, depth=DEPTH, factored=True, bf16_sim=True)
    e2.train_step(x.to(DEV), y.to(DEV), None)
    _, fref, fg = O.train_step_as_written(x, y, w, cp, head, s=0.1, depth=DEPTH)
    fworst = max(rel(getattr(m2, n).grad, fg[n][:getattr(m2, n).shape[0]]) for n in O.CP_NAMES)
    print(f"K = {K}: logits r_ref {r_ref:.2e} r_model {r_model:.2e}, worst CP gradient {worst:.2e}, head {rh:.2e}, loss {loss.item():.5f} vs "
          f"{float(rloss):.5f}; control (36 patches): r_ref {rel(full, fref):.2e} r_model {rel(fsim, fref):.2e}, worst CP gradient {fworst:.2e}")
    assert TOL.logits_ok(r_ref, r_model), (r_ref, r_model)
    assert worst < TOL.CP_GRAD and rh < TOL.CP_GRAD, (worst, rh)
    assert not torch.equal(logits, full)


# ---- 6. sample isolation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", OPERANDS)
def test_another_keep_row_for_one_sample_leaves_the_others_logits_alone(precision):
    x, _ = _batch(96, seed=5)
    m = _model(96, precision)
    eng = m._cara_engine
    cp = eng.trainable_parameters()[:-2]
    keep = _keep_table(9, P=36, seed=60)
    other = keep.clone()
    other[1] = torch.randperm(36, generator=torch.Generator().manual_seed(77))[:9].to(torch.int32)
    assert not torch.equal(other[1].sort().values, keep[1].sort().values)
    with torch.no_grad():
        a = eng._run_forward(x.to(DEV), None, m.head.weight, m.head.bias, cp, False, keep=keep.to(DEV)).clone()
        b = eng._run_forward(x.to(DEV), None, m.head.weight, m.head.bias, cp, False, keep=other.to(DEV)).clone()
    assert torch.equal(a[[0, 2]], b[[0, 2]]) and not torch.equal(a[1], b[1]) and bool(torch.isfinite(a).all())


# ---- the position table is never read past its end --------------------------------------------------------------------------------
def test_images_larger_than_the_models_get_a_position_table_padded_with_zero_rows():
    """the assembly kernels add row t (or 1 + keep[b][j]) of pos_embed without knowing its length: for images with more patches than
    the model has positions the engine hands them a zero-padded copy (only the state is built here: no forward runs)"""
    m = _model(64)
    eng = m._cara_engine
    with pytest.warns(UserWarning, match="pos_embed"):
        eng._state(m, B, 96, torch.device(DEV, torch.cuda.current_device()))
    t, w = eng._ingested
    own = m.pos_embed.detach().reshape(-1, 768)
    assert tuple(t["pos"].shape) == (37, 768) and torch.equal(t["pos"][:17], own) and not bool(t["pos"][17:].any())
    assert w.pos == t["pos"].data_ptr()
    eng._state(m, B, 64, torch.device(DEV, torch.cuda.current_device()))       # the model's own size: the table stays
    assert tuple(eng._ingested[0]["pos"].shape) == (37, 768)


# ---- 9. fit (eager; the graphed step refuses the table) --------------------------------------------------------------------------
def test_fit_over_a_resident_feed_with_a_patch_dropout_and_evaluation_on_all_tokens():
    from cara_amd.data import MixupCutmix, PatchDropout, RandomResizedCropFlip, ResidentSplit
    from cara_amd.recipe import fit
    g = torch.Generator().manual_seed(12)
    split = ResidentSplit.from_tensors(torch.randint(0, 256, (32, 3, 80, 80), generator=g, dtype=torch.uint8).to(DEV),
                                       torch.randint(0, 100, (32,), generator=g).to(DEV))
    test = ResidentSplit.from_tensors(torch.randint(0, 256, (8, 3, 64, 64), generator=g, dtype=torch.uint8).to(DEV),
                                      torch.randint(0, 100, (8,), generator=g).to(DEV))
    m = _model(64)
    eng = m._cara_engine
    start = _trainable(m)
    feed = split.train_rows(8, seed=5, rank=0, world=1, augment=RandomResizedCropFlip(64), mix=MixupCutmix(64),
                            patch_drop=PatchDropout(0.5, size=64, patch=16))
    seen = [item for e in range(2) for item in feed(e)]
    assert len(seen) == 8 and all(len(item) == 5 and item[3] is None and tuple(item[4].shape) == (8, 8) for item in seen)
    fit(m, (split, feed), None, epochs=2, lr=1e-3, seed=5, feed="resident", label_smoothing=0.1)
    assert torch.isfinite(eng._loss_buf[0]) and float(eng._loss_buf[0]) > 0 and eng.resident_bad_rows() == 0
    assert eng._ws[eng._last_key]["shape"].tokens == 9                  # the steps ran on 1 + 8 tokens
    after = _trainable(m)
    assert all(torch.isfinite(after[n]).all() for n in after) and any(not torch.equal(after[n], start[n]) for n in after)
    # the evaluation sees every patch: its logits are forward_resident's without a table, on the same weights
    got = []
    res = eng.evaluate(test, batch_size=8, debug_hook=lambda logits, y, n: got.append(logits.clone()))
    want = eng.forward_resident(test, torch.arange(8, device=DEV))
    assert res["n"] == 8 and torch.equal(got[0], want)
    # the same feed through the graphed step: fit(graph=True) runs, on 9 tokens, without a bad entry
    m2 = _model(64)
    fit(m2, (split, feed), None, epochs=2, lr=1e-3, seed=5, feed="resident", label_smoothing=0.1, graph=True)
    e2 = m2._cara_engine
    assert torch.isfinite(e2._loss_buf[0]) and e2.resident_bad_rows() == 0 and e2._ws[e2._last_key]["shape"].tokens == 9
    now = _trainable(m2)
    assert all(torch.isfinite(now[n]).all() for n in now) and any(not torch.equal(now[n], start[n]) for n in now)


# ---- 8. the graphed step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["images", "resident"])
def test_graph_replay_rereads_the_keep_table(form):
    """warm, capture + replay, replay, replay with different tables (the last differs from the one before in its keep table alone):
    every loss and the final parameters are the eager run's, bit for bit; another K captures another graph"""
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    x, y = _batch(96)
    x, y = x.to(DEV), y.to(DEV)
    sp = _split(96, 96)
    rows = [torch.tensor(r, device=DEV) for r in ([3, 0, 3], [1, 2, 4], [0, 0, 1], [0, 0, 1])]
    mixes = [T.table([(2 - i, 0, 0, 0, 0, 0.2 * k + 0.1, 0.2 * k + 0.1) for i in range(B)]).to(DEV) for k in (0, 1, 2, 2)]
    keeps = [_keep_table(16, P=36, seed=100 + 7 * k).to(DEV) for k in range(4)]
    other_k = _keep_table(9, P=36, seed=5).to(DEV)
    out = {}
    for mode in ("eager", "graph"):
        m = _model(96)
        eng = m._cara_engine
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        gstep = GraphedTrainStep(eng, opt, label_smoothing=0.1) if mode == "graph" else None
        losses = []
        for it in range(4):
            opt.param_groups[0]["lr"] = 1e-3 * (0.7 ** it)
            if gstep is not None:
                loss = gstep(x, y, keep=keeps[it]) if form == "images" else gstep(sp, (rows[it], None, mixes[it], None, keeps[it]))
            else:
                opt.advance()
                loss = eng.train_step(x, y, opt, keep=keeps[it], label_smoothing=0.1) if form == "images" else \
                    eng.train_step_resident(sp, rows[it], opt, mix=mixes[it], keep=keeps[it], label_smoothing=0.1)
            losses.append(loss.item())
        params = _trainable(m)
        if gstep is not None:
            (ent,) = gstep._graphs.values()
            if form == "resident":
                assert ent[1] is sp and sum(t.numel() * t.element_size() for t in ent[2]) == (8 + 32 + 4 * 16) * B
            else:
                assert ent[1] is None and ent[2][2].numel() * ent[2][2].element_size() == 4 * 16 * B
            # another K: a new key, warm again, the first graph stays
            if form == "images":
                gstep(x, y, keep=other_k)
            else:
                gstep(sp, (rows[0], None, mixes[0], None, other_k))
            assert len(gstep._graphs) == 2 and list(gstep._graphs.values())[1] == "warm"
        assert eng.resident_bad_rows() == 0
        out[mode] = (losses, params)
    print(f"[{form}] losses eager {out['eager'][0]} graph {out['graph'][0]}")
    assert out["graph"][0] == out["eager"][0] and len(set(out["eager"][0])) == 4
    for n in out["eager"][1]:
        assert torch.equal(out["graph"][1][n], out["eager"][1][n]), n


# ---- fit(patch_drop=) on the batches feed ----------------------------------------------------------------------------------------
def test_fit_draws_a_keep_table_per_epoch_for_the_batches_feed():
    """two epochs of four batches, eager, graphed and in accumulation windows of two: the tables are data.PatchDropout's on the
    keep_seed stream of (seed, epoch, rank 0), one row set per batch in order; eager == graphed == the steps by hand, bit for bit"""
    from cara_amd._lib import CaraError
    from cara_amd.data import PatchDropout, keep_seed
    from cara_amd.optim import AdamW
    from cara_amd.recipe import KEEP_AHEAD, CosineLRScheduler, fit
    batches = [tuple(t.to(DEV) for t in _batch(64, seed=20 + i)) for i in range(4)]
    pd = PatchDropout(0.5)
    m = _model(64)
    fit(m, lambda epoch: batches, None, epochs=2, lr=1e-3, seed=9, patch_drop=pd)
    eng = m._cara_engine
    assert eng._ws[eng._last_key]["shape"].tokens == 9 and torch.isfinite(eng._loss_buf[0])
    got = _trainable(m)
    def by_hand(capturable):
        """the same steps without fit (the optimiser in the form fit builds for an eager / a graphed run)"""
        h = _model(64)
        he = h._cara_engine
        he.seed_rank_streams(9, 0)
        opt = AdamW(he.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=capturable)
        sched = CosineLRScheduler(opt, t_initial=100, warmup_t=10, lr_min=1e-5, warmup_lr_init=1e-6, decay_rate=0.1)
        for epoch in range(2):
            table = pd.draw(16, B, KEEP_AHEAD, torch.Generator().manual_seed(keep_seed(9, epoch, 0))).to(DEV)
            for i, (x, y) in enumerate(batches):
                if capturable:
                    opt.advance()
                he.train_step(x, y, opt, keep=table[i])
                sched.step(epoch)
        return _trainable(h)
    want = by_hand(False)
    for n in want:
        assert torch.equal(got[n], want[n]), n
    g = _model(64)
    fit(g, lambda epoch: batches, None, epochs=2, lr=1e-3, seed=9, patch_drop=pd, graph=True)
    now, want = _trainable(g), by_hand(True)
    for n in want:
        assert torch.equal(now[n], want[n]), n
    # accumulation windows of two: one optimiser step per window, every micro-batch on its own rows of the table
    a = _model(64)
    start = _trainable(a)
    _, aopt = fit(a, lambda epoch: batches, None, epochs=1, lr=1e-3, seed=9, patch_drop=pd, accum_steps=2, clip_grad=1.0)
    ae = a._cara_engine
    assert {float(aopt.state[p]["step"]) for p in ae.trainable_parameters()} == {2.0} and ae._ws[ae._last_key]["shape"].tokens == 9
    after = _trainable(a)
    assert all(torch.isfinite(after[n]).all() for n in after) and any(not torch.equal(after[n], start[n]) for n in after)
    with pytest.raises(CaraError):
        fit(a, (_split(64, 64), None), None, epochs=1, feed="resident", patch_drop=pd)
    with pytest.raises(CaraError):
        fit(a, lambda epoch: batches, None, epochs=1, patch_drop=PatchDropout(0.5, size=96))      # another grid than the images'


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_entries_without_keep_refuse_fewer_tokens_than_the_grid_and_the_engine_refuses_bad_tables():
    from cara_amd._lib import CaraError
    m = _model(96)
    eng = m._cara_engine
    x, y = _batch(96)
    x, y = x.to(DEV), y.to(DEV)
    keep = _keep_table(16, P=36).to(DEV)
    eng.train_step(x, y, None, keep=keep)                        # sizes the 17-token workspace and ingests the weights
    st = eng._ws[eng._last_key]
    assert st["shape"].tokens == 17
    torch.cuda.synchronize()
    before = st["ws"].clone()
    logits = torch.full((B, 100), 7.0, device=DEV)
    cps = eng._cp_ptrs([t.detach() for t in eng.trainable_parameters()[:-2]])
    ptr, lib = L().ptr, eng._lib()
    args = (C.byref(st["geom"]), C.byref(st["shape"]), C.byref(eng._ingested[1]), C.byref(cps), ptr(m.head.weight.detach()), ptr(m.head.bias.detach()))
    assert lib.cara_vit_forward(*args, ptr(x), None, ptr(st["ws"]), ptr(logits), L().stream()) == 1
    sp = _split(96, 96)
    idx = torch.tensor(ROWS, device=DEV)
    mean, std = _norm()
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.cara_vit_forward_u8_rows(*args, ptr(sp.pixels), 5, ptr(idx), ptr(mean), ptr(std), None, ptr(st["ws"]), ptr(logits), ptr(bad), L().stream()) == 1
    assert lib.cara_vit_forward_u8_rows_mix(*args, ptr(sp.pixels), 5, 96, 96, ptr(idx), None, ptr(MIX.to(DEV)), ptr(mean), ptr(std), None, ptr(st["ws"]),
                                            ptr(logits), ptr(bad), L().stream()) == 1
    assert lib.cara_vit_forward_keep(*args, ptr(x), None, None, ptr(st["ws"]), ptr(logits), ptr(bad), L().stream()) == 1      # no table
    torch.cuda.synchronize()
    assert torch.equal(st["ws"], before) and bool((logits == 7.0).all()) and int(bad) == 0
    # the engine, before anything is enqueued
    for table in (keep[:, :0], _keep_table(16, P=36).repeat(1, 3)[:, :37].contiguous().to(DEV), keep.to(torch.int64), keep.cpu(), keep[:2],
                  keep.t().contiguous().t()):
        with pytest.raises(CaraError):
            eng.train_step(x, y, None, keep=table)
        with pytest.raises(CaraError):
            eng.train_step_resident(sp, idx, None, keep=table)
        with pytest.raises(CaraError):
            eng.forward_resident(sp, idx, keep=table)
    torch.cuda.synchronize()
    assert torch.equal(st["ws"], before)
    # a kept step and a full step of the same batch have workspaces of their own
    eng._keep_ws = True
    eng.train_step(x, y, None)
    eng.train_step(x, y, None, keep=keep)
    assert sorted(k[-1] for k in eng._ws) == [17, 37]
