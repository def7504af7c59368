"""Patch dropout on the host: data.PatchDropout against its definition (timm's PatchDropout, restated), check_keep's refusals, the
seed streams, the host restatement of the dropped forward (tests/patchdrop_model.py) against the oracle on the whole image, and the
workspace layout at 2 <= tokens <= grid + 1.  CPU only."""
import ctypes as C

import pytest
import torch

from cara_amd.data import PatchDropout, aug_seed, box_seed, check_keep, identity_keep, keep_reference, keep_seed, mix_seed
from tests import patchdrop_model as PM
from tests import tolerances as T


@pytest.mark.parametrize("prob", [0.0, 0.25, 0.5, 0.75, 0.99])
@pytest.mark.parametrize("P", [16, 36, 196])
def test_draw_keeps_k_distinct_patches_per_sample(prob, P):
    B, steps = 3, 4
    K = max(1, int(P * (1 - prob)))
    pd = PatchDropout(prob)
    assert pd.num_keep(P) == K
    t = pd.draw(P, B, steps, torch.Generator().manual_seed(5))
    assert t.dtype == torch.int32 and tuple(t.shape) == (steps, B, K) and t.is_contiguous()
    assert int(t.min()) >= 0 and int(t.max()) < P
    for row in t.reshape(-1, K):
        assert len(set(row.tolist())) == K
    check_keep(t, B, P)
    # the definition: the first K of argsort(randn(P)) per sample, from the same generator
    noise = torch.randn(steps * B * P, generator=torch.Generator().manual_seed(5)).reshape(steps, B, P)
    assert torch.equal(t.to(torch.int64), torch.argsort(noise, dim=-1)[..., :K])
    # ordered: the same sets, ascending
    o = PatchDropout(prob, ordered=True).draw(P, B, steps, torch.Generator().manual_seed(5))
    assert torch.equal(o, t.sort(dim=-1).values)
    # the same seed gives the same table, another seed another (where there is anything to draw)
    assert torch.equal(pd.draw(P, B, steps, torch.Generator().manual_seed(5)), t)
    if 1 < K < P:
        assert not torch.equal(pd.draw(P, B, steps, torch.Generator().manual_seed(6)), t)
        assert not torch.equal(t, t.sort(dim=-1).values)          # timm's default is unordered


def test_prob_zero_keeps_every_patch_and_the_grid_follows_size_and_patch():
    t = PatchDropout(0.0, ordered=True).draw(16, 2, 1)
    assert torch.equal(t[0], identity_keep(2, 16))
    assert torch.equal(identity_keep(2, 16, steps=3)[2], identity_keep(2, 16))
    assert PatchDropout(0.25, size=224, patch=16).grid == 196 and PatchDropout(0.25, size=(96, 64)).grid == 24
    assert PatchDropout(0.25, grid=36).grid == 36 and PatchDropout(0.25).grid is None
    for bad in (dict(prob=1.0), dict(prob=-0.1), dict(prob=float("nan")), dict(prob=0.5, size=100), dict(prob=0.5, grid=0)):
        with pytest.raises(ValueError):
            PatchDropout(**bad)


def test_keep_seed_is_a_stream_of_its_own():
    seen = {}
    for seed in (0, 1):
        for epoch in range(4):
            for rank in range(4):
                k = keep_seed(seed, epoch, rank)
                assert 0 <= k < 2 ** 32
                assert k not in (box_seed(seed, epoch, rank), mix_seed(seed, epoch, rank), aug_seed(seed, epoch, rank))
                seen[(seed, epoch, rank)] = k
    assert len(set(seen.values())) == len(seen)
    others = {f(s, e, r) for f in (box_seed, mix_seed, aug_seed) for s in (0, 1) for e in range(4) for r in range(4)}
    assert not others & set(seen.values())


def test_check_keep_refuses_what_the_host_must_not_upload():
    good = torch.tensor([[3, 0, 15, 7], [1, 2, 4, 8]], dtype=torch.int32)
    check_keep(good, 2, 16)
    check_keep(good[None], 2, 16)
    for bad in ([[3, 0, 3, 7], [1, 2, 4, 8]], [[3, 0, 16, 7], [1, 2, 4, 8]], [[3, 0, -1, 7], [1, 2, 4, 8]]):
        with pytest.raises(ValueError):
            check_keep(torch.tensor(bad, dtype=torch.int32), 2, 16)
    with pytest.raises(ValueError):
        check_keep(good.to(torch.int64), 2, 16)                   # dtype
    with pytest.raises(ValueError):
        check_keep(good, 3, 16)                                   # batch
    with pytest.raises(ValueError):
        check_keep(good, 2, 3)                                    # wider than the grid
    with pytest.raises(ValueError):
        check_keep(good[:, :0], 2, 16)                            # K = 0


def test_keep_reference_is_the_gather():
    x = torch.arange(2 * 5 * 3, dtype=torch.float32).reshape(2, 5, 3)
    keep = torch.tensor([[4, 0], [1, 3]], dtype=torch.int32)
    got = keep_reference(x, keep)
    assert torch.equal(got, torch.stack([x[0, [4, 0]], x[1, [1, 3]]]))


def test_train_rows_yields_a_fifth_element():
    from cara_amd.data import ResidentSplit
    g = torch.Generator().manual_seed(2)
    split = ResidentSplit.from_tensors(torch.randint(0, 256, (16, 3, 32, 32), generator=g, dtype=torch.uint8), torch.arange(16))
    pd = PatchDropout(0.5, size=32, patch=16)
    feed = split.train_rows(4, seed=3, rank=0, world=1, patch_drop=pd)
    e0, e1 = list(feed(0)), list(feed(1))
    assert len(e0) == 4 and all(len(item) == 5 and item[1] is None and item[2] is None and item[3] is None for item in e0)
    assert all(tuple(item[4].shape) == (4, 2) and item[4].dtype == torch.int32 and item[4].is_contiguous() for item in e0)
    table = torch.stack([item[4] for item in e0])
    assert torch.equal(table, pd.draw(4, 4, 4, torch.Generator().manual_seed(keep_seed(3, 0, 0))))
    assert not torch.equal(table, torch.stack([item[4] for item in e1]))
    plain = list(split.train_rows(4, seed=3, rank=0, world=1)(0))
    assert all(torch.equal(a[0], b) for a, b in zip(e0, plain))   # the index vectors are the ones they were
    with pytest.raises(ValueError):
        split.train_rows(4, patch_drop=PatchDropout(0.5))         # no grid


def test_the_restatement_with_every_patch_kept_is_the_oracle_on_the_whole_image():
    from oracle import cara_oracle as O
    depth, img = 2, 64
    w = O.synthetic_backbone(depth=depth, img=img)
    cp = O.synthetic_cp(rank=16, depth=depth)
    x, _ = O.synthetic_batch(batch=2, img=img)
    keep = identity_keep(2, 16)
    with torch.no_grad():
        want = O.vit_cara_forward(x, w, cp, s=0.1, depth=depth)
        got = PM.dropped_forward(x, w, cp, keep, s=0.1, depth=depth)
    assert float((got - want).abs().max()) <= T.HOST_ATOL
    # and a permutation of the tokens changes nothing behind the position embedding but the summation order
    perm = torch.stack([torch.randperm(16, generator=torch.Generator().manual_seed(b)) for b in range(2)]).to(torch.int32)
    with torch.no_grad():
        got = PM.dropped_forward(x, w, cp, perm, s=0.1, depth=depth)
    assert float((got - want).abs().max()) <= 10 * T.HOST_ATOL
    assert torch.equal(PM.kept_image(x[0], keep[0]), x[0])


@pytest.mark.parametrize("K", [9, 16])
def test_the_rounding_model_itself_is_inside_the_logit_bound_on_the_device_tests_inputs(K):
    """before the GPU run: the restatement with the bf16 build's rounding points against the fp32 restatement, on the inputs of
    tests/test_patchdrop_gpu.py case 5 -- were r_model above LOGITS_ABS, no device could pass logits_ok there"""
    from oracle import cara_oracle as O
    from tests.test_model_gpu import rel
    w, cp = O.synthetic_backbone(depth=2, img=96), O.synthetic_cp(rank=16, depth=2)
    x, _, keep = PM.case5_inputs(K)
    with torch.no_grad():
        ref = PM.dropped_forward(x, w, cp, keep, s=0.1, depth=2)
        sim = PM.dropped_forward(x, w, cp, keep, s=0.1, depth=2, factored=True, bf16_sim=True)
    r_model = rel(sim, ref)
    print(f"K = {K}: r_model {r_model:.2e}")
    assert T.logits_ok(r_model, r_model) and r_model > 0


def _bytes(img, tokens, batch=3, depth=2, inference=0):
    from cara_amd import _lib
    geom = _lib.Geom(depth, 768, 12, 16, 32, 0.1, 4)
    shape = _lib.VitShape(batch, img, 16, 3, tokens, 100, 1e-6, 0, 0.1, 0, inference)
    return int(_lib.lib().cara_vit_workspace_bytes(C.byref(geom), C.byref(shape)))


@pytest.mark.parametrize("img", [64, 96])
def test_workspace_layout_takes_any_token_count_up_to_the_grid(img):
    P = (img // 16) ** 2
    ks = sorted({1, 9, 16, P})
    sizes = [_bytes(img, 1 + K) for K in ks]
    assert all(s > 0 for s in sizes), sizes
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert _bytes(img, P + 2) == 0 and _bytes(img, 1) == 0 and _bytes(img, 0) == 0
    inf = [_bytes(img, 1 + K, inference=1) for K in ks]
    assert all(0 < i < s for i, s in zip(inf, sizes))


def test_workspace_sizes_at_the_full_grid_are_what_they_were():
    from cara_amd import _lib
    geom = _lib.Geom(2, 768, 12, 16, 32, 0.1, 4)
    shape = _lib.VitShape(2, 384, 16, 3, 577, 100, 1e-6, 0, 0.1, 0)
    assert int(_lib.lib().cara_vit_workspace_bytes(C.byref(geom), C.byref(shape))) == 154016256      # tests/test_long_sequence.py
    # a kept subset at 384 px: the workspace of the 224-px model with as many tokens, but for nothing (the layout reads `tokens` only)
    shape.tokens = 197
    small = _lib.VitShape(2, 224, 16, 3, 197, 100, 1e-6, 0, 0.1, 0)
    assert int(_lib.lib().cara_vit_workspace_bytes(C.byref(geom), C.byref(shape))) == \
        int(_lib.lib().cara_vit_workspace_bytes(C.byref(geom), C.byref(small))) > 0
