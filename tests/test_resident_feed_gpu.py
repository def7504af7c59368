"""GPU side of the resident training feed: the indexed patch-row kernel against cara_im2col_patches_u8 on the gathered
batch, out-of-range rows counted and never read, CaraEngine.train_step_resident against train_step on the CPU-normalised
(correctly rounded) images, fit(feed="resident") against fit over such batches, and a replayed graph that re-reads its
index vector.  Every comparison is bitwise."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEPTH, N_SPLIT = 2, 12
SENTINEL = 0x5a5a     # 16-bit pattern of the guard elements around a patches buffer (not a value the kernels write there)


def L():
    from cara_amd import _lib
    return _lib


def _norm():
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD
    return torch.tensor(IMAGENET_MEAN, device=DEV), torch.tensor(IMAGENET_STD, device=DEV)


def _bytes_everywhere(n, size, seed):
    """uint8 [n,3,size,size] with every byte value in every channel of every image"""
    px = torch.randint(0, 256, (n, 3, size, size), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    px.view(n, 3, -1)[:, :, :256] = torch.arange(256, dtype=torch.uint8)
    return px


def _u8_reference(lib, dt, px_dev, size):
    """patch rows of a contiguous uint8 batch by cara_im2col_patches_u8"""
    B = px_dev.shape[0]
    mean, std = _norm()
    out = torch.empty(B * (size // 16) ** 2, 3 * 256, dtype=dt, device=DEV)
    L().check(lib.cara_im2col_patches_u8(L().ptr(px_dev), L().ptr(mean), L().ptr(std), L().ptr(out), B, 3, size, size, 16, L().stream()),
              "cara_im2col_patches_u8")
    return out


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
@pytest.mark.parametrize("size,n,rows", [(32, 5, [4, 0, 4, 2]), (224, 3, [2, 0, 1])])
def test_indexed_patch_rows_are_bitwise_the_gathered_batch(size, n, rows, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    px = _bytes_everywhere(n, size, seed=size).to(DEV)
    idx = torch.tensor(rows, device=DEV)
    want = _u8_reference(lib, dt, px.index_select(0, idx).contiguous(), size)
    mean, std = _norm()
    nel = want.numel()
    buf = torch.full((nel + 128,), SENTINEL, dtype=torch.int16, device=DEV)
    got = buf[64:64 + nel]
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    L().check(lib.cara_im2col_patches_u8_rows(L().ptr(px), n, L().ptr(idx), L().ptr(mean), L().ptr(std), L().ptr(got), L().ptr(bad),
                                              len(rows), 3, size, size, 16, L().stream()), "cara_im2col_patches_u8_rows")
    torch.cuda.synchronize()
    differ = got != want.view(torch.int16).reshape(-1)
    print(f"indexed patch rows {size} px rows {rows} [{operands}]: {int(differ.sum())} of {nel} elements differ")
    assert not differ.any(), differ.nonzero()[:20].tolist()
    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + nel:] == SENTINEL).all())
    assert int(bad) == 0


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_out_of_range_rows_are_counted_and_never_read(operands):
    """the split is the middle five images of a seven-image allocation (and the middle five labels of seven), so that a read
    at -1 or n_split would land in memory the test owns and show up as a non-zero row / label"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    size, n = 32, 5
    alloc = _bytes_everywhere(7, size, seed=9).to(DEV)
    px = alloc[1:6]
    labels_all = torch.tensor([91, 11, 12, 13, 14, 15, 97], device=DEV)
    labels = labels_all[1:6]
    assert px.is_contiguous() and px.data_ptr() % 4 == 0
    idx = torch.tensor([1, 5, -1, 3], device=DEV)
    mean, std = _norm()
    per = (size // 16) ** 2
    got = torch.ones(4 * per, 3 * 256, dtype=dt, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    L().check(lib.cara_im2col_patches_u8_rows(L().ptr(px), n, L().ptr(idx), L().ptr(mean), L().ptr(std), L().ptr(got), L().ptr(bad),
                                              4, 3, size, size, 16, L().stream()), "cara_im2col_patches_u8_rows")
    torch.cuda.synchronize()
    assert int(bad) == 2
    got = got.view(4, per, -1)
    assert not got[1].view(torch.int16).any() and not got[2].view(torch.int16).any()
    want = _u8_reference(lib, dt, px[[1, 3]].contiguous(), size).view(2, per, -1)
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16))
    assert torch.equal(got[3].view(torch.int16), want[1].view(torch.int16))
    out = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    L().check(lib.cara_gather_labels(L().ptr(labels), n, L().ptr(idx), L().ptr(out), 4, L().ptr(bad), L().stream()), "cara_gather_labels")
    torch.cuda.synchronize()
    assert out.tolist() == [12, 0, 0, 14] and int(bad) == 4
    # a NULL counter is allowed
    L().check(lib.cara_gather_labels(L().ptr(labels), n, L().ptr(idx), L().ptr(out), 4, None, L().stream()), "cara_gather_labels")
    torch.cuda.synchronize()
    assert out.tolist() == [12, 0, 0, 14]
    # argument checks: nothing is launched
    P = L().ptr
    a = dict(pixels=P(px), n=n, rows=P(idx), p=16, size=size)

    def call(**kw):
        v = dict(a, **kw)
        return lib.cara_im2col_patches_u8_rows(v["pixels"], v["n"], v["rows"], P(mean), P(std), P(got), P(bad), 4, 3, v["size"], v["size"],
                                               v["p"], L().stream())
    assert call(rows=None) == 1 and call(n=0) == 1 and call(n=-3) == 1 and call(pixels=None) == 1
    # p % 4 and Wi % 4: Wi is a multiple of p, so a Wi that is no multiple of 4 comes with such a p -- the two conditions
    # cannot be met apart, and these calls are refused by either
    assert call(p=6, size=36) == 1            # p % 4 != 0, Wi % 4 == 0
    assert call(p=2, size=34) == 1            # p % 4 != 0 and Wi % 4 != 0
    assert lib.cara_gather_labels(P(labels), n, None, P(out), 4, P(bad), L().stream()) == 1
    assert lib.cara_gather_labels(P(labels), 0, P(idx), P(out), 4, P(bad), L().stream()) == 1
    torch.cuda.synchronize()
    assert int(bad) == 4


# ---- whole model: depth 2, dim 768, 12 heads, rank 16, the synthetic backbone with a trained-like adapter ----------------------
@functools.lru_cache(maxsize=None)
def _weights():
    from oracle import cara_oracle as O
    return O.synthetic_backbone(depth=DEPTH), O.synthetic_cp(rank=16)     # CP_A2 / CP_P2 non-zero


def _model(precision="bf16", drop_path_rate=0.1):
    from tests.test_model_gpu import build
    w, cp = _weights()
    return build(w, cp, 16, 0.1, DEPTH, 224, drop_path_rate=drop_path_rate, precision=precision)


@functools.lru_cache(maxsize=None)
def _split_cpu():
    """12 images of 224 px whose level and contrast vary per image, and their labels (host tensors: left unchanged)"""
    g = torch.Generator().manual_seed(31)
    level = torch.rand(N_SPLIT, 3, 1, 1, generator=g) * 160 + 40
    contrast = torch.rand(N_SPLIT, 1, 1, 1, generator=g) * 60 + 10
    px = (torch.randn(N_SPLIT, 3, 224, 224, generator=g) * contrast + level).clamp_(0, 255).to(torch.uint8)
    return px, torch.randint(0, 100, (N_SPLIT,), generator=g)


def _split():
    from cara_amd.data import ResidentSplit
    px, labels = _split_cpu()
    return ResidentSplit.from_tensors(px.to(DEV), labels.to(DEV))


def _trainable(m):
    return {n: p.detach().clone() for n, p in m.named_parameters() if "CP" in n or "head" in n}


@pytest.mark.parametrize("precision,weight_dropout", [("bf16", "off"), ("fp16", "off"), ("bf16", "exact")])
def test_resident_step_is_bitwise_the_step_on_cpu_normalised_images(precision, weight_dropout):
    from cara_amd._lib import CaraError
    from cara_amd.data import normalize_u8
    px, labels = _split_cpu()
    split = _split()
    m = _model(precision).train()
    eng = m._cara_engine
    eng.weight_dropout = weight_dropout
    eng.weight_dropout_seed = 77 if weight_dropout == "exact" else None
    rows = [7, 0, 7, 11]
    idx = torch.tensor(rows, device=DEV)
    dp = ((torch.rand(DEPTH, 2, 4, generator=torch.Generator().manual_seed(2)) > 0.3).float() / 0.9).to(DEV)
    assert 0 < int((dp == 0).sum()) < dp.numel()
    loss_r = eng.train_step_resident(split, idx, None, droppath=dp).clone()
    flat_r = eng._flat_grad.clone()
    x, y = normalize_u8(px[rows]).to(DEV), labels[rows].to(DEV)
    loss_b = eng.train_step(x, y, None, droppath=dp).clone()
    flat_b = eng._flat_grad.clone()
    print(f"[{precision}, weight_dropout {weight_dropout}] loss resident {loss_r.item()!r} batches {loss_b.item()!r}; "
          f"gradient elements that differ: {int((flat_r != flat_b).sum())} of {flat_r.numel()}")
    assert torch.equal(loss_r, loss_b) and torch.isfinite(loss_r)
    assert torch.equal(flat_r.view(torch.int32), flat_b.view(torch.int32)) and bool(flat_r.any())
    # the logits: forward_resident (no backward kept) against the forward of that step
    cp = [getattr(m, "CP_" + n) for n in eng.cp_fields]
    with torch.no_grad():
        want = eng._run_forward(x, dp, m.head.weight, m.head.bias, cp).clone()
    got = eng.forward_resident(split, idx, droppath=dp)
    assert torch.equal(got, want)
    assert eng.resident_bad_rows() == 0
    if precision == "fp16":      # the refusals of train_step
        eng.weight_dropout = "exact"
        with pytest.raises(CaraError, match="fp16"):
            eng.train_step_resident(split, idx, None, droppath=dp)
        eng.weight_dropout = "off"
    with pytest.raises(CaraError, match="rows"):
        eng.train_step_resident(split, idx.to(torch.int32), None)
    with pytest.raises(CaraError, match="split"):
        eng.train_step_resident((x, y), idx, None)
    torch.cuda.synchronize()


def test_fit_resident_feed_equals_fit_over_cpu_normalised_batches():
    from cara_amd import dist as D
    from cara_amd.data import normalize_u8
    from cara_amd.recipe import fit
    px, labels = _split_cpu()
    split = _split()
    seed, batch = 5, 4

    def batches(epoch):
        return [(normalize_u8(px[i]).to(DEV), labels[i].to(DEV)) for i in D.epoch_shard(N_SPLIT, epoch, 0, 1, batch, seed)]
    assert len(batches(0)) == 3
    m_b, m_r = _model(), _model()
    start = _trainable(m_b)
    fit(m_b, batches, None, epochs=2, lr=1e-3, seed=seed)
    fit(m_r, (split, split.train_rows(batch, seed=seed)), None, epochs=2, lr=1e-3, seed=seed, feed="resident")
    a, b = _trainable(m_b), _trainable(m_r)
    assert a.keys() == b.keys() and len(a) == 14
    for n in a:
        assert torch.equal(a[n], b[n]), n
    assert any(not torch.equal(a[n], start[n]) for n in a)
    assert m_r._cara_engine.resident_bad_rows() == 0


def test_graph_replay_rereads_the_index_vector():
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    split = _split()
    g = torch.Generator().manual_seed(8)
    rows = [torch.randint(0, N_SPLIT, (4,), generator=g).to(DEV) for _ in range(5)]
    assert len({tuple(r.tolist()) for r in rows}) == 5
    out = {}
    for mode in ("eager", "graph"):
        m = _model(drop_path_rate=0.0).train()
        eng = m._cara_engine
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        gstep = GraphedTrainStep(eng, opt) if mode == "graph" else None
        losses = []
        for it, r in enumerate(rows):
            opt.param_groups[0]["lr"] = 1e-3 * (0.7 ** it)
            if gstep is not None:
                loss = gstep(split, r)
            else:
                opt.advance()
                loss = eng.train_step_resident(split, r, opt)
            losses.append(loss.item())
        if gstep is not None:
            (ent,) = gstep._graphs.values()
            assert ent[1] is split and sum(t.numel() * t.element_size() for t in ent[2]) == 8 * 4     # the static input: the index vector
        out[mode] = (losses, _trainable(m))
    print(f"losses eager {out['eager'][0]} graph {out['graph'][0]}")
    assert out["graph"][0] == out["eager"][0] and len(set(out["eager"][0])) == 5
    for n in out["eager"][1]:
        assert torch.equal(out["graph"][1][n], out["eager"][1][n]), n


def test_fit_raises_on_a_row_outside_the_split_even_in_a_short_fit():
    """a hand-made feed whose one batch holds the index n_split (train_rows would have refused it on the host): the step runs
    on a zero image, and fit reads the counter after its last epoch -- one epoch never reaches an evaluation epoch.  The split
    is the middle twelve images of fourteen, as in the kernel test above"""
    from cara_amd._lib import CaraError
    from cara_amd.data import ResidentSplit
    from cara_amd.recipe import fit
    px, labels = _split_cpu()
    px_all = torch.cat([px[:1], px, px[:1]]).to(DEV)
    lb_all = torch.cat([labels[:1], labels, labels[:1]]).to(DEV)
    split = ResidentSplit.from_tensors(px_all[1:1 + N_SPLIT], lb_all[1:1 + N_SPLIT])
    rows = torch.tensor([1, N_SPLIT, 2, 3], device=DEV)
    m = _model()
    with pytest.raises(CaraError, match="2 row index"):     # the image row and the label row count one each
        fit(m, (split, lambda epoch: iter([rows])), None, epochs=1, lr=1e-3, seed=5, feed="resident")
    assert m._cara_engine.resident_bad_rows() == 0          # read and cleared


def test_graph_replay_survives_an_eager_step_of_another_batch_size():
    """the captured step holds the addresses of the engine's label, loss and dlogits buffers of its batch size; an eager step of
    another batch size in between must not free them.  Same losses and parameters as the all-eager sequence"""
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    split = _split()
    g = torch.Generator().manual_seed(12)
    rows4 = [torch.randint(0, N_SPLIT, (4,), generator=g).to(DEV) for _ in range(4)]
    rows2 = torch.randint(0, N_SPLIT, (2,), generator=g).to(DEV)
    out = {}
    for mode in ("eager", "graph"):
        m = _model(drop_path_rate=0.0).train()
        eng = m._cara_engine
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        gstep = GraphedTrainStep(eng, opt) if mode == "graph" else None
        losses = []
        for it, r in enumerate(rows4[:3] + [rows2] + rows4[3:]):     # warm, capture + replay, replay, eager batch 2, replay
            if gstep is not None and r.shape[0] == 4:
                losses.append(gstep(split, r).item())
            else:
                opt.advance()
                losses.append(eng.train_step_resident(split, r, opt).item())
            if it == 3:
                junk = [torch.full((n,), -1, dtype=torch.int64, device=DEV) for n in (4, 4, 4 * 100, 4 * 100)]   # noqa: F841
        out[mode] = (losses, _trainable(m))
    print(f"losses eager {out['eager'][0]} graph {out['graph'][0]}")
    assert out["graph"][0] == out["eager"][0]
    for n in out["eager"][1]:
        assert torch.equal(out["graph"][1][n], out["eager"][1][n]), n
