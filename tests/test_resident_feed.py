"""Host side of the resident training feed: ResidentSplit.train_rows draws the indices of train_batches, fit() refuses an
unknown feed, get_data() without resident_feed returns what it returned before.  CPU only."""
import os

import pytest
import torch

from cara_amd import dist as D
from cara_amd._lib import CaraError
from cara_amd.data import ResidentSplit, get_data, normalize_u8

N, BATCH = 37, 8


def _split():
    """37 images whose pixel values and labels name the image: image i is filled with i + 1, its label is 100 + i"""
    px = (torch.arange(N, dtype=torch.uint8) + 1).reshape(N, 1, 1, 1).expand(N, 3, 8, 8).contiguous()
    return ResidentSplit.from_tensors(px, torch.arange(N) + 100)


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_train_rows_draws_the_indices_of_train_batches(rank, world):
    split = _split()
    batches = split.train_batches(BATCH, seed=3, rank=rank, world=world)
    rows_of = split.train_rows(BATCH, seed=3, rank=rank, world=world)
    steps = min(len(range(r, N, world)) for r in range(world)) // BATCH      # drop_last per rank
    assert steps >= 2
    seen = []
    for epoch in range(3):
        want, got = list(batches(epoch)), list(rows_of(epoch))
        assert len(got) == len(want) == steps, (epoch, len(got), len(want), steps)
        shard = D.epoch_shard(N, epoch, rank, world, BATCH, 3)
        for (x, y), rows, idx in zip(want, got, shard):
            assert rows.dtype == torch.int64 and tuple(rows.shape) == (BATCH,) and rows.device == split.pixels.device
            assert rows.is_contiguous() and torch.equal(rows, idx)
            assert torch.equal(split.labels.index_select(0, rows), y)
            assert torch.equal(normalize_u8(split.pixels.index_select(0, rows)), x)
        # one upload per epoch: every step's vector is a row of one [steps, batch] tensor
        base = got[0].untyped_storage().data_ptr()
        assert all(r.untyped_storage().data_ptr() == base for r in got)
        assert [r.storage_offset() for r in got] == [i * BATCH for i in range(steps)]
        seen.append(torch.stack(got))
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])     # (an epoch-seeded permutation)


def test_train_rows_refuses_an_index_outside_the_split(monkeypatch):
    split = _split()
    monkeypatch.setattr(D, "epoch_shard", lambda *a, **k: [torch.arange(BATCH), torch.arange(BATCH) + N - BATCH + 1])
    with pytest.raises(ValueError, match="outside"):
        list(split.train_rows(BATCH)(0))


def test_fit_refuses_an_unknown_feed():
    from cara_amd.recipe import fit
    split = _split()
    with pytest.raises(CaraError, match="feed"):
        fit(torch.nn.Linear(2, 2), (split, split.train_rows(BATCH)), epochs=1, feed="nonsense")


def test_get_data_without_resident_feed_returns_what_it_returned(tmp_path):
    from PIL import Image
    root = str(tmp_path)
    g = torch.Generator().manual_seed(0)
    for name, n in (("train800val200.txt", 5), ("test.txt", 3)):
        with open(os.path.join(root, name), "w") as fh:
            for i in range(n):
                fn = f"{name[:2]}{i}.png"
                Image.fromarray(torch.randint(0, 256, (12, 10, 3), generator=g, dtype=torch.uint8).numpy()).save(os.path.join(root, fn))
                fh.write(f"{fn} {i % 3}\n")
    for kw in ({}, {"resident_feed": False}):
        out = get_data("cifar", batch_size=2, root=root, device="cpu", seed=1, workers=1, **kw)
        assert isinstance(out, tuple) and len(out) == 2
        train, test = out
        assert callable(train) and callable(test) and not isinstance(train, tuple)
        ep = list(train(0))
        assert len(ep) == 2 and all(len(b) == 2 for b in ep)
        x, y = ep[0]
        assert x.dtype == torch.float32 and tuple(x.shape) == (2, 3, 224, 224) and y.dtype == torch.int64 and tuple(y.shape) == (2,)
        (tx, ty), = list(test())
        assert tx.dtype == torch.float32 and tuple(tx.shape) == (3, 3, 224, 224) and ty.tolist() == [0, 1, 2]
    # and the resident form: the split itself and its train_rows, drawing the samples of the default form
    (split, rows_of), test = get_data("cifar", batch_size=2, root=root, device="cpu", seed=1, workers=1, resident_feed=True)
    assert isinstance(split, ResidentSplit) and len(split) == 5 and callable(test)
    for rows, (x, y) in zip(rows_of(0), ep):
        assert torch.equal(normalize_u8(split.pixels.index_select(0, rows)), x) and torch.equal(split.labels.index_select(0, rows), y)
