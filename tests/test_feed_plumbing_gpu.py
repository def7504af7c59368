"""The five feed tables through the public API alone: with each table's neutral input -- same-size boxes, identity_mix,
identity_aug, identity_keep over the whole grid, identity_ra; each shown neutral singly by its own feature's tests -- every one of
the 32 combinations selects some cara_vit_forward_u8_rows* entry with some argument list, and every one must give the logits of
the plain forward, bit for bit.  Then one training step with all five tables, eager and through GraphedTrainStep: equal losses.
Depth 1, a 32-px model, four images; both operand builds."""
import functools
import itertools

import pytest
import torch

from tests import test_augmented_feed_gpu as A
from tests.test_augmented_feed_gpu import BATCH, DEV, IMG

pytestmark = pytest.mark.gpu
TABLES = ("boxes", "mix", "aug", "keep", "ra")
ROWS = [7, 0, 7, 11]


@functools.lru_cache(maxsize=None)
def _weights():
    from oracle import cara_oracle as O
    return O.synthetic_backbone(depth=1, img=IMG), O.synthetic_cp(rank=16)


def _model(precision):
    from tests.test_model_gpu import build
    w, cp = _weights()
    return build(w, cp, 16, 0.1, 1, IMG, drop_path_rate=0.0, precision=precision)


def _neutral():
    from cara_amd.data import identity_aug, identity_keep, identity_mix, identity_ra
    return {"boxes": A._same_size_boxes(BATCH, seed=1).to(DEV), "mix": identity_mix(BATCH).to(DEV), "aug": identity_aug(BATCH).to(DEV),
            "keep": identity_keep(BATCH, (IMG // 16) ** 2).to(DEV), "ra": identity_ra(BATCH).to(DEV)}


def _sources(boxes):
    """(split, rows) read through the boxes, and the split of those crops cut by torch with the rows that read it without boxes"""
    idx = torch.tensor(ROWS, device=DEV)
    return (A._split(), idx), (A._precropped_split(ROWS, boxes.cpu()), torch.arange(BATCH, device=DEV))


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_every_combination_of_neutral_tables_gives_the_plain_logits(precision):
    neutral = _neutral()
    boxed, cut = _sources(neutral["boxes"])
    eng = _model(precision).eval()._cara_engine
    plain = eng.forward_resident(*cut).clone()
    assert torch.isfinite(plain).all() and plain.abs().max() > 0
    patterns = [p for n in range(len(TABLES) + 1) for p in itertools.combinations(TABLES, n)]
    assert len(patterns) == 32
    for present in patterns:
        split, rows = boxed if "boxes" in present else cut
        got = eng.forward_resident(split, rows, **{n: neutral[n] for n in present})
        assert torch.equal(got, plain), (present, (got - plain).abs().max().item())
    assert eng.resident_bad_rows() == 0


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_step_with_all_five_tables_eager_and_graphed(precision):
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    neutral = _neutral()
    (split, rows), _ = _sources(neutral["boxes"])
    losses = {}
    for mode in ("eager", "graph"):
        m = _model(precision).train()
        eng = m._cara_engine
        opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        gstep = GraphedTrainStep(eng, opt)
        out = []
        for _ in range(3):   # warm, capture + replay, replay
            if mode == "graph":
                out.append(gstep(split, (rows, *(neutral[n] for n in TABLES))).item())
            else:
                opt.advance()
                out.append(eng.train_step_resident(split, rows, opt, **neutral).item())
        assert eng.resident_bad_rows() == 0
        losses[mode] = out
    print(f"[{precision}] losses eager {losses['eager']} graph {losses['graph']}")
    assert losses["graph"] == losses["eager"] and len(set(losses["eager"])) == 3
