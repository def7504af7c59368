"""Host restatement of a forward behind a patch dropout, for tests/test_patchdrop_model.py and tests/test_patchdrop_gpu.py, built on
oracle.cara_oracle UNCHANGED: with K a perfect square, the kept patches of one sample are laid out row-major as an image of
sqrt(K) x sqrt(K) patches, and the oracle is called on that image with batch 1 and ``pos_embed`` replaced by rows [0] + (1 + keep[b])
-- behind the position embedding the model does not know where a token came from.  The loss is a mean over the batch, so the
gradients of the batch are the mean of the per-sample ones."""
import math

import torch

from oracle import cara_oracle as O


def kept_image(x_b, keep_b, patch=16):
    """[C, H, W] (any dtype) -> [C, s patch, s patch], s = sqrt(K): patch keep_b[j] at grid position (j // s, j % s)"""
    K = len(keep_b)
    s = math.isqrt(K)
    assert s * s == K, "the restatement lays the kept patches out as a square image"
    gw = x_b.shape[2] // patch
    cut = [x_b[:, (k // gw) * patch:(k // gw + 1) * patch, (k % gw) * patch:(k % gw + 1) * patch] for k in (int(v) for v in keep_b)]
    return torch.cat([torch.cat(cut[r * s:(r + 1) * s], dim=2) for r in range(s)], dim=1).contiguous()


def kept_pos(pos_embed, keep_b):
    """pos_embed [1, 1 + P, D] -> [1, 1 + K, D]: row 0 and rows 1 + keep_b"""
    return pos_embed[:, [0] + [1 + int(k) for k in keep_b]].contiguous()


def kept_weights(w, keep_b):
    ww = dict(w)
    ww["pos_embed"] = kept_pos(w["pos_embed"], keep_b)
    return ww


def _dp_of(drop_path_keep, b):
    return None if drop_path_keep is None else drop_path_keep[:, :, b:b + 1]


def dropped_forward(x, w, cp, keep, *, drop_path_keep=None, **kw):
    """logits [B, classes] of O.vit_cara_forward, sample by sample, on the kept patches; ``kw`` as there (s, depth, bf16_sim ...)"""
    return torch.cat([O.vit_cara_forward(kept_image(x[b], keep[b])[None], kept_weights(w, keep[b]), cp, drop_path_keep=_dp_of(drop_path_keep, b), **kw)
                      for b in range(x.shape[0])])


def dropped_train_step(x, y, w, cp, head, keep, *, s, depth, drop_path_keep=None):
    """(loss, logits, gradients) of O.train_step_as_written on the kept patches: the mean over the per-sample calls"""
    B = x.shape[0]
    loss, logits, grads = 0.0, [], None
    for b in range(B):
        l_b, lg, g = O.train_step_as_written(kept_image(x[b], keep[b])[None], y[b:b + 1], kept_weights(w, keep[b]), cp, head, s=s, depth=depth,
                                             drop_path_keep=_dp_of(drop_path_keep, b))
        loss = loss + l_b / B
        logits.append(lg)
        grads = {n: t / B for n, t in g.items()} if grads is None else {n: grads[n] + g[n] / B for n in g}
    return loss, torch.cat(logits), grads


def case5_inputs(K, B=3, img=96, P=36):
    """the batch, labels and keep table (unordered, another subset per sample) of the oracle comparison at K kept patches: shared by the
    host pre-check of the rounding model (tests/test_patchdrop_model.py) and the device test (tests/test_patchdrop_gpu.py)"""
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(B, 3, img, img, generator=g), torch.randint(0, 100, (B,), generator=g)
    keep = torch.stack([torch.randperm(P, generator=torch.Generator().manual_seed(40 + b))[:K] for b in range(B)]).to(torch.int32)
    return x, y, keep
