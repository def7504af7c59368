"""The counting of ``cara_eval_accumulate`` (include/cara_hip.h) in plain torch, on whatever device the logits are on.

Not a forward: the model has no CPU path.  This is only what happens to a batch of logits once it exists -- rows scored,
top-1 hits, top-5 hits, the sum of the per-row cross-entropy, rows with an invalid label -- so that the shard and
all-reduce logic of ``CaraEngine.evaluate`` can be tested under gloo without a GPU, and so that the kernel has a yardstick
that shares no code with it.  Everything is computed in fp64 from the fp32 logits.

State: ``float64 [5] = (n, top1, top5, loss_sum, bad_labels)``, the kernel's five words (counts are exact in fp64 up to
2^53).  Tie rule, as in the kernel: the label's position in a stable descending sort of its row,
``rank = #{c: l[c] > l[y]} + #{c < y: l[c] == l[y]}``; top-1 is ``rank == 0`` (numpy.argmax's lowest index), top-5 is
``rank < 5``.  A row whose label is outside ``[0, classes)`` adds to the last word only.
"""
from __future__ import annotations

import torch

STATE_WORDS = 5
N, TOP1, TOP5, LOSS, BAD = range(STATE_WORDS)


def new_state(device="cpu") -> torch.Tensor:
    return torch.zeros(STATE_WORDS, dtype=torch.float64, device=device)


def accumulate(state: torch.Tensor, logits: torch.Tensor, labels: torch.Tensor, n_valid: int = None) -> torch.Tensor:
    """Add the first ``n_valid`` rows (default: all) of ``logits`` [B, classes] / ``labels`` int64 [B] into ``state``."""
    n_valid = logits.shape[0] if n_valid is None else int(n_valid)
    if not 0 <= n_valid <= logits.shape[0] or labels.shape[0] != logits.shape[0]:
        raise ValueError("n_valid must lie in [0, B] and labels must hold B entries")
    l = logits[:n_valid].to(torch.float64)
    y = labels[:n_valid].to(torch.int64)
    classes = l.shape[1]
    ok = (y >= 0) & (y < classes)
    l, y = l[ok], y[ok]
    state[BAD] += float((~ok).sum())
    if l.shape[0] == 0:
        return state
    v = l.gather(1, y.view(-1, 1))
    cols = torch.arange(classes, device=l.device).view(1, -1)
    rank = (l > v).sum(1) + ((l == v) & (cols < y.view(-1, 1))).sum(1)
    state[N] += float(l.shape[0])
    state[TOP1] += float((rank == 0).sum())
    state[TOP5] += float((rank < 5).sum())
    state[LOSS] += (torch.logsumexp(l, dim=1) - v.view(-1)).sum()
    return state


def result(state) -> dict:
    """``dict(top1, top5, loss, n)`` of a state (a tensor or five numbers), the form ``CaraEngine.evaluate`` returns."""
    n, t1, t5, loss, bad = [float(v) for v in state]
    if bad:
        raise ValueError(f"{int(bad)} label(s) outside [0, classes)")
    d = max(n, 1.0)
    return {"top1": t1 / d, "top5": t5 / d, "loss": loss / d, "n": int(n)}
