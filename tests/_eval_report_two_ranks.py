"""Child process of test_two_ranks_on_one_gpu_return_the_one_rank_report: rank `argv[1]` of `argv[2]`, every rank on cuda:0 over
gloo.  Scores its shard of a 300-image synthetic split with CaraEngine.evaluate(report=True) at batch 64 and writes the returned
dict (tensors as lists, NaN as None; plus the number of batches every rank ran) to `argv[3]`.<rank>.json.  The test imports
`score` and `as_json` for the one-rank dict."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

IMAGES, BATCH, CLASSES, BINS = 300, 64, 7, 15


def score(batches_seen, group=None):
    """evaluate(report=True) of the depth-2 model on the split; `batches_seen` (a list or None) collects every batch's n_valid"""
    from cara_amd.data import ResidentSplit
    from tests.test_eval_gpu import _model, _pixels
    m = _model(2, num_classes=CLASSES)
    with torch.no_grad():
        m.head.weight.mul_(10.0)
    px, labels = _pixels(IMAGES, seed=9, classes=CLASSES)
    split = ResidentSplit.from_tensors(px.cuda(), labels.cuda())
    hook = None if batches_seen is None else (lambda lg, lb, nv: batches_seen.append(nv))
    return m._cara_engine.evaluate(split, BATCH, group=group, debug_hook=hook, report=True, bins=BINS)


def as_json(res):
    def plain(v):
        if isinstance(v, dict):
            return {k: plain(w) for k, w in v.items()}
        if torch.is_tensor(v):
            return [None if x != x else x for x in v.tolist()]
        return None if isinstance(v, float) and v != v else v
    return plain(res)


def main():
    rank, world, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    batches = []
    res = as_json(score(batches))
    counts = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([len(batches)]))
    res["batches"] = [int(c) for c in counts]
    with open(f"{out}.{rank}.json", "w") as fh:
        json.dump(res, fh)
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
