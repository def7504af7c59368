"""Child process of test_views_two_ranks_on_one_gpu_return_the_same_dict: rank `argv[1]` of `argv[2]`, every rank on cuda:0 over
gloo.  Scores its shard of the 256-pixel synthetic split of tests/test_eval_views_gpu.py through centre crop + flip with
CaraEngine.evaluate(views=) and writes the returned dict (plus the samples every rank scored) to `argv[3]`.<rank>.json."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    rank, world, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from cara_amd.data import EvalViews
    from tests.test_eval_views_gpu import BATCH, N_TWO_RANKS, model_and_split
    m, split = model_and_split(N_TWO_RANKS)
    valid = []
    res = m._cara_engine.evaluate(split, BATCH, views=EvalViews.center(224, flip=True),
                                  debug_hook=lambda lg, lb, nv, comb: valid.append(nv))
    counts = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([sum(valid)]))
    res["samples"] = [int(c) for c in counts]
    with open(f"{out}.{rank}.json", "w") as fh:
        json.dump(res, fh)
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
