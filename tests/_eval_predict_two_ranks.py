"""Child process of test_predict_two_ranks_on_one_gpu_assemble_the_one_rank_table: rank `argv[1]` of `argv[2]`, every rank on cuda:0
over gloo.  Fills its shard of the synthetic split of tests/test_eval_views_gpu.py with CaraEngine.predict -- the plain pass on the
224-pixel split, centre crop + flip on the 256-pixel one -- and writes the assembled tables as 32-bit words (and the number of rows
its own shard holds) to `argv[3]`.<rank>.pt."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def words(p):
    return {"topk": p.topk.cpu(), "prob": p.prob.view(torch.int32).cpu(), "loss": p.loss.view(torch.int32).cpu(), "rank": p.rank.cpu()}


def main():
    rank, world, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from cara_amd.data import EvalViews
    from cara_amd.dist import eval_shard
    from tests.test_eval_views_gpu import BATCH, N_SPLIT, model_and_split
    m, split = model_and_split(N_SPLIT)
    _, split224 = model_and_split(N_SPLIT, size=224)
    eng = m._cara_engine
    res = {"filled": len(eval_shard(N_SPLIT, rank, world, BATCH)),
           "plain": words(eng.predict(split224, 5, BATCH)),
           "views": words(eng.predict(split, 5, BATCH, views=EvalViews.center(224, flip=True)))}
    torch.save(res, f"{out}.{rank}.pt")
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
